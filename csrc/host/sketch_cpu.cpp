// CPU twin of csrc/kernels/sketch.hip (hm_hll_update / hm_hll_hist / hm_bloom_add /
// hm_bloom_test): the same contract, OpenMP over the values.
//
// Contract.  mm3 = MurmurHash3_x86_32 over the UTF-8 bytes of a value, unsigned.
//   64-bit hash  h64 = (mm3(s, hm::SKETCH_SEED_HI) << 32) | mm3(s, hm::SKETCH_SEED_LO)  (murmur3.h)
//   HyperLogLog  p in 4..16, m = 2^p; idx = h64 >> (64 - p); w = (h64 << p) mod 2^64;
//                rho = min(clz64(w), 64 - p) + 1 with clz64(0) = 64;
//                reg[g, idx] = max(reg[g, idx], rho)
//   histogram    hist[g, r] = number of registers of group g equal to r, int32 [G, 66]
//   Bloom        h1 = mm3(s, 0), h2 = mm3(s, h1); bit i_j = (h1 + j * h2) mod m, j = 0..k-1, in
//                64-bit arithmetic; bit i is bit i & 7 of byte i >> 3; m a multiple of 32 in
//                32..2^26, k in 1..16
// Integer only.  Every thread fills a private register file (bitmap) and the files are merged by
// max (or); a sketch too large for that (SK_PRIVATE_BYTES over all threads) is updated in place
// with atomic byte max / or.  max and or are commutative and idempotent, so either way the
// result is the same for any thread count, and bit-exact with the kernels.
#include <omp.h>

#include <cstdint>
#include <cstring>
#include <vector>

#include "../kernels/murmur3.h"

#define HM_API extern "C" __attribute__((visibility("default")))

namespace {

constexpr int SK_HIST = 66;
constexpr int64_t SK_PRIVATE_BYTES = int64_t(64) << 20;   // all private copies together
constexpr int64_t SK_PARALLEL_MIN = 4096;                 // values below which one thread runs

// The twin's own loops over the shared steps: 64-bit counters and the tail premix unconditional
// (hm::murmur3_bytes, with int counters and the premix behind its switch, made bloom_add 4-6 %
// slower here: docs/perf_notes.md "Sketches").
inline uint32_t mm3(const uint8_t* p, int64_t len, uint32_t seed) {
    uint32_t h = seed;
    const int64_t nw = len >> 2;
    for (int64_t i = 0; i < nw; ++i) {
        uint32_t k1;
        std::memcpy(&k1, p + 4 * i, 4);               // little-endian host
        h = hm::mm_chain(h, hm::mm_premix(k1));
    }
    h ^= hm::mm_premix(hm::mm_tail_word(p + 4 * nw, (int)(len & 3)));   // 0 when no tail
    return hm::mm_fmix(h, (uint32_t)len);
}

// one premix per word, two chains
inline uint64_t mm3_h64(const uint8_t* p, int64_t len) {
    uint32_t ha = hm::SKETCH_SEED_HI, hb = hm::SKETCH_SEED_LO;
    const int64_t nw = len >> 2;
    for (int64_t i = 0; i < nw; ++i) {
        uint32_t k1;
        std::memcpy(&k1, p + 4 * i, 4);               // little-endian host
        const uint32_t k = hm::mm_premix(k1);
        ha = hm::mm_chain(ha, k);
        hb = hm::mm_chain(hb, k);
    }
    const uint32_t k = hm::mm_premix(hm::mm_tail_word(p + 4 * nw, (int)(len & 3)));   // 0 when no tail
    ha ^= k;
    hb ^= k;
    return ((uint64_t)hm::mm_fmix(ha, (uint32_t)len) << 32) | hm::mm_fmix(hb, (uint32_t)len);
}

inline void hll_slot(uint64_t h, int p, uint32_t& idx, uint8_t& rho) {
    idx = (uint32_t)(h >> (64 - p));
    const uint64_t w = h << p;
    const int lz = w ? __builtin_clzll(w) : 64;
    rho = (uint8_t)((lz < 64 - p ? lz : 64 - p) + 1);
}

inline void atomic_byte_max(uint8_t* b, uint8_t v) {
    uint8_t old = __atomic_load_n(b, __ATOMIC_RELAXED);
    while (old < v && !__atomic_compare_exchange_n(b, &old, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {
    }
}

int team_size(int64_t n, int64_t sketch_bytes, bool& shared) {
    int threads = n < SK_PARALLEL_MIN ? 1 : omp_get_max_threads();
    if (threads < 1) threads = 1;
    shared = threads > 1 && sketch_bytes * threads > SK_PRIVATE_BYTES;
    return threads;
}

bool hll_args_ok(int G, int p) { return G >= 1 && p >= 4 && p <= 16; }
bool bloom_args_ok(int G, int64_t m, int k) {
    return G >= 1 && m >= 32 && m <= (1 << 26) && m % 32 == 0 && k >= 1 && k <= 16;
}

}  // namespace

// reg uint8 [G, 2^p], in/out
HM_API int hm_hll_update_cpu(const uint8_t* buf, const int64_t* off, const int32_t* gid, int64_t n, int G,
                             int p, uint8_t* reg) {
    if (!hll_args_ok(G, p)) return 1;
    if (n <= 0) return 0;
    const int64_t bytes = (int64_t)G << p;
    bool shared;
    const int threads = team_size(n, bytes, shared);
#pragma omp parallel num_threads(threads)
    {
        std::vector<uint8_t> mine;
        uint8_t* r = reg;
        const bool priv = !shared && omp_get_num_threads() > 1;
        if (priv) {
            mine.assign((size_t)bytes, 0);
            r = mine.data();
        }
#pragma omp for schedule(static)
        for (int64_t s = 0; s < n; ++s) {
            const int g = gid[s];
            if ((unsigned)g >= (unsigned)G) continue;
            uint32_t idx;
            uint8_t rho;
            hll_slot(mm3_h64(buf + off[s], off[s + 1] - off[s]), p, idx, rho);
            uint8_t* b = r + ((int64_t)g << p) + idx;
            if (shared) atomic_byte_max(b, rho);
            else if (*b < rho) *b = rho;
        }
        if (priv) {
#pragma omp critical(hm_sketch_merge)
            for (int64_t i = 0; i < bytes; ++i)
                if (mine[i] > reg[i]) reg[i] = mine[i];
        }
    }
    return 0;
}

// hist int32 [G, 66]
HM_API int hm_hll_hist_cpu(const uint8_t* reg, int G, int p, int32_t* hist) {
    if (G <= 0) return 0;
    if (!hll_args_ok(G, p)) return 1;
    const int64_t m = int64_t(1) << p;
#pragma omp parallel for schedule(static) if ((int64_t)G * m > 65536)
    for (int g = 0; g < G; ++g) {
        int32_t* h = hist + (int64_t)g * SK_HIST;
        for (int r = 0; r < SK_HIST; ++r) h[r] = 0;
        const uint8_t* row = reg + (int64_t)g * m;
        for (int64_t i = 0; i < m; ++i) ++h[row[i] < SK_HIST ? row[i] : SK_HIST - 1];
    }
    return 0;
}

// bits uint8 [G, m / 8], in/out
HM_API int hm_bloom_add_cpu(const uint8_t* buf, const int64_t* off, const int32_t* gid, int64_t n, int G,
                            int64_t m, int k, uint8_t* bits) {
    if (!bloom_args_ok(G, m, k)) return 1;
    if (n <= 0) return 0;
    const int64_t row_bytes = m >> 3, bytes = row_bytes * G;
    bool shared;
    const int threads = team_size(n, bytes, shared);
#pragma omp parallel num_threads(threads)
    {
        std::vector<uint8_t> mine;
        uint8_t* r = bits;
        const bool priv = !shared && omp_get_num_threads() > 1;
        if (priv) {
            mine.assign((size_t)bytes, 0);
            r = mine.data();
        }
#pragma omp for schedule(static)
        for (int64_t s = 0; s < n; ++s) {
            const int g = gid[s];
            if ((unsigned)g >= (unsigned)G) continue;
            const uint8_t* q = buf + off[s];
            const int64_t len = off[s + 1] - off[s];
            const uint64_t h1 = mm3(q, len, 0u), h2 = mm3(q, len, (uint32_t)h1);
            uint8_t* row = r + (int64_t)g * row_bytes;
            for (int j = 0; j < k; ++j) {
                const uint64_t i = (h1 + (uint64_t)j * h2) % (uint64_t)m;
                const uint8_t bit = (uint8_t)(1u << (i & 7));
                uint8_t* b = row + (i >> 3);
                if (shared) {
                    if (!(__atomic_load_n(b, __ATOMIC_RELAXED) & bit)) __atomic_fetch_or(b, bit, __ATOMIC_RELAXED);
                } else {
                    *b |= bit;
                }
            }
        }
        if (priv) {
#pragma omp critical(hm_sketch_merge)
            for (int64_t i = 0; i < bytes; ++i) bits[i] |= mine[i];
        }
    }
    return 0;
}

// hit uint8 [n]: 1 when all k bits of key s are set in filter fid[s] of bits uint8 [F, m / 8]
HM_API int hm_bloom_test_cpu(const uint8_t* buf, const int64_t* off, const int32_t* fid, int64_t n,
                             const uint8_t* bits, int F, int64_t m, int k, uint8_t* hit) {
    if (!bloom_args_ok(F, m, k)) return 1;
    const int64_t row_bytes = m >> 3;
#pragma omp parallel for schedule(static) if (n >= SK_PARALLEL_MIN)
    for (int64_t s = 0; s < n; ++s) {
        const int f = fid[s];
        if ((unsigned)f >= (unsigned)F) { hit[s] = 0; continue; }
        const uint8_t* q = buf + off[s];
        const int64_t len = off[s + 1] - off[s];
        const uint64_t h1 = mm3(q, len, 0u), h2 = mm3(q, len, (uint32_t)h1);
        const uint8_t* row = bits + (int64_t)f * row_bytes;
        unsigned all = 1;
        for (int j = 0; j < k; ++j) {
            const uint64_t i = (h1 + (uint64_t)j * h2) % (uint64_t)m;
            all &= (unsigned)row[i >> 3] >> (i & 7);
        }
        hit[s] = (uint8_t)(all & 1u);
    }
    return 0;
}
