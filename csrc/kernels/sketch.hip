// HyperLogLog and Bloom sketches over one packed string column on gfx950 (upstream
// core/src/main/java/hivemall/sketch/{hll/ApproxCountDistinctUDAF,bloom/*}.java; here
// hivemall_amd/misc approx_count_distinct / bloom / bloom_contains[_any], ops/sketch.py).
//
// Contract (docs/compat.md "Sketches"; the classes misc.HyperLogLog / misc.Bloom are the
// definition).  mm3 = MurmurHash3_x86_32 over the UTF-8 bytes of a value, unsigned.
//   64-bit hash  h64 = (mm3(s, hm::SKETCH_SEED_HI) << 32) | mm3(s, hm::SKETCH_SEED_LO)  (murmur3.h)
//   HyperLogLog  p in 4..16, m = 2^p; idx = h64 >> (64 - p); w = (h64 << p) mod 2^64;
//                rho = min(clz64(w), 64 - p) + 1 with clz64(0) = 64 (so rho <= 65 - p);
//                reg[g, idx] = max(reg[g, idx], rho)
//   histogram    hist[g, r] = number of registers of group g equal to r, int32 [G, 66]
//   Bloom        h1 = mm3(s, 0), h2 = mm3(s, h1); bit i_j = (h1 + j * h2) mod m, j = 0..k-1, in
//                64-bit arithmetic (no wrap at 2^32); bit i is bit i & 7 of byte i >> 3, i.e. bit
//                i & 31 of the little-endian 32-bit word i >> 5; m a multiple of 32 in
//                32..2^26, k in 1..16
// Integer only; max and or are commutative and idempotent, so the result does not depend on the
// schedule: bit-exact with csrc/host/sketch_cpu.cpp and with the Python classes.
//
// Input: buf uint8 + off int64 [n + 1] (value s = buf[off[s] .. off[s + 1])) and one int32 group
// (filter) id per value, unsorted.
//
// Front end, shared by the four kernels: hm::sweep of strspan.h (which states what it asks of
// buf), SK_STRINGS values and an SK_BYTES window per 256-thread workgroup and step; each lane
// hashes its own value.  HyperLogLog does the seed-independent premix rotl(k * c1, 15) * c2 once
// per word and runs the two seed chains over it; Bloom's second seed is the first hash, so it
// walks the words twice.
//
// HyperLogLog update.  The byte maximum is a read filter (stop when the byte is already >= rho)
// plus a 32-bit compare-and-swap loop on the containing word.  A stale read (this CU's L1,
// another XCD's L2) can only be too low, never too high - registers only grow - so the filter
// never drops an update; the CAS itself returns the word as memory has it.
//   * LDS path, G * 2^p <= SK_LDS_REG_BYTES: every workgroup keeps a private register file in
//     (dynamic) LDS for its whole sweep, updates it with the same helper, and merges its non-zero
//     words into reg once at the end, four registers per compare-and-swap.  The flush reads reg
//     past L1 first, so it skips what earlier flushes already raised, and every workgroup starts
//     at another word.  The grid is capped at SK_LDS_MAX_GRID so the flushes stay a small part
//     of the work.
//   * direct path, anything larger: the filtered CAS goes straight to reg.
// Bloom add is atomicOr behind the same kind of filter (a stale read can only miss a set bit).
#include "common.h"
#include "murmur3.h"
#include "strspan.h"

namespace {

constexpr int SK_THREADS = 256;
constexpr int SK_STRINGS = 256;              // values per workgroup and sweep step (one per lane)
constexpr int SK_BYTES = 8192;               // bytes staged per step
constexpr int SK_LDS_REG_BYTES = 64 * 1024;  // largest register file kept in LDS
constexpr int SK_MAX_GRID = 2048;
constexpr int SK_LDS_MAX_GRID = 512;         // LDS path: docs/perf_notes.md "Sketches", grid sweep
constexpr int SK_HIST = 66;                  // rho is in 0..65 - p <= 61; 66 as the contract says

// the two halves of h64: one premix per word, two chains
template <typename Words>
__device__ __forceinline__ uint64_t mm3_h64(const Words& word, int len) {
    uint32_t ha = hm::SKETCH_SEED_HI, hb = hm::SKETCH_SEED_LO;
    const int nw = len >> 2, r = len & 3;
    for (int i = 0; i < nw; ++i) {
        const uint32_t k = hm::mm_premix(word(i));
        ha = hm::mm_chain(ha, k);
        hb = hm::mm_chain(hb, k);
    }
    if (r) {
        const uint32_t k = hm::mm_premix(word(nw) & ((1u << (8 * r)) - 1u));
        ha ^= k;
        hb ^= k;
    }
    return ((uint64_t)hm::mm_fmix(ha, (uint32_t)len) << 32) | hm::mm_fmix(hb, (uint32_t)len);
}

// reg byte = max(reg byte, rho) on the 32-bit word that holds it (global memory or LDS)
__device__ __forceinline__ void byte_max(uint32_t* word, int sh, uint32_t rho) {
    uint32_t old = *word;
    while (((old >> sh) & 0xFFu) < rho) {
        const uint32_t want = (old & ~(0xFFu << sh)) | (rho << sh);
        const uint32_t seen = atomicCAS(word, old, want);
        if (seen == old) break;
        old = seen;
    }
}

__device__ __forceinline__ uint32_t max_bytes(uint32_t a, uint32_t b) {
    uint32_t r = 0;
#pragma unroll
    for (int sh = 0; sh < 32; sh += 8) {
        const uint32_t x = (a >> sh) & 0xFFu, y = (b >> sh) & 0xFFu;
        r |= (x > y ? x : y) << sh;
    }
    return r;
}

// every byte of the word at once: the flush of a workgroup's LDS register file
__device__ __forceinline__ void word_max(uint32_t* word, uint32_t v) {
    uint32_t old = hm::ld_coherent(word);       // past L1: see what earlier flushes left
    for (;;) {
        const uint32_t want = max_bytes(old, v);
        if (want == old) break;
        const uint32_t seen = atomicCAS(word, old, want);
        if (seen == old) break;
        old = seen;
    }
}

struct HllOp {
    const int32_t* gid;
    uint32_t* reg;          // words of the register file: global [G * m / 4] or the LDS copy
    int G, p;
    template <typename Words>
    __device__ __forceinline__ void operator()(int64_t s, const Words& word, int len) const {
        const int g = gid[s];
        if ((unsigned)g >= (unsigned)G) return;
        const uint64_t h = mm3_h64(word, len);
        const uint32_t idx = (uint32_t)(h >> (64 - p));
        const uint64_t w = h << p;
        const int lz = w ? __clzll((long long)w) : 64;
        const uint32_t rho = (uint32_t)(lz < 64 - p ? lz : 64 - p) + 1u;
        const int64_t byte = ((int64_t)g << p) + idx;
        byte_max(reg + (byte >> 2), 8 * (int)(byte & 3), rho);
    }
};

__global__ __launch_bounds__(SK_THREADS) void hll_direct_kernel(
        const uint8_t* __restrict__ buf, const int64_t* __restrict__ off,
        const int32_t* __restrict__ gid, int64_t n, int G, int p, uint32_t* __restrict__ reg) {
    __shared__ uint4 s_stage[hm::stage_vecs(SK_BYTES)];
    HllOp op{gid, reg, G, p};
    hm::sweep<SK_STRINGS, SK_BYTES>(buf, off, n, s_stage, op);
}

__global__ __launch_bounds__(SK_THREADS) void hll_lds_kernel(
        const uint8_t* __restrict__ buf, const int64_t* __restrict__ off,
        const int32_t* __restrict__ gid, int64_t n, int G, int p, uint32_t* __restrict__ reg) {
    __shared__ uint4 s_stage[hm::stage_vecs(SK_BYTES)];
    extern __shared__ uint32_t s_reg[];         // G * 2^p / 4 words
    const int nwords = (G << p) >> 2;
    for (int i = threadIdx.x; i < nwords; i += SK_THREADS) s_reg[i] = 0;
    __syncthreads();
    HllOp op{gid, s_reg, G, p};
    hm::sweep<SK_STRINGS, SK_BYTES>(buf, off, n, s_stage, op);            // ends with a barrier
    // workgroups that finish together start their flushes at different words
    const int rot = (int)((blockIdx.x * 2654435761u) % (uint32_t)nwords);
    for (int j = threadIdx.x; j < nwords; j += SK_THREADS) {
        const int i = j + rot < nwords ? j + rot : j + rot - nwords;
        const uint32_t v = s_reg[i];
        if (v) word_max(reg + i, v);
    }
}

__global__ __launch_bounds__(SK_THREADS) void hll_hist_kernel(const uint4* __restrict__ reg, int G, int p,
                                                              int32_t* __restrict__ hist) {
    __shared__ int32_t s_cnt[SK_THREADS / HM_WAVE][SK_HIST];     // one set per wave
    const int t = threadIdx.x, wv = t / HM_WAVE;
    const int nvec = (1 << p) >> 4;                               // 16 registers per load, m >= 16
    for (int g = blockIdx.x; g < G; g += gridDim.x) {
        for (int i = t; i < (SK_THREADS / HM_WAVE) * SK_HIST; i += SK_THREADS) (&s_cnt[0][0])[i] = 0;
        __syncthreads();
        const uint4* row = reg + (int64_t)g * nvec;
        for (int v = t; v < nvec; v += SK_THREADS) {
            const uint4 q = row[v];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t w = j == 0 ? q.x : j == 1 ? q.y : j == 2 ? q.z : q.w;
#pragma unroll
                for (int sh = 0; sh < 32; sh += 8) {
                    const uint32_t r = (w >> sh) & 0xFFu;
                    atomicAdd(&s_cnt[wv][r < SK_HIST ? r : SK_HIST - 1], 1);
                }
            }
        }
        __syncthreads();
        if (t < SK_HIST) {
            int32_t c = 0;
            for (int k = 0; k < SK_THREADS / HM_WAVE; ++k) c += s_cnt[k][t];
            hist[(int64_t)g * SK_HIST + t] = c;
        }
        __syncthreads();
    }
}

// Bit j of a key is (h1 + j * h2) mod m.  With a = h1 mod m and d = h2 mod m that is
// (a + j * d) mod m, kept reduced by one conditional subtraction per step: m <= 2^26, so nothing
// here leaves 32 bits and the result is the 64-bit formula's.
struct BloomAddOp {
    const int32_t* gid;
    uint32_t* bits;
    int G, k;
    uint32_t m;
    template <typename Words>
    __device__ __forceinline__ void operator()(int64_t s, const Words& word, int len) const {
        const int g = gid[s];
        if ((unsigned)g >= (unsigned)G) return;
        const uint32_t h1 = hm::mm3(word, len, 0u), h2 = hm::mm3(word, len, h1);
        uint32_t i = h1 % m;
        const uint32_t d = h2 % m;
        uint32_t* row = bits + (int64_t)g * (m >> 5);
        for (int j = 0; j < k; ++j) {
            const uint32_t bit = 1u << (i & 31);
            uint32_t* w = row + (i >> 5);
            if (!(*w & bit)) atomicOr(w, bit);
            i += d;
            if (i >= m) i -= m;
        }
    }
};

struct BloomTestOp {
    const int32_t* fid;
    const uint32_t* bits;
    uint8_t* hit;
    int F, k;
    uint32_t m;
    template <typename Words>
    __device__ __forceinline__ void operator()(int64_t s, const Words& word, int len) const {
        const int f = fid[s];
        if ((unsigned)f >= (unsigned)F) { hit[s] = 0; return; }
        const uint32_t h1 = hm::mm3(word, len, 0u), h2 = hm::mm3(word, len, h1);
        uint32_t i = h1 % m;
        const uint32_t d = h2 % m;
        const uint32_t* row = bits + (int64_t)f * (m >> 5);
        uint32_t all = 1;
        for (int j = 0; j < k; ++j) {
            all &= row[i >> 5] >> (i & 31);
            i += d;
            if (i >= m) i -= m;
        }
        hit[s] = (uint8_t)(all & 1u);
    }
};

__global__ __launch_bounds__(SK_THREADS) void bloom_add_kernel(
        const uint8_t* __restrict__ buf, const int64_t* __restrict__ off,
        const int32_t* __restrict__ gid, int64_t n, int G, uint32_t m, int k, uint32_t* __restrict__ bits) {
    __shared__ uint4 s_stage[hm::stage_vecs(SK_BYTES)];
    BloomAddOp op{gid, bits, G, k, m};
    hm::sweep<SK_STRINGS, SK_BYTES>(buf, off, n, s_stage, op);
}

__global__ __launch_bounds__(SK_THREADS) void bloom_test_kernel(
        const uint8_t* __restrict__ buf, const int64_t* __restrict__ off,
        const int32_t* __restrict__ fid, int64_t n, const uint32_t* __restrict__ bits, int F, uint32_t m,
        int k, uint8_t* __restrict__ hit) {
    __shared__ uint4 s_stage[hm::stage_vecs(SK_BYTES)];
    BloomTestOp op{fid, bits, hit, F, k, m};
    hm::sweep<SK_STRINGS, SK_BYTES>(buf, off, n, s_stage, op);
}

int sweep_grid(int64_t n, int cap) {
    const int64_t blocks = (n + SK_STRINGS - 1) / SK_STRINGS;
    return (int)(blocks < cap ? blocks : cap);
}

bool hll_args_ok(int G, int p) { return G >= 1 && p >= 4 && p <= 16; }
bool bloom_args_ok(int G, int64_t m, int k) {
    return G >= 1 && m >= 32 && m <= (1 << 26) && m % 32 == 0 && k >= 1 && k <= 16;
}

}  // namespace

// reg uint8 [G, 2^p], in/out.  lds_grid: the grid cap of the LDS path (<= 0: SK_LDS_MAX_GRID);
// the result does not depend on it (benchmarks/sketch_bench.py sweeps it).
HM_API int hm_hll_update_grid(const uint8_t* buf, const int64_t* off, const int32_t* gid, int64_t n,
                              int G, int p, uint8_t* reg, int lds_grid, hipStream_t stream) {
    if (!hll_args_ok(G, p)) return (int)hipErrorInvalidValue;
    if (n <= 0) return 0;
    const int64_t bytes = (int64_t)G << p;
    uint32_t* words = reinterpret_cast<uint32_t*>(reg);
    if (bytes <= SK_LDS_REG_BYTES) {
        // above the default dynamic-LDS limit once the window is added: ask for it (once)
        static const hipError_t attr = hipFuncSetAttribute(
            reinterpret_cast<const void*>(hll_lds_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
            SK_LDS_REG_BYTES);
        if (attr != hipSuccess) return (int)attr;
        const int grid = sweep_grid(n, lds_grid > 0 ? lds_grid : SK_LDS_MAX_GRID);
        hipLaunchKernelGGL(hll_lds_kernel, dim3(grid), dim3(SK_THREADS), (size_t)bytes, stream, buf, off,
                           gid, n, G, p, words);
    } else {
        hipLaunchKernelGGL(hll_direct_kernel, dim3(sweep_grid(n, SK_MAX_GRID)), dim3(SK_THREADS), 0,
                           stream, buf, off, gid, n, G, p, words);
    }
    HM_LAUNCH_RET();
}

HM_API int hm_hll_update(const uint8_t* buf, const int64_t* off, const int32_t* gid, int64_t n, int G,
                         int p, uint8_t* reg, hipStream_t stream) {
    return hm_hll_update_grid(buf, off, gid, n, G, p, reg, 0, stream);
}

// hist int32 [G, 66]
HM_API int hm_hll_hist(const uint8_t* reg, int G, int p, int32_t* hist, hipStream_t stream) {
    if (G <= 0) return 0;
    if (!hll_args_ok(G, p)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(hll_hist_kernel, dim3(G < SK_MAX_GRID ? G : SK_MAX_GRID), dim3(SK_THREADS), 0,
                       stream, reinterpret_cast<const uint4*>(reg), G, p, hist);
    HM_LAUNCH_RET();
}

// bits uint8 [G, m / 8], in/out
HM_API int hm_bloom_add(const uint8_t* buf, const int64_t* off, const int32_t* gid, int64_t n, int G,
                        int64_t m, int k, uint8_t* bits, hipStream_t stream) {
    if (!bloom_args_ok(G, m, k)) return (int)hipErrorInvalidValue;
    if (n <= 0) return 0;
    hipLaunchKernelGGL(bloom_add_kernel, dim3(sweep_grid(n, SK_MAX_GRID)), dim3(SK_THREADS), 0, stream,
                       buf, off, gid, n, G, (uint32_t)m, k, reinterpret_cast<uint32_t*>(bits));
    HM_LAUNCH_RET();
}

// hit uint8 [n]: 1 when all k bits of key s are set in filter fid[s] of bits uint8 [F, m / 8]
HM_API int hm_bloom_test(const uint8_t* buf, const int64_t* off, const int32_t* fid, int64_t n,
                         const uint8_t* bits, int F, int64_t m, int k, uint8_t* hit, hipStream_t stream) {
    if (!bloom_args_ok(F, m, k)) return (int)hipErrorInvalidValue;
    if (n <= 0) return 0;
    hipLaunchKernelGGL(bloom_test_kernel, dim3(sweep_grid(n, SK_MAX_GRID)), dim3(SK_THREADS), 0, stream,
                       buf, off, fid, n, reinterpret_cast<const uint32_t*>(bits), F, (uint32_t)m, k, hit);
    HM_LAUNCH_RET();
}
