// MinHash signatures over packed feature strings on gfx950 (upstream
// core/src/main/java/hivemall/knn/lsh/{MinHashUDTF,MinHashesUDF,bBitMinHashUDF}.java; here
// hivemall_amd/knn minhash / minhashes / bbit_minhash, ops/minhash.py).
//
// Contract: sig[r, h] = unsigned min over the names of row r of
// MurmurHash3_x86_32(name, seed0 + h mod 2^32); an empty row gives 0.  Name s is
// buf[off[s] .. off[s] + nlen[s]) (the text before the first ':'); rows are rowptr spans of
// strings.  Integer only, bit-exact with csrc/host/minhash_cpu.cpp.
//
// Shape.  A 256-thread workgroup owns MH_ROWS consecutive rows (grid stride), i.e. one contiguous
// span of strings and of bytes.  It walks that span in passes of at most MH_FEATS strings whose
// bytes fit the MH_BYTES window:
//   1. the bytes are copied to LDS (hm::stage_span of strspan.h, which states what it asks of
//      buf);
//   2. one thread per string does the seed-independent half of Murmur3 once: every 4-byte word
//      (hm::LdsWords) k1 -> rotl(k1 * c1, 15) * c2, and the same for the tail word, written to
//      LDS next to the string's length, its word offset and its local row;
//   3. every thread owns one hash index h of one of S = 256 / H "slots" (H <= 256; S = 1 and
//      several hash passes of MH_HASHES above that), walks the strings slot, slot + S, ... and
//      runs only the h1 chain and the final mix.  Lanes of one slot read the same premixed word
//      (an LDS broadcast).  The running minimum stays in a register while the row stays the
//      same and goes to the workgroup's [MH_ROWS][MH_HASHES] LDS table with one atomicMin when
//      the row changes.
// A single name longer than the window is hashed from global memory by each of its H threads
// (the window then holds nothing of it); a row with more bytes or strings than a pass holds
// simply takes more passes.  The table is written out with coalesced vector stores.
#include "common.h"
#include "murmur3.h"
#include "strspan.h"

namespace {

constexpr int MH_THREADS = 256;
constexpr int MH_ROWS = 16;        // rows per workgroup
constexpr int MH_FEATS = 256;      // strings per pass (one premix thread each)
constexpr int MH_BYTES = 8192;     // bytes staged per pass
constexpr int MH_HASHES = 256;     // hash indices per pass over the rows
constexpr int MH_MAX_GRID = 4096;

__global__ __launch_bounds__(MH_THREADS) void minhash_kernel(
        const uint8_t* __restrict__ buf, const int64_t* __restrict__ off,
        const int32_t* __restrict__ nlen, const int64_t* __restrict__ rowptr, int64_t n_rows,
        int H, uint32_t seed0, int32_t* __restrict__ out) {
    __shared__ uint4 s_raw[hm::stage_vecs(MH_BYTES)];
    __shared__ uint32_t s_words[(MH_BYTES + 16) / 4 + 1];
    __shared__ int32_t s_wbeg[MH_FEATS];     // first premixed word, -1: hash from global memory
    __shared__ int32_t s_len[MH_FEATS];
    __shared__ uint32_t s_tail[MH_FEATS];
    __shared__ int32_t s_row[MH_FEATS];      // row of the string, local to the workgroup
    __shared__ uint32_t s_min[MH_ROWS * MH_HASHES];
    __shared__ int64_t s_rowptr[MH_ROWS + 1];
    __shared__ int32_t s_end[MH_FEATS];      // end of the string inside the pass, capped at the window

    const int t = threadIdx.x;
    const int hc_all = H < MH_HASHES ? H : MH_HASHES;
    const int slots = MH_THREADS / hc_all;            // >= 1
    const int slot = t / hc_all, hl = t - slot * hc_all;
    const int64_t n_groups = (n_rows + MH_ROWS - 1) / MH_ROWS;

    for (int64_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
        const int64_t r0 = g * MH_ROWS;
        const int nr = (int)(n_rows - r0 < MH_ROWS ? n_rows - r0 : MH_ROWS);
        __syncthreads();                              // the previous group is done with s_rowptr
        if (t <= nr) s_rowptr[t] = rowptr[r0 + t];
        __syncthreads();
        const int64_t f0 = s_rowptr[0], f1 = s_rowptr[nr];

        for (int hbase = 0; hbase < H; hbase += MH_HASHES) {
            const int hc = H - hbase < MH_HASHES ? H - hbase : MH_HASHES;
            const bool active = slot < slots && hl < hc;
            for (int i = t; i < nr * MH_HASHES; i += MH_THREADS) s_min[i] = 0xFFFFFFFFu;

            for (int64_t p = f0; p < f1;) {
                // ---- the pass: strings [p, pe), as many as fit MH_FEATS and MH_BYTES (>= 1).
                // Thread t looks at string p + t: the strings that end inside the window are a
                // prefix (off is non-decreasing), so their count is the pass, found by one
                // counting barrier; the same loads serve the premix below.
                const int cap = (int)(f1 - p < MH_FEATS ? f1 - p : MH_FEATS);
                const int64_t span0 = off[p];
                int64_t my_b = 0, my_e = 0;
                int my_len = 0;
                if (t < cap) {
                    my_b = off[p + t];
                    my_e = off[p + t + 1];
                    my_len = nlen[p + t];
                    s_end[t] = (int32_t)(my_e - span0 < MH_BYTES ? my_e - span0 : MH_BYTES);
                }
                const int fit = __syncthreads_count(t < cap && my_e - span0 <= MH_BYTES);
                const int nf = fit > 0 ? fit : 1;      // a first string beyond the window goes alone
                const int64_t pe = p + nf;
                const int staged = s_end[nf - 1];      // bytes of the pass, at most the window
                // ---- 1. bytes -> LDS; byte i of the span is byte lead + i of s_raw
                const int lead = hm::stage_span<MH_THREADS>(buf + span0, staged, s_raw);
                __syncthreads();
                // ---- 2. the seed-independent half, one thread per string
                if (t < nf) {
                    const int64_t s = p + t;
                    const int b = (int)(my_b - span0);
                    const int L = my_len;
                    // local row: the last row whose first string is <= s (empty rows skipped)
                    int lo = 0, hi = nr - 1;
                    while (lo < hi) {
                        const int mid = (lo + hi + 1) >> 1;
                        if (s_rowptr[mid] <= s) lo = mid; else hi = mid - 1;
                    }
                    s_row[t] = lo;
                    s_len[t] = L;
                    if ((int64_t)b + L <= staged) {
                        const int a = lead + b;
                        const hm::LdsWords word{reinterpret_cast<const uint32_t*>(s_raw) + (a >> 2), 8 * (a & 3)};
                        const int w0 = (a + 3) >> 2, nw = L >> 2, r = L & 3;
                        for (int i = 0; i < nw; ++i) s_words[w0 + i] = hm::mm_premix(word(i));
                        s_tail[t] = r ? hm::mm_premix(word(nw) & ((1u << (8 * r)) - 1u)) : 0;
                        s_wbeg[t] = w0;
                    } else {
                        s_tail[t] = 0;
                        s_wbeg[t] = -1;
                    }
                }
                __syncthreads();
                // ---- 3. the seed-dependent chain per (string, hash)
                if (active) {
                    const uint32_t seed = seed0 + (uint32_t)(hbase + hl);
                    int cur_row = -1;
                    uint32_t cur = 0xFFFFFFFFu;
                    for (int j = slot; j < nf; j += slots) {
                        const int row = s_row[j];
                        if (row != cur_row) {
                            if (cur_row >= 0) atomicMin(&s_min[cur_row * MH_HASHES + hl], cur);
                            cur_row = row;
                            cur = 0xFFFFFFFFu;
                        }
                        const int L = s_len[j], w0 = s_wbeg[j];
                        uint32_t h1;
                        if (w0 >= 0) {
                            h1 = seed;
                            const int nw = L >> 2;
                            for (int i = 0; i < nw; ++i) h1 = hm::mm_chain(h1, s_words[w0 + i]);
                            h1 = hm::mm_fmix(h1 ^ s_tail[j], (uint32_t)L);
                        } else {
                            h1 = hm::mm3(hm::GlobalWords{buf + off[p + j], L}, L, seed);
                        }
                        cur = h1 < cur ? h1 : cur;
                    }
                    if (cur_row >= 0) atomicMin(&s_min[cur_row * MH_HASHES + hl], cur);
                }
                __syncthreads();
                p = pe;
            }
            if (f0 == f1) __syncthreads();            // s_min initialised before it is read
            // ---- the group's [nr, hc] block of the result; empty rows give 0
            for (int i = t; i < nr * hc; i += MH_THREADS) {
                const int r = i / hc, h = i - r * hc;
                const bool empty = s_rowptr[r + 1] == s_rowptr[r];
                out[(r0 + r) * (int64_t)H + hbase + h] = empty ? 0 : (int32_t)s_min[r * MH_HASHES + h];
            }
            __syncthreads();                          // before the next hash pass resets s_min
        }
    }
}

}  // namespace

// sig int32 [n_rows, H] (uint32 bit patterns)
HM_API int hm_minhash_sig(const uint8_t* buf, const int64_t* off, const int32_t* nlen,
                          const int64_t* rowptr, int64_t n_rows, int H, uint32_t seed0,
                          int32_t* out, hipStream_t stream) {
    if (n_rows <= 0 || H <= 0) return 0;
    int64_t blocks = (n_rows + MH_ROWS - 1) / MH_ROWS;
    if (blocks > MH_MAX_GRID) blocks = MH_MAX_GRID;
    hipLaunchKernelGGL(minhash_kernel, dim3((int)blocks), dim3(MH_THREADS), 0, stream, buf, off, nlen,
                       rowptr, n_rows, H, seed0, out);
    HM_LAUNCH_RET();
}
