// Fused top-k maximum-inner-product search with fp32 operands on the gfx950 matrix cores.
//
//   out[q] = top-KT over items n of  s(q, n) = <Q[q], I[n]> + item_bias[n]
//
// The contract of topk_mips.hip (hm_mips_topk) in every respect but the operands: Q and I are
// fp32, the products are fp32 and the accumulation is fp32, so a score carries the rounding of
// one fp32 dot product and the ranking is the ranking of mf_predict's own fp32 scores
// (mips_topk(..., precision="fp32") in ops/topk_mips.py).
//
// Padded Kd set: 16, 32, 64, 128, 256.  The fp32 MFMAs step k by 2 and 4, but one 16-B LDS read
// feeds four of them (below), which makes the granule 8 floats in the register kernel and 16 in
// the LDS-candidate kernel, and the XOR swizzle wants a power-of-two chunk count per row.  Powers
// of two from 16 keep it at 5 x (3 list sizes + 1) x 2 = 40 instantiations; d = 10 pays for 16,
// not for 32.
//
// Data movement (what differs from the bf16 kernels):
//   * Fragment reads.  v_mfma_f32_32x32x2_f32 takes ONE float per lane per operand (lane l:
//     row l & 31, k = l >> 5), v_mfma_f32_16x16x4_f32 likewise (row l & 15, k = l >> 4).  Read
//     naively that is a ds_read_b32 per MFMA at a row stride of Kd * 4 bytes.  Instead k is
//     relabelled: of every chunk of 8 (16) consecutive floats, lane half (lane group) h owns floats
//     4h .. 4h+3, read with one ds_read_b128, and MFMA j of the four that follow takes component
//     j.  MFMA j then sums over h the products at k = 8c + 4h + j (16c + 4h + j): the four
//     together cover the chunk exactly once.  The query fragments are loaded with the same
//     relabelling, so the dot product is the same sum in another order.
//   * With 16-B reads the swizzle of topk_mips.hip carries over with CPR = Kd / 4 chunks per row:
//     the 16 lanes of a ds_read_b128 phase read 16 consecutive rows at one chunk index and land
//     on 16 distinct chunk columns, i.e. all 64 banks.
//   * Stages.  fp32 doubles the bytes per item.  The register kernel keeps the 32 KB stage
//     (8192 / Kd items: 512 at Kd 16, one 32-item tile at Kd 256) and the 8-chunk (32 VGPR)
//     register prefetch; at Kd = 256 one tile is 128 MFMAs of 16 passes, about 8K cycles per
//     wave, which is several L2/MALL latencies, so a barrier pair per tile still hides the
//     prefetch.  The LDS-candidate kernel owns 48 KB of candidate buffers; its stage is 16 KB
//     up to Kd 64 (two blocks per CU in 160 KB), and one 64-item tile above (32 KB at Kd 128,
//     64 KB at Kd 256, one block per CU).
//   * The tile loop of the no-exclusion variants holds no global load; the next stage is
//     prefetched into registers (see the header of topk_mips.hip for the measurements behind
//     both rules).
//   * Query fragments stay in VGPRs for the whole sweep: Kd / 2 floats per lane in the register
//     kernel (128 at Kd 256; with one wave per SIMD the kernel has 512 registers, and the
//     resource report shows no scratch for any instantiation — docs/perf_notes.md has the table),
//     Kd / 4 in the LDS-candidate kernel.
//
// Selection (sorted per-lane lists with an exact threshold and a 4-entry queue for KT <= 32;
// ballot / append / compact candidate buffers in LDS for KT 33..64) is a copy of topk_mips.hip's,
// not a shared template: moving that code would change how the bf16 kernels are compiled, and
// they are the flagship recommendation path whose 2.8 ms rests on details of the generated code
// (waitcnt placement, register classes of the prefetch vectors).  Leaving topk_mips.hip
// untouched keeps its code objects identical; the price is the duplicated selection code below.
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;

constexpr int BM = 64;      // query rows per block (LDS-candidate kernel)
constexpr int BN = 64;      // items per tile (LDS-candidate kernel); splits start at multiples
constexpr int NT = 256;     // threads per block
constexpr int KT_MAX = 64;
constexpr int CAPV = 96;    // candidate slots per row (KT 33..64)

struct MipsF32Params {
    int M, N, KT, splits, n_per_split;
    int self_offset;        // exclude n == q + self_offset when use_self
    int use_self;
};

// Entry order: higher score first; equal scores -> lower item index first.
__device__ __forceinline__ bool better(float sa, int ia, float sb, int ib) {
    return sa > sb || (sa == sb && ia < ib);
}

__device__ __forceinline__ bool is_excluded(const int64_t* __restrict__ ptr,
                                            const int32_t* __restrict__ ex, int q, int n) {
    int64_t lo = ptr[q], hi = ptr[q + 1];
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        const int v = ex[mid];
        if (v == n) return true;
        if (v < n) lo = mid + 1; else hi = mid;
    }
    return false;
}

// Swizzled chunk position: 16-B chunk c of tile row n (CPR chunks per row, a power of two).
template <int CPR>
__device__ __forceinline__ int swz(int n, int c) {
    if constexpr (CPR >= 16) return n * CPR + (c ^ (n & 15));
    else return n * CPR + (c ^ ((n / (16 / CPR)) & (CPR - 1)));
}

// Stage prefetch (global -> registers) and commit (registers -> swizzled LDS), shared by both
// kernels.  Rows past n_end are clamped to the last item: in bounds, and masked by the filters.
#define MIPSF_FETCH(N0)                                                                        \
    do {                                                                                       \
        _Pragma("unroll") for (int r = 0; r < PRE; ++r) {                                      \
            const int e = tid + NT * r;                                                        \
            const int n = min((N0) + e / CPR, n_end - 1);                                      \
            const uint4 v_ = reinterpret_cast<const uint4*>(I)[(size_t)n * CPR + (e % CPR)];  \
            pre[4 * r] = v_.x; pre[4 * r + 1] = v_.y; pre[4 * r + 2] = v_.z; pre[4 * r + 3] = v_.w; \
        }                                                                                      \
        _Pragma("unroll") for (int r = 0; r < (STAGE + NT - 1) / NT; ++r)                      \
            pre_b[r] = item_bias ? item_bias[min((N0) + tid + NT * r, n_end - 1)] : 0.f;       \
    } while (0)
#define MIPSF_COMMIT()                                                                         \
    do {                                                                                       \
        _Pragma("unroll") for (int r = 0; r < PRE; ++r) {                                      \
            const int e = tid + NT * r;                                                        \
            s_tile[swz<CPR>(e / CPR, e % CPR)] =                                               \
                make_uint4(pre[4 * r], pre[4 * r + 1], pre[4 * r + 2], pre[4 * r + 3]);         \
        }                                                                                      \
        _Pragma("unroll") for (int r = 0; r < (STAGE + NT - 1) / NT; ++r)                      \
            if (tid + NT * r < STAGE) s_bias[tid + NT * r] = pre_b[r];                         \
    } while (0)

// ---------------------------------------------------------------------------------------------
// KT <= 32: per-lane register lists.  The score tile is computed transposed on
// v_mfma_f32_32x32x2_f32 — 32 items as the A (row) operand, the wave's 32 queries as B — so lane
// l owns query l & 31 for the whole sweep and holds 16 of every 32 items' scores (lane l ^ 32
// the other 16): accumulator r is item (r & 3) + 8 (r >> 2) + 4 (l >> 5).  KC = Kd / 8 chunks of
// k; per chunk one 16-B read of the item row and four MFMAs against b[c].xyzw.
template <int KD, int KTC, bool EXCL>
__global__ __launch_bounds__(NT) void mips_topk_reg_f32_kernel(
    MipsF32Params P, const f32x4* __restrict__ Q, const f32x4* __restrict__ I,
    const float* __restrict__ item_bias, const int64_t* __restrict__ ex_ptr,
    const int32_t* __restrict__ ex_idx, int32_t* __restrict__ out_idx, float* __restrict__ out_score)
{
    constexpr int CPR = KD / 4;                          // 16-B chunks per row
    constexpr int KC = KD / 8;                           // k chunks of 8 floats
    constexpr int STAGE = 32768 / (KD * 4);              // items per 32 KB stage
    constexpr int PRE = STAGE * CPR / NT;                // = 8 chunks per thread
    constexpr int BQ = 128;                              // queries per block (32 per wave)
    __shared__ uint4 s_tile[STAGE * CPR];
    __shared__ __attribute__((aligned(16))) float s_bias[STAGE];

    const int tid = threadIdx.x, lane = hm::lane_id(), w = hm::wave_id();
    const int h = lane >> 5;
    const int rb = blockIdx.x / P.splits, split = blockIdx.x % P.splits;
    const int q = rb * BQ + w * 32 + (lane & 31);
    const int n_begin = split * P.n_per_split;
    const int n_end = min(P.N, n_begin + P.n_per_split);
    const int KT = P.KT;

    // B fragments: this lane's query, floats 8c + 4h .. 8c + 4h + 3 of every chunk c
    f32x4 b[KC];
#pragma unroll
    for (int c = 0; c < KC; ++c) b[c] = q < P.M ? Q[(size_t)q * CPR + 2 * c + h] : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < KC; ++c) asm volatile("" ::"v"(b[c]));       // retire before the loop

    typedef uint32_t preg_t __attribute__((ext_vector_type(4 * PRE)));
    preg_t pre;
    float pre_b[(STAGE + NT - 1) / NT];

    // sorted (descending) private top-KTC of this lane
    typedef __attribute__((ext_vector_type(KTC))) float lsv_t;   // vectors stay in VGPRs
    typedef __attribute__((ext_vector_type(KTC))) int liv_t;
    lsv_t ls;
    liv_t li;
#pragma unroll
    for (int i = 0; i < KTC; ++i) { ls[i] = -INFINITY; li[i] = INT_MAX; }
    float thr = -INFINITY;
    auto insert = [&](float sv, int nv) {
#pragma unroll
        for (int i = 0; i < KTC; ++i) {
            const bool c = better(sv, nv, ls[i], li[i]);
            const float ts = ls[i];
            const int ti = li[i];
            ls[i] = c ? sv : ts;
            li[i] = c ? nv : ti;
            sv = c ? ts : sv;
            nv = c ? ti : nv;
        }
    };
    auto kth = [&]() {
        float t = ls[0];
#pragma unroll
        for (int i = 1; i < KTC; ++i) t = (i == KT - 1) ? ls[i] : t;
        return t;
    };

    // per-lane queue of candidates not yet in the sorted list
    float qs0 = 0.f, qs1 = 0.f, qs2 = 0.f, qs3 = 0.f;
    int qi0 = 0, qi1 = 0, qi2 = 0, qi3 = 0, qn = 0;
    auto flush_queue = [&]() {
        if (qn > 0) insert(qs0, qi0);
        if (qn > 1) insert(qs1, qi1);
        if (qn > 2) insert(qs2, qi2);
        if (qn > 3) insert(qs3, qi3);
        qn = 0;
        thr = kth();
    };

    if (n_begin < n_end) MIPSF_FETCH(n_begin);
    __syncthreads();
    if (n_begin < n_end) MIPSF_COMMIT();
    __syncthreads();

    for (int s0 = n_begin; s0 < n_end; s0 += STAGE) {
        if (s0 + STAGE < n_end) MIPSF_FETCH(s0 + STAGE);

        for (int t = 0; t < STAGE / 32; ++t) {
            const int n0 = s0 + t * 32;
            if (n0 >= n_end) break;
            f32x16 acc = {};
            const int it = t * 32 + (lane & 31);
#pragma unroll
            for (int c = 0; c < KC; ++c) {
                const uint4 raw = s_tile[swz<CPR>(it, 2 * c + h)];
                f32x4 a;
                __builtin_memcpy(&a, &raw, 16);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b[c].x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b[c].y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b[c].z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b[c].w, acc, 0, 0, 0);
            }
            // lane's items: n0 + (reg & 3) + 8 (reg >> 2) + 4 h
            const int ib = t * 32 + 4 * h;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float4 bb = *reinterpret_cast<const float4*>(&s_bias[ib + 8 * j]);
                acc[4 * j] += bb.x; acc[4 * j + 1] += bb.y; acc[4 * j + 2] += bb.z; acc[4 * j + 3] += bb.w;
            }
            const int nb = n0 + 4 * h;
            if (n0 + 32 > n_end) {                       // tail tile only (uniform branch)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (nb + (r & 3) + 8 * (r >> 2) >= n_end) acc[r] = -INFINITY;
            }
            // fast path: 16 compares against the exact threshold
            bool any = false;
#pragma unroll
            for (int r = 0; r < 16; ++r) any |= acc[r] > thr;
            if (!__builtin_amdgcn_ballot_w64(any)) continue;
            // pending candidates of this lane as a bit mask; one insertion site
            uint32_t pend = 0u;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int n = nb + (r & 3) + 8 * (r >> 2);
                bool c = acc[r] > thr;
                if (EXCL) {
                    if (c && P.use_self && n == q + P.self_offset) c = false;
                    if (c && ex_ptr && q < P.M) c = !is_excluded(ex_ptr, ex_idx, q, n);
                }
                pend |= (uint32_t)c << r;
            }
            // append to the lane's 4-entry queue; the sorted lists are updated only when some
            // lane's queue is full
            while (__builtin_amdgcn_ballot_w64(pend != 0u)) {
                if (pend && qn < 4) {
                    const int r = __builtin_ctz(pend);
                    pend &= pend - 1u;
                    float sv = acc[0];
#pragma unroll
                    for (int k = 1; k < 16; ++k) sv = r == k ? acc[k] : sv;
                    const int nv = nb + (r & 3) + 8 * (r >> 2);
                    qs0 = qn == 0 ? sv : qs0; qi0 = qn == 0 ? nv : qi0;
                    qs1 = qn == 1 ? sv : qs1; qi1 = qn == 1 ? nv : qi1;
                    qs2 = qn == 2 ? sv : qs2; qi2 = qn == 2 ? nv : qi2;
                    qs3 = qn == 3 ? sv : qs3; qi3 = qn == 3 ? nv : qi3;
                    ++qn;
                }
                if (__builtin_amdgcn_ballot_w64(qn == 4 && pend != 0u)) {
                    flush_queue();
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        if (!(acc[r] > thr)) pend &= ~(1u << r);
                }
            }
        }
        __syncthreads();
        if (s0 + STAGE < n_end) MIPSF_COMMIT();
        __syncthreads();
    }

    flush_queue();
    // merge the two half-lists of each query: lanes l + 32 publish theirs through LDS (the
    // stage buffer is free now: 4 waves x 32 queries x KTC entries x 8 B <= 32 KB), lanes l
    // insert them
    float2* s_half = reinterpret_cast<float2*>(s_tile) + (size_t)w * 32 * KTC;
    if (h == 1) {
#pragma unroll
        for (int i = 0; i < KTC; ++i) s_half[(lane & 31) * KTC + i] = make_float2(ls[i], __int_as_float(li[i]));
    }
    __syncthreads();
    if (h == 0) {
        for (int i = 0; i < KT; ++i) {
            const float2 e = s_half[lane * KTC + i];
            insert(e.x, __float_as_int(e.y));
        }
    }
    if (h == 0 && q < P.M) {
        const size_t o = ((size_t)split * P.M + q) * KT;
#pragma unroll
        for (int i = 0; i < KTC; ++i) {
            if (i < KT) {
                const bool ok = ls[i] != -INFINITY || li[i] != INT_MAX;
                out_idx[o + i] = ok ? li[i] : -1;
                out_score[o + i] = ok ? ls[i] : -INFINITY;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// KT 33..64: LDS candidate buffers.  256-thread block = 4 waves, BM = 64 query rows (16 per
// wave), 64-item tiles of four 16x16 sub-tiles on v_mfma_f32_16x16x4_f32 with the queries as A:
// lane l holds score(row 4 (l >> 4) + r, item l & 15) in accumulator r.  KC = Kd / 16 chunks of
// k; lane group g = l >> 4 owns floats 16c + 4g .. 16c + 4g + 3 of chunk c.
template <int KD, bool EXCL>
__global__ __launch_bounds__(NT, KD <= 64 ? 2 : 1) void mips_topk_lds_f32_kernel(
    MipsF32Params P, const f32x4* __restrict__ Q, const f32x4* __restrict__ I,
    const float* __restrict__ item_bias, const int64_t* __restrict__ ex_ptr,
    const int32_t* __restrict__ ex_idx, int32_t* __restrict__ out_idx, float* __restrict__ out_score)
{
    constexpr int CPR = KD / 4;                          // 16-B chunks per row
    constexpr int KC = KD / 16;                          // k chunks of 16 floats
    constexpr int TILES = 64 / KD > 0 ? 64 / KD : 1;     // 16 KB stage, at least one tile
    constexpr int STAGE = BN * TILES;                    // items per stage
    constexpr int PRE = STAGE * CPR / NT;                // 4 chunks per thread (8, 16 at Kd 128, 256)
    __shared__ uint4 s_tile[STAGE * CPR];
    __shared__ float s_bias[STAGE];
    __shared__ float2 s_cand[BM * CAPV];                 // (score, item index bits)

    const int tid = threadIdx.x, lane = hm::lane_id(), w = hm::wave_id();
    const int g = lane >> 4;                             // lane group: rows 4g..4g+3 of the wave
    const int rb = blockIdx.x / P.splits, split = blockIdx.x % P.splits;
    const int q0 = rb * BM;
    const int n_begin = split * P.n_per_split;
    const int n_end = min(P.N, n_begin + P.n_per_split);
    const int KT = P.KT;

    // A fragments: the wave's 16 query rows, held for the whole sweep
    f32x4 a[KC];
    {
        const int q = q0 + w * 16 + (lane & 15);
#pragma unroll
        for (int c = 0; c < KC; ++c) a[c] = q < P.M ? Q[(size_t)q * CPR + 4 * c + g] : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < KC; ++c) asm volatile("" ::"v"(a[c]));   // retire before the loop
    }

    typedef uint32_t preg_t __attribute__((ext_vector_type(4 * PRE)));
    preg_t pre;
    float pre_b[(STAGE + NT - 1) / NT];

    // Per-row state of this lane's 4 rows (uniform over the 16 lanes of the group): running
    // threshold and candidate count.  Kept in registers; no LDS atomics.
    const int rl0 = w * 16 + 4 * g;
    float thr[4];
    int cnt[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { thr[r] = -INFINITY; cnt[r] = 0; }
    const uint64_t grp = 0xFFFFull << (16 * g);

    // Compact row rl (count c, wave-uniform) to its best KT by rank: entry j sits in lane j (and
    // lane j - 64), each lane ranks its own entries against all c of them through v_readlane
    // broadcasts, and the KT best move to their rank.  Returns the new count; *kth receives the
    // KT-th score when c >= KT.
    auto compact = [&](int rl, int c, float* kth) -> int {
        float2* row = s_cand + rl * CAPV;
        const float2 e0 = lane < c ? row[lane] : make_float2(-INFINITY, 0.f);
        const float2 e1 = lane + 64 < c ? row[lane + 64] : make_float2(-INFINITY, 0.f);
        const int i0 = __float_as_int(e0.y), i1 = __float_as_int(e1.y);
        const int s0b = __float_as_int(e0.x), s1b = __float_as_int(e1.x);
        int r0 = 0, r1 = 0;
        const int c0 = c < 64 ? c : 64;
        for (int j = 0; j < c0; ++j) {
            const float oj = __int_as_float(__builtin_amdgcn_readlane(s0b, j));
            const int ij = __builtin_amdgcn_readlane(i0, j);
            r0 += better(oj, ij, e0.x, i0);
            r1 += better(oj, ij, e1.x, i1);
        }
        for (int j = 64; j < c; ++j) {
            const float oj = __int_as_float(__builtin_amdgcn_readlane(s1b, j - 64));
            const int ij = __builtin_amdgcn_readlane(i1, j - 64);
            r0 += better(oj, ij, e0.x, i0);
            r1 += better(oj, ij, e1.x, i1);
        }
        const bool v0 = lane < c, v1 = lane + 64 < c;
        if (v0 && r0 < KT) row[r0] = e0;
        if (v1 && r1 < KT) row[r1] = e1;
        if (c >= KT) {
            const uint64_t m0 = __builtin_amdgcn_ballot_w64(v0 && r0 == KT - 1);
            const uint64_t m1 = __builtin_amdgcn_ballot_w64(v1 && r1 == KT - 1);
            *kth = m0 ? __shfl(e0.x, __builtin_ctzll(m0), 64) : __shfl(e1.x, __builtin_ctzll(m1), 64);
        }
        return c < KT ? c : KT;
    };
    auto wave_sync = [&]() {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };

    if (n_begin < n_end) MIPSF_FETCH(n_begin);
    __syncthreads();
    if (n_begin < n_end) MIPSF_COMMIT();
    __syncthreads();

    for (int s0 = n_begin; s0 < n_end; s0 += STAGE) {
        if (s0 + STAGE < n_end) MIPSF_FETCH(s0 + STAGE);  // in flight during the whole stage

        for (int t = 0; t < TILES; ++t) {
            const int n0 = s0 + t * BN;
            if (n0 >= n_end) break;
            // ---- 64 x 64 score tile on the matrix cores ----
            f32x4 acc[4];
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
                const int n = t * BN + nt * 16 + (lane & 15);
#pragma unroll
                for (int c = 0; c < KC; ++c) {
                    const uint4 raw = s_tile[swz<CPR>(n, 4 * c + g)];
                    f32x4 bv;
                    __builtin_memcpy(&bv, &raw, 16);
                    acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[c].x, bv.x, acc[nt], 0, 0, 0);
                    acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[c].y, bv.y, acc[nt], 0, 0, 0);
                    acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[c].z, bv.z, acc[nt], 0, 0, 0);
                    acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[c].w, bv.w, acc[nt], 0, 0, 0);
                }
            }
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const float bn = s_bias[t * BN + nt * 16 + (lane & 15)];
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[nt][r] += bn;
            }

            // ---- filter against the running thresholds, two 32-item halves ----
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                bool any = false;
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int n = n0 + (2 * h + u) * 16 + (lane & 15);
#pragma unroll
                    for (int r = 0; r < 4; ++r) any |= (n < n_end) & (acc[2 * h + u][r] > thr[r]);
                }
                if (!__builtin_amdgcn_ballot_w64(any)) continue;
                // candidate ballots of this half: m[r][u] (per row r of the lane group, 16-item
                // sub-tile u) and the number each row would append
                uint64_t m[4][2];
                int add[4];
#define MIPSF_BALLOTS()                                                                        \
                _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                \
                    const int q = q0 + rl0 + r;                                                \
                    add[r] = 0;                                                                \
                    _Pragma("unroll") for (int u = 0; u < 2; ++u) {                            \
                        const int n = n0 + (2 * h + u) * 16 + (lane & 15);                     \
                        bool c = (n < n_end) & (acc[2 * h + u][r] > thr[r]) & (q < P.M);       \
                        if (EXCL) {                                                            \
                            if (c && P.use_self && n == q + P.self_offset) c = false;          \
                            if (c && ex_ptr) c = !is_excluded(ex_ptr, ex_idx, q, n);           \
                        }                                                                      \
                        m[r][u] = __builtin_amdgcn_ballot_w64(c);                              \
                        add[r] += __popcll(m[r][u] & grp);                                     \
                    }                                                                          \
                }
                MIPSF_BALLOTS();
                // a row whose buffer would overflow is compacted first, or, eagerly, once 16
                // entries beyond KT have accumulated (a tight threshold keeps later halves on
                // the fast path)
                bool need = false;
#pragma unroll
                for (int r = 0; r < 4; ++r) need |= (cnt[r] + add[r] > CAPV) | (cnt[r] + add[r] >= KT + 16);
                if (__builtin_amdgcn_ballot_w64(need)) {
                    wave_sync();
                    // one (not unrolled) pass over the wave's 16 rows: a single copy of the
                    // compaction code in the loop
                    for (int rr = 0; rr < 16; ++rr) {
                        const int gg = rr >> 2, r = rr & 3;
                        const int cr = r == 0 ? cnt[0] : r == 1 ? cnt[1] : r == 2 ? cnt[2] : cnt[3];
                        const int ar = r == 0 ? add[0] : r == 1 ? add[1] : r == 2 ? add[2] : add[3];
                        const int c = __shfl(cr, 16 * gg, 64);
                        const int ca = c + __shfl(ar, 16 * gg, 64);
                        if (ca > CAPV || ca >= KT + 16) {
                            float kth = -INFINITY;
                            const int nc = compact(w * 16 + rr, c, &kth);
                            if (g == gg) {
#pragma unroll
                                for (int k = 0; k < 4; ++k) {
                                    if (k == r) {
                                        cnt[k] = nc;
                                        if (c >= KT) thr[k] = kth;
                                    }
                                }
                            }
                        }
                    }
                    wave_sync();
                    MIPSF_BALLOTS();    // thresholds moved
                }
#undef MIPSF_BALLOTS
                // append: slot = count + prefix of the group's ballot (no atomics)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    int base = cnt[r];
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        const uint64_t mu = m[r][u];
                        if ((mu >> lane) & 1ull) {
                            const uint64_t mg = mu & grp;
                            const int pos = base + (int)__builtin_amdgcn_mbcnt_hi(
                                (uint32_t)(mg >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mg, 0u));
                            s_cand[(rl0 + r) * CAPV + pos] =
                                make_float2(acc[2 * h + u][r], __int_as_float(n0 + (2 * h + u) * 16 + (lane & 15)));
                        }
                        base += __popcll(mu & grp);
                    }
                    cnt[r] = base;
                }
            }
        }
        __syncthreads();                                 // every wave is done with the stage
        if (s0 + STAGE < n_end) MIPSF_COMMIT();
        __syncthreads();                                 // next stage visible
    }

    // ---- final: best KT of every row of this wave, in order ----
    wave_sync();
    for (int rr = 0; rr < 16; ++rr) {
        const int gg = rr >> 2, r = rr & 3;
        const int rl = w * 16 + rr;
        const int q = q0 + rl;
        const int cr = r == 0 ? cnt[0] : r == 1 ? cnt[1] : r == 2 ? cnt[2] : cnt[3];
        const int c = __shfl(cr, 16 * gg, 64);
        if (q < P.M) {
            float kth;
            const int nc = compact(rl, c, &kth);
            wave_sync();
            if (lane < KT) {
                const size_t o = ((size_t)split * P.M + q) * KT + lane;
                const float2 e = s_cand[rl * CAPV + lane];
                const bool ok = lane < nc;
                out_idx[o] = ok ? __float_as_int(e.y) : -1;
                out_score[o] = ok ? e.x : -INFINITY;
            }
        }
    }
}

#undef MIPSF_FETCH
#undef MIPSF_COMMIT

template <int KD>
int launch_f32(const MipsF32Params& P, const void* Q, const void* I, const float* bias,
               const int64_t* ex_ptr, const int32_t* ex_idx, int32_t* oi, float* os, hipStream_t st) {
    const auto* q = reinterpret_cast<const f32x4*>(Q);
    const auto* it = reinterpret_cast<const f32x4*>(I);
    const bool ex = P.use_self || ex_ptr;
    if (P.KT <= 32) {
        const int blocks = ((P.M + 127) / 128) * P.splits;
#define MIPSF_GO(KTC, EX) hipLaunchKernelGGL((mips_topk_reg_f32_kernel<KD, KTC, EX>), dim3(blocks), dim3(NT), 0, st, \
                                            P, q, it, bias, ex_ptr, ex_idx, oi, os)
        if (P.KT <= 8) { if (ex) MIPSF_GO(8, true); else MIPSF_GO(8, false); }
        else if (P.KT <= 16) { if (ex) MIPSF_GO(16, true); else MIPSF_GO(16, false); }
        else { if (ex) MIPSF_GO(32, true); else MIPSF_GO(32, false); }
#undef MIPSF_GO
    } else {
        const int blocks = ((P.M + BM - 1) / BM) * P.splits;
        if (ex) hipLaunchKernelGGL((mips_topk_lds_f32_kernel<KD, true>), dim3(blocks), dim3(NT), 0, st,
                                   P, q, it, bias, ex_ptr, ex_idx, oi, os);
        else hipLaunchKernelGGL((mips_topk_lds_f32_kernel<KD, false>), dim3(blocks), dim3(NT), 0, st,
                                P, q, it, bias, ex_ptr, ex_idx, oi, os);
    }
    HM_LAUNCH_RET();
}

}  // namespace

// Q [M][Kd] fp32, I [N][Kd] fp32 (Kd = 16, 32, 64, 128 or 256; zero-padded by the caller, rows
// 16-B aligned), item_bias [N] fp32 or null, exclusion CSR (ex_ptr [M+1] int64, ex_idx sorted per
// row) or null, self_offset: exclude item q + self_offset for query q (use_self = 1).
// Output [splits][M][KT] (idx int32, -1 = none; score fp32, -inf = none), best first.
HM_API int hm_mips_topk_f32(int M, int N, int Kd, int KT, int splits, int use_self, int self_offset,
                            const void* Q, const void* I, const float* item_bias,
                            const int64_t* ex_ptr, const int32_t* ex_idx,
                            int32_t* out_idx, float* out_score, hipStream_t stream) {
    if (M <= 0 || N <= 0 || KT <= 0 || KT > KT_MAX || splits <= 0) return (int)hipErrorInvalidValue;
    MipsF32Params P;
    P.M = M; P.N = N; P.KT = KT; P.splits = splits;
    P.n_per_split = ((N + splits - 1) / splits + BN - 1) / BN * BN;
    P.use_self = use_self; P.self_offset = self_offset;
    switch (Kd) {
        case 16: return launch_f32<16>(P, Q, I, item_bias, ex_ptr, ex_idx, out_idx, out_score, stream);
        case 32: return launch_f32<32>(P, Q, I, item_bias, ex_ptr, ex_idx, out_idx, out_score, stream);
        case 64: return launch_f32<64>(P, Q, I, item_bias, ex_ptr, ex_idx, out_idx, out_score, stream);
        case 128: return launch_f32<128>(P, Q, I, item_bias, ex_ptr, ex_idx, out_idx, out_score, stream);
        case 256: return launch_f32<256>(P, Q, I, item_bias, ex_ptr, ex_idx, out_idx, out_score, stream);
        default: return (int)hipErrorInvalidValue;
    }
}
