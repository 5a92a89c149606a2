// Fused top-k maximum-inner-product search for wide lists, KT = 65..256 (top-100 recommendation,
// candidate generation for a re-ranker), bf16 and fp32 operands.
//
//   out[q] = top-KT over items n of  s(q, n) = <Q[q], I[n]> + item_bias[n]
//
// The contract of topk_mips.hip / topk_mips_f32.hip (hm_mips_topk, hm_mips_topk_f32) in every
// respect but the list length: higher score first, equal scores by lower item index, exclusion
// CSR and self offset, splits that start at multiples of 64 items, output [splits][M][KT] with
// -1 / -inf for "none", padded Kd 32/64/128/256 (bf16) and 16/32/64/128/256 (fp32).  Those two
// files stay as they are; ops/topk_mips.py sends k <= 64 to them and k above 64 here.
//
// Score tiles.  The MFMA tiles of the siblings' LDS-candidate kernels: a wave owns 16 query rows
// whose fragments stay in VGPRs for the whole sweep, items are staged in LDS in XOR-swizzled 16-B
// chunks, and lane l holds score(row 4 (l >> 4) + r, item l & 15) of a 16 x 16 sub-tile in
// accumulator r (v_mfma_f32_16x16x32_bf16, or four v_mfma_f32_16x16x4_f32 per 16-B read with k
// relabelled as in topk_mips_f32.hip).  The two operand types are "tile producers" (TileBf16,
// TileF32: fragment load + one sub-tile of scores); everything below them is one template.
//
// Stage.  Always 16 KB (1024 chunks): 16384 / row bytes items, 256 at Kd 32 bf16 down to 16 at
// Kd 256 fp32, so the LDS budget below does not depend on Kd.  The next stage is prefetched into
// registers while the current one is scored (4 chunks a thread with 256 threads, 8 with 128), and
// the tile loop of the no-exclusion variant holds no global load (see topk_mips.hip's header).
//
// Selection (new here).  Every row has a buffer of CAP = 2 KTC 64-bit keys in LDS,
//     key = order-preserving score bits << 32 | ~item index,
// so that "better" (higher score, then lower index) is simply "larger key" and the tie rule needs
// no code of its own; key 0 is below every real key (scores are finite or +inf) and stands for
// an empty slot.  Per 16-item sub-tile a lane group compares its 4 rows against the rows' running
// thresholds (registers); a sub-tile with no candidate costs 4 compares and a ballot.  Candidates
// are appended at count + prefix of the group's ballot: counts and thresholds live in registers,
// there are no LDS atomics.  The threshold of a row is exact, the KT-th best key's score at the
// last compaction; items arrive in index order, so an equal score later in the sweep has a
// higher index and `score > threshold` is the whole admission test.
//   A row is compacted only when an append would overflow CAP.  (Compacting eagerly at KT + 64
// keys, as the siblings do at KT + 16, kept thresholds fresher but sorted 2.4 to 4 times as
// often: ML-20M all users, dim 64, 42 / 49 ms bf16 / fp32 at KT = 100 and 182 / 202 ms at 256,
// against 25 / 30 ms and 70 / 78 ms with the capacity trigger.)  Compaction is a bitonic sort of
// the row in LDS, descending, over the smallest power of two n >= count (the slots from count to
// n are cleared first): log2(n) (log2(n) + 1) / 2 compare-exchange steps of n / 2 pairs spread
// over the wave's 64 lanes, i.e. 36 steps of 2 pairs a lane at n = 256 against the 256 x 4
// readlane rounds the rank-by-broadcast scheme of the siblings would need.  The first KT slots
// are then the new list, in output order, and slot KT - 1 is the new threshold.  The same sort
// finishes every row before the store.
//
// LDS budget (160 KB a CU), query rows a block, occupancy:
//   tier    KT        CAP   BM   threads   candidates   stage + bias   total      blocks / CU
//   KTC128  65..128   256   64   256       128 KB       16 KB + 1 KB   145 KB     1 (4 waves)
//   KTC256  129..256  512   32   128       128 KB       16 KB + 1 KB   145 KB     1 (2 waves)
// A key is 8 bytes and a row needs KT plus a tile of appends, so 64 rows of the wide tier do not
// fit one CU and it runs 32 rows (two waves) a block.  One wave per SIMD means 512 registers a
// lane; the resource report (hipcc -Rpass-analysis=kernel-resource-usage, docs/perf_notes.md
// has the table) shows 83 to 188 VGPRs (Kd 32 bf16 narrow tier to Kd 256 fp32 wide tier), 4
// AGPRs, occupancy 1 and no scratch for any of the 36 instantiations.
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

constexpr int BN = 64;          // splits start at multiples of this many items
constexpr int KT_MAX = 256;
constexpr int STAGE_CHUNKS = 1024;   // 16 KB of 16-B chunks

struct MipsWideParams {
    int M, N, KT, splits, n_per_split;
    int self_offset;        // exclude n == q + self_offset when use_self
    int use_self;
};

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

// (score, item) -> key: larger key = better entry.  -0.0 is folded into +0.0 first, so that equal
// scores have equal score bits.
__device__ __forceinline__ uint64_t make_key(float s, int n) {
    const uint32_t u = __float_as_uint(s == 0.f ? 0.f : s);
    const uint32_t m = u ^ ((uint32_t)((int32_t)u >> 31) | 0x80000000u);
    return ((uint64_t)m << 32) | (uint32_t)~n;
}
__device__ __forceinline__ float key_score(uint64_t k) {
    const uint32_t m = (uint32_t)(k >> 32);
    return __uint_as_float(m ^ ((m & 0x80000000u) ? 0x80000000u : 0xFFFFFFFFu));
}
__device__ __forceinline__ int key_item(uint64_t k) { return (int)~(uint32_t)k; }

// ---- tile producers: query fragments of a wave's 16 rows, and the scores of one 16-item
// sub-tile (lane: row 4 g + r in accumulator r, item n_local & 15 == lane & 15) ----
template <int KD>
struct TileBf16 {
    static constexpr int CPR = KD / 8;                   // 16-B chunks per row
    static constexpr int KS = KD / 32;
    struct Frag { bf16x8 a[KS]; };
    static __device__ __forceinline__ void load(Frag& f, const uint4* __restrict__ Q, int q, int M, int g) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const uint4 raw = q < M ? Q[(size_t)q * CPR + ks * 4 + g] : make_uint4(0u, 0u, 0u, 0u);
            __builtin_memcpy(&f.a[ks], &raw, 16);
        }
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) asm volatile("" ::"v"(f.a[ks]));   // retire before the loop
    }
    static __device__ __forceinline__ f32x4 scores(const uint4* s_tile, int n, int g, const Frag& f) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const uint4 raw = s_tile[swz<CPR>(n, ks * 4 + g)];
            bf16x8 b;
            __builtin_memcpy(&b, &raw, 16);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f.a[ks], b, acc, 0, 0, 0);
        }
        return acc;
    }
};

template <int KD>
struct TileF32 {
    static constexpr int CPR = KD / 4;
    static constexpr int KC = KD / 16;                   // k chunks of 16 floats; group g owns 4g..4g+3
    struct Frag { f32x4 a[KC]; };
    static __device__ __forceinline__ void load(Frag& f, const uint4* __restrict__ Q, int q, int M, int g) {
#pragma unroll
        for (int c = 0; c < KC; ++c) {
            const uint4 raw = q < M ? Q[(size_t)q * CPR + 4 * c + g] : make_uint4(0u, 0u, 0u, 0u);
            __builtin_memcpy(&f.a[c], &raw, 16);
        }
#pragma unroll
        for (int c = 0; c < KC; ++c) asm volatile("" ::"v"(f.a[c]));       // retire before the loop
    }
    static __device__ __forceinline__ f32x4 scores(const uint4* s_tile, int n, int g, const Frag& f) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < KC; ++c) {
            const uint4 raw = s_tile[swz<CPR>(n, 4 * c + g)];
            f32x4 b;
            __builtin_memcpy(&b, &raw, 16);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(f.a[c].x, b.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(f.a[c].y, b.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(f.a[c].z, b.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(f.a[c].w, b.w, acc, 0, 0, 0);
        }
        return acc;
    }
};

// ---------------------------------------------------------------------------------------------
// T: tile producer.  KTC: list capacity tier (128 or 256).
template <class T, int KTC, bool EXCL>
__global__ __launch_bounds__(KTC <= 128 ? 256 : 128, 1) void mips_topk_wide_kernel(
    MipsWideParams P, const uint4* __restrict__ Q, const uint4* __restrict__ I,
    const float* __restrict__ item_bias, const int64_t* __restrict__ ex_ptr,
    const int32_t* __restrict__ ex_idx, int32_t* __restrict__ out_idx, float* __restrict__ out_score)
{
    constexpr int CAP = 2 * KTC;                         // key slots per row, a power of two
    constexpr int BM = KTC <= 128 ? 64 : 32;             // query rows per block, 16 per wave
    constexpr int NT = BM * 4;                           // threads per block
    constexpr int CPR = T::CPR;
    constexpr int STAGE = STAGE_CHUNKS / CPR;            // items per stage, a multiple of 16
    constexpr int PRE = STAGE_CHUNKS / NT;               // 16-B chunks per thread per stage
    constexpr int PRB = (STAGE + NT - 1) / NT;
    static_assert(KTC + BN <= CAP, "a compacted row must take a tile of appends");
    __shared__ uint4 s_tile[STAGE_CHUNKS];
    __shared__ float s_bias[STAGE];
    __shared__ uint64_t s_cand[BM * CAP];

    const int tid = threadIdx.x, lane = hm::lane_id(), w = hm::wave_id();
    const int g = lane >> 4;                             // lane group: rows 4g..4g+3 of the wave
    const int rb = blockIdx.x / P.splits, split = blockIdx.x % P.splits;
    const int q0 = rb * BM;
    const int n_begin = split * P.n_per_split;
    const int n_end = min(P.N, n_begin + P.n_per_split);
    const int KT = P.KT;

    typename T::Frag frag;
    T::load(frag, Q, q0 + w * 16 + (lane & 15), P.M, g);

    // register prefetch of one stage; rows past n_end are clamped to the last item: in bounds,
    // and masked by the filters
    typedef uint32_t preg_t __attribute__((ext_vector_type(4 * PRE)));
    preg_t pre;
    float pre_b[PRB];
#define MIPSW_FETCH(N0)                                                                        \
    do {                                                                                       \
        _Pragma("unroll") for (int r = 0; r < PRE; ++r) {                                      \
            const int e = tid + NT * r;                                                        \
            const int n = min((N0) + e / CPR, n_end - 1);                                      \
            const uint4 v_ = I[(size_t)n * CPR + (e % CPR)];                                   \
            pre[4 * r] = v_.x; pre[4 * r + 1] = v_.y; pre[4 * r + 2] = v_.z; pre[4 * r + 3] = v_.w; \
        }                                                                                      \
        _Pragma("unroll") for (int r = 0; r < PRB; ++r)                                        \
            pre_b[r] = item_bias ? item_bias[min((N0) + tid + NT * r, n_end - 1)] : 0.f;       \
    } while (0)
#define MIPSW_COMMIT()                                                                         \
    do {                                                                                       \
        _Pragma("unroll") for (int r = 0; r < PRE; ++r) {                                      \
            const int e = tid + NT * r;                                                        \
            s_tile[swz<CPR>(e / CPR, e % CPR)] =                                               \
                make_uint4(pre[4 * r], pre[4 * r + 1], pre[4 * r + 2], pre[4 * r + 3]);         \
        }                                                                                      \
        _Pragma("unroll") for (int r = 0; r < PRB; ++r)                                        \
            if (tid + NT * r < STAGE) s_bias[tid + NT * r] = pre_b[r];                         \
    } while (0)

    // Per-row state of this lane's 4 rows (uniform over the 16 lanes of the group): running
    // threshold and key count.  Kept in registers; no LDS atomics.
    const int rl0 = w * 16 + 4 * g;
    float thr[4];
    int cnt[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {                        // rows past M admit nothing
        thr[r] = q0 + rl0 + r < P.M ? -INFINITY : INFINITY;
        cnt[r] = 0;
    }
    const uint64_t grp = 0xFFFFull << (16 * g);

    auto wave_sync = [&]() {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };
    // Bitonic sort, descending, of the first c (wave-uniform, <= CAP) keys of a row: n is the
    // smallest power of two >= max(c, 64), slots c..n-1 are cleared (key 0 sorts last).  Step
    // (k, j) compare-exchanges slot i with slot i + j for the n / 2 values of i whose bit j is
    // clear; blocks of k slots alternate between descending and ascending.
    auto sort_row = [&](uint64_t* row, int c) {
        int n = 64;
        while (n < c) n <<= 1;
        for (int i = c + lane; i < n; i += 64) row[i] = 0ull;
        wave_sync();
        for (int k = 2; k <= n; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = lane; t < (n >> 1); t += 64) {
                    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                    const uint64_t x = row[i], y = row[i + j];
                    if ((x < y) == ((i & k) == 0)) { row[i] = y; row[i + j] = x; }
                }
                wave_sync();
            }
        }
    };

    if (n_begin < n_end) MIPSW_FETCH(n_begin);
    __syncthreads();
    if (n_begin < n_end) MIPSW_COMMIT();
    __syncthreads();

    for (int s0 = n_begin; s0 < n_end; s0 += STAGE) {
        if (s0 + STAGE < n_end) MIPSW_FETCH(s0 + STAGE);  // in flight during the whole stage

        for (int t = 0; t < STAGE / 16; ++t) {
            const int n0 = s0 + t * 16;
            if (n0 >= n_end) break;
            // ---- 16 rows x 16 items of scores on the matrix cores ----
            f32x4 acc = T::scores(s_tile, t * 16 + (lane & 15), g, frag);
            const float bn = s_bias[t * 16 + (lane & 15)];
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] += bn;

            // ---- filter against the running thresholds ----
            const int n = n0 + (lane & 15);
            bool any = false;
#pragma unroll
            for (int r = 0; r < 4; ++r) any |= acc[r] > thr[r];
            if (!__builtin_amdgcn_ballot_w64(any & (n < n_end))) continue;
            // candidate ballots m[r] (per row r of the lane group) and the number each row
            // would append
            uint64_t m[4];
            int add[4];
#define MIPSW_BALLOTS()                                                                        \
            _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                    \
                const int q = q0 + rl0 + r;                                                    \
                bool c = (n < n_end) & (acc[r] > thr[r]) & (q < P.M);                          \
                if (EXCL) {                                                                    \
                    if (c && P.use_self && n == q + P.self_offset) c = false;                  \
                    if (c && ex_ptr) c = !is_excluded(ex_ptr, ex_idx, q, n);                   \
                }                                                                              \
                m[r] = __builtin_amdgcn_ballot_w64(c);                                         \
                add[r] = __popcll(m[r] & grp);                                                 \
            }
            MIPSW_BALLOTS();
            bool need = false;
#pragma unroll
            for (int r = 0; r < 4; ++r) need |= cnt[r] + add[r] > CAP;
            if (__builtin_amdgcn_ballot_w64(need)) {
                wave_sync();
                // one (not unrolled) pass over the wave's 16 rows: a single copy of the sort
                for (int rr = 0; rr < 16; ++rr) {
                    const int gg = rr >> 2, r = rr & 3;
                    const int cr = r == 0 ? cnt[0] : r == 1 ? cnt[1] : r == 2 ? cnt[2] : cnt[3];
                    const int ar = r == 0 ? add[0] : r == 1 ? add[1] : r == 2 ? add[2] : add[3];
                    const int c = __shfl(cr, 16 * gg, 64);
                    const int ca = c + __shfl(ar, 16 * gg, 64);
                    if (ca > CAP) {
                        uint64_t* row = s_cand + (w * 16 + rr) * CAP;
                        sort_row(row, c);
                        const float kth = c >= KT ? key_score(row[KT - 1]) : -INFINITY;
                        if (g == gg) {
#pragma unroll
                            for (int k = 0; k < 4; ++k) {
                                if (k == r) {
                                    cnt[k] = c < KT ? c : KT;
                                    thr[k] = kth;
                                }
                            }
                        }
                    }
                }
                wave_sync();
                MIPSW_BALLOTS();        // thresholds moved
            }
#undef MIPSW_BALLOTS
            // append: slot = count + prefix of the group's ballot (no atomics); count + add <= CAP
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const uint64_t mg = m[r] & grp;
                if ((mg >> lane) & 1ull) {
                    const int pos = cnt[r] + (int)__builtin_amdgcn_mbcnt_hi(
                        (uint32_t)(mg >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mg, 0u));
                    s_cand[(rl0 + r) * CAP + pos] = make_key(acc[r], n);
                }
                cnt[r] += __popcll(mg);
            }
        }
        __syncthreads();                                 // every wave is done with the stage
        if (s0 + STAGE < n_end) MIPSW_COMMIT();
        __syncthreads();                                 // next stage visible
    }
#undef MIPSW_FETCH
#undef MIPSW_COMMIT

    // ---- final: best KT of every row of this wave, in order ----
    wave_sync();
    for (int rr = 0; rr < 16; ++rr) {
        const int gg = rr >> 2, r = rr & 3;
        const int rl = w * 16 + rr;
        const int q = q0 + rl;
        const int cr = r == 0 ? cnt[0] : r == 1 ? cnt[1] : r == 2 ? cnt[2] : cnt[3];
        const int c = __shfl(cr, 16 * gg, 64);
        if (q < P.M) {
            uint64_t* row = s_cand + rl * CAP;
            sort_row(row, c);
            const int nc = c < KT ? c : KT;
            const size_t o = ((size_t)split * P.M + q) * KT;
            for (int i = lane; i < KT; i += 64) {
                const bool ok = i < nc;
                const uint64_t key = ok ? row[i] : 0ull;
                out_idx[o + i] = ok ? key_item(key) : -1;
                out_score[o + i] = ok ? key_score(key) : -INFINITY;
            }
        }
    }
}

template <class T>
int launch_wide(const MipsWideParams& P, const void* Q, const void* I, const float* bias,
                const int64_t* ex_ptr, const int32_t* ex_idx, int32_t* oi, float* os, hipStream_t st) {
    const auto* q = reinterpret_cast<const uint4*>(Q);
    const auto* it = reinterpret_cast<const uint4*>(I);
    const bool ex = P.use_self || ex_ptr;
#define MIPSW_GO(KTC, EX)                                                                      \
    hipLaunchKernelGGL((mips_topk_wide_kernel<T, KTC, EX>),                                    \
                       dim3(((P.M + (KTC <= 128 ? 64 : 32) - 1) / (KTC <= 128 ? 64 : 32)) * P.splits), \
                       dim3(KTC <= 128 ? 256 : 128), 0, st, P, q, it, bias, ex_ptr, ex_idx, oi, os)
    if (P.KT <= 128) { if (ex) MIPSW_GO(128, true); else MIPSW_GO(128, false); }
    else { if (ex) MIPSW_GO(256, true); else MIPSW_GO(256, false); }
#undef MIPSW_GO
    HM_LAUNCH_RET();
}

bool wide_params(MipsWideParams& P, int M, int N, int KT, int splits, int use_self, int self_offset) {
    if (M <= 0 || N <= 0 || KT <= 0 || KT > KT_MAX || splits <= 0) return false;
    P.M = M; P.N = N; P.KT = KT; P.splits = splits;
    P.n_per_split = ((N + splits - 1) / splits + BN - 1) / BN * BN;
    P.use_self = use_self; P.self_offset = self_offset;
    return true;
}

}  // namespace

// The argument list and output layout of hm_mips_topk (topk_mips.hip): Q [M][Kd] bf16, I [N][Kd]
// bf16 (Kd = 32, 64, 128 or 256; zero-padded by the caller), item_bias [N] fp32 or null, exclusion
// CSR or null, self_offset.  KT up to 256; the launch layer uses it above 64.
HM_API int hm_mips_topk_wide(int M, int N, int Kd, int KT, int splits, int use_self, int self_offset,
                             const void* Q, const void* I, const float* item_bias,
                             const int64_t* ex_ptr, const int32_t* ex_idx,
                             int32_t* out_idx, float* out_score, hipStream_t stream) {
    MipsWideParams P;
    if (!wide_params(P, M, N, KT, splits, use_self, self_offset)) return (int)hipErrorInvalidValue;
    switch (Kd) {
        case 32: return launch_wide<TileBf16<32>>(P, Q, I, item_bias, ex_ptr, ex_idx, out_idx, out_score, stream);
        case 64: return launch_wide<TileBf16<64>>(P, Q, I, item_bias, ex_ptr, ex_idx, out_idx, out_score, stream);
        case 128: return launch_wide<TileBf16<128>>(P, Q, I, item_bias, ex_ptr, ex_idx, out_idx, out_score, stream);
        case 256: return launch_wide<TileBf16<256>>(P, Q, I, item_bias, ex_ptr, ex_idx, out_idx, out_score, stream);
        default: return (int)hipErrorInvalidValue;
    }
}

// The same with fp32 operands (hm_mips_topk_f32's arguments): Kd = 16, 32, 64, 128 or 256, rows
// 16-B aligned.
HM_API int hm_mips_topk_wide_f32(int M, int N, int Kd, int KT, int splits, int use_self, int self_offset,
                                 const void* Q, const void* I, const float* item_bias,
                                 const int64_t* ex_ptr, const int32_t* ex_idx,
                                 int32_t* out_idx, float* out_score, hipStream_t stream) {
    MipsWideParams P;
    if (!wide_params(P, M, N, KT, splits, use_self, self_offset)) return (int)hipErrorInvalidValue;
    switch (Kd) {
        case 16: return launch_wide<TileF32<16>>(P, Q, I, item_bias, ex_ptr, ex_idx, out_idx, out_score, stream);
        case 32: return launch_wide<TileF32<32>>(P, Q, I, item_bias, ex_ptr, ex_idx, out_idx, out_score, stream);
        case 64: return launch_wide<TileF32<64>>(P, Q, I, item_bias, ex_ptr, ex_idx, out_idx, out_score, stream);
        case 128: return launch_wide<TileF32<128>>(P, Q, I, item_bias, ex_ptr, ex_idx, out_idx, out_score, stream);
        case 256: return launch_wide<TileF32<256>>(P, Q, I, item_bias, ex_ptr, ex_idx, out_idx, out_score, stream);
        default: return (int)hipErrorInvalidValue;
    }
}
