// Grouped ROC AUC on gfx950: the engine behind evaluation.auc_batch and the (score, label) form of
// SQL's auc(...) [GROUP BY ...]  (ops/auc.py; docs/compat.md "AUC engine").
//
// Per group the kernels count, in integers,
//     2U = sum over positives p and negatives n of 2 * [p > n] + [p == n]
// and the two class sizes; AUC = (2U / 2) / (n_pos * n_neg) is one fp64 division of exact values on
// the caller's side, equal to metrics.auc's rank-sum formula bit for bit below 2^26 rows a group.
// No floating-point sum exists here, so no order of additions does either.
//
//   auc_prepare   one pass over the rows in group order (gathered through `order`): the monotone
//                 int64 key and the class of every row (auc_key.h).
//   auc_small     groups of up to 64 rows: 8, 16, 32 or 64 lanes a group, so a wave serves up to
//                 eight.  A lane holds one row; the rows are broadcast lane by lane inside the
//                 sub-wave and every positive lane counts against the negative ones.  Class sizes
//                 from ballots, 2U from a sub-wave butterfly.  No LDS, no atomics.
//   auc_medium    groups of up to 2048 rows, one 256-thread workgroup each.  Both classes are
//                 compacted into one 16 KB LDS buffer (negatives from the front, positives from
//                 the back; wave ballots give the places).  The threads take the larger class in
//                 strides and walk the smaller one: every lane reads the same LDS address, a
//                 broadcast without bank conflicts.
//   auc_long_*    longer groups, on keys the caller has sorted inside every group (torch.sort):
//                 negatives per tile of 2048, then (after the caller's cumsum of the tile counts)
//                 an in-tile scan that writes the exclusive negative prefix negpre[NL + 1], then
//                 per positive a lower- and an upper-bound search inside its group's segment:
//                 2 * (negpre[lb] - negpre[seg0]) + (negpre[ub] - negpre[lb]).  Tie runs and groups
//                 cross tiles freely; the searches never look at a tile.  Sums leave as integer
//                 atomics, one a wave where the wave lies in one group.
//
// Every group has one writer (small, medium) or starts from the caller's zeros (long).  The C++
// twin is csrc/host/auc_cpu.cpp.
#include "auc_key.h"
#include "common.h"

namespace {

constexpr int AUC_THREADS = 256;
constexpr int AUC_WAVES = AUC_THREADS / HM_WAVE;
constexpr int AUC_MEDIUM_MAX = 2048;
constexpr int AUC_TILE = 2048;
constexpr int AUC_PER_THREAD = AUC_TILE / AUC_THREADS;

__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, HM_WAVE);
    return v;
}

__device__ __forceinline__ void add_i64(int64_t* at, long long v) {
    atomicAdd((unsigned long long*)at, (unsigned long long)v);
}

__global__ __launch_bounds__(AUC_THREADS) void auc_prepare_kernel(
    const void* __restrict__ scores, int score_kind, const void* __restrict__ labels, int label_kind,
    int64_t n, const int64_t* __restrict__ order, int64_t N, int64_t* __restrict__ keys,
    uint8_t* __restrict__ cls) {
    const int64_t p = (int64_t)blockIdx.x * AUC_THREADS + threadIdx.x;
    if (p >= N) return;
    int64_t key;
    const int c = auc_row(scores, score_kind, labels, label_kind, n, order ? order[p] : p, &key);
    keys[p] = key;
    cls[p] = (uint8_t)c;
}

// Row jj of the lane's group, to every lane of the group.
template <int LPR>
__device__ __forceinline__ int64_t group_bcast(int64_t key, int jj) {
    if constexpr (LPR == HM_WAVE) {                // one group a wave: a scalar lane read
        const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)key, jj);
        const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(key >> 32), jj);
        return (int64_t)(((unsigned long long)hi << 32) | lo);
    } else {
        return __shfl((long long)key, jj, LPR);
    }
}

template <int LPR>
__global__ __launch_bounds__(AUC_THREADS) void auc_small_kernel(
    const int64_t* __restrict__ keys, const uint8_t* __restrict__ cls, const int64_t* __restrict__ rowptr,
    const int64_t* __restrict__ ids, int64_t count, int64_t* __restrict__ two_u,
    int64_t* __restrict__ n_pos, int64_t* __restrict__ n_neg) {
    constexpr int GPW = HM_WAVE / LPR;             // groups per wave
    const int lane = hm::lane_id();
    const int sub = lane / LPR, j = lane % LPR;
    const int64_t slot = ((int64_t)blockIdx.x * AUC_WAVES + hm::wave_id()) * GPW + sub;
    const bool live = slot < count;                // a tail wave holds fewer groups than slots
    int64_t g = 0, r0 = 0;
    int m = 0;
    if (live) {
        g = ids[slot];
        r0 = rowptr[g];
        m = (int)min(rowptr[g + 1] - r0, (int64_t)LPR);
    }
    int64_t key = 0;
    int c = AUC_ABSENT;
    if (j < m) {
        key = keys[r0 + j];
        c = cls[r0 + j];
    }
    unsigned long long negm = __ballot(c == AUC_NEG), posm = __ballot(c == AUC_POS);
    if constexpr (LPR < HM_WAVE) {                 // the group's lanes only
        negm = (negm >> (sub * LPR)) & ((1ull << LPR) - 1ull);
        posm = (posm >> (sub * LPR)) & ((1ull << LPR) - 1ull);
    }
    int acc = 0;                                   // at most 2 * 64 * 64
#pragma unroll
    for (int jj = 0; jj < LPR; ++jj) {
        const int64_t kj = group_bcast<LPR>(key, jj);
        if ((negm >> jj) & 1ull) acc += 2 * (int)(key > kj) + (int)(key == kj);
    }
    if (c != AUC_POS) acc = 0;
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o, HM_WAVE);
    if (live && j == 0) {
        two_u[g] = acc;
        n_pos[g] = __popcll(posm);
        n_neg[g] = __popcll(negm);
    }
}

__global__ __launch_bounds__(AUC_THREADS) void auc_medium_kernel(
    const int64_t* __restrict__ keys, const uint8_t* __restrict__ cls, const int64_t* __restrict__ rowptr,
    const int64_t* __restrict__ ids, int64_t* __restrict__ two_u, int64_t* __restrict__ n_pos,
    int64_t* __restrict__ n_neg) {
    __shared__ int64_t buf[AUC_MEDIUM_MAX];        // negatives from [0] up, positives from [MAX - 1] down
    __shared__ int cnt[2];
    __shared__ long long part[AUC_WAVES];
    const int tid = threadIdx.x, lane = hm::lane_id();
    const int64_t g = ids[blockIdx.x];
    const int64_t r0 = rowptr[g];
    const int m = (int)min(rowptr[g + 1] - r0, (int64_t)AUC_MEDIUM_MAX);
    if (tid < 2) cnt[tid] = 0;
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int base = 0; base < m; base += AUC_THREADS) {    // the same trip count for every thread
        const int i = base + tid;
        int64_t key = 0;
        int c = AUC_ABSENT;
        if (i < m) {
            key = keys[r0 + i];
            c = cls[r0 + i];
        }
        const unsigned long long bn = __ballot(c == AUC_NEG), bp = __ballot(c == AUC_POS);
        int sn = 0, sp = 0;                        // where the wave's rows of either class start
        if (lane == 0) {
            sn = atomicAdd(&cnt[0], __popcll(bn));
            sp = atomicAdd(&cnt[1], __popcll(bp));
        }
        sn = __shfl(sn, 0, HM_WAVE);
        sp = __shfl(sp, 0, HM_WAVE);
        // negatives + positives <= m <= MAX, so the two ends never meet
        if (c == AUC_NEG) buf[sn + __popcll(bn & below)] = key;
        else if (c == AUC_POS) buf[AUC_MEDIUM_MAX - 1 - (sp + __popcll(bp & below))] = key;
    }
    __syncthreads();
    const int nn = cnt[0], np = cnt[1];
    // 2U is symmetric in the two classes: stride over the larger one, walk the smaller one
    const bool walk_neg = nn <= np;
    const int n_stride = walk_neg ? np : nn, n_walk = walk_neg ? nn : np;
    long long acc = 0;
    for (int i = tid; i < n_stride; i += AUC_THREADS) {
        int far = 0, eq = 0;                       // walked rows on the counting side of x, and equal to it
        if (walk_neg) {
            const int64_t x = buf[AUC_MEDIUM_MAX - 1 - i];
#pragma unroll 4
            for (int w = 0; w < n_walk; ++w) {
                const int64_t y = buf[w];
                far += (int)(x > y);
                eq += (int)(x == y);
            }
        } else {
            const int64_t x = buf[i];
#pragma unroll 4
            for (int w = 0; w < n_walk; ++w) {
                const int64_t y = buf[AUC_MEDIUM_MAX - 1 - w];
                far += (int)(y > x);
                eq += (int)(x == y);
            }
        }
        acc += 2 * far + eq;
    }
    acc = wave_sum_i64(acc);
    if (lane == 0) part[hm::wave_id()] = acc;
    __syncthreads();
    if (tid == 0) {
        long long t = 0;
        for (int w = 0; w < AUC_WAVES; ++w) t += part[w];
        two_u[g] = t;
        n_pos[g] = np;
        n_neg[g] = nn;
    }
}

__global__ __launch_bounds__(AUC_THREADS) void auc_tile_count_kernel(
    const uint8_t* __restrict__ cls, int64_t NL, int64_t* __restrict__ counts) {
    __shared__ int part[AUC_WAVES];
    const int64_t base = (int64_t)blockIdx.x * AUC_TILE;
    int c = 0;
#pragma unroll
    for (int k = 0; k < AUC_PER_THREAD; ++k) {
        const int64_t p = base + k * AUC_THREADS + threadIdx.x;
        if (p < NL) c += (int)(cls[p] == AUC_NEG);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, HM_WAVE);
    if (hm::lane_id() == 0) part[hm::wave_id()] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int w = 0; w < AUC_WAVES; ++w) t += part[w];
        counts[blockIdx.x] = t;
    }
}

// inc[t] = negatives in tiles 0..t.  A thread owns AUC_PER_THREAD consecutive rows of the tile.
__global__ __launch_bounds__(AUC_THREADS) void auc_tile_scan_kernel(
    const uint8_t* __restrict__ cls, int64_t NL, const int64_t* __restrict__ inc,
    int32_t* __restrict__ negpre) {
    __shared__ int part[AUC_WAVES];
    const int lane = hm::lane_id(), wave = hm::wave_id();
    const int64_t p0 = (int64_t)blockIdx.x * AUC_TILE + (int64_t)threadIdx.x * AUC_PER_THREAD;
    bool neg[AUC_PER_THREAD];
    int mine = 0;
#pragma unroll
    for (int k = 0; k < AUC_PER_THREAD; ++k) {
        neg[k] = p0 + k < NL && cls[p0 + k] == AUC_NEG;
        mine += (int)neg[k];
    }
    int incl = mine;                               // inclusive scan over the wave's threads
#pragma unroll
    for (int o = 1; o < HM_WAVE; o <<= 1) {
        const int v = __shfl_up(incl, o, HM_WAVE);
        if (lane >= o) incl += v;
    }
    if (lane == HM_WAVE - 1) part[wave] = incl;
    __syncthreads();
    int run = (int)(blockIdx.x ? inc[blockIdx.x - 1] : 0) + incl - mine;
    for (int w = 0; w < wave; ++w) run += part[w];
#pragma unroll
    for (int k = 0; k < AUC_PER_THREAD; ++k) {
        if (p0 + k < NL) {
            negpre[p0 + k] = run;
            run += (int)neg[k];
            if (p0 + k == NL - 1) negpre[NL] = run;
        }
    }
}

// gid[p] = the long group (0..GL-1) of sorted row p, NULL when there is one; segptr [GL + 1] its
// segments; ids [GL] the groups' places in the outputs.
__global__ __launch_bounds__(AUC_THREADS) void auc_long_kernel(
    const int64_t* __restrict__ keys, const uint8_t* __restrict__ cls, const int32_t* __restrict__ negpre,
    const int32_t* __restrict__ gid, const int64_t* __restrict__ segptr, const int64_t* __restrict__ ids,
    int64_t NL, int64_t* __restrict__ two_u, int64_t* __restrict__ n_pos, int64_t* __restrict__ n_neg) {
    const int64_t p = (int64_t)blockIdx.x * AUC_THREADS + threadIdx.x;
    const bool live = p < NL;
    int g = -1;                                    // a lane past the end shares no group
    int64_t s0 = 0, s1 = 0, out = 0;
    if (live) {
        g = gid ? gid[p] : 0;
        s0 = segptr[g];
        s1 = segptr[g + 1];
        out = ids[g];
    }
    long long add = 0;
    bool pos = false;
    if (live && cls[p] == AUC_POS) {
        pos = true;
        const int64_t key = keys[p];
        int64_t lo = s0, hi = s1;                  // the first row of the segment with a key >= key
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (keys[mid] < key) lo = mid + 1;
            else hi = mid;
        }
        const int64_t lb = lo;
        hi = s1;                                   // the first with a key > key
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (keys[mid] <= key) lo = mid + 1;
            else hi = mid;
        }
        const long long below = negpre[lb] - negpre[s0], equal = negpre[lo] - negpre[lb];
        add = 2 * below + equal;
    }
    if (live && p == s0) n_neg[out] = negpre[s1] - negpre[s0];     // the segment's first row: one writer
    if (__all(g == __builtin_amdgcn_readfirstlane(g))) {           // the wave lies in one group
        const long long total = wave_sum_i64(add);
        const int np = __popcll(__ballot(pos));
        if (hm::lane_id() == 0 && np) {
            add_i64(two_u + out, total);
            add_i64(n_pos + out, np);
        }
    } else if (pos) {
        add_i64(two_u + out, add);
        add_i64(n_pos + out, 1);
    }
}

inline bool grid_of(int64_t work, int64_t per_block, unsigned* grid) {
    const int64_t b = (work + per_block - 1) / per_block;
    *grid = (unsigned)b;
    return b <= INT32_MAX;
}

}  // namespace

// scores / labels: n rows stored as score_kind (AUC_F64, AUC_F32) / label_kind (any AUC_* kind);
// order int64 [N] or NULL (then N == n): prepared row p is the caller's row order[p], and an entry
// outside 0..n-1 is an absent row.  keys int64 [N], cls uint8 [N].
HM_API int hm_auc_prepare(const void* scores, int score_kind, const void* labels, int label_kind, int64_t n,
                          const int64_t* order, int64_t N, int64_t* keys, uint8_t* cls, hipStream_t stream) {
    if (N <= 0) return 0;
    unsigned grid;
    if (score_kind < AUC_F64 || score_kind > AUC_F32 || label_kind < AUC_F64 || label_kind > AUC_I32 ||
        n < 0 || (!order && N != n) || !grid_of(N, AUC_THREADS, &grid))
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(auc_prepare_kernel, dim3(grid), dim3(AUC_THREADS), 0, stream, scores, score_kind,
                       labels, label_kind, n, order, N, keys, cls);
    HM_LAUNCH_RET();
}

// The groups ids[0..count) (each of at most lpr rows; lpr is 8, 16, 32 or 64): group g is the
// prepared rows rowptr[g]..rowptr[g + 1]; two_u, n_pos, n_neg int64 [G] get one store each.
HM_API int hm_auc_small(const int64_t* keys, const uint8_t* cls, const int64_t* rowptr, const int64_t* ids,
                        int64_t count, int lpr, int64_t* two_u, int64_t* n_pos, int64_t* n_neg,
                        hipStream_t stream) {
    if (count <= 0) return 0;
    unsigned grid;
    if ((lpr != 8 && lpr != 16 && lpr != 32 && lpr != 64) ||
        !grid_of(count, (int64_t)AUC_WAVES * (HM_WAVE / lpr), &grid))
        return (int)hipErrorInvalidValue;
#define AUC_LAUNCH(LPR)                                                                               \
    hipLaunchKernelGGL(auc_small_kernel<LPR>, dim3(grid), dim3(AUC_THREADS), 0, stream, keys, cls, rowptr, \
                       ids, count, two_u, n_pos, n_neg)
    if (lpr == 8) AUC_LAUNCH(8);
    else if (lpr == 16) AUC_LAUNCH(16);
    else if (lpr == 32) AUC_LAUNCH(32);
    else AUC_LAUNCH(64);
#undef AUC_LAUNCH
    HM_LAUNCH_RET();
}

// The same for groups of at most 2048 rows, one workgroup each.
HM_API int hm_auc_medium(const int64_t* keys, const uint8_t* cls, const int64_t* rowptr, const int64_t* ids,
                         int64_t count, int64_t* two_u, int64_t* n_pos, int64_t* n_neg, hipStream_t stream) {
    if (count <= 0) return 0;
    if (count > INT32_MAX) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(auc_medium_kernel, dim3((unsigned)count), dim3(AUC_THREADS), 0, stream, keys, cls,
                       rowptr, ids, two_u, n_pos, n_neg);
    HM_LAUNCH_RET();
}

// cls uint8 [NL] of the long groups' rows, sorted by (group, key); counts int64 [ceil(NL / 2048)].
HM_API int hm_auc_long_count(const uint8_t* cls, int64_t NL, int64_t* counts, hipStream_t stream) {
    if (NL <= 0) return 0;
    unsigned grid;
    if (!grid_of(NL, AUC_TILE, &grid)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(auc_tile_count_kernel, dim3(grid), dim3(AUC_THREADS), 0, stream, cls, NL, counts);
    HM_LAUNCH_RET();
}

// inc = the inclusive cumsum of counts; negpre int32 [NL + 1].
HM_API int hm_auc_long_scan(const uint8_t* cls, int64_t NL, const int64_t* inc, int32_t* negpre,
                            hipStream_t stream) {
    if (NL <= 0) return 0;
    unsigned grid;
    if (NL > INT32_MAX || !grid_of(NL, AUC_TILE, &grid)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(auc_tile_scan_kernel, dim3(grid), dim3(AUC_THREADS), 0, stream, cls, NL, inc, negpre);
    HM_LAUNCH_RET();
}

// Adds into two_u and n_pos and stores n_neg at ids[0..GL): the caller zeroes those entries.
HM_API int hm_auc_long_sum(const int64_t* keys, const uint8_t* cls, const int32_t* negpre, const int32_t* gid,
                           const int64_t* segptr, const int64_t* ids, int64_t NL, int64_t* two_u,
                           int64_t* n_pos, int64_t* n_neg, hipStream_t stream) {
    if (NL <= 0) return 0;
    unsigned grid;
    if (!grid_of(NL, AUC_THREADS, &grid)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(auc_long_kernel, dim3(grid), dim3(AUC_THREADS), 0, stream, keys, cls, negpre, gid,
                       segptr, ids, NL, two_u, n_pos, n_neg);
    HM_LAUNCH_RET();
}
