// Cosine k-nearest-neighbour search over the sparse columns of a CSC matrix on gfx950: the
// item-item similarity + each_top_k step in front of train_slim, with no dense matrix formed.
//
//   hm_knn_rnorm  1 / |column| per column (0 for an empty one)
//   hm_knn_cols   per query column i: the k best columns j != i with <i, j> != 0 under
//                 "score descending, then column id ascending",
//                 score = (<i, j> * rnorm[i]) * rnorm[j]
//
// One workgroup serves one query.  The dots of i with a tile of T candidate columns are
// accumulated in an fp64 array in dynamic LDS: the waves take the users of column i round-robin,
// find the tile's range inside the user's row of the transposed matrix and add v_ui * v_uj with
// LDS atomics (a native ds_add_f64, no compare-and-swap loop).  A row holds a column at most
// once, so the addresses of one wave instruction are distinct and only hits from different waves
// serialise.  Selection keeps a sorted running top-k in LDS across tiles.  All arithmetic is
// fp64.  The C++ twin is csrc/host/knn_sparse_cpu.cpp.
#include "common.h"

#include <math.h>

namespace {

constexpr int KNN_THREADS = 1024;          // 16 waves: a full tile owns the CU's LDS, so the
constexpr int KNN_WAVES = KNN_THREADS / HM_WAVE;   // workgroup is all the latency hiding there is
constexpr int KNN_KMAX = 128;
constexpr int KNN_TILE_MAX = 16384;        // 128 KiB of fp64 accumulators

__global__ __launch_bounds__(256) void knn_rnorm_kernel(const int64_t* __restrict__ colptr,
                                                        const double* __restrict__ vals, int C,
                                                        double* __restrict__ rnorm) {
    const int c = blockIdx.x * (256 / HM_WAVE) + hm::wave_id();
    if (c >= C) return;
    const int lane = hm::lane_id();
    // lane-strided partial sums, then the butterfly: one fixed order for a given column length
    double acc = 0.0;
    for (int64_t p = colptr[c] + lane; p < colptr[c + 1]; p += HM_WAVE) acc += vals[p] * vals[p];
    acc = hm::wave_sum(acc);
    if (lane == 0) rnorm[c] = acc > 0.0 ? 1.0 / sqrt(acc) : 0.0;
}

// (s, j) beats (s2, j2) in the total order; j < 0 is "nothing".
__device__ __forceinline__ bool knn_better(double s, int j, double s2, int j2) {
    return j >= 0 && (j2 < 0 || s > s2 || (s == s2 && j < j2));
}

// First position in [lo, hi) whose column id is >= key.
__device__ __forceinline__ int64_t knn_lower_bound(const int32_t* __restrict__ cols, int64_t lo,
                                                   int64_t hi, int key) {
    while (lo < hi) {
        const int64_t m = (lo + hi) >> 1;
        if (cols[m] < key) lo = m + 1; else hi = m;
    }
    return lo;
}

__global__ __launch_bounds__(KNN_THREADS) void knn_cols_kernel(
    const int64_t* __restrict__ colptr, const int32_t* __restrict__ rows,
    const double* __restrict__ vals, int C, const int64_t* __restrict__ rowptr,
    const int32_t* __restrict__ cols, const double* __restrict__ rvals,
    const double* __restrict__ rnorm, const int32_t* __restrict__ query,
    const int32_t* __restrict__ order, int k, int T, int32_t* __restrict__ out_idx,
    double* __restrict__ out_score) {
    extern __shared__ __attribute__((aligned(16))) double s_acc[];   // [T]
    __shared__ double s_top_s[2][KNN_KMAX];        // running top-k, best first (ping-pong)
    __shared__ int s_top_j[2][KNN_KMAX];
    __shared__ double s_wave_s[2][KNN_WAVES];      // per-wave arg-max of a round (ping-pong)
    __shared__ int s_wave_j[2][KNN_WAVES];

    const int tid = threadIdx.x, lane = hm::lane_id(), wave = hm::wave_id();
    const int64_t slot = order ? order[blockIdx.x] : (int64_t)blockIdx.x;
    const int i = query[slot];
    const int64_t q0 = colptr[i], q1 = colptr[i + 1];
    const double rn_i = rnorm[i];
    const double nan = __longlong_as_double(0x7ff8000000000000ll);

    int cur = 0, n_top = 0;                        // list in use, entries in it
    unsigned round = 0;
    for (int j0 = 0; j0 < C; j0 += T) {
        const int tc = min(T, C - j0);
        for (int t = tid; t < tc; t += KNN_THREADS) s_acc[t] = 0.0;
        __syncthreads();

        // ---- accumulate: wave w takes users w, w + 16, ... of column i
        for (int64_t p = q0 + wave; p < q1; p += KNN_WAVES) {
            const int u = __builtin_amdgcn_readfirstlane(rows[p]);
            const double v = vals[p];
            int64_t lo = rowptr[u], hi = rowptr[u + 1];
            if (j0 > 0) lo = knn_lower_bound(cols, lo, hi, j0);
            if (j0 + tc < C) hi = knn_lower_bound(cols, lo, hi, j0 + tc);
            for (int64_t e = lo + lane; e < hi; e += HM_WAVE)
                atomicAdd(&s_acc[cols[e] - j0], v * rvals[e]);
        }
        __syncthreads();

        // ---- scores in place (NaN = no candidate) and every thread's best of its slice:
        // tile entries tid, tid + 1024, ... and entry `tid` of the running list
        double best_s = 0.0;
        int best_j = -1;
        if (tid < n_top) {
            best_s = s_top_s[cur][tid];
            best_j = s_top_j[cur][tid];
        }
        for (int t = tid; t < tc; t += KNN_THREADS) {
            const double d = s_acc[t];
            const int j = j0 + t;
            double s = nan;
            if (d != 0.0 && j != i) s = (d * rn_i) * rnorm[j];
            s_acc[t] = s;
            if (s == s && knn_better(s, j, best_s, best_j)) { best_s = s; best_j = j; }
        }

        // ---- k rounds of block arg-max over the threads' bests; the winner's owner rescans
        const int nxt = cur ^ 1;
        int n_new = 0;
        for (int r = 0; r < k; ++r, ++round) {
            double ws = best_s;
            int wj = best_j;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double os = __shfl_xor(ws, o, HM_WAVE);
                const int oj = __shfl_xor(wj, o, HM_WAVE);
                if (knn_better(os, oj, ws, wj)) { ws = os; wj = oj; }
            }
            const int pb = round & 1;
            if (lane == 0) { s_wave_s[pb][wave] = ws; s_wave_j[pb][wave] = wj; }
            __syncthreads();
            ws = s_wave_s[pb][0];
            wj = s_wave_j[pb][0];
#pragma unroll
            for (int w = 1; w < KNN_WAVES; ++w) {
                const double os = s_wave_s[pb][w];
                const int oj = s_wave_j[pb][w];
                if (knn_better(os, oj, ws, wj)) { ws = os; wj = oj; }
            }
            if (wj < 0) break;                     // nothing left: uniform across the block
            if (tid == 0) { s_top_s[nxt][r] = ws; s_top_j[nxt][r] = wj; }
            n_new = r + 1;
            if (wj == best_j) {                    // ids are unique: exactly one owner
                if (wj < j0) s_top_s[cur][tid] = nan;
                else s_acc[wj - j0] = nan;
                best_s = 0.0;
                best_j = -1;
                if (tid < n_top) {
                    const double s = s_top_s[cur][tid];
                    if (s == s) { best_s = s; best_j = s_top_j[cur][tid]; }
                }
                for (int t = tid; t < tc; t += KNN_THREADS) {
                    const double s = s_acc[t];
                    if (s == s && knn_better(s, j0 + t, best_s, best_j)) { best_s = s; best_j = j0 + t; }
                }
            }
        }
        __syncthreads();                           // list `nxt` is complete and visible
        cur = nxt;
        n_top = n_new;
    }

    for (int r = tid; r < k; r += KNN_THREADS) {
        out_idx[slot * k + r] = r < n_top ? s_top_j[cur][r] : -1;
        out_score[slot * k + r] = r < n_top ? s_top_s[cur][r] : 0.0;
    }
}

}  // namespace

// rnorm [C] = 1 / sqrt(sum of squares) of every column of the CSC matrix, 0 for an empty column.
HM_API int hm_knn_rnorm(const int64_t* colptr, const double* vals, int C, double* rnorm,
                        hipStream_t stream) {
    if (C <= 0) return 0;
    const int per = 256 / HM_WAVE;
    hipLaunchKernelGGL(knn_rnorm_kernel, dim3((unsigned)((C + per - 1) / per)), dim3(256), 0, stream,
                       colptr, vals, C, rnorm);
    HM_LAUNCH_RET();
}

// The matrix as CSC (colptr int64 [C+1], rows int32 strictly increasing inside a column, vals)
// and as its transpose (rowptr int64 [U+1], cols int32 ascending inside a row, rvals), rnorm [C]
// from hm_knn_rnorm, query int32 [n] column ids.  order int32 [n] (or NULL) is the launch order:
// workgroup b serves query[order[b]].  idx int32 [n, k] (-1 = padding) and score fp64 [n, k]
// (0 = padding) are written at the query's own row.  1 <= k <= 128, 1 <= tile <= 16384.
HM_API int hm_knn_cols(const int64_t* colptr, const int32_t* rows, const double* vals, int C,
                       const int64_t* rowptr, const int32_t* cols, const double* rvals,
                       const double* rnorm, const int32_t* query, const int32_t* order, int64_t n,
                       int k, int tile, int32_t* idx, double* score, hipStream_t stream) {
    if (n <= 0) return 0;
    if (n > INT32_MAX || C <= 0 || k < 1 || k > KNN_KMAX || tile < 1 || tile > KNN_TILE_MAX)
        return (int)hipErrorInvalidValue;
    static bool attr_set = false;
    if (!attr_set) {
        // a full tile; the kernel's static LDS (3.4 KiB of selection state) comes on top of it
        const hipError_t e = hipFuncSetAttribute(
            reinterpret_cast<const void*>(&knn_cols_kernel),
            hipFuncAttributeMaxDynamicSharedMemorySize, KNN_TILE_MAX * (int)sizeof(double));
        if (e != hipSuccess) return (int)e;
        attr_set = true;
    }
    const int T = C < tile ? C : tile;
    hipLaunchKernelGGL(knn_cols_kernel, dim3((unsigned)n), dim3(KNN_THREADS),
                       (size_t)T * sizeof(double), stream, colptr, rows, vals, C, rowptr, cols, rvals,
                       rnorm, query, order, k, T, idx, score);
    HM_LAUNCH_RET();
}
