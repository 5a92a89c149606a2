// train_slim on gfx950: per-item Gram build over sparse rating columns and non-negative
// elastic-net coordinate descent in Gram form (Ning & Karypis, ICDM'11; upstream SlimUDTF).
//
//   hm_slim_gram  ratings as CSC over rating vectors -> G [n, K, K], b [n, K] per item
//   hm_slim_cd    (G, b) -> W [n, K], the rule of models/recommend.py::_slim_cd_chunk
//
// All arithmetic is fp64: the learner's contract is "matches the upstream residual loop to
// rounding", and the coordinate loop is a latency chain (LDS row read, wave reduction, one-lane
// update), not a throughput problem.  The C++ twin is csrc/host/slim_cpu.cpp.
#include "common.h"

namespace {

constexpr int GRAM_THREADS = 256;
constexpr int GRAM_WAVES = GRAM_THREADS / HM_WAVE;

// <column x, column y> by one wave: the shorter column is walked 64 entries at a time and every
// lane binary-searches its row id in the longer one.  Returns the wave-uniform total.
__device__ __forceinline__ double wave_col_dot(const int32_t* __restrict__ rows,
                                               const double* __restrict__ vals, int64_t x0,
                                               int64_t x1, int64_t y0, int64_t y1, bool same) {
    const int lane = hm::lane_id();
    double acc = 0.0;
    if (same) {
        for (int64_t p = x0 + lane; p < x1; p += HM_WAVE) acc += vals[p] * vals[p];
        return hm::wave_sum(acc);
    }
    if (x1 - x0 > y1 - y0) {
        int64_t t = x0; x0 = y0; y0 = t;
        t = x1; x1 = y1; y1 = t;
    }
    if (x1 == x0) return 0.0;
    for (int64_t p = x0 + lane; p < x1; p += HM_WAVE) {
        const int32_t u = rows[p];
        int64_t lo = y0, hi = y1;                      // first position in y with rows >= u
        while (lo < hi) {
            const int64_t m = (lo + hi) >> 1;
            if (rows[m] < u) lo = m + 1; else hi = m;
        }
        if (lo < y1 && rows[lo] == u) acc += vals[p] * vals[lo];
    }
    return hm::wave_sum(acc);
}

// One workgroup per item; its waves take the (a, c >= a) pairs and the (a, target) pairs
// round-robin.  Every entry of G[t] and b[t] is written (padding: zeros).
__global__ __launch_bounds__(GRAM_THREADS) void slim_gram_kernel(
    const int64_t* __restrict__ colptr, const int32_t* __restrict__ rows,
    const double* __restrict__ vals, int C, const int32_t* __restrict__ target,
    const int32_t* __restrict__ nbr, int K, double* __restrict__ G, double* __restrict__ b) {
    const int64_t t = blockIdx.x;
    const int lane = hm::lane_id();
    const int32_t* nb = nbr + t * K;
    double* Gt = G + (size_t)t * K * K;
    double* bt = b + (size_t)t * K;
    const int tc = target[t];
    const bool t_ok = tc >= 0 && tc < C;
    // q = a * (K + 1) + c;  c == K is the target column, c < a is the mirrored half
    const int total = K * (K + 1);
    for (int q = hm::wave_id(); q < total; q += GRAM_WAVES) {
        const int a = q / (K + 1), c = q - a * (K + 1);
        if (c < a) continue;
        const int ia = nb[a];
        const int ic = c < K ? nb[c] : tc;
        const bool ok = ia >= 0 && ia < C && (c < K ? (ic >= 0 && ic < C) : t_ok);
        double v = 0.0;
        if (ok)
            v = wave_col_dot(rows, vals, colptr[ia], colptr[ia + 1], colptr[ic], colptr[ic + 1],
                             ia == ic);
        if (lane == 0) {
            if (c < K) {
                Gt[(size_t)a * K + c] = v;
                Gt[(size_t)c * K + a] = v;
            } else {
                bt[a] = v;
            }
        }
    }
}

// One wave per item.  LDS per wave: G as [KP][KP] fp64 (row k contiguous), then b [KP].
// w lives in registers, w[m] in lane m & 63, register m >> 6.
template <int KP>
__global__ __launch_bounds__(KP == 128 ? 64 : 256) void slim_cd_kernel(
    const double* __restrict__ G, const double* __restrict__ b, int64_t n, int K, double l1,
    double l2, int iters, double eps, double* __restrict__ W) {
    constexpr int NR = KP > HM_WAVE ? KP / HM_WAVE : 1;
    constexpr int WAVES = KP == 128 ? 1 : 4;
    extern __shared__ __attribute__((aligned(16))) double s_slim[];
    const int lane = hm::lane_id();
    const int64_t t = (int64_t)blockIdx.x * WAVES + hm::wave_id();
    double* sG = s_slim + (size_t)hm::wave_id() * (KP * KP + KP);
    double* sb = sG + KP * KP;
    if (t < n) {
        const double* Gt = G + (size_t)t * K * K;
        for (int e = lane; e < KP * KP; e += HM_WAVE) {
            const int r = e / KP, c = e % KP;
            sG[e] = (r < K && c < K) ? Gt[(size_t)r * K + c] : 0.0;
        }
        for (int e = lane; e < KP; e += HM_WAVE) sb[e] = e < K ? b[(size_t)t * K + e] : 0.0;
    }
    __syncthreads();
    if (t >= n) return;

    double w[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) w[r] = 0.0;
    for (int it = 0; it < iters; ++it) {
        double dmax = 0.0;
        for (int k = 0; k < K; ++k) {
            const double* row = sG + k * KP;
            const double gkk = row[k];
            if (!(gkk > 0.0)) continue;                      // padding and empty columns stay 0
            double part = 0.0, wsel = 0.0;
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const int m = lane + r * HM_WAVE;
                if (m < KP) part += row[m] * w[r];
                if (r == (k >> 6)) wsel = w[r];
            }
            const double dot = hm::wave_sum(part);
            const double wk = __shfl(wsel, k & 63, HM_WAVE);
            const double rho = sb[k] - dot + gkk * wk;
            const double nw = fmax(rho - l1, 0.0) / (gkk + l2);
            dmax = fmax(dmax, fabs(nw - wk));
#pragma unroll
            for (int r = 0; r < NR; ++r)
                if (r == (k >> 6) && lane == (k & 63)) w[r] = nw;
        }
        if (!(dmax >= eps)) break;                           // the per-item convergence test
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const int m = lane + r * HM_WAVE;
        if (m < K) W[(size_t)t * K + m] = w[r];
    }
}

template <int KP>
int launch_cd(const double* G, const double* b, int64_t n, int K, double l1, double l2, int iters,
              double eps, double* W, hipStream_t stream) {
    constexpr int WAVES = KP == 128 ? 1 : 4;
    constexpr size_t lds = (size_t)WAVES * (KP * KP + KP) * sizeof(double);
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&slim_cd_kernel<KP>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        attr_set = true;
    }
    const int64_t blocks = (n + WAVES - 1) / WAVES;
    hipLaunchKernelGGL(slim_cd_kernel<KP>, dim3((unsigned)blocks), dim3(WAVES * HM_WAVE), lds,
                       stream, G, b, n, K, l1, l2, iters, eps, W);
    HM_LAUNCH_RET();
}

}  // namespace

// Ratings as CSC over rating vectors: colptr int64 [C+1], rows int32 [nnz] strictly increasing
// inside a column, vals fp64 [nnz].  target int32 [n]: the column of item t's own vector;
// nbr int32 [n, K]: its neighbours' columns, -1 = padding.
// G [n, K, K] = <col nbr[t,a], col nbr[t,c]>, b [n, K] = <col nbr[t,a], col target[t]>;
// rows and columns of padded slots are zero.
HM_API int hm_slim_gram(const int64_t* colptr, const int32_t* rows, const double* vals, int C,
                        const int32_t* target, const int32_t* nbr, int64_t n, int K, double* G,
                        double* b, hipStream_t stream) {
    if (n <= 0 || K <= 0) return 0;
    if (n > INT32_MAX || C < 0 || K > 32767) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(slim_gram_kernel, dim3((unsigned)n), dim3(GRAM_THREADS), 0, stream, colptr,
                       rows, vals, C, target, nbr, K, G, b);
    HM_LAUNCH_RET();
}

// W [n, K]: coordinates in index order, rho = b_k - sum_m G_km w_m + G_kk w_k,
// w_k = max(0, rho - l1) / (G_kk + l2); coordinates with G_kk <= 0 are skipped; an item stops
// after the sweep whose largest |dw| is < eps.  K <= 128.
HM_API int hm_slim_cd(const double* G, const double* b, int64_t n, int K, double l1, double l2,
                      int iters, double eps, double* W, hipStream_t stream) {
    if (n <= 0 || K <= 0) return 0;
    if (K > 128 || n > (int64_t)INT32_MAX) return (int)hipErrorInvalidValue;
    if (K <= 32) return launch_cd<32>(G, b, n, K, l1, l2, iters, eps, W, stream);
    if (K <= 64) return launch_cd<64>(G, b, n, K, l1, l2, iters, eps, W, stream);
    return launch_cd<128>(G, b, n, K, l1, l2, iters, eps, W, stream);
}
