// Singular spectrum transformation (sst) change-point scores on gfx950: per time point, the
// subspace distance 1 - sigma_max(U^T Q)^2 between the leading left singular vectors of a past
// and of a current Hankel matrix (docs/compat.md, "sst -engine").
//
//   hm_sst_scores  x fp64 [S, N] -> score fp64 [S, N] (and the sweep counts, int32 [S, N])
//
// One workgroup of two waves serves one scored point at a time (grid-stride over the
// S * (N - need + 1) scored points).  Wave 0 builds the w x n past matrix P and wave 1 the w x m
// current matrix Q0 in dynamic LDS, column-major fp64 with lane = row, straight from the w + n - 1
// (w + m - 1) contiguous samples in x and scaled by a power of two so that the largest |entry| is
// in [0.5, 1); a ds_read_b64 of a column then touches consecutive doubles.
// Each wave runs a one-sided (Hestenes) Jacobi SVD on its matrix:
//
//   pair order   plain row-cyclic: p = 0 .. cols - 2, q = p + 1 .. cols - 1
//   per pair     a = |A_p|^2, b = |A_q|^2, c = A_p . A_q, all three recomputed: separately
//                rounded products, summed over the lanes on DPP permutes, one lane's total
//                broadcast through scalar registers (sst_dot, hm::wave_sum_uniform)
//   skip         a or b <= (max(rows, cols) * eps * |A|_F)^2   (numerically null column)
//   skip         |c| <= rows * eps * sqrt(a * b)
//   rotate       z = (b - a) / 2c, t = sign(z) / (|z| + sqrt(1 + z^2)) (1 for z = 0),
//                cs = 1 / sqrt(1 + t^2), sn = cs * t, A_p' = cs A_p - sn A_q, A_q' = sn A_p + cs A_q
//   stop         after a sweep without a rotation; the cap is 30 sweeps (reported as 31)
//
// Column p stays in registers over its q loop.  After convergence lane j ranks column j by
// "norm descending, then index ascending" against the others through lane shuffles; the kept
// columns (rank below the requested rank and sigma > max(rows, cols) * eps * sigma_1) leave their
// index and 1 / sigma in LDS.  After a barrier both waves form M = U^T Q in LDS (entries
// round-robin over the waves), after a second barrier wave 0 runs the same routine on M (on M^T
// when that has fewer columns) and takes the largest column norm.  Nothing but the samples and the
// score touches HBM; no atomics, no state across workgroups.  All arithmetic is fp64.  The C++
// twin with the same order and thresholds is csrc/host/sst_cpu.cpp.
#include "common.h"

#include <math.h>

namespace {

constexpr int SST_THREADS = 2 * HM_WAVE;
constexpr int SST_DIM_MAX = 64;            // rows = one wave; 3 * 64 * 64 fp64 = 96 KiB of LDS
constexpr int SST_SWEEP_CAP = 30;
constexpr double SST_EPS = 2.220446049250313e-16;      // 2^-52
constexpr int64_t SST_GRID_MAX = 1 << 20;

__device__ __forceinline__ double sst_wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, HM_WAVE));
    return v;
}

// Wave-wide dot of two lane-held vectors, the same bits in every lane.  Two constraints.  The
// product is rounded on its own, as the twin rounds it: under -ffp-contract=fast the compiler
// otherwise folds it into the first add of the reduction as fma(u, v, neighbour's rounded
// product), and in a butterfly whose lanes each keep their own total the lanes then differ in the
// last bit, disagree on a threshold and rotate by different angles.  And one lane's total is
// broadcast (hm::wave_sum_uniform reads lane 63 into scalar registers), which keeps a, b and c
// uniform whatever the compiler does.  The DPP sum also takes 22 % less time than the
// ds_bpermute butterfly of hm::wave_sum (docs/perf_notes.md, sst).  EXEC must be full.
__device__ __forceinline__ double sst_dot(double u, double v) {
    double p = u * v;
    asm volatile("" : "+v"(p));
    return hm::wave_sum_uniform(p);
}

// One-sided Jacobi on the rows x cols column-major matrix A (leading dimension rows) in LDS, by
// one full wave; lane = row, lanes >= rows carry zeros.  Returns the number of sweeps, 31 when
// the 30th still rotated.  a, b, c are bit-identical in every lane (sst_dot), so every branch is
// wave-uniform and every lane rotates by the same angle.
__device__ int sst_jacobi(double* __restrict__ A, int rows, int cols, int lane) {
    const bool on = lane < rows;
    double f = 0.0;
    for (int j = 0; j < cols; ++j) {
        const double v = on ? A[lane + j * rows] : 0.0;
        f += v * v;
    }
    const double tn = (double)max(rows, cols) * SST_EPS * sqrt(hm::wave_sum_uniform(f));
    const double null2 = tn * tn;
    const double ctol = (double)rows * SST_EPS;
    int sweeps = 0;
    for (;;) {
        ++sweeps;
        bool rotated = false;
        for (int p = 0; p + 1 < cols; ++p) {
            double ap = on ? A[lane + p * rows] : 0.0;
            for (int q = p + 1; q < cols; ++q) {
                const double aq = on ? A[lane + q * rows] : 0.0;
                const double a = sst_dot(ap, ap);
                const double b = sst_dot(aq, aq);
                const double c = sst_dot(ap, aq);
                if (a <= null2 || b <= null2) continue;
                if (fabs(c) <= ctol * sqrt(a * b)) continue;
                const double z = (b - a) / (2.0 * c);
                const double t = z == 0.0 ? 1.0 : copysign(1.0, z) / (fabs(z) + sqrt(1.0 + z * z));
                const double cs = 1.0 / sqrt(1.0 + t * t);
                const double sn = cs * t;
                const double np = cs * ap - sn * aq;
                const double nq = sn * ap + cs * aq;
                ap = np;
                if (on) A[lane + q * rows] = nq;
                rotated = true;
            }
            if (on) A[lane + p * rows] = ap;
        }
        if (!rotated) break;
        if (sweeps == SST_SWEEP_CAP) { sweeps = SST_SWEEP_CAP + 1; break; }
    }
    return sweeps;
}

__global__ __launch_bounds__(SST_THREADS) void sst_kernel(
    const double* __restrict__ x, int64_t S, int64_t N, int w, int n, int m, int g, int kr, int kk,
    int64_t need, double* __restrict__ out, int32_t* __restrict__ sweeps_out) {
    extern __shared__ __attribute__((aligned(16))) double s_mat[];   // P [w, n], Q0 [w, m], M [kr, kk]
    __shared__ double s_isg[2][SST_DIM_MAX];       // 1 / sigma of the kept columns, by rank
    __shared__ int s_ord[2][SST_DIM_MAX];          // their column index, by rank
    __shared__ int s_kept[2];
    __shared__ int s_sweeps[2];

    const int tid = threadIdx.x, lane = hm::lane_id(), wave = hm::wave_id();

    // ---- the unscored prefix of every series: exactly 0.0 and 0 sweeps
    const int64_t pre = need - 1 < N ? need - 1 : N;
    for (int64_t e = (int64_t)blockIdx.x * SST_THREADS + tid; e < S * pre;
         e += (int64_t)gridDim.x * SST_THREADS) {
        const int64_t o = (e / pre) * N + e % pre;
        out[o] = 0.0;
        if (sweeps_out) sweeps_out[o] = 0;
    }
    if (N < need) return;

    double* const sP = s_mat;
    double* const sQ = s_mat + w * n;
    double* const sM = sQ + w * m;
    double* const A = wave == 0 ? sP : sQ;
    const int cols = wave == 0 ? n : m;
    const int want = wave == 0 ? kr : kk;
    const bool on = lane < w;
    const double dim_eps = (double)max(w, cols) * SST_EPS;

    const int64_t per = N - need + 1;
    for (int64_t pt = blockIdx.x; pt < S * per; pt += gridDim.x) {
        const int64_t s = pt / per, end = pt % per + need;
        // P[l, i] = x[end + g - m - n - w + 1 + i + l], Q0[l, i] = x[end - m - w + 1 + i + l]
        const int64_t base = s * N + (wave == 0 ? end + g - m - n - w + 1 : end - m - w + 1);
        // scaled by the power of two that brings the largest |entry| into [0.5, 1): the score does
        // not depend on the scale, the scaling is exact, and no square over- or underflows
        double big = 0.0;
        if (on)
            for (int i = 0; i < cols; ++i) big = fmax(big, fabs(x[base + i + lane]));
        int ex = 0;
        frexp(sst_wave_max(big), &ex);
        if (on)
            for (int i = 0; i < cols; ++i) A[lane + i * w] = ldexp(x[base + i + lane], -ex);

        const int sw = sst_jacobi(A, w, cols, lane);

        // ---- lane j: the squared norm of column j, its rank, and whether it is kept
        double mine = 0.0;
        for (int j = 0; j < cols; ++j) {
            const double v = on ? A[lane + j * w] : 0.0;
            const double nj = sst_dot(v, v);
            if (lane == j) mine = nj;
        }
        const double top = sst_wave_max(mine);
        int rank = 0;
        for (int i = 0; i < cols; ++i) {
            const double ni = __shfl(mine, i, HM_WAVE);
            rank += (ni > mine || (ni == mine && i < lane)) ? 1 : 0;
        }
        const double sigma = sqrt(mine);
        const bool keep = lane < cols && rank < want && sigma > dim_eps * sqrt(top);
        if (keep) {
            s_ord[wave][rank] = lane;
            s_isg[wave][rank] = 1.0 / sigma;
        }
        const int kept = __popcll(__ballot(keep));
        if (lane == 0) {
            s_kept[wave] = kept;
            s_sweeps[wave] = sw;
        }
        __syncthreads();

        // ---- M = U^T Q, stored so that the Jacobi below runs on the side with fewer columns
        const int nu = s_kept[0], nq = s_kept[1];
        int sw_all = max(s_sweeps[0], s_sweeps[1]);
        const bool flip = nq > nu;                 // M^T: rows = nq, cols = nu
        const int mrows = flip ? nq : nu, mcols = flip ? nu : nq;
        for (int e = wave; e < nu * nq; e += 2) {
            const int i = e / nq, j = e % nq;
            const double u = on ? sP[lane + s_ord[0][i] * w] * s_isg[0][i] : 0.0;
            const double v = on ? sQ[lane + s_ord[1][j] * w] * s_isg[1][j] : 0.0;
            const double d = sst_dot(u, v);
            if (lane == 0) sM[flip ? j + i * mrows : i + j * mrows] = d;
        }
        __syncthreads();

        if (wave == 0) {
            double score;
            if (nu == 0 || nq == 0) {
                score = nu == nq ? 0.0 : 1.0;      // two empty subspaces are identical
            } else {
                sw_all = max(sw_all, sst_jacobi(sM, mrows, mcols, lane));
                double best = 0.0;
                for (int j = 0; j < mcols; ++j) {
                    const double v = lane < mrows ? sM[lane + j * mrows] : 0.0;
                    best = fmax(best, sst_dot(v, v));
                }
                score = fmin(fmax(1.0 - best, 0.0), 1.0);
            }
            if (lane == 0) {
                const int64_t o = s * N + end - 1;
                out[o] = score;
                if (sweeps_out) sweeps_out[o] = sw_all;
            }
        }
        // wave 1 may start the next point: it writes Q0, s_*[1] (read above, before the second
        // barrier) and, only after the next first barrier, M
    }
}

}  // namespace

// x, out fp64 [S, N] (contiguous rows); sweeps int32 [S, N] or NULL: the largest sweep count of
// the point's three Jacobi runs, 0 in the unscored prefix, 31 when the cap of 30 was hit.
// 2 <= w <= 64, 1 <= n, m <= 64, r, k >= 1, g <= m.
HM_API int hm_sst_scores(const double* x, int64_t S, int64_t N, int w, int n, int m, int g, int r,
                         int k, double* out, int32_t* sweeps, hipStream_t stream) {
    if (w < 2 || w > SST_DIM_MAX || n < 1 || n > SST_DIM_MAX || m < 1 || m > SST_DIM_MAX ||
        r < 1 || k < 1 || g > m || S < 0 || N < 0)
        return (int)hipErrorInvalidValue;
    if (S == 0 || N == 0) return 0;
    const int64_t need = (int64_t)w + n + (g < 0 ? -(int64_t)g : 0) + m;
    const int kr = min(r, min(w, n)), kk = min(k, min(w, m));
    const size_t lds = (size_t)(w * n + w * m + kr * kk) * sizeof(double);
    static bool attr_set = false;
    if (!attr_set) {
        const hipError_t e = hipFuncSetAttribute(
            reinterpret_cast<const void*>(&sst_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
            3 * SST_DIM_MAX * SST_DIM_MAX * (int)sizeof(double));
        if (e != hipSuccess) return (int)e;
        attr_set = true;
    }
    // (S * N never overflows int64 for tensors that exist)
    const int64_t points = N >= need ? S * (N - need + 1) : 0;
    const int64_t pre_blocks = (S * (need - 1 < N ? need - 1 : N) + SST_THREADS - 1) / SST_THREADS;
    int64_t grid = points > 0 ? points : pre_blocks;
    if (grid > SST_GRID_MAX) grid = SST_GRID_MAX;
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL(sst_kernel, dim3((unsigned)grid), dim3(SST_THREADS), lds, stream, x, S, N, w,
                       n, m, g, kr, kk, need, out, sweeps);
    HM_LAUNCH_RET();
}
