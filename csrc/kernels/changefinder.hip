// ChangeFinder (two-stage SDAR) scores on gfx950, parallel over time (docs/compat.md,
// "changefinder -engine").
//
//   hm_changefinder  x fp64 [S, D, N] -> outlier fp64 [S, N], changepoint fp64 [S, N]
//
// Every piece of SDAR state is an exponentially weighted sum with the constant decay a = 1 - r:
//
//   mu_t    = a mu_(t-1)    + r x_t                                   mu_(-1)    = x_0
//   C_t[j]  = a C_(t-1)[j]  + r (x_t - mu_t) (x_(t-j) - mu_t)         C_(-1)     = 0, j = 0..k
//   sigma_t = a sigma_(t-1) + r (x_t - xhat_t)^2                      sigma_(-1) = 1e-6
//
// and the inputs of each sum are known once the one before it is, so a series is three
// first-order linear scans with pointwise work (Levinson-Durbin, the prediction, the score)
// between them.  A workgroup of 256 lanes owns a chunk of 256 consecutive points of one row
// (series, dimension), one lane per point.  A scan inside a chunk starts from zero: Kogge-Stone
// over a wave on lane shuffles with the factors a^(2^s), then the three preceding waves' totals
// through LDS.  What crosses a chunk seam is the carry y_(c0-1); it enters point i of the chunk
// as a^(i+1) carry.  Carries cross workgroups only through separate launches on one stream:
//
//   cf_mu_agg       chunk aggregate of the mu scan
//   cf_carry        per row, the chunk aggregates in order: carry' = a^256 carry + aggregate,
//                   itself a scan, 256 chunks at a time by one workgroup
//   cf_cov<KB, 0>   mu_t, the k + 1 covariance scans in one pass, their aggregates
//   cf_carry        the same walk for the k + 1 covariance sums
//   cf_cov<KB, 1>   mu_t and C_t again, now with carries; Levinson-Durbin in the point's lane,
//                   xhat_t, (x_t - xhat_t)^2 to the workspace, aggregate of the sigma scan
//   cf_carry
//   cf_score        sigma_t, sigma_(t-1) and the score
//   cf_sum_dims     o_t = sum of the D stage-1 scores (D > 1 only)
//   cf_window_mean  mean over the last min(T, t + 1) points
//
// and the same again for stage 2 over y.  No kernel waits on another workgroup; every loop bound
// is a launch argument or a template constant.  The samples x_(t-1..t-k) before a chunk are a halo
// read from global memory into LDS.  The covariance sums and the Levinson coefficients live in
// registers: KB in {8, 16, 32} is a compile-time bound of k, every loop over j is unrolled to KB
// with wave-uniform `j <= k` guards, so no array is indexed at run time (no scratch).  The powers
// a^1..a^256 and (a^256)^1..(a^256)^256 come in as a table from the caller.  All arithmetic is
// fp64; plain vector stores only.  The sequential C++ twin is csrc/host/changefinder_cpu.cpp.
#include "common.h"

#include <math.h>

namespace {

constexpr int CF_CHUNK = 256;
constexpr int CF_WAVES = CF_CHUNK / HM_WAVE;
constexpr int CF_K_MAX = 32;
constexpr int CF_T_MAX = 1024;
constexpr double CF_SIGMA0 = 1e-6;
constexpr double CF_SIGMA_MIN = 1e-12;

// The scan factors of a chunk: a^(2^s) for the wave steps, a^64 across waves, a^(lane+1) and
// a^(tid+1) for what enters a lane from before its wave / its chunk.
struct CfPow {
    double step[6];
    double wave;
    double lane;
    double tid;
};

__device__ __forceinline__ CfPow cf_pow(const double* __restrict__ pw) {
    CfPow p;
#pragma unroll
    for (int s = 0; s < 6; ++s) p.step[s] = pw[(1 << s) - 1];
    p.wave = pw[HM_WAVE - 1];
    p.lane = pw[hm::lane_id()];
    p.tid = pw[threadIdx.x];
    return p;
}

// Inclusive scan y_i = a y_(i-1) + v_i over the lanes of a wave, from zero.
__device__ __forceinline__ double cf_wave_scan(double v, const CfPow& p, int lane) {
#pragma unroll
    for (int s = 0; s < 6; ++s) {
        const double up = __shfl_up(v, 1u << s, HM_WAVE);
        if (lane >= (1 << s)) v += p.step[s] * up;
    }
    return v;
}

// What the waves before `wave` contribute to its lanes, from the wave totals tot[0..CF_WAVES).
__device__ __forceinline__ double cf_wave_prefix(const double* tot, const CfPow& p, int wave) {
    double pre = 0.0;
#pragma unroll
    for (int u = 0; u < CF_WAVES - 1; ++u)
        if (u < wave) pre = p.wave * pre + tot[u];
    return pre;
}

// The same scan over the 256 lanes of the workgroup; tot is this scan's own CF_WAVES doubles of
// LDS.  One barrier.
__device__ __forceinline__ double cf_chunk_scan(double v, const CfPow& p, double* tot) {
    const int lane = hm::lane_id(), wave = hm::wave_id();
    v = cf_wave_scan(v, p, lane);
    if (lane == HM_WAVE - 1) tot[wave] = v;
    __syncthreads();
    if (wave > 0) v += p.lane * cf_wave_prefix(tot, p, wave);
    return v;
}

__global__ __launch_bounds__(CF_CHUNK) void cf_mu_agg(
    const double* __restrict__ x, int64_t N, int64_t nch, double r, const double* __restrict__ pw,
    double* __restrict__ agg) {
    __shared__ double s_tot[CF_WAVES];
    const int64_t b = blockIdx.x, row = b / nch, t = (b % nch) * CF_CHUNK + threadIdx.x;
    const CfPow p = cf_pow(pw);
    const double v = cf_chunk_scan(t < N ? r * x[row * N + t] : 0.0, p, s_tot);
    if (threadIdx.x == CF_CHUNK - 1) agg[b] = v;
}

// agg, car [rows, nch, nv].  One workgroup per (row, j) walks the row's chunk aggregates in
// order, 256 at a time: the same scan one level up, with the factors (a^256)^(i+1) of pwc and the
// running carry in a register.  car[ch] is the sum before chunk ch.  The first carry is
// x[row * N] where x is given (mu_(-1) = x_0), `init` otherwise.
__global__ __launch_bounds__(CF_CHUNK) void cf_carry(
    const double* __restrict__ agg, double* __restrict__ car, int64_t nch, int nv,
    const double* __restrict__ pwc, const double* __restrict__ x, int64_t N, double init) {
    __shared__ double s_tot[CF_WAVES];
    __shared__ double s_y[CF_CHUNK];
    const int tid = threadIdx.x;
    const int64_t row = blockIdx.x / nv, j = blockIdx.x % nv;
    const CfPow p = cf_pow(pwc);
    const int64_t base = row * nch * nv + j;
    double run = x ? x[row * N] : init;
    for (int64_t c0 = 0; c0 < nch; c0 += CF_CHUNK) {
        const int64_t ch = c0 + tid;
        const double v = cf_chunk_scan(ch < nch ? agg[base + ch * nv] : 0.0, p, s_tot) + p.tid * run;
        s_y[tid] = v;
        __syncthreads();
        if (ch < nch) car[base + ch * nv] = tid > 0 ? s_y[tid - 1] : run;
        run = s_y[CF_CHUNK - 1];
        // the next round writes s_tot before and s_y after the barrier inside its scan; this
        // round's reads of s_tot are before the barrier above, those of s_y before that one
    }
}

// Levinson-Durbin on C[0..k] as anomaly._levinson does it; w[i >= k] = 0.  The update
// new[j] = w[j] - kappa w[i-1-j] runs in place on the pairs (j, i-1-j).
template <int KB>
__device__ __forceinline__ void cf_levinson(const double (&C)[KB + 1], int k, double (&w)[KB]) {
#pragma unroll
    for (int j = 0; j < KB; ++j) w[j] = 0.0;
    const bool ok = C[0] > 0.0;
    double e = C[0];
#pragma unroll
    for (int i = 0; i < KB; ++i) {
        if (i < k) {
            double s = 0.0;
#pragma unroll
            for (int j = 0; j < i; ++j) s += w[j] * C[i - j];
            const double acc = C[i + 1] - s;
            double kappa = (ok && e > 0.0) ? acc / e : 0.0;
            kappa = fmax(-0.999, fmin(0.999, kappa));
#pragma unroll
            for (int j = 0; 2 * j < i; ++j) {
                const double lo = w[j], hi = w[i - 1 - j];
                w[j] = lo - kappa * hi;
                w[i - 1 - j] = hi - kappa * lo;
            }
            w[i] = kappa;
            e *= 1.0 - kappa * kappa;
        }
    }
}

// x [rows, N].  FINAL = false: agg_c [rows, nch, k + 1] gets the chunk aggregates of the
// covariance scans.  FINAL = true: car_c holds their carries; e2 [rows, N] gets (x_t - xhat_t)^2
// and agg_s [rows, nch] the chunk aggregate of the sigma scan.
template <int KB, bool FINAL>
__global__ __launch_bounds__(CF_CHUNK) void cf_cov(
    const double* __restrict__ x, int64_t N, int64_t nch, int k, double r,
    const double* __restrict__ pw, const double* __restrict__ car_mu,
    const double* __restrict__ car_c, double* __restrict__ agg_c, double* __restrict__ e2,
    double* __restrict__ agg_s) {
    __shared__ double s_x[CF_CHUNK + KB];               // x[c0 - KB .. c0 + 256), 0 outside [0, N)
    __shared__ double s_tot[KB + 3][CF_WAVES];          // [0..KB] C[j], [KB + 1] mu, [KB + 2] sigma
    const int tid = threadIdx.x, lane = hm::lane_id(), wave = hm::wave_id();
    const int64_t b = blockIdx.x, row = b / nch, c0 = (b % nch) * CF_CHUNK, t = c0 + tid;
    const double* __restrict__ xr = x + row * N;
    for (int i = tid; i < CF_CHUNK + KB; i += CF_CHUNK) {
        const int64_t tt = c0 - KB + i;
        s_x[i] = (tt >= 0 && tt < N) ? xr[tt] : 0.0;
    }
    const CfPow p = cf_pow(pw);
    __syncthreads();
    const bool on = t < N;
    const double xt = s_x[KB + tid];
    const double mu = cf_chunk_scan(on ? r * xt : 0.0, p, s_tot[KB + 1]) + p.tid * car_mu[b];

    // ---- the k + 1 covariance scans; a term whose sample is before the series is exactly 0
    const double rdx = r * (xt - mu);
    double C[KB + 1];
#pragma unroll
    for (int j = 0; j <= KB; ++j) {
        C[j] = 0.0;
        if (j <= k) {
            const double v = (on && t >= j) ? rdx * (s_x[KB + tid - j] - mu) : 0.0;
            C[j] = cf_wave_scan(v, p, lane);
            if (lane == HM_WAVE - 1) s_tot[j][wave] = C[j];
        }
    }
    __syncthreads();
    if (wave > 0) {
#pragma unroll
        for (int j = 0; j <= KB; ++j)
            if (j <= k) C[j] += p.lane * cf_wave_prefix(s_tot[j], p, wave);
    }
    if constexpr (!FINAL) {
        if (tid == CF_CHUNK - 1) {
#pragma unroll
            for (int j = 0; j <= KB; ++j)
                if (j <= k) agg_c[b * (k + 1) + j] = C[j];
        }
    } else {
#pragma unroll
        for (int j = 0; j <= KB; ++j)
            if (j <= k) C[j] += p.tid * car_c[b * (k + 1) + j];
        double w[KB];
        cf_levinson<KB>(C, k, w);
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < KB; ++i)
            if (i < k) s += w[i] * (t >= i + 1 ? s_x[KB + tid - 1 - i] - mu : 0.0);
        const double d = xt - (mu + s);
        const double dd = d * d;
        if (on) e2[row * N + t] = dd;
        const double sg = cf_chunk_scan(on ? r * dd : 0.0, p, s_tot[KB + 2]);
        if (tid == CF_CHUNK - 1) agg_s[b] = sg;
    }
}

// loss 0: the Hellinger distance between the predictive normals before and after the update;
// loss 1: the negative log-likelihood.
__global__ __launch_bounds__(CF_CHUNK) void cf_score(
    const double* __restrict__ e2, int64_t N, int64_t nch, double r, const double* __restrict__ pw,
    const double* __restrict__ car_s, int loss, double* __restrict__ score) {
    __shared__ double s_tot[CF_WAVES];
    __shared__ double s_sig[CF_CHUNK];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x, row = b / nch, t = (b % nch) * CF_CHUNK + tid;
    const CfPow p = cf_pow(pw);
    const bool on = t < N;
    const double dd = on ? e2[row * N + t] : 0.0;
    const double carry = car_s[b];
    const double sig = cf_chunk_scan(r * dd, p, s_tot) + p.tid * carry;
    s_sig[tid] = sig;
    __syncthreads();
    const double prev = tid > 0 ? s_sig[tid - 1] : carry;
    if (!on) return;
    const double s2 = fmax(sig, CF_SIGMA_MIN);
    double sc;
    if (loss == 1) {
        sc = 0.5 * log(2.0 * M_PI * s2) + dd / (2.0 * s2);
    } else {
        const double s1 = fmax(prev, CF_SIGMA_MIN);
        const double bc = sqrt(2.0 * sqrt(s1 * s2) / (s1 + s2));
        sc = fmax(0.0, 2.0 - 2.0 * bc * exp(-dd / (4.0 * (s1 + s2))));
    }
    score[row * N + t] = sc;
}

// score [S, D, N] -> out [S, N], the dimensions added in order.
__global__ __launch_bounds__(CF_CHUNK) void cf_sum_dims(
    const double* __restrict__ score, int64_t S, int64_t D, int64_t N, double* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * CF_CHUNK + threadIdx.x;
    if (e >= S * N) return;
    const int64_t s = e / N, t = e % N;
    double o = 0.0;
    for (int64_t d = 0; d < D; ++d) o += score[(s * D + d) * N + t];
    out[e] = o;
}

// in, out [S, N]: out_t = mean of in over the last min(T, t + 1) points, added oldest first.
__global__ __launch_bounds__(CF_CHUNK) void cf_window_mean(
    const double* __restrict__ in, int64_t S, int64_t N, int T, double* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * CF_CHUNK + threadIdx.x;
    if (e >= S * N) return;
    const int64_t t = e % N;
    const int n = t + 1 < T ? (int)(t + 1) : T;
    double sum = 0.0;
    for (int i = n - 1; i >= 0; --i) sum += in[e - i];
    out[e] = sum / (double)n;
}

struct CfWork {
    double *agg1, *car1, *aggc, *carc, *e2;
};

template <int KB>
void cf_launch_cov(const double* x, int64_t rows, int64_t N, int64_t nch, int k, double r,
                   const double* pw, const CfWork& ws, hipStream_t stream) {
    const dim3 grid((unsigned)(rows * nch)), block(CF_CHUNK);
    const int nv = k + 1;
    hipLaunchKernelGGL((cf_cov<KB, false>), grid, block, 0, stream, x, N, nch, k, r, pw, ws.car1,
                       (const double*)nullptr, ws.aggc, (double*)nullptr, (double*)nullptr);
    hipLaunchKernelGGL(cf_carry, dim3((unsigned)(rows * nv)), block, 0, stream, ws.aggc, ws.carc, nch,
                       nv, pw + CF_CHUNK, (const double*)nullptr, N, 0.0);
    hipLaunchKernelGGL((cf_cov<KB, true>), grid, block, 0, stream, x, N, nch, k, r, pw, ws.car1,
                       ws.carc, (double*)nullptr, ws.e2, ws.agg1);
}

// One SDAR over x [rows, N] -> score [rows, N].
int cf_sdar(const double* x, int64_t rows, int64_t N, int k, double r, int loss, const double* pw,
            const CfWork& ws, double* score, hipStream_t stream) {
    const int64_t nch = (N + CF_CHUNK - 1) / CF_CHUNK;
    const dim3 grid((unsigned)(rows * nch)), block(CF_CHUNK);
    const dim3 cgrid((unsigned)rows);
    hipLaunchKernelGGL(cf_mu_agg, grid, block, 0, stream, x, N, nch, r, pw, ws.agg1);
    hipLaunchKernelGGL(cf_carry, cgrid, block, 0, stream, ws.agg1, ws.car1, nch, 1, pw + CF_CHUNK, x,
                       N, 0.0);
    HM_LAUNCH_RET_IF_ERR();
    if (k <= 8) cf_launch_cov<8>(x, rows, N, nch, k, r, pw, ws, stream);
    else if (k <= 16) cf_launch_cov<16>(x, rows, N, nch, k, r, pw, ws, stream);
    else cf_launch_cov<32>(x, rows, N, nch, k, r, pw, ws, stream);
    HM_LAUNCH_RET_IF_ERR();
    // the sigma carries overwrite the mu carries, which cf_cov<KB, true> has read by now
    hipLaunchKernelGGL(cf_carry, cgrid, block, 0, stream, ws.agg1, ws.car1, nch, 1, pw + CF_CHUNK,
                       (const double*)nullptr, N, CF_SIGMA0);
    hipLaunchKernelGGL(cf_score, grid, block, 0, stream, ws.e2, N, nch, r, pw, ws.car1, loss, score);
    HM_LAUNCH_RET();
}

}  // namespace

// x fp64 [S, D, N] (every row one dimension of one series); outlier, changepoint fp64 [S, N].
// 1 <= k <= 32, 0 < r1, r2 < 1, 1 <= T1, T2 <= 1024, loss 0 = hellinger, 1 = logloss.
// pw1, pw2 [512]: (1 - r)^(i+1), then (1 - r)^(256 (i+1)), i = 0..255.  Workspace, all fp64:
// agg1, car1 [S * D * nch], aggc, carc [S * D * nch * (k + 1)] with nch = ceil(N / 256); e2, score
// [S * D * N]; y [S * N].
HM_API int hm_changefinder(const double* x, int64_t S, int64_t D, int64_t N, int k, double r1,
                           double r2, int T1, int T2, int loss1, int loss2, const double* pw1,
                           const double* pw2, double* agg1, double* car1, double* aggc,
                           double* carc, double* e2, double* score, double* y, double* outlier,
                           double* changepoint, hipStream_t stream) {
    if (S < 0 || D < 0 || N < 0 || k < 1 || k > CF_K_MAX || !(r1 > 0.0 && r1 < 1.0) ||
        !(r2 > 0.0 && r2 < 1.0) || T1 < 1 || T1 > CF_T_MAX || T2 < 1 || T2 > CF_T_MAX ||
        (loss1 | loss2) < 0 || loss1 > 1 || loss2 > 1)
        return (int)hipErrorInvalidValue;
    if (S == 0 || D == 0 || N == 0) return 0;
    const int64_t nch = (N + CF_CHUNK - 1) / CF_CHUNK;
    if (S * D > INT32_MAX / nch / (k + 1)) return (int)hipErrorInvalidValue;     // grid limit
    const CfWork ws{agg1, car1, aggc, carc, e2};
    const dim3 block(CF_CHUNK), pgrid((unsigned)((S * N + CF_CHUNK - 1) / CF_CHUNK));
    int rc = cf_sdar(x, S * D, N, k, r1, loss1, pw1, ws, D > 1 ? score : outlier, stream);
    if (rc != 0) return rc;
    if (D > 1) hipLaunchKernelGGL(cf_sum_dims, pgrid, block, 0, stream, score, S, D, N, outlier);
    hipLaunchKernelGGL(cf_window_mean, pgrid, block, 0, stream, outlier, S, N, T1, y);
    HM_LAUNCH_RET_IF_ERR();
    rc = cf_sdar(y, S, N, k, r2, loss2, pw2, ws, score, stream);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(cf_window_mean, pgrid, block, 0, stream, score, S, N, T2, changepoint);
    HM_LAUNCH_RET();
}
