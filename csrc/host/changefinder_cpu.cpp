// CPU twin of csrc/kernels/changefinder.hip (hm_changefinder): the same contract, sequential in t
// and in the operation order of the Python path (anomaly.SDAR1D.update, anomaly._levinson,
// ChangeFinder.step), numpy's pairwise summation inside the window means included.  OpenMP over
// the S * D rows in stage 1 and over the S series in stage 2.  Used for CPU tensors and as the
// kernel's oracle in the tests; the kernel differs from it by the order of the additions inside a
// scan and by FMA contraction.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

#define HM_API extern "C" __attribute__((visibility("default")))

namespace {
constexpr int K_MAX = 32;
constexpr int T_MAX = 1024;

// anomaly._levinson: w[0..k) from C[0..k].
void levinson(const double* C, int k, double* w) {
    double nw[K_MAX];
    for (int j = 0; j < k; ++j) w[j] = 0.0;
    if (C[0] <= 0) return;
    double e = C[0];
    for (int i = 0; i < k; ++i) {
        double s = 0.0;
        for (int j = 0; j < i; ++j) s += w[j] * C[i - j];
        const double acc = C[i + 1] - s;
        double kappa = e > 0 ? acc / e : 0.0;
        kappa = std::max(-0.999, std::min(0.999, kappa));
        for (int j = 0; j < i; ++j) nw[j] = w[j] - kappa * w[i - 1 - j];
        for (int j = 0; j < i; ++j) w[j] = nw[j];
        w[i] = kappa;
        e *= (1 - kappa * kappa);
    }
}

// One SDAR1D over x[0..N): score[t] is what update(x[t], loss) returns.
void sdar(const double* x, int64_t N, int k, double r, int loss, double* score) {
    double C[K_MAX + 1] = {0.0}, w[K_MAX];
    const double a = 1 - r;
    double mu = 0.0, sigma = 0.0;
    for (int64_t t = 0; t < N; ++t) {
        const double xt = x[t];
        if (t == 0) {
            mu = xt;
            sigma = 1e-6;
        }
        mu = a * mu + r * xt;
        for (int j = 0; j <= k; ++j) {
            const double xj = t >= j ? x[t - j] : mu;
            C[j] = a * C[j] + r * (xt - mu) * (xj - mu);
        }
        levinson(C, k, w);
        double s = 0.0;
        for (int i = 0; i < k; ++i) s += w[i] * ((t >= i + 1 ? x[t - 1 - i] : mu) - mu);
        const double xhat = mu + s;
        const double prev = sigma;
        const double dd = (xt - xhat) * (xt - xhat);
        sigma = a * sigma + r * dd;
        const double s2 = std::max(sigma, 1e-12);
        if (loss == 1) {
            score[t] = 0.5 * std::log(2 * M_PI * s2) + dd / (2 * s2);
        } else {
            const double s1 = std::max(prev, 1e-12);
            const double bc = std::sqrt(2 * std::sqrt(s1 * s2) / (s1 + s2));
            score[t] = std::max(0.0, 2.0 - 2.0 * bc * std::exp(-dd / (4 * (s1 + s2))));
        }
    }
}

// numpy's pairwise sum of a contiguous fp64 run (what numpy.mean adds up).
double pairwise_sum(const double* a, int n) {
    if (n < 8) {
        double res = 0.0;
        for (int i = 0; i < n; ++i) res += a[i];
        return res;
    }
    if (n <= 128) {
        double r[8];
        for (int j = 0; j < 8; ++j) r[j] = a[j];
        int i = 8;
        for (; i < n - n % 8; i += 8)
            for (int j = 0; j < 8; ++j) r[j] += a[i + j];
        double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) res += a[i];
        return res;
    }
    int n2 = n / 2;
    n2 -= n2 % 8;
    return pairwise_sum(a, n2) + pairwise_sum(a + n2, n - n2);
}

// out_t = numpy.mean(in[max(0, t - T + 1) .. t]) per row of in, out [S, N].
void window_mean(const double* in, int64_t S, int64_t N, int T, double* out) {
#pragma omp parallel for schedule(static) collapse(2)
    for (int64_t s = 0; s < S; ++s)
        for (int64_t t = 0; t < N; ++t) {
            const int n = (int)std::min<int64_t>(T, t + 1);
            out[s * N + t] = pairwise_sum(in + s * N + t - n + 1, n) / (double)n;
        }
}
}  // namespace

// The arguments of hm_changefinder without the stream.  pw1, pw2, agg1, car1, aggc, carc and e2
// are the kernel's scan workspace and are not read here (they may be NULL).
HM_API int hm_changefinder_cpu(const double* x, int64_t S, int64_t D, int64_t N, int k, double r1,
                               double r2, int T1, int T2, int loss1, int loss2, const double* pw1,
                               const double* pw2, double* agg1, double* car1, double* aggc,
                               double* carc, double* e2, double* score, double* y, double* outlier,
                               double* changepoint) {
    (void)pw1, (void)pw2, (void)agg1, (void)car1, (void)aggc, (void)carc, (void)e2;
    if (S < 0 || D < 0 || N < 0 || k < 1 || k > K_MAX || !(r1 > 0.0 && r1 < 1.0) ||
        !(r2 > 0.0 && r2 < 1.0) || T1 < 1 || T1 > T_MAX || T2 < 1 || T2 > T_MAX || loss1 < 0 ||
        loss1 > 1 || loss2 < 0 || loss2 > 1)
        return 1;
    if (S == 0 || D == 0 || N == 0) return 0;
#pragma omp parallel for schedule(dynamic, 1)
    for (int64_t row = 0; row < S * D; ++row) sdar(x + row * N, N, k, r1, loss1, score + row * N);
#pragma omp parallel for schedule(static) collapse(2)
    for (int64_t s = 0; s < S; ++s)
        for (int64_t t = 0; t < N; ++t) {
            double o = 0.0;
            for (int64_t d = 0; d < D; ++d) o += score[(s * D + d) * N + t];
            outlier[s * N + t] = o;
        }
    window_mean(outlier, S, N, T1, y);
#pragma omp parallel for schedule(dynamic, 1)
    for (int64_t s = 0; s < S; ++s) sdar(y + s * N, N, k, r2, loss2, score + s * N);
    window_mean(score, S, N, T2, changepoint);
    return 0;
}
