// CPU twin of csrc/kernels/sst.hip (hm_sst_scores): the same contract, the same one-sided Jacobi
// (plain row-cyclic pair order, a / b / c recomputed per pair, the same skip thresholds and the
// cap of 30 sweeps), the same ranking and rank cut of the singular vectors.  OpenMP over points.
// It differs from the kernel in the order of the additions inside a dot (sequential here, a tree
// over the lanes there) and in FMA contraction outside the dots.  Used for CPU tensors and as the
// kernel's twin in the tests.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#define HM_API extern "C" __attribute__((visibility("default")))

namespace {
constexpr int DIM_MAX = 64;
constexpr int SWEEP_CAP = 30;
constexpr double EPS = 2.220446049250313e-16;      // 2^-52

inline double dot(const double* a, const double* b, int n) {
    double s = 0.0;
    for (int l = 0; l < n; ++l) s += a[l] * b[l];
    return s;
}

// One-sided Jacobi on the rows x cols column-major matrix A; the sweeps done, 31 at the cap.
int jacobi(double* A, int rows, int cols) {
    double f = 0.0;
    for (int j = 0; j < cols; ++j) f += dot(A + j * rows, A + j * rows, rows);
    const double tn = (double)std::max(rows, cols) * EPS * std::sqrt(f);
    const double null2 = tn * tn;
    const double ctol = (double)rows * EPS;
    int sweeps = 0;
    for (;;) {
        ++sweeps;
        bool rotated = false;
        for (int p = 0; p + 1 < cols; ++p) {
            double* Ap = A + p * rows;
            for (int q = p + 1; q < cols; ++q) {
                double* Aq = A + q * rows;
                const double a = dot(Ap, Ap, rows), b = dot(Aq, Aq, rows), c = dot(Ap, Aq, rows);
                if (a <= null2 || b <= null2) continue;
                if (std::fabs(c) <= ctol * std::sqrt(a * b)) continue;
                const double z = (b - a) / (2.0 * c);
                const double t = z == 0.0 ? 1.0
                                          : std::copysign(1.0, z) / (std::fabs(z) + std::sqrt(1.0 + z * z));
                const double cs = 1.0 / std::sqrt(1.0 + t * t);
                const double sn = cs * t;
                for (int l = 0; l < rows; ++l) {
                    const double vp = Ap[l], vq = Aq[l];
                    Ap[l] = cs * vp - sn * vq;
                    Aq[l] = sn * vp + cs * vq;
                }
                rotated = true;
            }
        }
        if (!rotated) break;
        if (sweeps == SWEEP_CAP) { sweeps = SWEEP_CAP + 1; break; }
    }
    return sweeps;
}

// A[l, i] = x[i + l] (rows x cols, column-major), scaled by the power of two that brings the
// largest |entry| into [0.5, 1): exact, the score does not depend on it, and no square over- or
// underflows.
void hankel(const double* x, int rows, int cols, double* A) {
    double big = 0.0;
    for (int t = 0; t < rows + cols - 1; ++t) big = std::max(big, std::fabs(x[t]));
    int ex = 0;
    std::frexp(big, &ex);
    for (int i = 0; i < cols; ++i)
        for (int l = 0; l < rows; ++l) A[(size_t)l + (size_t)i * rows] = std::ldexp(x[i + l], -ex);
}

// The kept columns of the converged A by "norm descending, then index ascending": at most `want`
// of them, each with sigma > max(rows, cols) * eps * sigma_1.  ord / isg by rank; the count.
int leading(const double* A, int rows, int cols, int want, int* ord, double* isg) {
    double nrm[DIM_MAX];
    double top = 0.0;
    for (int j = 0; j < cols; ++j) {
        nrm[j] = dot(A + j * rows, A + j * rows, rows);
        top = std::max(top, nrm[j]);
    }
    const double cut = (double)std::max(rows, cols) * EPS * std::sqrt(top);
    int kept = 0;
    for (int j = 0; j < cols; ++j) {
        int rank = 0;
        for (int i = 0; i < cols; ++i) rank += (nrm[i] > nrm[j] || (nrm[i] == nrm[j] && i < j)) ? 1 : 0;
        const double sigma = std::sqrt(nrm[j]);
        if (rank < want && sigma > cut) {
            ord[rank] = j;
            isg[rank] = 1.0 / sigma;
            ++kept;
        }
    }
    return kept;
}
}  // namespace

HM_API int hm_sst_scores_cpu(const double* x, int64_t S, int64_t N, int w, int n, int m, int g, int r,
                             int k, double* out, int32_t* sweeps) {
    if (w < 2 || w > DIM_MAX || n < 1 || n > DIM_MAX || m < 1 || m > DIM_MAX || r < 1 || k < 1 ||
        g > m || S < 0 || N < 0)
        return 1;
    if (S == 0 || N == 0) return 0;
    const int64_t need = (int64_t)w + n + (g < 0 ? -(int64_t)g : 0) + m;
    const int kr = std::min(r, std::min(w, n)), kk = std::min(k, std::min(w, m));
    const int64_t pre = std::min<int64_t>(need - 1, N);
    for (int64_t s = 0; s < S; ++s)
        for (int64_t t = 0; t < pre; ++t) {
            out[s * N + t] = 0.0;
            if (sweeps) sweeps[s * N + t] = 0;
        }
    if (N < need) return 0;
    const int64_t per = N - need + 1;
#pragma omp parallel
    {
        std::vector<double> P((size_t)w * n), Q((size_t)w * m), M((size_t)kr * kk), U((size_t)w), V((size_t)w);
        int ordP[DIM_MAX], ordQ[DIM_MAX];
        double isgP[DIM_MAX], isgQ[DIM_MAX];
#pragma omp for schedule(dynamic, 16)
        for (int64_t pt = 0; pt < S * per; ++pt) {
            const int64_t s = pt / per, end = pt % per + need;
            const double* xs = x + s * N;
            const int64_t bp = end + g - m - n - w + 1, bq = end - m - w + 1;
            hankel(xs + bp, w, n, P.data());
            hankel(xs + bq, w, m, Q.data());
            int sw = std::max(jacobi(P.data(), w, n), jacobi(Q.data(), w, m));
            const int nu = leading(P.data(), w, n, kr, ordP, isgP);
            const int nq = leading(Q.data(), w, m, kk, ordQ, isgQ);
            double score;
            if (nu == 0 || nq == 0) {
                score = nu == nq ? 0.0 : 1.0;
            } else {
                const bool flip = nq > nu;
                const int mrows = flip ? nq : nu, mcols = flip ? nu : nq;
                for (int i = 0; i < nu; ++i) {
                    for (int l = 0; l < w; ++l) U[l] = P[(size_t)l + (size_t)ordP[i] * w] * isgP[i];
                    for (int j = 0; j < nq; ++j) {
                        for (int l = 0; l < w; ++l) V[l] = Q[(size_t)l + (size_t)ordQ[j] * w] * isgQ[j];
                        M[flip ? j + i * mrows : i + j * mrows] = dot(U.data(), V.data(), w);
                    }
                }
                sw = std::max(sw, jacobi(M.data(), mrows, mcols));
                double best = 0.0;
                for (int j = 0; j < mcols; ++j)
                    best = std::max(best, dot(M.data() + j * mrows, M.data() + j * mrows, mrows));
                score = std::min(std::max(1.0 - best, 0.0), 1.0);
            }
            out[s * N + end - 1] = score;
            if (sweeps) sweeps[s * N + end - 1] = sw;
        }
    }
    return 0;
}
