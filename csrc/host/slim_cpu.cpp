// CPU engine for train_slim: the contracts of csrc/kernels/slim.hip (hm_slim_gram, hm_slim_cd)
// with a sorted merge of two rating columns and the scalar coordinate loop of upstream SlimUDTF
// in Gram form.  OpenMP over items.  Used for CPU sessions and as the oracle of the kernels.
#include <cmath>
#include <cstddef>
#include <cstdint>

#define HM_API extern "C" __attribute__((visibility("default")))

namespace {
double col_dot(const int32_t* rows, const double* vals, int64_t x, int64_t x1, int64_t y,
               int64_t y1) {
    double acc = 0.0;
    while (x < x1 && y < y1) {
        const int32_t u = rows[x], v = rows[y];
        if (u == v) acc += vals[x++] * vals[y++];
        else if (u < v) ++x;
        else ++y;
    }
    return acc;
}
}  // namespace

HM_API int hm_slim_gram_cpu(const int64_t* colptr, const int32_t* rows, const double* vals, int C,
                            const int32_t* target, const int32_t* nbr, int64_t n, int K, double* G,
                            double* b) {
    if (n <= 0 || K <= 0) return 0;
    if (C < 0) return 1;
#pragma omp parallel for schedule(dynamic, 16)
    for (int64_t t = 0; t < n; ++t) {
        const int32_t* nb = nbr + t * K;
        double* Gt = G + (size_t)t * K * K;
        double* bt = b + (size_t)t * K;
        const int tc = target[t];
        const bool t_ok = tc >= 0 && tc < C;
        for (int a = 0; a < K; ++a) {
            const int ia = nb[a];
            const bool a_ok = ia >= 0 && ia < C;
            for (int c = a; c < K; ++c) {
                const int ic = nb[c];
                double v = 0.0;
                if (a_ok && ic >= 0 && ic < C)
                    v = col_dot(rows, vals, colptr[ia], colptr[ia + 1], colptr[ic], colptr[ic + 1]);
                Gt[(size_t)a * K + c] = v;
                Gt[(size_t)c * K + a] = v;
            }
            bt[a] = a_ok && t_ok
                        ? col_dot(rows, vals, colptr[ia], colptr[ia + 1], colptr[tc], colptr[tc + 1])
                        : 0.0;
        }
    }
    return 0;
}

HM_API int hm_slim_cd_cpu(const double* G, const double* b, int64_t n, int K, double l1, double l2,
                          int iters, double eps, double* W) {
    if (n <= 0 || K <= 0) return 0;
#pragma omp parallel for schedule(dynamic, 16)
    for (int64_t t = 0; t < n; ++t) {
        const double* Gt = G + (size_t)t * K * K;
        const double* bt = b + (size_t)t * K;
        double* w = W + (size_t)t * K;
        for (int k = 0; k < K; ++k) w[k] = 0.0;
        for (int it = 0; it < iters; ++it) {
            double dmax = 0.0;
            for (int k = 0; k < K; ++k) {
                const double* row = Gt + (size_t)k * K;
                const double gkk = row[k];
                if (!(gkk > 0.0)) continue;
                double dot = 0.0;
                for (int m = 0; m < K; ++m) dot += row[m] * w[m];
                const double rho = bt[k] - dot + gkk * w[k];
                const double nw = std::fmax(rho - l1, 0.0) / (gkk + l2);
                dmax = std::fmax(dmax, std::fabs(nw - w[k]));
                w[k] = nw;
            }
            if (!(dmax >= eps)) break;
        }
    }
    return 0;
}
