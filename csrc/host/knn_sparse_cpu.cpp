// CPU twin of csrc/kernels/knn_sparse.hip (hm_knn_rnorm, hm_knn_cols): the same contract with
// one dense fp64 accumulator of `tile` candidate columns per thread and a sequential walk over
// the query column's users.  OpenMP over queries.  Used for CPU tensors and as the kernels' twin
// in the tests.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#define HM_API extern "C" __attribute__((visibility("default")))

namespace {
using Cand = std::pair<double, int32_t>;               // (score, column)

// score descending, then column id ascending
inline bool better(const Cand& a, const Cand& b) {
    return a.first > b.first || (a.first == b.first && a.second < b.second);
}
}  // namespace

HM_API int hm_knn_rnorm_cpu(const int64_t* colptr, const double* vals, int C, double* rnorm) {
    if (C <= 0) return 0;
#pragma omp parallel for schedule(static)
    for (int c = 0; c < C; ++c) {
        double acc = 0.0;
        for (int64_t p = colptr[c]; p < colptr[c + 1]; ++p) acc += vals[p] * vals[p];
        rnorm[c] = acc > 0.0 ? 1.0 / std::sqrt(acc) : 0.0;
    }
    return 0;
}

HM_API int hm_knn_cols_cpu(const int64_t* colptr, const int32_t* rows, const double* vals, int C,
                           const int64_t* rowptr, const int32_t* cols, const double* rvals,
                           const double* rnorm, const int32_t* query, int64_t n, int k, int tile,
                           int32_t* idx, double* score) {
    if (n <= 0) return 0;
    if (C <= 0 || k < 1 || k > 128 || tile < 1 || tile > 16384) return 1;
    const int T = std::min(C, tile);
#pragma omp parallel
    {
        std::vector<double> acc((size_t)T);
        std::vector<Cand> top;
        top.reserve((size_t)T + (size_t)k);
#pragma omp for schedule(dynamic, 4)
        for (int64_t q = 0; q < n; ++q) {
            const int i = query[q];
            const double rn_i = rnorm[i];
            top.clear();
            for (int j0 = 0; j0 < C; j0 += T) {
                const int tc = std::min(T, C - j0);
                std::fill(acc.begin(), acc.begin() + tc, 0.0);
                for (int64_t p = colptr[i]; p < colptr[i + 1]; ++p) {
                    const int32_t u = rows[p];
                    const double v = vals[p];
                    const int32_t* lo = cols + rowptr[u];
                    const int32_t* hi = cols + rowptr[u + 1];
                    if (j0 > 0) lo = std::lower_bound(lo, hi, j0);
                    if (j0 + tc < C) hi = std::lower_bound(lo, hi, j0 + tc);
                    for (const int32_t* e = lo; e < hi; ++e) acc[*e - j0] += v * rvals[e - cols];
                }
                for (int t = 0; t < tc; ++t) {
                    const int j = j0 + t;
                    if (acc[t] == 0.0 || j == i) continue;
                    const double s = (acc[t] * rn_i) * rnorm[j];
                    if (s == s) top.emplace_back(s, j);
                }
                if ((int)top.size() > k) {
                    std::partial_sort(top.begin(), top.begin() + k, top.end(), better);
                    top.resize((size_t)k);
                }
            }
            std::sort(top.begin(), top.end(), better);
            for (int r = 0; r < k; ++r) {
                const bool have = r < (int)top.size();
                idx[q * k + r] = have ? top[r].second : -1;
                score[q * k + r] = have ? top[r].first : 0.0;
            }
        }
    }
    return 0;
}
