// CPU engine for train_slim: the contracts of csrc/kernels/slim.hip (hm_slim_gram, hm_slim_cd)
// with a sorted merge of two rating columns and the scalar coordinate loop of upstream SlimUDTF
// in Gram form.  OpenMP over items.  Used for CPU sessions and as the oracle of the kernels.
//
// hm_slim_topk_cpu is the twin of csrc/kernels/slim_topk.hip (docs/compat.md "SLIM
// recommendation"): OpenMP over users, per user the candidates from the transposed model, every
// score as one sequential loop (products rounded before their adds), the same (key, item) order.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <limits>
#include <utility>
#include <vector>

#include "../kernels/slim_topk_key.h"      // st_key / st_unkey / st_better, shared with the kernel

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

// ------------------------------------------------------------------ hm_slim_topk_cpu
// Every product below rounds before its add, as in the kernel.
#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif

// The arguments of hm_slim_topk (slim_topk.hip) without the stream.
HM_API int hm_slim_topk_cpu(const int64_t* rowptr, const int32_t* cols, const double* vals, int64_t U,
                            const int64_t* mptr, const int32_t* mnn, const double* mw,
                            const int64_t* tptr, const int32_t* ti, int I, int k, int exclude,
                            int32_t* items, double* scores) {
    if (U <= 0) return 0;
    if (I < 0 || k < 1 || k > 256) return 1;
#pragma omp parallel
    {
        std::vector<uint8_t> mark((size_t)I, 0);
        std::vector<int32_t> cand;
        std::vector<std::pair<uint64_t, uint32_t>> best;
#pragma omp for schedule(dynamic, 16)
        for (int64_t u = 0; u < U; ++u) {
            const int64_t r0 = rowptr[u], r1 = rowptr[u + 1];
            const int32_t* rc = cols + r0;
            const double* rv = vals + r0;
            const int64_t nr = r1 - r0;
            cand.clear();
            best.clear();
            // mark: bit 0 = a candidate already, bit 1 = rated (most neighbours are not: one byte
            // read instead of a search)
            for (int64_t p = 0; p < nr; ++p)
                if ((uint32_t)rc[p] < (uint32_t)I) mark[rc[p]] = 2;
            for (int64_t p = 0; p < nr; ++p) {
                const int32_t c = rc[p];
                if ((uint32_t)c >= (uint32_t)I) continue;
                for (int64_t q = tptr[c]; q < tptr[c + 1]; ++q) {
                    const int32_t i = ti[q];
                    if ((uint32_t)i < (uint32_t)I && !(mark[i] & 1) && !(exclude && (mark[i] & 2))) {
                        mark[i] |= 1;
                        cand.push_back(i);
                    }
                }
            }
            for (const int32_t i : cand) {
                mark[i] &= 2;
                double acc = 0.0;
                const int32_t* from = rc;
                for (int64_t q = mptr[i]; q < mptr[i + 1] && from < rc + nr; ++q) {
                    if ((uint32_t)mnn[q] >= (uint32_t)I || !(mark[mnn[q]] & 2)) continue;
                    from = std::lower_bound(from, rc + nr, mnn[q]);
                    if (from < rc + nr && *from == mnn[q]) acc = acc + mw[q] * rv[from - rc];
                }
                best.emplace_back(st_key(acc), (uint32_t)i);
            }
            for (int64_t p = 0; p < nr; ++p)
                if ((uint32_t)rc[p] < (uint32_t)I) mark[rc[p]] = 0;
            const size_t n_out = std::min(best.size(), (size_t)k);
            std::partial_sort(best.begin(), best.begin() + n_out, best.end(),
                              [](const auto& x, const auto& y) {
                                  return st_better(x.first, x.second, y.first, y.second);
                              });
            for (int r = 0; r < k; ++r) {
                const bool in = (size_t)r < n_out;
                items[u * k + r] = in ? (int32_t)best[r].second : -1;
                scores[u * k + r] = in ? st_unkey(best[r].first) : -std::numeric_limits<double>::infinity();
            }
        }
    }
    return 0;
}
