// CPU twin of csrc/kernels/rank_eval.hip (hm_rank_eval / hm_rank_eval_idcg): the same contract,
// OpenMP over the rows, sequential inside one.
//
// Contract (docs/compat.md "Ranking-measures engine").  Row u holds a rank list (rank[u, 0..L'),
// best first, duplicates allowed; L' = min(lengths[u] or L, k or L)) and a truth slice
// (items[rowptr[u]..rowptr[u + 1]), sorted ascending and distinct).  The seven outputs are those of
// metrics.py's *_one functions and ranking_auc bit for bit: quotients of integers, and sums in
// list order of hits_upto_i / (i + 1) and of gain / log2(i + 2).  The logarithms and the binary
// ideal DCG are the caller's tables; nothing here computes one.
#include <omp.h>

#include <algorithm>
#include <cstdint>

#define HM_API extern "C" __attribute__((visibility("default")))

namespace {

constexpr int RE_LMAX = 1024;
enum { RE_PRECISION = 0, RE_RECALL, RE_HITRATE, RE_MRR, RE_AP, RE_NDCG, RE_AUC };

}  // namespace

// The arguments of hm_rank_eval (rank_eval.hip) without the stream.
HM_API int hm_rank_eval_cpu(const int64_t* rank, const int32_t* lengths, const int64_t* rowptr,
                            const int64_t* items, const double* gain, const double* idcg,
                            const double* log2tab, const double* ideal, int64_t tab_n, int64_t U,
                            int L, int k, int measures, double* out) {
    if (U <= 0) return 0;
    if (L < 1 || L > RE_LMAX || k < 0 || tab_n <= L || (gain == nullptr) != (idcg == nullptr)) return 1;
    const bool want_ap = measures & (1 << RE_AP), want_dcg = measures & (1 << RE_NDCG);
#pragma omp parallel for schedule(static, 256)
    for (int64_t row = 0; row < U; ++row) {
        int Lp = lengths ? std::min(std::max(lengths[row], 0), L) : L;
        if (k > 0) Lp = std::min(Lp, k);
        const int64_t t0 = rowptr[row], t1 = rowptr[row + 1], n_gt = t1 - t0;
        const int64_t* r = rank + row * L;
        int64_t hits = 0, first = -1, misses = 0, miss_sum = 0;    // miss_sum: misses before, over the hits
        double s_ap = 0.0, s_dcg = 0.0;
        for (int i = 0; i < Lp; ++i) {
            const int64_t* at = std::lower_bound(items + t0, items + t1, r[i]);
            if (at == items + t1 || *at != r[i]) {
                ++misses;
                continue;
            }
            ++hits;
            if (first < 0) first = i;
            miss_sum += misses;
            if (want_ap) s_ap += (double)hits / (double)(i + 1);
            if (want_dcg) s_dcg += (gain ? gain[at - items] : 1.0) / log2tab[std::min<int64_t>(i, tab_n - 1)];
        }
        double v[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (Lp) v[RE_PRECISION] = (double)hits / (double)Lp;
        if (n_gt) v[RE_RECALL] = (double)hits / (double)n_gt;
        v[RE_HITRATE] = hits ? 1.0 : 0.0;
        if (first >= 0) v[RE_MRR] = 1.0 / (double)(first + 1);
        if (n_gt) v[RE_AP] = s_ap / (double)(k > 0 ? std::min<int64_t>(n_gt, k) : n_gt);
        const int64_t mm = k > 0 ? std::min<int64_t>(n_gt, Lp) : n_gt;
        double id = 0.0;
        if (mm > 0) id = gain ? idcg[t0 + mm - 1] : ideal[std::min(mm, tab_n - 1)];
        if (id > 0.0) v[RE_NDCG] = s_dcg / id;
        const int64_t n_pos = hits, n_neg = Lp - hits;
        if (n_pos == 0) v[RE_AUC] = 0.0;
        else if (n_neg == 0) v[RE_AUC] = 1.0;
        else v[RE_AUC] = (double)(n_pos * n_neg - miss_sum) / (double)(n_pos * n_neg);
        for (int m = 0; m < 7; ++m)
            if ((measures >> m) & 1) out[(int64_t)m * U + row] = v[m];
    }
    return 0;
}

// The arguments of hm_rank_eval_idcg (rank_eval.hip) without the stream.
HM_API int hm_rank_eval_idcg_cpu(const int64_t* rowptr, const double* gain_desc, const double* log2tab,
                                 int64_t tab_n, int64_t U, double* idcg) {
    if (U <= 0) return 0;
    if (tab_n < 1) return 1;
#pragma omp parallel for schedule(static, 256)
    for (int64_t row = 0; row < U; ++row) {
        const int64_t t0 = rowptr[row], t1 = rowptr[row + 1];
        double s = 0.0;
        for (int64_t p = t0; p < t1; ++p) {
            s += gain_desc[p] / log2tab[std::min(p - t0, tab_n - 1)];
            idcg[p] = s;
        }
    }
    return 0;
}
