// CPU twin of csrc/kernels/auc.hip: the same contract (docs/compat.md "AUC engine"), OpenMP over
// the groups.  Per group it sorts the (key, class) pairs of the rows that count and walks the tie
// runs: a run with p positives and q negatives after b negatives adds p * (2 * b + q) to 2U.
// Integers only, so kernel and twin agree exactly.
#include <omp.h>

#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "../kernels/auc_key.h"

#define HM_API extern "C" __attribute__((visibility("default")))

// The arguments of hm_auc_prepare (auc.hip) without the prepared arrays and the stream, then
// rowptr int64 [G + 1] over the N rows in group order and the outputs int64 [G].
HM_API int hm_auc_groups_cpu(const void* scores, int score_kind, const void* labels, int label_kind, int64_t n,
                             const int64_t* order, int64_t N, const int64_t* rowptr, int64_t G,
                             int64_t* two_u, int64_t* n_pos, int64_t* n_neg) {
    if (G <= 0) return 0;
    if (score_kind < AUC_F64 || score_kind > AUC_F32 || label_kind < AUC_F64 || label_kind > AUC_I32 ||
        n < 0 || N < 0 || (!order && N != n))
        return 1;
#pragma omp parallel
    {
        std::vector<std::pair<int64_t, int>> rows;
#pragma omp for schedule(dynamic, 64)
        for (int64_t g = 0; g < G; ++g) {
            rows.clear();
            for (int64_t p = rowptr[g]; p < rowptr[g + 1]; ++p) {
                int64_t key;
                const int c = auc_row(scores, score_kind, labels, label_kind, n, order ? order[p] : p, &key);
                if (c != AUC_ABSENT) rows.emplace_back(key, c);
            }
            std::sort(rows.begin(), rows.end());
            int64_t u2 = 0, pos = 0, neg = 0;
            for (size_t i = 0; i < rows.size();) {
                int64_t p = 0, q = 0;
                size_t j = i;
                for (; j < rows.size() && rows[j].first == rows[i].first; ++j) (rows[j].second == AUC_POS ? p : q) += 1;
                u2 += p * (2 * neg + q);
                pos += p;
                neg += q;
                i = j;
            }
            two_u[g] = u2;
            n_pos[g] = pos;
            n_neg[g] = neg;
        }
    }
    return 0;
}
