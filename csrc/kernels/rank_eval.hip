// Per-row ranking measures on gfx950: the engine behind evaluation.ranking_measures_batch and the
// grouped forms of precision_at, recall_at, hitrate, mrr, average_precision, ndcg and auc(array).
//
// Row u holds a rank list (rank[u, 0..L'), best first, duplicates allowed) and a truth slice
// (items[rowptr[u]..rowptr[u + 1]), sorted ascending and distinct).  The seven outputs are those
// of hivemall_amd/evaluation/metrics.py's *_one functions and ranking_auc, bit for bit
// (docs/compat.md "Ranking-measures engine"): every value is a quotient of two integers, or a
// sum in list order of such quotients, or a sum in list order of gain / log2(i + 2).
//
//   hm_rank_eval       LPR lanes per row (8, 16, 32 or 64, from max L'), so a wave serves 64 / LPR
//                      rows.  A lane binary-searches its rank item in the row's truth slice; the
//                      integer parts (hits, first hit, hits up to i, the position sum behind AUC)
//                      come from the ballot of the hit lanes.  The two ordered sums walk the set
//                      bits of the row's hit mask from low to high and add the hit lane's own term,
//                      read with a lane read: never a tree.  Lists longer than 64 go in chunks of
//                      64 positions that carry the counts and the running sums.
//   hm_rank_eval_idcg  graded truth only, once per index: idcg[rowptr[u] + m - 1] = the sequential
//                      sum over the row's m largest gains of gain / log2(i + 2); one thread a row.
//
// log2(i + 2) and the binary ideal DCG are host tables (math.log2, sequential adds): the device
// computes no logarithm, and its value arithmetic is fp64 adds and divides only, so there is
// nothing for -ffp-contract to fuse.  No atomics; every output element has one writer.
//
// The C++ twin is csrc/host/rank_eval_cpu.cpp.
#include "common.h"

namespace {

constexpr int RE_THREADS = 256;
constexpr int RE_WAVES = RE_THREADS / HM_WAVE;
constexpr int RE_LMAX = 1024;
constexpr int RE_NMEAS = 7;
enum { RE_PRECISION = 0, RE_RECALL, RE_HITRATE, RE_MRR, RE_AP, RE_NDCG, RE_AUC };

template <int LPR>
__global__ __launch_bounds__(RE_THREADS) void re_kernel(
    const int64_t* __restrict__ rank, const int32_t* __restrict__ lengths,
    const int64_t* __restrict__ rowptr, const int64_t* __restrict__ items,
    const double* __restrict__ gain, const double* __restrict__ idcg,
    const double* __restrict__ log2tab, const double* __restrict__ ideal, int64_t tab_n, int64_t U,
    int L, int k, int measures, double* __restrict__ out) {
    constexpr int RPW = HM_WAVE / LPR;             // rows per wave
    const int lane = hm::lane_id();
    const int sub = lane / LPR, j = lane % LPR;
    const int64_t row = ((int64_t)blockIdx.x * RE_WAVES + hm::wave_id()) * RPW + sub;
    const bool live = row < U;                     // a tail wave holds fewer rows than slots

    int Lp = 0;
    int64_t t0 = 0, t1 = 0;
    if (live) {
        Lp = lengths ? min(max(lengths[row], 0), L) : L;
        if (k > 0) Lp = min(Lp, k);
        t0 = rowptr[row];
        t1 = rowptr[row + 1];
    }
    // LPR < 64: the launcher chose LPR >= max L', one chunk serves every row of the wave.
    // LPR == 64: the wave is one row, so the trip count is wave-uniform.
    const int n_chunks = LPR == HM_WAVE ? __builtin_amdgcn_readfirstlane((Lp + HM_WAVE - 1) / HM_WAVE) : 1;
    const bool want_ap = measures & (1 << RE_AP), want_dcg = measures & (1 << RE_NDCG);
    const bool walk = want_ap || want_dcg || (measures & (1 << RE_AUC));

    int hits = 0, first = -1;
    int64_t pos_sum = 0;                           // sum of the hit positions
    double s_ap = 0.0, s_dcg = 0.0;
    for (int c = 0; c < n_chunks; ++c) {
        const int base = c * LPR, i = base + j;
        bool hit = false;
        double g = 1.0;
        if (i < Lp) {
            const int64_t item = rank[row * L + i];
            int64_t lo = t0, hi = t1;
            while (lo < hi) {
                const int64_t mid = lo + ((hi - lo) >> 1);
                if (items[mid] < item) lo = mid + 1;
                else hi = mid;
            }
            if (lo < t1 && items[lo] == item) {
                hit = true;
                if (gain) g = gain[lo];
            }
        }
        const unsigned long long bal = __ballot(hit);
        unsigned long long m = bal;                // the row's lanes only
        if constexpr (LPR < HM_WAVE) m = (bal >> (sub * LPR)) & ((1ull << LPR) - 1ull);
        if (first < 0 && m) first = base + __builtin_ctzll(m);
        double t_ap = 0.0, t_dcg = 0.0;            // the hit lane's own terms
        if (hit) {
            const int upto = hits + __popcll(m & ((1ull << j) - 1ull)) + 1;
            if (want_ap) t_ap = (double)upto / (double)(i + 1);
            if (want_dcg) t_dcg = g / log2tab[min((int64_t)i, tab_n - 1)];
        }
        // The set bits of the row's mask, low to high.  The loop runs for the whole wave until the
        // row with the most hits is done, so every lane is active at the lane reads.
        unsigned long long w = walk ? m : 0ull;
        while (__ballot(w != 0ull)) {
            const int b = w ? __builtin_ctzll(w) : 0;
            const int src = sub * LPR + b;
            if (want_ap) {
                const double v = __shfl(t_ap, src, HM_WAVE);
                if (w) s_ap += v;
            }
            if (want_dcg) {
                const double v = __shfl(t_dcg, src, HM_WAVE);
                if (w) s_dcg += v;
            }
            if (w) pos_sum += base + b;
            w &= w - 1ull;
        }
        hits += __popcll(m);
    }

    if (!live || j >= RE_NMEAS || !((measures >> j) & 1)) return;
    const int64_t n_gt = t1 - t0;
    double v = 0.0;
    switch (j) {
    case RE_PRECISION:
        if (Lp) v = (double)hits / (double)Lp;
        break;
    case RE_RECALL:
        if (n_gt) v = (double)hits / (double)n_gt;
        break;
    case RE_HITRATE:
        v = hits ? 1.0 : 0.0;
        break;
    case RE_MRR:
        if (first >= 0) v = 1.0 / (double)(first + 1);
        break;
    case RE_AP:
        if (n_gt) v = s_ap / (double)(k > 0 ? min(n_gt, (int64_t)k) : n_gt);
        break;
    case RE_NDCG: {
        const int64_t mm = k > 0 ? min(n_gt, (int64_t)Lp) : n_gt;
        double id = 0.0;
        if (mm > 0) id = gain ? idcg[t0 + mm - 1] : ideal[min(mm, tab_n - 1)];
        if (id > 0.0) v = s_dcg / id;
        break;
    }
    default: {                                     // RE_AUC
        const int64_t n_pos = hits, n_neg = Lp - hits;
        if (n_pos == 0) v = 0.0;
        else if (n_neg == 0) v = 1.0;
        else {
            // sum over the hits of (n_neg - misses before) with misses before = position - hits before
            const int64_t correct = n_pos * n_neg - (pos_sum - n_pos * (n_pos - 1) / 2);
            v = (double)correct / (double)(n_pos * n_neg);
        }
    }
    }
    out[(int64_t)j * U + row] = v;
}

__global__ __launch_bounds__(RE_THREADS) void re_idcg_kernel(
    const int64_t* __restrict__ rowptr, const double* __restrict__ gain_desc,
    const double* __restrict__ log2tab, int64_t tab_n, int64_t U, double* __restrict__ idcg) {
    const int64_t row = (int64_t)blockIdx.x * RE_THREADS + threadIdx.x;
    if (row >= U) return;
    const int64_t t0 = rowptr[row], t1 = rowptr[row + 1];
    double s = 0.0;
    for (int64_t p = t0; p < t1; ++p) {
        s += gain_desc[p] / log2tab[min(p - t0, tab_n - 1)];
        idcg[p] = s;
    }
}

}  // namespace

// rank int64 [U, L]; lengths int32 [U] or NULL; rowptr int64 [U + 1]; items int64 [nnz] sorted
// and distinct inside a row; gain fp64 [nnz] and idcg fp64 [nnz] for graded truth, both NULL for
// binary; log2tab[i] = log2(i + 2) and ideal[m] = the binary ideal DCG of m items, tab_n entries
// each, tab_n > max(L, longest truth row); k = 0 for no cut; measures = bit mask of the rows of
// out fp64 [7, U] to fill.
HM_API int hm_rank_eval(const int64_t* rank, const int32_t* lengths, const int64_t* rowptr,
                        const int64_t* items, const double* gain, const double* idcg,
                        const double* log2tab, const double* ideal, int64_t tab_n, int64_t U, int L,
                        int k, int measures, double* out, hipStream_t stream) {
    if (U <= 0) return 0;
    if (L < 1 || L > RE_LMAX || k < 0 || tab_n <= L || (gain == nullptr) != (idcg == nullptr))
        return (int)hipErrorInvalidValue;
    const int max_lp = (k > 0 && k < L) ? k : L;
    const int lpr = max_lp <= 8 ? 8 : max_lp <= 16 ? 16 : max_lp <= 32 ? 32 : 64;
    const int64_t rows_per_block = (int64_t)RE_WAVES * (HM_WAVE / lpr);
    const int64_t grid = (U + rows_per_block - 1) / rows_per_block;
    if (grid > INT32_MAX) return (int)hipErrorInvalidValue;
#define RE_LAUNCH(LPR)                                                                                 \
    hipLaunchKernelGGL(re_kernel<LPR>, dim3((unsigned)grid), dim3(RE_THREADS), 0, stream, rank, lengths, \
                       rowptr, items, gain, idcg, log2tab, ideal, tab_n, U, L, k, measures, out)
    if (lpr == 8) RE_LAUNCH(8);
    else if (lpr == 16) RE_LAUNCH(16);
    else if (lpr == 32) RE_LAUNCH(32);
    else RE_LAUNCH(64);
#undef RE_LAUNCH
    HM_LAUNCH_RET();
}

// gain_desc fp64 [nnz]: every row's gains, largest first; tab_n > the longest row.
HM_API int hm_rank_eval_idcg(const int64_t* rowptr, const double* gain_desc, const double* log2tab,
                             int64_t tab_n, int64_t U, double* idcg, hipStream_t stream) {
    if (U <= 0) return 0;
    if (tab_n < 1) return (int)hipErrorInvalidValue;
    const int64_t grid = (U + RE_THREADS - 1) / RE_THREADS;
    if (grid > INT32_MAX) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(re_idcg_kernel, dim3((unsigned)grid), dim3(RE_THREADS), 0, stream, rowptr, gain_desc,
                       log2tab, tab_n, U, idcg);
    HM_LAUNCH_RET();
}
