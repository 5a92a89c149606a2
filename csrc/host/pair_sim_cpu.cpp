// CPU twin of csrc/kernels/pair_sim.hip (hm_pair_sim / hm_pair_sim_sq): the same contract, OpenMP
// over the pairs, sequential inside one.
//
// Contract (docs/compat.md "Pair-similarity engine").  List l holds ids / vals in entry order
// (distinct ids) and the same entries ascending by id (sids / svals).  For a pair (A, B):
//   DOT    over A's entries in entry order that also occur in B:  s = s + a * b
//   SQ     over A's entries in entry order: d = a - b (b = 0.0 on a miss), s = s + d * d; then over
//          B's entries in entry order that do not occur in A:  s = s + v * v
//   ABS    the walk of SQ with |d| and |v|
//   INTER  the number of common ids
// Every product rounds before its add (no fused multiply-add), as in the kernel.
#include <omp.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif

#define HM_API extern "C" __attribute__((visibility("default")))

namespace {

enum { PS_DOT = 0, PS_SQ, PS_ABS, PS_INTER, PS_NPRIM };

// The position of `id` in the ascending slice keys[lo..hi), or -1.
inline int64_t ps_find(const int32_t* keys, int64_t lo, int64_t hi, int32_t id) {
    const int32_t* at = std::lower_bound(keys + lo, keys + hi, id);
    return at != keys + hi && *at == id ? at - keys : -1;
}

}  // namespace

// The arguments of hm_pair_sim (pair_sim.hip) without the stream.
HM_API int hm_pair_sim_cpu(const int64_t* ptr, const int32_t* ids, const double* vals, const int32_t* sids,
                           const double* svals, const int32_t* ia, const int32_t* ib, int64_t P, int64_t M,
                           int64_t max_len, int mask, double* out) {
    if (P <= 0 || !(mask & ((1 << PS_NPRIM) - 1))) return 0;
    if (M < 0 || max_len < 0 || (M > 0 && P % M != 0)) return 1;
    const bool want_walk = mask & ((1 << PS_SQ) | (1 << PS_ABS));
#pragma omp parallel for schedule(static, 256)
    for (int64_t p = 0; p < P; ++p) {
        const int64_t la = M > 0 ? ia[p / M] : ia[p], lb = M > 0 ? ib[p % M] : ib[p];
        const int64_t a0 = ptr[la], a1 = ptr[la + 1], b0 = ptr[lb], b1 = ptr[lb + 1];
        int64_t inter = 0;
        double s_dot = 0.0, s_sq = 0.0, s_abs = 0.0;
        for (int64_t e = a0; e < a1; ++e) {
            const int64_t at = ps_find(sids, b0, b1, ids[e]);
            const double a = vals[e], b = at >= 0 ? svals[at] : 0.0;
            const double d = a - b;
            if (at >= 0) {
                ++inter;
                const double t = a * b;
                s_dot = s_dot + t;
            }
            const double t = d * d;
            s_sq = s_sq + t;
            s_abs = s_abs + std::fabs(d);
        }
        if (want_walk)
            for (int64_t e = b0; e < b1; ++e) {
                if (ps_find(sids, a0, a1, ids[e]) >= 0) continue;
                const double v = vals[e];
                const double t = v * v;
                s_sq = s_sq + t;
                s_abs = s_abs + std::fabs(v);
            }
        const double v[PS_NPRIM] = {s_dot, s_sq, s_abs, (double)inter};
        for (int m = 0; m < PS_NPRIM; ++m)
            if ((mask >> m) & 1) out[(int64_t)m * P + p] = v[m];
    }
    return 0;
}

// The arguments of hm_pair_sim_sq (pair_sim.hip) without the stream.
HM_API int hm_pair_sim_sq_cpu(const int64_t* ptr, const double* vals, int64_t n, double* sq) {
#pragma omp parallel for schedule(static, 256)
    for (int64_t l = 0; l < n; ++l) {
        double s = 0.0;
        for (int64_t e = ptr[l]; e < ptr[l + 1]; ++e) {
            const double t = vals[e] * vals[e];
            s = s + t;
        }
        sq[l] = s;
    }
    return 0;
}
