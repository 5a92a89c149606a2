// CPU twin of csrc/kernels/kpa.hip (hm_kpa_table / hm_kpa_train / hm_kpa_score): the same three
// entry points for CPU tensors.
//
// Contract (docs/compat.md "KPA engine"; models/recommend.py KPA.fit and _kpa_score are the
// definition).  The trainer is the learner expression by expression, in its order of operations,
// sequential over rows, entries and pairs: the same fp64 weights bit for bit.  `x ** 4` and
// `(xh * xk) ** 2` are std::pow, as CPython's float power is the C library's pow(); every product
// rounds before its add (no fused multiply-add).  Table build and scoring are OpenMP over rows.
#include <omp.h>

#include <cmath>
#include <cstdint>

#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif

#define HM_API extern "C" __attribute__((visibility("default")))

namespace {

constexpr int64_t KPA_EMPTY = -1;

inline uint64_t kpa_mix64(uint64_t z) {            // hm::mix64 of common.h
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// The exponents of the learner's `**`.  CPython's float power is pow(fabs(x), e) of the C library
// for these; read through a volatile, the compiler cannot turn the call into products of its own.
const volatile double KPA_TWO = 2.0, KPA_FOUR = 4.0;

inline int64_t kpa_key(int32_t ia, int32_t ib) {
    return (int64_t)(((uint64_t)(uint32_t)ia << 32) | (uint32_t)ib);
}

}  // namespace

// The arguments of hm_kpa_table (kpa.hip) without the stream.
HM_API int hm_kpa_table_cpu(const int64_t* ptr, const int32_t* ids, const int64_t* pair_base, int64_t row0,
                            int64_t row1, int64_t n_occ, int64_t* keys, uint64_t* first, int64_t cap_mask,
                            int32_t* occ, int* full) {
    if (row1 <= row0 || n_occ <= 0) return 0;
    if (cap_mask < 0 || (cap_mask & (cap_mask + 1)) != 0 || cap_mask >= ((int64_t)1 << 31)) return 1;
#pragma omp parallel for schedule(dynamic, 16)
    for (int64_t r = row0; r < row1; ++r) {
        const int64_t e0 = ptr[r], n = ptr[r + 1] - e0;
        int64_t g = pair_base[r];
        for (int64_t a = 0; a < n; ++a)
            for (int64_t b = a + 1; b < n; ++b, ++g) {
                const int64_t key = kpa_key(ids[e0 + a], ids[e0 + b]);
                int64_t h = (int64_t)(kpa_mix64((uint64_t)key) & (uint64_t)cap_mask), at = -1;
                for (int64_t step = 0; step <= cap_mask; ++step) {
                    int64_t cur = __atomic_load_n(&keys[h], __ATOMIC_RELAXED);
                    if (cur == KPA_EMPTY) {
                        int64_t expected = KPA_EMPTY;
                        cur = __atomic_compare_exchange_n(&keys[h], &expected, key, false, __ATOMIC_RELAXED,
                                                          __ATOMIC_RELAXED)
                                  ? KPA_EMPTY
                                  : expected;
                    }
                    if (cur == KPA_EMPTY || cur == key) {
                        at = h;
                        break;
                    }
                    h = (h + 1) & cap_mask;
                }
                if (at < 0) {
                    __atomic_store_n(full, 1, __ATOMIC_RELAXED);
                    occ[g] = -1;
                    continue;
                }
                uint64_t seen = __atomic_load_n(&first[at], __ATOMIC_RELAXED);
                while ((uint64_t)g < seen &&
                       !__atomic_compare_exchange_n(&first[at], &seen, (uint64_t)g, true, __ATOMIC_RELAXED,
                                                    __ATOMIC_RELAXED)) {
                }
                occ[g] = (int32_t)at;
            }
    }
    return 0;
}

// The arguments of hm_kpa_train (kpa.hip) without the stream.
HM_API int hm_kpa_train_cpu(const int64_t* ptr, const int32_t* ids, const double* vals, const double* y,
                            const int64_t* pair_base, const int32_t* occ, int64_t n_rows, int iters, double c,
                            double pkc, double s0, double s1, double s2, double* w0p, double* w1, double* w2,
                            double* w3) {
    if (n_rows <= 0 || iters <= 0) return 0;
    double w0 = w0p[0];
    for (int it = 0; it < iters; ++it)
        for (int64_t r = 0; r < n_rows; ++r) {
            const int64_t e0 = ptr[r], n = ptr[r + 1] - e0;
            const int32_t* slot = occ + pair_base[r];
            const double yy = y[r];
            double p = w0 * s0;
            double sq = s0 * s0;
            for (int64_t e = 0; e < n; ++e) {
                const double x = vals[e0 + e];
                const int32_t h = ids[e0 + e];
                const double t1 = w1[h] * s1 * x, t2 = w2[h] * x * x;
                const double t = t1 + t2;
                p = p + t;
                const double u1 = 2.0 * pkc * x * x, u2 = std::pow(std::fabs(x), KPA_FOUR);
                const double u = u1 + u2;
                sq = sq + u;
            }
            int64_t g = 0;
            for (int64_t a = 0; a < n; ++a)
                for (int64_t b = a + 1; b < n; ++b, ++g) {
                    const double xh = vals[e0 + a], xk = vals[e0 + b];
                    const double t = w3[slot[g]] * s2 * xh * xk;
                    p = p + t;
                    const double pr = xh * xk;
                    const double u = 2.0 * std::pow(std::fabs(pr), KPA_TWO);
                    sq = sq + u;
                }
            const double margin = yy * p;
            const double gap = 1.0 - margin;
            const double loss = gap > 0.0 ? gap : 0.0;          // max(0.0, gap)
            if (loss <= 0.0) continue;
            const double q = loss / sq;
            const double eta = (q < c ? q : c) * yy;            // min(c, q) * y
            const double d0 = eta * s0;
            w0 = w0 + d0;
            for (int64_t e = 0; e < n; ++e) {
                const double x = vals[e0 + e];
                const int32_t h = ids[e0 + e];
                const double d1 = eta * s1 * x, d2 = eta * x * x;
                w1[h] = w1[h] + d1;
                w2[h] = w2[h] + d2;
            }
            g = 0;
            for (int64_t a = 0; a < n; ++a)
                for (int64_t b = a + 1; b < n; ++b, ++g) {
                    const double d3 = eta * s2 * vals[e0 + a] * vals[e0 + b];
                    w3[slot[g]] = w3[slot[g]] + d3;
                }
        }
    w0p[0] = w0;
    return 0;
}

// The arguments of hm_kpa_score (kpa.hip) without the stream.  Sequential inside a row, in
// _kpa_score's order.
HM_API int hm_kpa_score_cpu(const int64_t* ptr, const int32_t* ids, const double* vals, int64_t n_rows,
                            const int64_t* keys, const int32_t* remap, int64_t cap_mask, const double* w0,
                            const double* w1, const double* w2, const double* w3, double s0, double s1, double s2,
                            double* out) {
    if (n_rows <= 0) return 0;
    if (keys && (cap_mask < 0 || (cap_mask & (cap_mask + 1)) != 0)) return 1;
#pragma omp parallel for schedule(dynamic, 64)
    for (int64_t r = 0; r < n_rows; ++r) {
        const int64_t e0 = ptr[r], n = ptr[r + 1] - e0;
        double p = w0[0] * s0;
        for (int64_t e = 0; e < n; ++e) {
            const int32_t h = ids[e0 + e];
            const double x = vals[e0 + e];
            const double wa = h >= 0 ? w1[h] : 0.0, wb = h >= 0 ? w2[h] : 0.0;
            const double t1 = wa * s1 * x, t2 = wb * x * x;
            const double t = t1 + t2;
            p = p + t;
        }
        for (int64_t a = 0; a < n; ++a)
            for (int64_t b = a + 1; b < n; ++b) {
                const int32_t ia = ids[e0 + a], ib = ids[e0 + b];
                double w = 0.0;
                if (ia >= 0 && ib >= 0 && keys) {
                    const int64_t key = kpa_key(ia, ib);
                    int64_t h = (int64_t)(kpa_mix64((uint64_t)key) & (uint64_t)cap_mask);
                    for (int64_t step = 0; step <= cap_mask; ++step) {
                        const int64_t cur = keys[h];
                        if (cur == key) {
                            w = w3[remap[h]];
                            break;
                        }
                        if (cur == KPA_EMPTY) break;
                        h = (h + 1) & cap_mask;
                    }
                }
                const double t = w * s2 * vals[e0 + a] * vals[e0 + b];
                p = p + t;
            }
        out[r] = p;
    }
    return 0;
}
