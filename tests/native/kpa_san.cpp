// The kpa twin (csrc/host/kpa_cpu.cpp) in a program of its own, to be built with
// -fsanitize=address,undefined: every buffer is a heap allocation of the exact size, so a read or
// write past a row, the table, the slot list or a weight vector is reported.  The fixed input: rows
// of 0, 1, 2, 5 and 128 entries, the table built in three chunks at the smallest capacity with a load
// factor <= 0.5, two epochs, scoring with names and pairs the model never saw.  The weights are
// checked against a std::map learner of this file's own, written in the same order of operations.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <numeric>
#include <random>
#include <utility>
#include <vector>

extern "C" int hm_kpa_table_cpu(const int64_t* ptr, const int32_t* ids, const int64_t* pair_base, int64_t row0,
                                int64_t row1, int64_t n_occ, int64_t* keys, uint64_t* first, int64_t cap_mask,
                                int32_t* occ, int* full);
extern "C" int hm_kpa_train_cpu(const int64_t* ptr, const int32_t* ids, const double* vals, const double* y,
                                const int64_t* pair_base, const int32_t* occ, int64_t n_rows, int iters, double c,
                                double pkc, double s0, double s1, double s2, double* w0, double* w1, double* w2,
                                double* w3);
extern "C" int hm_kpa_score_cpu(const int64_t* ptr, const int32_t* ids, const double* vals, int64_t n_rows,
                                const int64_t* keys, const int32_t* remap, int64_t cap_mask, const double* w0,
                                const double* w1, const double* w2, const double* w3, double s0, double s1,
                                double s2, double* out);

namespace {

int failures = 0;

void expect(bool ok, const char* what, int64_t at) {
    if (!ok && ++failures <= 20) std::printf("FAIL %s at %lld\n", what, (long long)at);
}

bool same(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }

}  // namespace

int main() {
    std::mt19937_64 rng(20261126);
    std::uniform_real_distribution<double> val(-2.0, 2.0);
    const int F = 140;
    const std::vector<int> lens = {5, 0, 1, 2, 128, 5, 5, 2, 128, 5};
    std::vector<int64_t> ptr{0}, base{0};
    std::vector<int32_t> ids;
    std::vector<double> vals, y;
    for (int len : lens) {
        std::vector<int32_t> pool(F);
        std::iota(pool.begin(), pool.end(), 0);
        std::shuffle(pool.begin(), pool.end(), rng);
        for (int e = 0; e < len; ++e) {
            ids.push_back(pool[e]);
            vals.push_back(val(rng));
        }
        ptr.push_back((int64_t)ids.size());
        base.push_back(base.back() + (int64_t)len * (len - 1) / 2);
        y.push_back(rng() & 1 ? 1.0 : -1.0);
    }
    const int64_t R = (int64_t)lens.size(), n_occ = base.back();
    const double c = 0.05, pkc = 0.5, s0 = pkc, s1 = std::sqrt(2 * pkc), s2 = std::sqrt(2.0);
    const int iters = 2;
    volatile double two = 2.0, four = 4.0;         // the C library's pow, not products the compiler chose

    // the learner over std::map, which also counts the distinct pairs
    double r0 = 0.0;
    std::vector<double> r1(F, 0.0), r2(F, 0.0);
    std::map<std::pair<int32_t, int32_t>, double> r3;
    for (int it = 0; it < iters; ++it)
        for (int64_t r = 0; r < R; ++r) {
            const int64_t e0 = ptr[r], n = ptr[r + 1] - e0;
            volatile double p = r0 * s0, sq = s0 * s0, t, u;
            for (int64_t e = 0; e < n; ++e) {
                const double x = vals[e0 + e];
                t = r1[ids[e0 + e]] * s1 * x;
                u = r2[ids[e0 + e]] * x * x;
                t = t + u;
                p = p + t;
                t = 2.0 * pkc * x * x;
                u = std::pow(std::fabs(x), four);
                t = t + u;
                sq = sq + t;
            }
            for (int64_t a = 0; a < n; ++a)
                for (int64_t b = a + 1; b < n; ++b) {
                    const double xh = vals[e0 + a], xk = vals[e0 + b];
                    t = r3[{ids[e0 + a], ids[e0 + b]}] * s2 * xh * xk;
                    p = p + t;
                    t = xh * xk;
                    t = 2.0 * std::pow(std::fabs(t), two);
                    sq = sq + t;
                }
            t = y[r] * p;
            const double loss = std::max(0.0, 1.0 - t);
            if (loss <= 0.0) continue;
            const double eta = std::min(c, loss / sq) * y[r];
            t = eta * s0;
            r0 = r0 + t;
            for (int64_t e = 0; e < n; ++e) {
                const double x = vals[e0 + e];
                t = eta * s1 * x;
                r1[ids[e0 + e]] += t;
                t = eta * x * x;
                r2[ids[e0 + e]] += t;
            }
            for (int64_t a = 0; a < n; ++a)
                for (int64_t b = a + 1; b < n; ++b) {
                    t = eta * s2 * vals[e0 + a] * vals[e0 + b];
                    r3[{ids[e0 + a], ids[e0 + b]}] += t;
                }
        }
    const int64_t S = (int64_t)r3.size();
    int64_t cap = 2;
    while (cap < 2 * S) cap *= 2;

    // the table in three chunks, then the rank by first occurrence
    std::vector<int64_t> keys(cap, -1);
    std::vector<uint64_t> first(cap, UINT64_MAX);
    std::vector<int32_t> occ(n_occ, -7), remap(cap, -1);
    int full = 0;
    const int64_t cuts[4] = {0, 4, 5, R};
    for (int k = 0; k < 3; ++k)
        if (hm_kpa_table_cpu(ptr.data(), ids.data(), base.data(), cuts[k], cuts[k + 1], base[cuts[k + 1]] - base[cuts[k]],
                             keys.data(), first.data(), cap - 1, occ.data(), &full) != 0)
            ++failures;
    expect(full == 0, "table full", cap);
    std::vector<int64_t> used;
    for (int64_t h = 0; h < cap; ++h)
        if (keys[h] != -1) used.push_back(h);
    expect((int64_t)used.size() == S, "distinct pairs", (int64_t)used.size());
    std::sort(used.begin(), used.end(), [&](int64_t a, int64_t b) { return first[a] < first[b]; });
    for (int64_t s = 0; s < (int64_t)used.size(); ++s) remap[used[s]] = (int32_t)s;
    for (int64_t g = 0; g < n_occ; ++g) {
        expect(occ[g] >= 0 && occ[g] < cap, "slot", g);
        occ[g] = remap[occ[g]];
    }

    double w0 = 0.0;
    std::vector<double> w1(F, 0.0), w2(F, 0.0), w3(S, 0.0);
    if (hm_kpa_train_cpu(ptr.data(), ids.data(), vals.data(), y.data(), base.data(), occ.data(), R, iters, c, pkc, s0,
                         s1, s2, &w0, w1.data(), w2.data(), w3.data()) != 0)
        ++failures;
    expect(same(w0, r0), "w0", 0);
    for (int f = 0; f < F; ++f) expect(same(w1[f], r1[f]) && same(w2[f], r2[f]), "w1 / w2", f);
    for (int64_t s = 0; s < S; ++s) {
        const int64_t key = keys[used[s]];
        expect(same(w3[s], r3[{(int32_t)(key >> 32), (int32_t)(key & 0xFFFFFFFF)}]), "w3", s);
    }

    // scoring: the training rows with every third name unknown and the pairs reversed
    std::vector<int32_t> sids(ids.rbegin(), ids.rend());
    std::vector<double> svals(vals.rbegin(), vals.rend());
    std::vector<int64_t> sptr{0};
    for (auto it = lens.rbegin(); it != lens.rend(); ++it) sptr.push_back(sptr.back() + *it);
    for (size_t e = 0; e < sids.size(); e += 3) sids[e] = -1;
    std::vector<double> out(R, 7.5);
    if (hm_kpa_score_cpu(sptr.data(), sids.data(), svals.data(), R, keys.data(), remap.data(), cap - 1, &w0, w1.data(),
                         w2.data(), w3.data(), s0, s1, s2, out.data()) != 0)
        ++failures;
    for (int64_t r = 0; r < R; ++r) expect(std::isfinite(out[r]), "score", r);
    // a model without a pair
    if (hm_kpa_score_cpu(sptr.data(), sids.data(), svals.data(), R, nullptr, nullptr, 0, &w0, w1.data(), w2.data(),
                         nullptr, s0, s1, s2, out.data()) != 0)
        ++failures;
    // nothing at all
    if (hm_kpa_table_cpu(nullptr, nullptr, nullptr, 0, 0, 0, nullptr, nullptr, 0, nullptr, nullptr) != 0) ++failures;
    if (hm_kpa_train_cpu(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 1, c, pkc, s0, s1, s2, nullptr, nullptr,
                         nullptr, nullptr) != 0)
        ++failures;
    if (hm_kpa_score_cpu(nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, s0, s1,
                         s2, nullptr) != 0)
        ++failures;
    if (failures) {
        std::printf("kpa_san: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("kpa_san ok\n");
    return 0;
}
