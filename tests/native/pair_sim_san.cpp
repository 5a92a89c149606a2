// The pair-similarity twin (csrc/host/pair_sim_cpu.cpp) in a program of its own, to be built with
// -fsanitize=address,undefined: every buffer is a heap allocation of the exact size, so a read or
// write past a list, an index array or the output is reported.  The edge corpus: empty lists,
// lists of 1, 8, 9, 64, 65 and 129 entries; pair arrays of 0, 1 and 65 pairs; the cross form with
// an empty side; every primitive mask.  INTER and the walked sums are checked against plain loops
// of this file's own (a linear search, no sorted slice).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <random>
#include <vector>

extern "C" int hm_pair_sim_cpu(const int64_t* ptr, const int32_t* ids, const double* vals, const int32_t* sids,
                               const double* svals, const int32_t* ia, const int32_t* ib, int64_t P, int64_t M,
                               int64_t max_len, int mask, double* out);
extern "C" int hm_pair_sim_sq_cpu(const int64_t* ptr, const double* vals, int64_t n, double* sq);

namespace {

int failures = 0;

void expect(bool ok, const char* what, int64_t p, int mask) {
    if (!ok && ++failures <= 20) std::printf("FAIL %s: pair=%lld mask=%d\n", what, (long long)p, mask);
}

bool same(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }

struct Lists {
    std::vector<int64_t> ptr{0};
    std::vector<int32_t> ids, sids;
    std::vector<double> vals, svals;
    int64_t max_len = 0;
    int64_t n() const { return (int64_t)ptr.size() - 1; }
};

Lists make_lists(const std::vector<int>& lens, int vocab, std::mt19937_64& rng) {
    Lists L;
    std::uniform_real_distribution<double> val(-3.0, 3.0);
    for (int len : lens) {
        std::vector<int32_t> pool(std::max(vocab, len));
        std::iota(pool.begin(), pool.end(), 0);
        std::shuffle(pool.begin(), pool.end(), rng);
        const int64_t at = (int64_t)L.ids.size();
        for (int e = 0; e < len; ++e) {
            L.ids.push_back(pool[e]);
            L.vals.push_back(val(rng));
        }
        std::vector<int> order(len);
        std::iota(order.begin(), order.end(), 0);
        std::sort(order.begin(), order.end(), [&](int x, int y) { return L.ids[at + x] < L.ids[at + y]; });
        for (int o : order) {
            L.sids.push_back(L.ids[at + o]);
            L.svals.push_back(L.vals[at + o]);
        }
        L.ptr.push_back((int64_t)L.ids.size());
        L.max_len = std::max<int64_t>(L.max_len, len);
    }
    return L;
}

// the value of `id` in list l by linear search over the entry order
bool lookup(const Lists& L, int64_t l, int32_t id, double* v) {
    for (int64_t e = L.ptr[l]; e < L.ptr[l + 1]; ++e)
        if (L.ids[e] == id) {
            *v = L.vals[e];
            return true;
        }
    return false;
}

void reference(const Lists& L, int64_t la, int64_t lb, double want[4]) {
    double dot = 0.0, sq = 0.0, ab = 0.0;
    int64_t inter = 0;
    for (int64_t e = L.ptr[la]; e < L.ptr[la + 1]; ++e) {
        double b = 0.0;
        const bool hit = lookup(L, lb, L.ids[e], &b);
        if (hit) {
            ++inter;
            volatile double t = L.vals[e] * b;
            dot = dot + t;
        }
        const double d = L.vals[e] - b;
        volatile double t = d * d;
        sq = sq + t;
        ab = ab + std::fabs(d);
    }
    for (int64_t e = L.ptr[lb]; e < L.ptr[lb + 1]; ++e) {
        double a;
        if (lookup(L, la, L.ids[e], &a)) continue;
        volatile double t = L.vals[e] * L.vals[e];
        sq = sq + t;
        ab = ab + std::fabs(L.vals[e]);
    }
    want[0] = dot;
    want[1] = sq;
    want[2] = ab;
    want[3] = (double)inter;
}

void check(const Lists& L, const std::vector<int32_t>& ia, const std::vector<int32_t>& ib, int64_t M) {
    const int64_t P = M > 0 ? (int64_t)ia.size() * M : (int64_t)ia.size();
    for (int mask = 0; mask < 16; ++mask) {
        std::vector<double> out(4 * P, 7.5);
        if (hm_pair_sim_cpu(L.ptr.data(), L.ids.data(), L.vals.data(), L.sids.data(), L.svals.data(), ia.data(),
                            ib.data(), P, M, L.max_len, mask, out.data()) != 0)
            ++failures;
        for (int64_t p = 0; p < P; ++p) {
            double want[4];
            reference(L, M > 0 ? ia[p / M] : ia[p], M > 0 ? ib[p % M] : ib[p], want);
            for (int m = 0; m < 4; ++m)
                expect(same(out[m * P + p], (mask >> m) & 1 ? want[m] : 7.5), "plane", p, mask);
        }
    }
}

}  // namespace

int main() {
    std::mt19937_64 rng(20261021);
    for (int vocab : {5, 80}) {
        const std::vector<int> lens = {0, 1, 129, 0, 8, 9, 64, 65, 1, 33, 129, 7};
        const Lists L = make_lists(lens, vocab, rng);
        std::vector<double> sq(L.n());
        if (hm_pair_sim_sq_cpu(L.ptr.data(), L.vals.data(), L.n(), sq.data()) != 0) ++failures;
        for (int64_t l = 0; l < L.n(); ++l) {
            double s = 0.0;
            for (int64_t e = L.ptr[l]; e < L.ptr[l + 1]; ++e) {
                volatile double t = L.vals[e] * L.vals[e];
                s = s + t;
            }
            expect(same(sq[l], s), "sq", l, 0);
        }
        for (int P : {0, 1, 65}) {
            std::vector<int32_t> ia(P), ib(P);
            for (int p = 0; p < P; ++p) {
                ia[p] = (int32_t)(rng() % L.n());
                ib[p] = p % 5 == 0 ? ia[p] : (int32_t)(rng() % L.n());      // a list against itself
            }
            check(L, ia, ib, 0);
        }
        // the cross form: every list against every list, and an empty side
        std::vector<int32_t> all(L.n());
        std::iota(all.begin(), all.end(), 0);
        check(L, all, all, (int64_t)all.size());
        check(L, std::vector<int32_t>(), all, (int64_t)all.size());
    }
    // no lists at all
    if (hm_pair_sim_sq_cpu(nullptr, nullptr, 0, nullptr) != 0) ++failures;
    if (hm_pair_sim_cpu(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 15, nullptr) != 0)
        ++failures;
    if (failures) {
        std::printf("pair_sim_san: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("pair_sim_san ok\n");
    return 0;
}
