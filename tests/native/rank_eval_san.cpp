// The ranking-measures twin (csrc/host/rank_eval_cpu.cpp) in a program of its own, to be built with
// -fsanitize=address,undefined: every buffer is a heap allocation of the exact size, so a read or
// write past a row, a table or the output is reported.  The edge corpus: L = 1, 8, 65 and 1024;
// truth rows of 0, 1 and many items; ids at both ends of int64; ragged lengths that include 0, 1,
// values below 0 and beyond L; k = 0, 1, L - 1, L, L + 1 and 2^31 - 1; every measures mask; graded
// truth with its idcg scan.  The results are checked against a plain loop of this file's own.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <set>
#include <vector>

extern "C" int hm_rank_eval_cpu(const int64_t* rank, const int32_t* lengths, const int64_t* rowptr,
                                const int64_t* items, const double* gain, const double* idcg,
                                const double* log2tab, const double* ideal, int64_t tab_n, int64_t U, int L,
                                int k, int measures, double* out);
extern "C" int hm_rank_eval_idcg_cpu(const int64_t* rowptr, const double* gain_desc, const double* log2tab,
                                     int64_t tab_n, int64_t U, double* idcg);

namespace {

int failures = 0;

void expect(bool ok, const char* what, int L, int k, int64_t row) {
    if (!ok && ++failures <= 20) std::printf("FAIL %s: L=%d k=%d row=%lld\n", what, L, k, (long long)row);
}

bool same(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }

void run(int U, int L, bool ragged, bool graded, std::mt19937_64& rng) {
    const int64_t lo = INT64_MIN, hi = INT64_MAX;
    std::vector<int64_t> rowptr(U + 1, 0), items;
    std::vector<double> gain;
    for (int u = 0; u < U; ++u) {
        const int size = u % 4 == 0 ? 0 : u % 4 == 1 ? 1 : u % 4 == 2 ? 37 : 700;
        std::set<int64_t> s;
        if (size >= 2) { s.insert(lo); s.insert(hi); }
        while ((int)s.size() < size) s.insert((int64_t)(rng() % 4000) * 2 - 4000);
        for (int64_t v : s) {
            items.push_back(v);
            gain.push_back(std::ldexp(1.0, (int)(rng() % 5)) - 1.0);
        }
        rowptr[u + 1] = (int64_t)items.size();
    }
    const int64_t nnz = (int64_t)items.size();
    int64_t max_len = 0;
    for (int u = 0; u < U; ++u) max_len = std::max(max_len, rowptr[u + 1] - rowptr[u]);
    const int64_t tab_n = std::max<int64_t>(L, max_len) + 1;
    std::vector<double> log2tab(tab_n), ideal(tab_n, 0.0);
    for (int64_t i = 0; i < tab_n; ++i) log2tab[i] = std::log2((double)(i + 2));
    for (int64_t m = 1; m < tab_n; ++m) ideal[m] = ideal[m - 1] + 1.0 / log2tab[m - 1];

    std::vector<double> desc(gain), idcg(nnz);
    for (int u = 0; u < U; ++u)
        std::sort(desc.begin() + rowptr[u], desc.begin() + rowptr[u + 1], [](double a, double b) { return a > b; });
    if (hm_rank_eval_idcg_cpu(rowptr.data(), desc.data(), log2tab.data(), tab_n, U, idcg.data()) != 0) ++failures;

    std::vector<int64_t> rank((size_t)U * L);
    for (int u = 0; u < U; ++u) {
        const int64_t t0 = rowptr[u], n = rowptr[u + 1] - t0;
        for (int i = 0; i < L; ++i) {
            const bool hit = n > 0 && (rng() & 1);
            rank[(size_t)u * L + i] = hit ? items[t0 + (int64_t)(rng() % (uint64_t)std::min<int64_t>(n, 5))]
                                          : (int64_t)(rng() % 7) * 2 + 1;       // odd: never in a truth row
        }
    }
    std::vector<int32_t> lengths(U);
    for (int u = 0; u < U; ++u) lengths[u] = (int32_t)(rng() % (uint64_t)(L + 1));
    lengths[0] = 0;
    lengths[U - 1] = 1;
    if (U > 3) { lengths[1] = L + 5; lengths[2] = -3; }

    const int ks[] = {0, 1, L - 1, L, L + 1, INT32_MAX};
    for (int k : ks) {
        if (k < 0) continue;
        std::vector<double> full((size_t)7 * U, -1.0);
        int rc = hm_rank_eval_cpu(rank.data(), ragged ? lengths.data() : nullptr, rowptr.data(), items.data(),
                                  graded ? gain.data() : nullptr, graded ? idcg.data() : nullptr, log2tab.data(),
                                  ideal.data(), tab_n, U, L, k, 127, full.data());
        if (rc != 0) ++failures;
        for (int u = 0; u < U; ++u) {
            int Lp = ragged ? std::min(std::max(lengths[u], 0), L) : L;
            if (k > 0) Lp = std::min(Lp, k);
            const int64_t t0 = rowptr[u], t1 = rowptr[u + 1], n = t1 - t0;
            int64_t hits = 0, first = -1, correct = 0, misses = 0;
            double ap = 0.0, dcg = 0.0;
            std::vector<char> is_hit(Lp);
            for (int i = 0; i < Lp; ++i) {
                const int64_t* at = std::find(items.data() + t0, items.data() + t1, rank[(size_t)u * L + i]);
                is_hit[i] = at != items.data() + t1;
                if (!is_hit[i]) continue;
                ++hits;
                if (first < 0) first = i;
                ap += (double)hits / (double)(i + 1);
                dcg += (graded ? gain[at - items.data()] : 1.0) / log2tab[i];
            }
            const int64_t n_neg = Lp - hits;
            for (int i = 0; i < Lp; ++i) {
                if (is_hit[i]) correct += n_neg - misses;
                else ++misses;
            }
            const int64_t m = k > 0 ? std::min<int64_t>(n, Lp) : n;
            const double id = m == 0 ? 0.0 : graded ? idcg[t0 + m - 1] : ideal[m];
            const double want[7] = {
                Lp ? (double)hits / (double)Lp : 0.0,
                n ? (double)hits / (double)n : 0.0,
                hits ? 1.0 : 0.0,
                first >= 0 ? 1.0 / (double)(first + 1) : 0.0,
                n ? ap / (double)(k > 0 ? std::min<int64_t>(n, k) : n) : 0.0,
                id > 0.0 ? dcg / id : 0.0,
                hits == 0 ? 0.0 : n_neg == 0 ? 1.0 : (double)correct / (double)(hits * n_neg),
            };
            for (int j = 0; j < 7; ++j) expect(same(full[(size_t)j * U + u], want[j]), "value", L, k, u);
        }
        for (int mask = 0; mask < 127; mask += 5) {
            std::vector<double> part((size_t)7 * U, 7.5);
            rc = hm_rank_eval_cpu(rank.data(), ragged ? lengths.data() : nullptr, rowptr.data(), items.data(),
                                  graded ? gain.data() : nullptr, graded ? idcg.data() : nullptr, log2tab.data(),
                                  ideal.data(), tab_n, U, L, k, mask, part.data());
            if (rc != 0) ++failures;
            for (int j = 0; j < 7; ++j)
                for (int u = 0; u < U; ++u)
                    expect(same(part[(size_t)j * U + u], (mask >> j) & 1 ? full[(size_t)j * U + u] : 7.5), "mask", L,
                           k, u);
        }
    }
}

}  // namespace

int main() {
    std::mt19937_64 rng(12345);
    const int Ls[] = {1, 8, 65, 1024};
    for (int L : Ls)
        for (int ragged = 0; ragged < 2; ++ragged)
            for (int graded = 0; graded < 2; ++graded) run(L == 1024 ? 5 : 67, L, ragged, graded, rng);
    // refused arguments return an error and touch nothing
    double out[7] = {0};
    const int64_t rowptr[2] = {0, 0}, r[1] = {1};
    const double tab[2] = {1.0, 1.5};
    if (hm_rank_eval_cpu(r, nullptr, rowptr, nullptr, nullptr, nullptr, tab, tab, 2, 1, 0, 0, 127, out) == 0) ++failures;
    if (hm_rank_eval_cpu(r, nullptr, rowptr, nullptr, nullptr, nullptr, tab, tab, 2, 1, 1, -1, 127, out) == 0) ++failures;
    if (hm_rank_eval_cpu(r, nullptr, rowptr, nullptr, nullptr, nullptr, tab, tab, 1, 1, 1, 0, 127, out) == 0) ++failures;
    if (hm_rank_eval_cpu(r, nullptr, rowptr, nullptr, nullptr, nullptr, tab, tab, 2, 1, 1, 0, 127, out) != 0) ++failures;
    if (failures) {
        std::printf("rank_eval_san: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("rank_eval_san ok\n");
    return 0;
}
