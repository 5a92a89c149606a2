// CPU twin of csrc/kernels/each_top_k.hip (hm_each_top_k / hm_each_top_k_items): the same
// contract, OpenMP over the segments (work items), sequential inside one.
//
// Contract.  The rows, sorted stably by group code (perm, or the identity when it is NULL), form G
// segments (segptr).  Inside a segment the order is the pair (key, p): key = the fp64 score as a
// u64 that sorts best first (-0.0 folded onto 0.0, direction by `largest`), p = the position in
// the sorted order.  Smaller pair = better; pairs are distinct, so the k best of a segment in
// order are one well-defined list: std::partial_sort gives it for any thread count, bit for bit
// what the kernels give.  Integer compares only.
#include <omp.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#define HM_API extern "C" __attribute__((visibility("default")))

namespace {

constexpr int ETK_KMAX = 128;

struct Pair {
    uint64_t key;
    uint32_t pos;
};

inline bool better(const Pair& a, const Pair& b) {
    return a.key < b.key || (a.key == b.key && a.pos < b.pos);
}

inline uint64_t key_of(double s, uint64_t flip) {
    uint64_t b;
    std::memcpy(&b, &s, 8);
    if ((b << 1) == 0) b = 0;
    const uint64_t u = b ^ ((b >> 63) ? ~uint64_t(0) : uint64_t(1) << 63);
    return u ^ flip;
}

// the best min(k, size) pairs of v, in order, at its front; returns how many
inline int64_t select(std::vector<Pair>& v, int k) {
    const int64_t m = std::min<int64_t>(k, (int64_t)v.size());
    std::partial_sort(v.begin(), v.begin() + m, v.end(), better);
    return m;
}

inline void load_rows(std::vector<Pair>& v, const double* score, const int32_t* perm, int64_t begin,
                      int64_t end, uint64_t flip) {
    v.resize((size_t)(end - begin));
    for (int64_t p = begin; p < end; ++p)
        v[(size_t)(p - begin)] = Pair{key_of(score[perm ? perm[p] : (int32_t)p], flip), (uint32_t)p};
}

}  // namespace

// score fp64 [n]; perm int32 [n] or NULL; segptr, outptr int64 [G + 1]; rows int32 [outptr[G]].
// max_len > 0: segments longer than it are left alone (the split the kernels make).
HM_API int hm_each_top_k_cpu(const double* score, const int32_t* perm, const int64_t* segptr,
                             const int64_t* outptr, int G, int k, int largest, int64_t max_len,
                             int32_t* rows) {
    if (G <= 0) return 0;
    if (k < 1 || k > ETK_KMAX) return 1;
    const uint64_t flip = largest ? ~uint64_t(0) : 0;
#pragma omp parallel
    {
        std::vector<Pair> v;
#pragma omp for schedule(dynamic, 64)
        for (int g = 0; g < G; ++g) {
            const int64_t begin = segptr[g], end = segptr[g + 1];
            if (end <= begin || (max_len > 0 && end - begin > max_len)) continue;
            load_rows(v, score, perm, begin, end, flip);
            const int64_t m = select(v, k);
            int32_t* out = rows + outptr[g];
            for (int64_t r = 0; r < m; ++r) out[r] = perm ? perm[v[(size_t)r].pos] : (int32_t)v[(size_t)r].pos;
        }
    }
    return 0;
}

// The work-item form of hm_each_top_k_items: item w selects among positions
// [item_begin[w], item_end[w]) of the sorted rows (ckey NULL) or of the candidate pairs, and
// writes row ids (item_final[w] != 0) or pairs at item_dst[w].
HM_API int hm_each_top_k_items_cpu(const double* score, const int32_t* perm, const uint64_t* ckey,
                                   const uint32_t* cpos, const int64_t* item_begin,
                                   const int64_t* item_end, const int64_t* item_dst,
                                   const int64_t* item_final, int64_t W, int k, int largest,
                                   uint64_t* okey, uint32_t* opos, int32_t* rows) {
    if (W <= 0) return 0;
    if (k < 1 || k > ETK_KMAX) return 1;
    const uint64_t flip = largest ? ~uint64_t(0) : 0;
#pragma omp parallel
    {
        std::vector<Pair> v;
#pragma omp for schedule(dynamic, 1)
        for (int64_t w = 0; w < W; ++w) {
            const int64_t begin = item_begin[w], end = item_end[w];
            if (end <= begin) continue;
            if (ckey) {
                v.resize((size_t)(end - begin));
                for (int64_t i = begin; i < end; ++i) v[(size_t)(i - begin)] = Pair{ckey[i], cpos[i]};
            } else {
                load_rows(v, score, perm, begin, end, flip);
            }
            const int64_t m = select(v, k), dst = item_dst[w];
            for (int64_t r = 0; r < m; ++r) {
                const Pair& b = v[(size_t)r];
                if (item_final[w]) {
                    rows[dst + r] = perm ? perm[b.pos] : (int32_t)b.pos;
                } else {
                    okey[dst + r] = b.key;
                    opos[dst + r] = b.pos;
                }
            }
        }
    }
    return 0;
}
