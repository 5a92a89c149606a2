// CPU twin of csrc/kernels/minhash.hip (hm_minhash_sig): the same contract and the same split of
// Murmur3 into a seed-independent premix per name (done once per row) and the h1 chain per
// (name, hash).  OpenMP over rows.  Integer only, so the two agree bit for bit.
//
// hm_minhash_names prepares a packed list<string> column for either engine: the name length of
// every feature string (the text before its FIRST ':', as knn._fv splits it) and whether every
// value text is a plain decimal (the rule of parse_plain_double in hashing.cpp), i.e. whether
// the per-row Python path would have accepted the column.
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../kernels/murmur3.h"

#define HM_API extern "C" __attribute__((visibility("default")))

namespace {

// [+-]digits[.digits][e[+-]digits] as strtod reads it: the forms Python's float() and strtod
// agree on.  Spaces, underscores, inf / nan words, hex and texts over 63 bytes are not plain.
bool plain_decimal(const char* p, int64_t n) {
    if (n <= 0 || n > 63) return false;
    for (int64_t i = 0; i < n; ++i) {
        const char c = p[i];
        if (!((c >= '0' && c <= '9') || c == '.' || c == '-' || c == '+' || c == 'e' || c == 'E')) return false;
    }
    char tmp[64];
    std::memcpy(tmp, p, (size_t)n);
    tmp[n] = 0;
    char* end = nullptr;
    (void)std::strtod(tmp, &end);
    return end == tmp + n;
}

}  // namespace

// nlen[s] = bytes before the first ':' of string s (the whole string when it has none).  Returns
// -1 when every value text is a plain decimal, else the index of the first string whose value
// text is not (nlen is filled either way).  -2: a string of 2^31 bytes or more.
HM_API int64_t hm_minhash_names(const uint8_t* buf, const int64_t* off, int64_t nnz, int32_t* nlen) {
    int64_t bad = INT64_MAX;
    bool too_long = false;
#pragma omp parallel for schedule(static) reduction(min : bad) reduction(|| : too_long) if (nnz > 65536)
    for (int64_t s = 0; s < nnz; ++s) {
        const uint8_t* p = buf + off[s];
        const int64_t L = off[s + 1] - off[s];
        if (L > INT32_MAX) { too_long = true; nlen[s] = 0; continue; }
        const void* c = L ? std::memchr(p, ':', (size_t)L) : nullptr;
        if (!c) { nlen[s] = (int32_t)L; continue; }
        const int64_t nl = (const uint8_t*)c - p;
        nlen[s] = (int32_t)nl;
        if (!plain_decimal((const char*)p + nl + 1, L - nl - 1) && s < bad) bad = s;
    }
    if (too_long) return -2;
    return bad == INT64_MAX ? -1 : bad;
}

HM_API int hm_minhash_sig_cpu(const uint8_t* buf, const int64_t* off, const int32_t* nlen,
                              const int64_t* rowptr, int64_t n_rows, int H, uint32_t seed0,
                              int32_t* out) {
    if (n_rows <= 0 || H <= 0) return 0;
#pragma omp parallel if (n_rows * (int64_t)H > 4096)
    {
        std::vector<uint32_t> words;       // premixed words of the row's names, back to back
        std::vector<int64_t> wbeg;         // name j: words[wbeg[j] .. wbeg[j + 1]), then its tail
        std::vector<uint32_t> tail, len;
#pragma omp for schedule(dynamic, 64)
        for (int64_t r = 0; r < n_rows; ++r) {
            uint32_t* o = reinterpret_cast<uint32_t*>(out) + r * (int64_t)H;
            const int64_t f0 = rowptr[r], f1 = rowptr[r + 1];
            if (f0 == f1) {
                for (int h = 0; h < H; ++h) o[h] = 0;
                continue;
            }
            words.clear(); tail.clear(); len.clear(); wbeg.clear();
            wbeg.push_back(0);
            for (int64_t s = f0; s < f1; ++s) {
                const uint8_t* p = buf + off[s];
                const int L = nlen[s], nw = L >> 2;
                for (int i = 0; i < nw; ++i) {
                    uint32_t k1;
                    std::memcpy(&k1, p + 4 * i, 4);   // little-endian host
                    words.push_back(hm::mm_premix(k1));
                }
                tail.push_back(hm::mm_premix(hm::mm_tail_word(p + 4 * nw, L & 3)));   // 0 when no tail
                len.push_back((uint32_t)L);
                wbeg.push_back((int64_t)words.size());
            }
            const int64_t nf = f1 - f0;
            for (int h = 0; h < H; ++h) {
                const uint32_t seed = seed0 + (uint32_t)h;
                uint32_t m = 0xFFFFFFFFu;
                for (int64_t j = 0; j < nf; ++j) {
                    uint32_t h1 = seed;
                    for (int64_t i = wbeg[j]; i < wbeg[j + 1]; ++i) h1 = hm::mm_chain(h1, words[i]);
                    h1 = hm::mm_fmix(h1 ^ tail[j], len[j]);
                    m = h1 < m ? h1 : m;
                }
                o[h] = m;
            }
        }
    }
    return 0;
}
