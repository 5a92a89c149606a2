// CPU engine for train_lda -engine native: the contracts of csrc/kernels/lda.hip
// (hm_lda_batch_eb, hm_lda_doc_estep, hm_lda_mstep) in fp32 with the kernels' orders of addition:
// a document's words go round-robin to four partial sums that are added in order (the kernels'
// four waves), the M-step adds a tile of 64 words in the same four strides and the tiles' column
// partials in fp64, chunk by chunk.  OpenMP over batch words, documents and tiles; no sum's order
// depends on the thread count.  digamma, exp and log are the host's, so results are close to the
// kernels', not bit-equal.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#define HM_API extern "C" __attribute__((visibility("default")))

namespace {
constexpr int TILE_WORDS = 64;                 // lda.hip: LDA_TILE_WORDS
constexpr int COLSUM_THREADS = 1024;           // lda.hip: lda_colsum_kernel's block

inline int64_t tiles_of(int64_t V) { return (V + TILE_WORDS - 1) / TILE_WORDS; }

inline float digammaf(float x) {
    float r = 0.f;
    while (x < 6.f) {
        r -= 1.f / x;
        x += 1.f;
    }
    const float f = 1.f / (x * x);
    const float t = f * (1.f / 12 - f * (1.f / 120 - f * (1.f / 252 - f * (1.f / 240 - f * (1.f / 132)))));
    return r + std::log(x) - 0.5f / x - t;
}

// et[k] = exp(digamma(g[k]) - digamma(sum_k g[k]))
inline void exp_elog(const float* g, int K, float* et) {
    float gs = 0.f;
    for (int k = 0; k < K; ++k) gs += g[k];
    const float dg = digammaf(gs);
    for (int k = 0; k < K; ++k) et[k] = std::exp(digammaf(g[k]) - dg);
}

inline float phinorm(const float* et, const float* e, int K) {
    float p = 0.f;
    for (int k = 0; k < K; ++k) p += et[k] * e[k];
    return p + 1e-30f;
}
}  // namespace

HM_API int hm_lda_batch_eb_cpu(const int32_t* uniq, const float* lamT, const float* T, int U, int K, float* EbU) {
    if (U <= 0) return 0;
    if (K < 1 || K > 256) return 1;
    std::vector<float> dg(K);
    for (int k = 0; k < K; ++k) dg[k] = digammaf(T[k]);
#pragma omp parallel for schedule(static)
    for (int u = 0; u < U; ++u) {
        const float* lam = lamT + (size_t)uniq[u] * K;
        float* out = EbU + (size_t)u * K;
        for (int k = 0; k < K; ++k) out[k] = std::exp(digammaf(lam[k]) - dg[k]);
    }
    return 0;
}

HM_API int hm_lda_doc_estep_cpu(const int32_t* doc_off, const int32_t* wpos, const float* cnt, const float* EbU,
                                int B, int K, float alpha, float delta, int max_iter, float* gamma,
                                float* contrib, int32_t* iters_out, double* bound) {
    if (B <= 0) return 0;
    if (K < 1 || K > 256 || max_iter < 0) return 1;
#pragma omp parallel
    {
        std::vector<float> et(K), acc(4 * (size_t)K);
#pragma omp for schedule(dynamic, 8)
        for (int d = 0; d < B; ++d) {
            const int n0 = doc_off[d], n1 = doc_off[d + 1];
            float* g = gamma + (size_t)d * K;
            if (n1 <= n0) {
                std::fill(g, g + K, alpha);
                iters_out[d] = 0;
                bound[d] = 0.0;
                continue;
            }
            int it = 0, cap = max_iter;
            for (;;) {
                exp_elog(g, K, et.data());
                if (it == cap) break;
                std::fill(acc.begin(), acc.end(), 0.f);
                for (int n = n0; n < n1; ++n) {
                    const float* e = EbU + (size_t)wpos[n] * K;
                    float* a = acc.data() + (size_t)((n - n0) & 3) * K;
                    const float s = cnt[n] / phinorm(et.data(), e, K);
                    for (int k = 0; k < K; ++k) a[k] += s * e[k];
                }
                float ch = 0.f;
                for (int k = 0; k < K; ++k) {
                    const float v = alpha + et[k] * (acc[k] + acc[K + k] + acc[2 * K + k] + acc[3 * K + k]);
                    ch += std::fabs(v - g[k]);
                    g[k] = v;
                }
                ++it;
                if (ch / (float)K < delta) cap = it;
            }
            double bw[4] = {0.0, 0.0, 0.0, 0.0};
            for (int n = n0; n < n1; ++n) {
                const float* e = EbU + (size_t)wpos[n] * K;
                const float p = phinorm(et.data(), e, K), s = cnt[n] / p;
                bw[(n - n0) & 3] += (double)cnt[n] * std::log((double)p);
                float* c = contrib + (size_t)n * K;
                for (int k = 0; k < K; ++k) c[k] = et[k] * e[k] * s;
            }
            iters_out[d] = it;
            bound[d] = ((bw[0] + bw[1]) + bw[2]) + bw[3];
        }
    }
    return 0;
}

// 4-byte words of scratch hm_lda_mstep_cpu needs: the tiles' column partials [tiles(V)][K].
HM_API int64_t hm_lda_mstep_scratch_words_cpu(int U, int V, int K) {
    if (U < 0 || V < 0 || K < 0) return 0;
    return tiles_of(V) * K;
}

HM_API int hm_lda_mstep_cpu(const int32_t* word_off, const int32_t* perm, const int32_t* uniq,
                            const float* contrib, int U, int V, int K, float rho, float eta, float scale,
                            float* lamT, float* T, void* scratch) {
    if (V <= 0) return 0;
    if (U < 0 || U > V || K < 1 || K > 256) return 1;
    float* part = (float*)scratch;
    const int64_t nb = tiles_of(V);
    const float keep = 1.f - rho;
#pragma omp parallel
    {
        std::vector<float> col(4 * (size_t)K), s(K);
#pragma omp for schedule(dynamic, 16)
        for (int64_t t = 0; t < nb; ++t) {
            const int64_t lo = t * TILE_WORDS, hi = std::min<int64_t>(V, lo + TILE_WORDS);
            // uniq ascends: the tile's batch words are one stretch of it, walked alongside the words
            int64_t u = std::lower_bound(uniq, uniq + U, lo, [](int32_t a, int64_t b) { return a < b; }) - uniq;
            std::fill(col.begin(), col.end(), 0.f);
            for (int64_t w = lo; w < hi; ++w) {
                std::fill(s.begin(), s.end(), 0.f);
                if (u < U && uniq[u] == w) {
                    for (int q = word_off[u]; q < word_off[u + 1]; ++q) {
                        const float* c = contrib + (size_t)perm[q] * K;
                        for (int k = 0; k < K; ++k) s[k] += c[k];
                    }
                    ++u;
                }
                float* lam = lamT + (size_t)w * K;
                float* cw = col.data() + (size_t)((w - lo) & 3) * K;
                for (int k = 0; k < K; ++k) {
                    // the kernel's two __fmaf_rn: the product of two floats is exact in fp64, so
                    // each line rounds once (this build has no hardware fma to call)
                    const float stat = (float)((double)scale * s[k] + (double)eta);
                    lam[k] = (float)((double)keep * lam[k] + (double)(rho * stat));
                    cw[k] += lam[k];
                }
            }
            for (int k = 0; k < K; ++k)
                part[(size_t)t * K + k] = ((col[k] + col[K + k]) + col[2 * K + k]) + col[3 * K + k];
        }
    }
    int KP = 1;
    while (KP < K) KP *= 2;
    const int RG = COLSUM_THREADS / KP;
    const int64_t chunk = (nb + RG - 1) / RG;
#pragma omp parallel for schedule(static)
    for (int k = 0; k < K; ++k) {
        double tot = 0.0;
        for (int g = 0; g < RG; ++g) {
            double sg = 0.0;
            for (int64_t b = g * chunk, b1 = std::min(nb, (g + 1) * chunk); b < b1; ++b) sg += (double)part[(size_t)b * K + k];
            tot = g == 0 ? sg : tot + sg;
        }
        T[k] = (float)tot;
    }
    return 0;
}
