// CPU engine for train_plsa: the contracts of csrc/kernels/plsa.hip (hm_plsa_doc_em,
// hm_plsa_mstep) in fp32.  OpenMP over documents for the EM; over words, fixed row chunks and
// topic columns for the M-step, so no sum's order depends on the thread count.  Used for CPU
// sessions and tested against the same fp64 oracle as the kernels.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#define HM_API extern "C" __attribute__((visibility("default")))

namespace {
constexpr int ROWS_PER_CHUNK = 256;            // M-step: rows of one column partial

inline int64_t chunks_of(int64_t rows) { return (rows + ROWS_PER_CHUNK - 1) / ROWS_PER_CHUNK; }

// q[k] = pzd[k] * pw[k] / max(sum_k pzd[k] * pw[k], 1e-30)
inline void posterior(const float* pzd, const float* pw, int K, float* q) {
    float z = 0.f;
    for (int k = 0; k < K; ++k) {
        q[k] = pzd[k] * pw[k];
        z += q[k];
    }
    z = std::fmax(z, 1e-30f);
    for (int k = 0; k < K; ++k) q[k] /= z;
}
}  // namespace

HM_API int hm_plsa_doc_em_cpu(const int32_t* doc_off, const int32_t* wid, const float* cnt,
                              const float* pwzT, int B, int K, float delta, int max_iter, float* pzd,
                              float* contrib, int32_t* iters_out) {
    if (B <= 0) return 0;
    if (K < 1 || K > 256 || max_iter < 0) return 1;
#pragma omp parallel
    {
        std::vector<float> q(K), nw(K);
#pragma omp for schedule(dynamic, 8)
        for (int d = 0; d < B; ++d) {
            const int n0 = doc_off[d], n1 = doc_off[d + 1];
            float* p = pzd + (size_t)d * K;
            if (n1 <= n0) {
                std::fill(p, p + K, 0.f);
                iters_out[d] = 0;
                continue;
            }
            std::fill(p, p + K, 1.f / (float)K);
            int it = 0;
            while (it < max_iter) {
                std::fill(nw.begin(), nw.end(), 0.f);
                for (int n = n0; n < n1; ++n) {
                    posterior(p, pwzT + (size_t)wid[n] * K, K, q.data());
                    for (int k = 0; k < K; ++k) nw[k] += cnt[n] * q[k];
                }
                float tot = 0.f;
                for (int k = 0; k < K; ++k) tot += nw[k];
                tot = std::fmax(tot, 1e-30f);
                float ch = 0.f;
                for (int k = 0; k < K; ++k) {
                    nw[k] /= tot;
                    ch += std::fabs(nw[k] - p[k]);
                    p[k] = nw[k];
                }
                ++it;
                if (ch / (float)K < delta) break;
            }
            for (int n = n0; n < n1; ++n) {
                posterior(p, pwzT + (size_t)wid[n] * K, K, q.data());
                float* c = contrib + (size_t)n * K;
                for (int k = 0; k < K; ++k) c[k] = cnt[n] * q[k];
            }
            iters_out[d] = it;
        }
    }
    return 0;
}

// 4-byte words of scratch hm_plsa_mstep_cpu needs: nwz [U][K] | column partials [chunks][K] |
// S [K] | T [K].
HM_API int64_t hm_plsa_mstep_scratch_words_cpu(int U, int V, int K) {
    if (U < 0 || V < 0 || K < 0) return 0;
    return (int64_t)U * K + (std::max(chunks_of(U), chunks_of(V)) + 2) * K;
}

namespace {
// out[k] = sum over the rows of a [rows][K] matrix: per-chunk partials (rows in order), then the
// chunks in order.
void column_sums(const float* m, int64_t rows, int K, float* part, float* out) {
    const int64_t nc = chunks_of(rows);
#pragma omp parallel for schedule(static)
    for (int64_t c = 0; c < nc; ++c) {
        float* pc = part + (size_t)c * K;
        std::fill(pc, pc + K, 0.f);
        const int64_t hi = std::min(rows, (c + 1) * ROWS_PER_CHUNK);
        for (int64_t r = c * ROWS_PER_CHUNK; r < hi; ++r)
            for (int k = 0; k < K; ++k) pc[k] += m[(size_t)r * K + k];
    }
#pragma omp parallel for schedule(static)
    for (int k = 0; k < K; ++k) {
        float s = 0.f;
        for (int64_t c = 0; c < nc; ++c) s += part[(size_t)c * K + k];
        out[k] = s;
    }
}
}  // namespace

HM_API int hm_plsa_mstep_cpu(const int32_t* word_off, const int32_t* perm, const int32_t* uniq,
                             const float* contrib, int U, int V, int K, float alpha, float* pwzT,
                             void* scratch) {
    if (V <= 0) return 0;
    if (U < 0 || U > V || K < 1 || K > 256) return 1;
    float* nwz = (float*)scratch;
    float* part = nwz + (size_t)U * K;
    float* S = part + (size_t)std::max(chunks_of(U), chunks_of(V)) * K;
    float* T = S + K;
#pragma omp parallel for schedule(dynamic, 64)
    for (int u = 0; u < U; ++u) {
        float* row = nwz + (size_t)u * K;
        std::fill(row, row + K, 0.f);
        for (int j = word_off[u]; j < word_off[u + 1]; ++j) {
            const float* c = contrib + (size_t)perm[j] * K;
            for (int k = 0; k < K; ++k) row[k] += c[k];
        }
    }
    column_sums(nwz, U, K, part, S);
    const float keep = 1.f - alpha;
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < (int64_t)V * K; ++i) pwzT[i] = keep * pwzT[i];
#pragma omp parallel for schedule(static)
    for (int u = 0; u < U; ++u) {               // uniq is strictly ascending: rows are distinct
        float* row = pwzT + (size_t)uniq[u] * K;
        const float* nz = nwz + (size_t)u * K;
        for (int k = 0; k < K; ++k) row[k] += alpha * (nz[k] / std::fmax(S[k], 1e-30f));
    }
    column_sums(pwzT, V, K, part, T);
#pragma omp parallel for schedule(static)
    for (int64_t w = 0; w < V; ++w)
        for (int k = 0; k < K; ++k) pwzT[(size_t)w * K + k] /= T[k];
    return 0;
}
