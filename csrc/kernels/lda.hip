// Online-VB LDA E-step (upstream hivemall/topicmodel/OnlineLDAModel.eStep,
// Hoffman et al. NIPS'10): for every document d of a mini-batch, iterate
//     Et[k]      = exp(digamma(gamma[k]) - digamma(sum_k gamma[k]))
//     phinorm[n] = sum_k Et[k] * Eb[w_n][k]
//     gamma'[k]  = alpha + Et[k] * sum_n c_n * Eb[w_n][k] / phinorm[n]
// until mean_k |gamma' - gamma| < delta (per document, as upstream) or max_iter, then emit the
// sufficient statistics contrib[n][k] = Et[k] * Eb[w_n][k] * c_n / phinorm[n].
//
// One 256-thread workgroup per document; lanes span topics (K <= 64 * KC) so a word's topic row
// Eb[w] (expElogbeta transposed to [V][K]: contiguous per word) is one coalesced load, phinorm is
// a DPP wave sum, and each of the 4 waves accumulates its quarter of the words into per-lane
// registers; the 4 partial sums meet in LDS once per iteration.  The document's Eb rows are
// staged in LDS when they fit (the loop re-reads them every iteration).  The whole fixed-point
// loop runs inside the kernel: the torch formulation paid ~10 launches and a host sync per
// inner iteration.
#include "common.h"

namespace {

constexpr int LDA_LDS_FLOATS = 12 * 1024;      // 48 KB of staged Eb rows per workgroup

__device__ __forceinline__ float digammaf(float x) {
    float r = 0.f;
    while (x < 6.f) {
        r -= 1.f / x;
        x += 1.f;
    }
    const float f = 1.f / (x * x);
    const float t = f * (1.f / 12 - f * (1.f / 120 - f * (1.f / 252 - f * (1.f / 240 - f * (1.f / 132)))));
    return r + logf(x) - 0.5f / x - t;
}

// The kernels that train_lda -engine native adds (lda_doc_estep_kernel, lda_batch_eb_kernel,
// lda_mstep_kernel, lda_colsum_kernel) are compiled without gfx950's packed fp32 arithmetic
// (v_pk_add/mul/fma_f32): where a rounding matters they say so with __fmaf_rn, and the backend is
// not to regroup their scalar operations into packed pairs.  A function attribute, so that
// lda_estep_kernel (hm_lda_estep) is compiled exactly as before.  Device pass only: the host
// pass does not know the feature.
#if defined(__HIP_DEVICE_COMPILE__)
#define LDA_NO_PACKED_FP32 __attribute__((target("no-packed-fp32-ops")))
#else
#define LDA_NO_PACKED_FP32
#endif

// The E-step of one document, inlined into its two kernels.  BOUND = false is hm_lda_estep (wid:
// word ids, EbT: the [V][K] table).  BOUND = true is hm_lda_doc_estep: the same fixed point read
// through wid = wpos (ranks in the batch's distinct words) from EbT = EbU [U][K], which also
// writes bound_out and ends an empty document at once.
template <int KC, bool BOUND>
__device__ __forceinline__ void lda_estep_body(const int32_t* __restrict__ doc_off,
                                               const int32_t* __restrict__ wid, const float* __restrict__ cnt,
                                               const float* __restrict__ EbT, int K, float alpha, float delta,
                                               int max_iter, float* __restrict__ gamma,
                                               float* __restrict__ contrib, int32_t* __restrict__ iters_out,
                                               double* __restrict__ bound_out) {
    __shared__ float s_acc[4][64 * KC];
    __shared__ float s_gamma[64 * KC];
    __shared__ float s_et[64 * KC];
    __shared__ float s_red[4];
    __shared__ int s_done;
    extern __shared__ float s_eb[];
    const int d = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n0 = doc_off[d], n1 = doc_off[d + 1], nd = n1 - n0;
    if constexpr (BOUND) {
        if (nd <= 0) {                           // uniform: an empty document
            for (int k = tid; k < K; k += 256) gamma[(size_t)d * K + k] = alpha;
            if (tid == 0) {
                iters_out[d] = 0;
                bound_out[d] = 0.0;
            }
            return;
        }
    }
    const bool staged = (int64_t)nd * K <= LDA_LDS_FLOATS;
    if (staged) {
        for (int i = tid; i < nd * K; i += 256) {
            const int n = i / K, k = i - n * K;
            s_eb[i] = EbT[(size_t)wid[n0 + n] * K + k];
        }
    }
    for (int k = tid; k < 64 * KC; k += 256) s_gamma[k] = k < K ? gamma[(size_t)d * K + k] : 0.f;
    __syncthreads();
    auto eb = [&](int n, int k) -> float {
        return staged ? s_eb[n * K + k] : EbT[(size_t)wid[n0 + n] * K + k];
    };
    int it = 0;
    for (;;) {
        // Et from the current gamma (wave 0; K <= 256 topics)
        if (wave == 0) {
            float gs = 0.f;
#pragma unroll
            for (int j = 0; j < KC; ++j) gs += s_gamma[lane + 64 * j];
            gs = hm::wave_sum(gs);
            const float dg = digammaf(gs);
#pragma unroll
            for (int j = 0; j < KC; ++j) {
                const int k = lane + 64 * j;
                s_et[k] = k < K ? __expf(digammaf(s_gamma[k]) - dg) : 0.f;
            }
        }
        __syncthreads();
        if (it == max_iter) break;           // final Et computed: emit the statistics below
        float et[KC], acc[KC];
#pragma unroll
        for (int j = 0; j < KC; ++j) {
            et[j] = s_et[lane + 64 * j];
            acc[j] = 0.f;
        }
        for (int n = wave; n < nd; n += 4) {
            float e[KC], p = 0.f;
#pragma unroll
            for (int j = 0; j < KC; ++j) {
                const int k = lane + 64 * j;
                e[j] = k < K ? eb(n, k) : 0.f;
                p += et[j] * e[j];
            }
            p = hm::wave_sum(p) + 1e-30f;
            const float s = cnt[n0 + n] / p;
#pragma unroll
            for (int j = 0; j < KC; ++j) acc[j] += s * e[j];
        }
#pragma unroll
        for (int j = 0; j < KC; ++j) s_acc[wave][lane + 64 * j] = acc[j];
        __syncthreads();
        if (wave == 0) {
            float ch = 0.f;
#pragma unroll
            for (int j = 0; j < KC; ++j) {
                const int k = lane + 64 * j;
                if (k < K) {
                    const float g = alpha + et[j] * (s_acc[0][k] + s_acc[1][k] + s_acc[2][k] + s_acc[3][k]);
                    ch += fabsf(g - s_gamma[k]);
                    s_gamma[k] = g;
                }
            }
            ch = hm::wave_sum(ch);
            if (lane == 0) s_done = (ch / (float)K < delta) ? 1 : 0;
        }
        __syncthreads();
        ++it;
        if (s_done) {
            max_iter = it;                   // uniform: recompute Et once more, then emit
        }
    }
    // sufficient statistics with the final Et
    float et[KC];
#pragma unroll
    for (int j = 0; j < KC; ++j) et[j] = s_et[lane + 64 * j];
    double bw = 0.0;                             // this wave's words, in index order
    for (int n = wave; n < nd; n += 4) {
        float e[KC], p = 0.f;
#pragma unroll
        for (int j = 0; j < KC; ++j) {
            const int k = lane + 64 * j;
            e[j] = k < K ? eb(n, k) : 0.f;
            p += et[j] * e[j];
        }
        p = hm::wave_sum(p) + 1e-30f;
        const float c = cnt[n0 + n];
        const float s = c / p;
        if constexpr (BOUND) bw += (double)c * log((double)p);
#pragma unroll
        for (int j = 0; j < KC; ++j) {
            const int k = lane + 64 * j;
            if (k < K) contrib[(size_t)(n0 + n) * K + k] = et[j] * e[j] * s;
        }
    }
    for (int k = tid; k < K; k += 256) gamma[(size_t)d * K + k] = s_gamma[k];
    if (tid == 0 && iters_out) iters_out[d] = it;
    if constexpr (BOUND) {
        __shared__ double s_bound[4];
        if (lane == 0) s_bound[wave] = bw;       // the butterfly sum left p equal in every lane
        __syncthreads();
        if (tid == 0) bound_out[d] = ((s_bound[0] + s_bound[1]) + s_bound[2]) + s_bound[3];
    }
}

template <int KC>
__global__ __launch_bounds__(256) void lda_estep_kernel(const int32_t* __restrict__ doc_off,
                                                        const int32_t* __restrict__ wid,
                                                        const float* __restrict__ cnt,
                                                        const float* __restrict__ EbT, int K, float alpha,
                                                        float delta, int max_iter, float* __restrict__ gamma,
                                                        float* __restrict__ contrib,
                                                        int32_t* __restrict__ iters_out) {
    lda_estep_body<KC, false>(doc_off, wid, cnt, EbT, K, alpha, delta, max_iter, gamma, contrib, iters_out, nullptr);
}

template <int KC>
__global__ __launch_bounds__(256) LDA_NO_PACKED_FP32 void lda_doc_estep_kernel(
    const int32_t* __restrict__ doc_off, const int32_t* __restrict__ wpos, const float* __restrict__ cnt,
    const float* __restrict__ EbU, int K, float alpha, float delta, int max_iter, float* __restrict__ gamma,
    float* __restrict__ contrib, int32_t* __restrict__ iters_out, double* __restrict__ bound_out) {
    lda_estep_body<KC, true>(doc_off, wpos, cnt, EbU, K, alpha, delta, max_iter, gamma, contrib, iters_out, bound_out);
}

// ------------------------------------------------------------------- batch-sparse E[log beta]
// EbU[u][k] = exp(digamma(lamT[uniq[u]][k]) - digamma(T[k])) for the batch's U distinct words: a
// block takes LDA_EB_WORDS consecutive ranks, a wave one word at a time with lanes over topics
// (one coalesced row load, one coalesced row store); digamma(T[k]) is computed once per lane.
constexpr int LDA_EB_WORDS = 16;

template <int KC>
__global__ __launch_bounds__(256) LDA_NO_PACKED_FP32 void lda_batch_eb_kernel(const int32_t* __restrict__ uniq,
                                                           const float* __restrict__ lamT,
                                                           const float* __restrict__ T, int U, int K,
                                                           float* __restrict__ EbU) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float dg[KC];
#pragma unroll
    for (int j = 0; j < KC; ++j) {
        const int k = lane + 64 * j;
        dg[j] = k < K ? digammaf(T[k]) : 0.f;
    }
    const int64_t lo = (int64_t)blockIdx.x * LDA_EB_WORDS;
    const int nu = (int)min((int64_t)LDA_EB_WORDS, (int64_t)U - lo);
    for (int i = wave; i < nu; i += 4) {
        const size_t u = (size_t)(lo + i), w = (size_t)uniq[u];
#pragma unroll
        for (int j = 0; j < KC; ++j) {
            const int k = lane + 64 * j;
            if (k < K) EbU[u * K + k] = expf(digammaf(lamT[w * K + k]) - dg[j]);
        }
    }
}

// ---------------------------------------------------------------------------------- M-step
// lam' = (1 - rho) * lam + rho * (eta + scale * s[w]) on lamT [V][K] in place, one read and one
// write of the table, and the column sums T[k] = sum_w lam'[w][k] without float atomics.
//
// A workgroup owns LDA_TILE_WORDS consecutive words.  uniq is ascending, so the tile's batch
// words are one contiguous stretch of it: one binary search for the tile's first word finds the
// stretch, and 64 lanes write its ranks into an LDS map of the tile (-1: not in the batch).  Wave
// v then takes words v, v + 4, ... of the tile, four rows of lamT in flight at a time, lanes over
// topics.  A batch word adds its run of perm (contrib rows, in run order) in registers.  Every
// wave keeps its per-topic column partial in registers; the four meet in LDS in wave order and
// the tile's partial goes to part[tile][K].  lda_colsum_kernel adds the partials in fp64: row
// group g of its block adds a contiguous chunk of tiles in tile order, then the chunks are added
// in chunk order.  Every order is a function of (V, K) alone, never of the device.
constexpr int LDA_TILE_WORDS = 64;

__host__ __device__ inline int64_t lda_tiles(int64_t V) { return (V + LDA_TILE_WORDS - 1) / LDA_TILE_WORDS; }

template <int KC>
__global__ __launch_bounds__(256) LDA_NO_PACKED_FP32 void lda_mstep_kernel(const int32_t* __restrict__ word_off,
                                                        const int32_t* __restrict__ perm,
                                                        const int32_t* __restrict__ uniq,
                                                        const float* __restrict__ contrib, int U, int V, int K,
                                                        float rho, float eta, float scale,
                                                        float* __restrict__ lamT, float* __restrict__ part) {
    __shared__ int s_rank[LDA_TILE_WORDS];
    __shared__ float s_col[4][64 * KC];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t lo = (int64_t)blockIdx.x * LDA_TILE_WORDS;
    const int nw = (int)min((int64_t)LDA_TILE_WORDS, (int64_t)V - lo);
    if (tid < LDA_TILE_WORDS) s_rank[tid] = -1;
    __syncthreads();
    if (tid < LDA_TILE_WORDS) {
        int a = 0, b = U;                        // uniform: first rank with uniq[rank] >= lo
        while (a < b) {
            const int m = a + (b - a) / 2;
            if (uniq[m] < lo) a = m + 1;
            else b = m;
        }
        const int64_t u = (int64_t)a + tid;      // at most LDA_TILE_WORDS ranks fall into the tile
        if (u < U) {
            const int64_t w = uniq[u];
            if (w < lo + nw) s_rank[w - lo] = (int)u;
        }
    }
    __syncthreads();
    const float keep = 1.f - rho;
    float col[KC];
#pragma unroll
    for (int j = 0; j < KC; ++j) col[j] = 0.f;
    for (int i0 = wave; i0 < nw; i0 += 16) {
        float lam[4][KC];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = i0 + 4 * r;
#pragma unroll
            for (int j = 0; j < KC; ++j) {
                const int k = lane + 64 * j;
                lam[r][j] = (i < nw && k < K) ? lamT[(size_t)(lo + i) * K + k] : 0.f;
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = i0 + 4 * r;
            if (i >= nw) break;                  // uniform
            const int u = __builtin_amdgcn_readfirstlane(s_rank[i]);
            float s[KC];
#pragma unroll
            for (int j = 0; j < KC; ++j) s[j] = 0.f;
            if (u >= 0) {
                for (int q = word_off[u], q1 = word_off[u + 1]; q < q1; ++q) {
                    const size_t row = (size_t)perm[q] * K;
#pragma unroll
                    for (int j = 0; j < KC; ++j) {
                        const int k = lane + 64 * j;
                        if (k < K) s[j] += contrib[row + k];
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < KC; ++j) {
                const int k = lane + 64 * j;
                if (k < K) {
                    // two fmas: eta + scale * s and keep * lam + rho * (...) round once each
                    const float v = __fmaf_rn(keep, lam[r][j], rho * __fmaf_rn(scale, s[j], eta));
                    lamT[(size_t)(lo + i) * K + k] = v;
                    col[j] += v;
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < KC; ++j) s_col[wave][lane + 64 * j] = col[j];
    __syncthreads();
    if (tid < K) part[(size_t)blockIdx.x * K + tid] = ((s_col[0][tid] + s_col[1][tid]) + s_col[2][tid]) + s_col[3][tid];
}

// T[k] = sum over the nb tile partials, fp64: a 1024-thread block is RG = 1024 / KP row groups
// of KP column lanes (KP: the power of two >= K); group g adds tiles g * chunk .. (g + 1) * chunk
// in tile order, then the groups' sums are added in group order and rounded to fp32 once.
__global__ __launch_bounds__(1024) LDA_NO_PACKED_FP32 void lda_colsum_kernel(const float* __restrict__ part, int64_t nb, int K, int KP,
                                                          float* __restrict__ T) {
    __shared__ double s_sum[1024];
    const int RG = 1024 / KP, g = threadIdx.x / KP, k = threadIdx.x & (KP - 1);
    const int64_t chunk = (nb + RG - 1) / RG;
    double s = 0.0;
    if (k < K) {
        const int64_t b1 = min(nb, (g + 1) * chunk);
#pragma unroll 8
        for (int64_t b = g * chunk; b < b1; ++b) s += (double)part[(size_t)b * K + k];
    }
    s_sum[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x < K) {
        double t = s_sum[threadIdx.x];
        for (int i = KP + threadIdx.x; i < 1024; i += KP) t += s_sum[i];
        T[threadIdx.x] = (float)t;
    }
}

}  // namespace

// Floats of EbT / EbU rows (nd * K) that the E-step kernels stage in LDS for one document.
HM_API int hm_lda_stage_floats() { return LDA_LDS_FLOATS; }

// doc_off int32 [B+1] (CSR over the mini-batch non-zeros), wid int32 [N] word ids, cnt f32 [N],
// EbT f32 [V][K] = exp(E[log beta]) transposed, gamma f32 [B][K] (in: initial, out: final),
// contrib f32 [N][K] (out), iters_out int32 [B] (optional: inner iterations per document).
HM_API int hm_lda_estep(const int32_t* doc_off, const int32_t* wid, const float* cnt, const float* EbT, int B,
                        int K, float alpha, float delta, int max_iter, float* gamma, float* contrib,
                        int32_t* iters_out, hipStream_t stream) {
    if (B <= 0) return 0;
    if (K <= 0 || K > 256 || max_iter < 0) return (int)hipErrorInvalidValue;
    const size_t sh = LDA_LDS_FLOATS * sizeof(float);
#define HM_LDA(KC)                                                                                          \
    hipLaunchKernelGGL(lda_estep_kernel<KC>, dim3(B), dim3(256), sh, stream, doc_off, wid, cnt, EbT, K, alpha, \
                       delta, max_iter, gamma, contrib, iters_out)
    if (K <= 64) HM_LDA(1);
    else if (K <= 128) HM_LDA(2);
    else HM_LDA(4);
#undef HM_LDA
    HM_LAUNCH_RET();
}

// uniq int32 [U] (the batch's distinct word ids), lamT f32 [V][K], T f32 [K] (column sums of
// lamT), EbU f32 [U][K] (out).
HM_API int hm_lda_batch_eb(const int32_t* uniq, const float* lamT, const float* T, int U, int K, float* EbU,
                           hipStream_t stream) {
    if (U <= 0) return 0;
    if (K < 1 || K > 256) return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)(((int64_t)U + LDA_EB_WORDS - 1) / LDA_EB_WORDS));
#define HM_LDA_EB(KC) \
    hipLaunchKernelGGL(lda_batch_eb_kernel<KC>, grid, dim3(256), 0, stream, uniq, lamT, T, U, K, EbU)
    if (K <= 64) HM_LDA_EB(1);
    else if (K <= 128) HM_LDA_EB(2);
    else HM_LDA_EB(4);
#undef HM_LDA_EB
    HM_LAUNCH_RET();
}

// hm_lda_estep read through wpos int32 [N] (rank of each non-zero's word in uniq) from EbU f32
// [U][K], plus bound f64 [B] (out): sum_n cnt_n * log(phinorm_n) with the final Et.  A document
// without non-zeros gets gamma = alpha, 0 iterations and bound 0.
HM_API int hm_lda_doc_estep(const int32_t* doc_off, const int32_t* wpos, const float* cnt, const float* EbU,
                            int B, int K, float alpha, float delta, int max_iter, float* gamma, float* contrib,
                            int32_t* iters_out, double* bound, hipStream_t stream) {
    if (B <= 0) return 0;
    if (K < 1 || K > 256 || max_iter < 0 || !iters_out || !bound) return (int)hipErrorInvalidValue;
    const size_t sh = LDA_LDS_FLOATS * sizeof(float);
#define HM_LDA(KC)                                                                                          \
    hipLaunchKernelGGL(lda_doc_estep_kernel<KC>, dim3(B), dim3(256), sh, stream, doc_off, wpos, cnt, EbU, K, \
                       alpha, delta, max_iter, gamma, contrib, iters_out, bound)
    if (K <= 64) HM_LDA(1);
    else if (K <= 128) HM_LDA(2);
    else HM_LDA(4);
#undef HM_LDA
    HM_LAUNCH_RET();
}

// 4-byte words of scratch hm_lda_mstep needs: the tiles' column partials [tiles(V)][K].
HM_API int64_t hm_lda_mstep_scratch_words(int U, int V, int K) {
    if (U < 0 || V < 0 || K < 0) return 0;
    return lda_tiles(V) * K;
}

// word_off int32 [U+1] (runs of perm), perm int32 [N] (non-zero indices sorted by (word, index)),
// uniq int32 [U] (the distinct word ids, ascending), contrib f32 [N][K], lamT f32 [V][K] (in/out),
// T f32 [K] (out: column sums of the new lamT), scratch: hm_lda_mstep_scratch_words(U, V, K) words.
HM_API int hm_lda_mstep(const int32_t* word_off, const int32_t* perm, const int32_t* uniq, const float* contrib,
                        int U, int V, int K, float rho, float eta, float scale, float* lamT, float* T,
                        void* scratch, hipStream_t stream) {
    if (V <= 0) return 0;
    if (U < 0 || U > V || K < 1 || K > 256) return (int)hipErrorInvalidValue;
    const int64_t nb = lda_tiles(V);
    float* part = (float*)scratch;
#define HM_LDA_M(KC)                                                                                        \
    hipLaunchKernelGGL(lda_mstep_kernel<KC>, dim3((unsigned)nb), dim3(256), 0, stream, word_off, perm, uniq, \
                       contrib, U, V, K, rho, eta, scale, lamT, part)
    if (K <= 64) HM_LDA_M(1);
    else if (K <= 128) HM_LDA_M(2);
    else HM_LDA_M(4);
#undef HM_LDA_M
    HM_LAUNCH_RET_IF_ERR();
    int KP = 1;
    while (KP < K) KP *= 2;
    hipLaunchKernelGGL(lda_colsum_kernel, dim3(1), dim3(1024), 0, stream, part, nb, K, KP, T);
    HM_LAUNCH_RET();
}

