// Incremental-EM pLSA (upstream hivemall/topicmodel/IncrementalPLSAModel): the
// per-document EM and the incremental P(w|z) update of train_plsa.
//
// hm_plsa_doc_em: for every document d of a mini-batch, from pzd[k] = 1/K, iterate
//     q[n][k] = pzd[k] * pwzT[w_n][k] / max(sum_k pzd[k] * pwzT[w_n][k], 1e-30)
//     new[k]  = sum_n c_n * q[n][k];   new /= max(sum_k new[k], 1e-30)
//     ch      = mean_k |new[k] - pzd[k]|;   pzd = new
// until ch < delta (per document, as upstream) or max_iter iterations, then emit pzd, the
// iteration count and contrib[n][k] = c_n * q[n][k] with q from the final pzd.
//
// The layout is lda.hip's: one 256-thread workgroup per document, lanes span topics
// (K <= 64 * KC), a word's row of pwzT ([V][K]: contiguous per word) is one coalesced load, the
// normaliser of q is a DPP wave sum, each of the 4 waves accumulates its quarter of the words in
// per-lane registers and the 4 partial sums meet in LDS once per iteration, in wave order.  The
// document's rows are staged in LDS when they fit (the loop re-reads them every iteration) and
// read from global memory otherwise.  The whole loop runs inside the kernel.
//
// hm_plsa_mstep: the update of PLSA.fit on pwzT in place,
//     nwz[w][k] = sum of contrib over the word's run of perm (in perm order)
//     p'        = (1 - alpha) * p + alpha * nwz / max(S_k, 1e-30),   S_k = sum_w nwz[w][k]
//     p''       = p' / T_k,                                          T_k = sum_w p'[w][k]
// without float atomics: a thread owns (word, topic) cells, column sums are per-block partials
// (rows in a fixed stride order, then the block's row groups in order) that a one-block kernel
// adds up in a fixed strided order.  Every order is a function of (U, V, K) alone.
#include "common.h"

namespace {

constexpr int PLSA_LDS_FLOATS = 12 * 1024;     // 48 KB of staged pwzT rows per workgroup
constexpr int PLSA_ROWS_PER_BLOCK = 64;        // M-step: rows (words) of one block's column partial

template <int KC>
__global__ __launch_bounds__(256) void plsa_doc_em_kernel(const int32_t* __restrict__ doc_off,
                                                          const int32_t* __restrict__ wid,
                                                          const float* __restrict__ cnt,
                                                          const float* __restrict__ pwzT, int K, float delta,
                                                          int max_iter, float* __restrict__ pzd,
                                                          float* __restrict__ contrib,
                                                          int32_t* __restrict__ iters_out) {
    __shared__ float s_acc[4][64 * KC];
    __shared__ float s_pzd[64 * KC];
    __shared__ int s_done;
    extern __shared__ float s_pw[];
    const int d = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n0 = doc_off[d], n1 = doc_off[d + 1], nd = n1 - n0;
    if (nd <= 0) {                               // uniform: an empty document
        for (int k = tid; k < K; k += 256) pzd[(size_t)d * K + k] = 0.f;
        if (tid == 0) iters_out[d] = 0;
        return;
    }
    const bool staged = (int64_t)nd * K <= PLSA_LDS_FLOATS;
    if (staged) {
        for (int i = tid; i < nd * K; i += 256) {
            const int n = i / K, k = i - n * K;
            s_pw[i] = pwzT[(size_t)wid[n0 + n] * K + k];
        }
    }
    const float p0 = 1.f / (float)K;
    for (int k = tid; k < 64 * KC; k += 256) s_pzd[k] = k < K ? p0 : 0.f;
    __syncthreads();
    auto pw = [&](int n, int k) -> float {
        return staged ? s_pw[n * K + k] : pwzT[(size_t)wid[n0 + n] * K + k];
    };
    int it = 0;
    while (it < max_iter) {
        float p[KC], acc[KC];
#pragma unroll
        for (int j = 0; j < KC; ++j) {
            p[j] = s_pzd[lane + 64 * j];
            acc[j] = 0.f;
        }
        for (int n = wave; n < nd; n += 4) {
            float t[KC], z = 0.f;
#pragma unroll
            for (int j = 0; j < KC; ++j) {
                const int k = lane + 64 * j;
                t[j] = k < K ? p[j] * pw(n, k) : 0.f;
                z += t[j];
            }
            z = fmaxf(hm::wave_sum_uniform(z), 1e-30f);
            const float c = cnt[n0 + n];
#pragma unroll
            for (int j = 0; j < KC; ++j) acc[j] += c * (t[j] / z);
        }
#pragma unroll
        for (int j = 0; j < KC; ++j) s_acc[wave][lane + 64 * j] = acc[j];
        __syncthreads();
        if (wave == 0) {
            float nw[KC], tot = 0.f;
#pragma unroll
            for (int j = 0; j < KC; ++j) {
                const int k = lane + 64 * j;
                nw[j] = ((s_acc[0][k] + s_acc[1][k]) + s_acc[2][k]) + s_acc[3][k];
                tot += nw[j];
            }
            tot = fmaxf(hm::wave_sum_uniform(tot), 1e-30f);
            float ch = 0.f;
#pragma unroll
            for (int j = 0; j < KC; ++j) {
                const int k = lane + 64 * j;
                nw[j] = nw[j] / tot;             // lanes k >= K hold 0
                ch += fabsf(nw[j] - p[j]);
                s_pzd[k] = nw[j];
            }
            ch = hm::wave_sum_uniform(ch);
            if (lane == 0) s_done = (ch / (float)K < delta) ? 1 : 0;
        }
        __syncthreads();
        ++it;
        if (s_done) break;                       // uniform
    }
    // p(z | d, w) from the final pzd, weighted by the counts
    float p[KC];
#pragma unroll
    for (int j = 0; j < KC; ++j) p[j] = s_pzd[lane + 64 * j];
    for (int n = wave; n < nd; n += 4) {
        float t[KC], z = 0.f;
#pragma unroll
        for (int j = 0; j < KC; ++j) {
            const int k = lane + 64 * j;
            t[j] = k < K ? p[j] * pw(n, k) : 0.f;
            z += t[j];
        }
        z = fmaxf(hm::wave_sum_uniform(z), 1e-30f);
        const float c = cnt[n0 + n];
#pragma unroll
        for (int j = 0; j < KC; ++j) {
            const int k = lane + 64 * j;
            if (k < K) contrib[(size_t)(n0 + n) * K + k] = c * (t[j] / z);
        }
    }
    for (int k = tid; k < K; k += 256) pzd[(size_t)d * K + k] = s_pzd[k];
    if (tid == 0) iters_out[d] = it;
}

// ---------------------------------------------------------------------------------- M-step
// A 256-thread block is RG = 256 / KP row groups of KP column lanes (KP: the power of two >= K);
// thread (g, k) owns column k of rows lo + g, lo + g + RG, ... of the block's
// PLSA_ROWS_PER_BLOCK rows.  column_partial adds the row groups' sums in group order.
__device__ __forceinline__ void column_partial(float col, float* __restrict__ part, int K, int KP) {
    __shared__ float s_col[256];
    s_col[threadIdx.x] = col;
    __syncthreads();
    const int k = threadIdx.x;
    if (k < K) {                                 // K <= KP: threads of row group 0
        float s = s_col[k];
        for (int t = KP + k; t < 256; t += KP) s += s_col[t];
        part[(size_t)blockIdx.x * K + k] = s;
    }
}

__global__ __launch_bounds__(256) void plsa_nwz_kernel(const int32_t* __restrict__ word_off,
                                                       const int32_t* __restrict__ perm,
                                                       const int32_t* __restrict__ uniq,
                                                       const float* __restrict__ contrib, int U, int K, int KP,
                                                       int32_t* __restrict__ inv, float* __restrict__ nwz,
                                                       float* __restrict__ part) {
    const int RG = 256 / KP, g = threadIdx.x / KP, k = threadIdx.x & (KP - 1);
    const int lo = blockIdx.x * PLSA_ROWS_PER_BLOCK, hi = min(U, lo + PLSA_ROWS_PER_BLOCK);
    float col = 0.f;
    if (k < K) {
        for (int u = lo + g; u < hi; u += RG) {
            float s = 0.f;
            for (int j = word_off[u], j1 = word_off[u + 1]; j < j1; ++j) s += contrib[(size_t)perm[j] * K + k];
            nwz[(size_t)u * K + k] = s;
            col += s;
            if (k == 0) inv[uniq[u]] = u;
        }
    }
    column_partial(col, part, K, KP);
}

// out[k] = sum_b part[b][k] in one 1024-thread block: row group g of 1024 / KP adds partials
// g, g + RG, ... in order, then the groups are added in group order.
__global__ __launch_bounds__(1024) void plsa_colsum_kernel(const float* __restrict__ part, int nb, int K, int KP,
                                                           float* __restrict__ out) {
    __shared__ float s_col[1024];
    const int RG = 1024 / KP, g = threadIdx.x / KP, k = threadIdx.x & (KP - 1);
    float s = 0.f;
    if (k < K)
        for (int b = g; b < nb; b += RG) s += part[(size_t)b * K + k];
    s_col[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x < K) {
        float t = s_col[threadIdx.x];
        for (int i = KP + threadIdx.x; i < 1024; i += KP) t += s_col[i];
        out[threadIdx.x] = t;
    }
}

__global__ __launch_bounds__(256) void plsa_blend_kernel(const int32_t* __restrict__ inv,
                                                         const float* __restrict__ nwz,
                                                         const float* __restrict__ S, int V, int K, int KP,
                                                         float alpha, float* __restrict__ pwzT,
                                                         float* __restrict__ part) {
    const int RG = 256 / KP, g = threadIdx.x / KP, k = threadIdx.x & (KP - 1);
    const int lo = blockIdx.x * PLSA_ROWS_PER_BLOCK, hi = min(V, lo + PLSA_ROWS_PER_BLOCK);
    float col = 0.f;
    if (k < K) {
        const float sk = fmaxf(S[k], 1e-30f), keep = 1.f - alpha;
        for (int w = lo + g; w < hi; w += RG) {
            const int u = inv[w];
            float v = keep * pwzT[(size_t)w * K + k];
            if (u >= 0) v += alpha * (nwz[(size_t)u * K + k] / sk);
            pwzT[(size_t)w * K + k] = v;
            col += v;
        }
    }
    column_partial(col, part, K, KP);
}

__global__ __launch_bounds__(256) void plsa_norm_kernel(const float* __restrict__ T, int V, int K, int KP,
                                                        float* __restrict__ pwzT) {
    const int RG = 256 / KP, g = threadIdx.x / KP, k = threadIdx.x & (KP - 1);
    const int lo = blockIdx.x * PLSA_ROWS_PER_BLOCK, hi = min(V, lo + PLSA_ROWS_PER_BLOCK);
    if (k >= K) return;
    const float tk = T[k];
    for (int w = lo + g; w < hi; w += RG) pwzT[(size_t)w * K + k] = pwzT[(size_t)w * K + k] / tk;
}

__host__ __device__ inline int64_t blocks_of(int64_t rows) {
    return (rows + PLSA_ROWS_PER_BLOCK - 1) / PLSA_ROWS_PER_BLOCK;
}

}  // namespace

// Rows of pwzT (in floats: rows * K) that hm_plsa_doc_em stages in LDS for one document.
HM_API int hm_plsa_stage_floats() { return PLSA_LDS_FLOATS; }

// doc_off int32 [B+1] (CSR over the mini-batch non-zeros), wid int32 [N] word ids, cnt f32 [N],
// pwzT f32 [V][K] = P(w|z) transposed, pzd f32 [B][K] (out), contrib f32 [N][K] (out),
// iters_out int32 [B] (out: EM iterations per document).
HM_API int hm_plsa_doc_em(const int32_t* doc_off, const int32_t* wid, const float* cnt, const float* pwzT,
                          int B, int K, float delta, int max_iter, float* pzd, float* contrib,
                          int32_t* iters_out, hipStream_t stream) {
    if (B <= 0) return 0;
    if (K < 1 || K > 256 || max_iter < 0) return (int)hipErrorInvalidValue;
    const size_t sh = PLSA_LDS_FLOATS * sizeof(float);
#define HM_PLSA_EM(KC)                                                                                   \
    hipLaunchKernelGGL(plsa_doc_em_kernel<KC>, dim3(B), dim3(256), sh, stream, doc_off, wid, cnt, pwzT, K, \
                       delta, max_iter, pzd, contrib, iters_out)
    if (K <= 64) HM_PLSA_EM(1);
    else if (K <= 128) HM_PLSA_EM(2);
    else HM_PLSA_EM(4);
#undef HM_PLSA_EM
    HM_LAUNCH_RET();
}

// 4-byte words of scratch hm_plsa_mstep needs: inv int32 [V] | nwz [U][K] | column partials of
// nwz | S [K] | column partials of p' | T [K].
HM_API int64_t hm_plsa_mstep_scratch_words(int U, int V, int K) {
    if (U < 0 || V < 0 || K < 0) return 0;
    return (int64_t)V + (int64_t)U * K + (blocks_of(U) + blocks_of(V) + 2) * K;
}

// word_off int32 [U+1] (runs of perm), perm int32 [N] (non-zero indices sorted by (word, index)),
// uniq int32 [U] (the distinct word ids, ascending), contrib f32 [N][K], pwzT f32 [V][K] (in/out),
// scratch: hm_plsa_mstep_scratch_words(U, V, K) words.
HM_API int hm_plsa_mstep(const int32_t* word_off, const int32_t* perm, const int32_t* uniq,
                         const float* contrib, int U, int V, int K, float alpha, float* pwzT, void* scratch,
                         hipStream_t stream) {
    if (V <= 0) return 0;
    if (U < 0 || U > V || K < 1 || K > 256) return (int)hipErrorInvalidValue;
    const int nbu = (int)blocks_of(U), nbv = (int)blocks_of(V);
    int32_t* inv = (int32_t*)scratch;
    float* nwz = (float*)scratch + V;
    float* part_s = nwz + (size_t)U * K;
    float* S = part_s + (size_t)nbu * K;
    float* part_t = S + K;
    float* T = part_t + (size_t)nbv * K;
    const hipError_t e = hipMemsetAsync(inv, 0xFF, (size_t)V * sizeof(int32_t), stream);   // -1
    if (e != hipSuccess) return (int)e;
    int KP = 1;
    while (KP < K) KP *= 2;
    if (nbu > 0)
        hipLaunchKernelGGL(plsa_nwz_kernel, dim3(nbu), dim3(256), 0, stream, word_off, perm, uniq, contrib, U, K,
                           KP, inv, nwz, part_s);
    hipLaunchKernelGGL(plsa_colsum_kernel, dim3(1), dim3(1024), 0, stream, part_s, nbu, K, KP, S);
    hipLaunchKernelGGL(plsa_blend_kernel, dim3(nbv), dim3(256), 0, stream, inv, nwz, S, V, K, KP, alpha, pwzT,
                       part_t);
    HM_LAUNCH_RET_IF_ERR();
    hipLaunchKernelGGL(plsa_colsum_kernel, dim3(1), dim3(1024), 0, stream, part_t, nbv, K, KP, T);
    hipLaunchKernelGGL(plsa_norm_kernel, dim3(nbv), dim3(256), 0, stream, T, V, K, KP, pwzT);
    HM_LAUNCH_RET();
}
