// SLIM recommendation on gfx950: sparse score + top-k fused, one workgroup per user.
//
//   score(u, i) = 0.0 + mw[i, nn_1] * r[u, nn_1] + mw[i, nn_2] * r[u, nn_2] + ...   (nn ascending,
//   only the nn of model row i that u has rated; fp64, every product rounded before its add)
//
// Item i is a candidate of u when at least one term exists; with `exclude` the user's own items
// are none.  The k best under "score descending, then item ascending" go out, padded with
// item -1 / score -inf.  docs/compat.md "SLIM recommendation" is the contract; the C++ twin is
// hm_slim_topk_cpu in csrc/host/slim_cpu.cpp.
//
// Why this shape.  A user's candidates are the union of the transposed-model rows of the items
// they rated: ~144 rows of ~50 entries on ML-20M, with many repeats.  Scoring by scatter (one
// atomic add per (rated item, target) pair) would make the sum's order depend on the schedule, so
// the kernel only uses the scatter to find WHO is a candidate and gathers every score afterwards:
//
//   1. mark     one wave per rated item walks its transposed-model row (tptr / ti) and sets the
//               target's bit in an LDS bitmap with atomicOr: deduplication for free.  The bitmap
//               covers a window of `words * 32` items (words <= ST_MAX_WORDS, 64 KiB = 524288
//               items; the launcher sizes it to the item count, so ML-20M's 27278 items take
//               3.4 KiB, twice with the bitmap of step 3, and four workgroups share a CU).  More
//               items than one window: the user is
//               walked once per window, every window feeding the same best-k list.
//               With `exclude` the user's own bits are cleared again (atomicAnd).
//   2. compact  256 bits a round, one per thread; ballots and popcounts place the set ones behind
//               each other in s_cand in ascending item order, no sort.
//   3. score    whenever s_cand may not take another round: one lane per candidate walks the
//               candidate's model row in order and looks each nn up: first in a second LDS bitmap,
//               of the items the user rated (kept when all items fit one window; most neighbours
//               are not rated and one LDS read says so), then, on a hit, in the user's rated slice
//               (staged in LDS when it has at most ST_RMAX entries, in global memory otherwise; nn
//               and the slice both ascend, so the lower bound of a lookup is the previous hit).
//               One lane adds one candidate's terms in their order: no floating-point atomics, no
//               tree, the same bits as the twin's loop.
//   4. top-k    the score becomes a u64 key that sorts best first, the pair (key, item) is a total
//               order.  Pairs that beat the list's k-th (the threshold, in registers) are appended
//               behind the sorted best-k list in LDS by wave ballot; the buffer is sorted
//               (bitonic) and cut to k when the next batch may not fit.  Same scheme as
//               each_top_k.hip's long segments, with the item index in the place of the position.
//
// The library is built with -ffp-contract=fast, which fuses across a contract pragma; the product
// therefore passes through an empty asm statement (as in pair_sim.hip).
#include "common.h"
#include "slim_topk_key.h"                 // st_key / st_unkey / st_better, shared with the twin

namespace {

constexpr int ST_THREADS = 256;
constexpr int ST_WAVES = ST_THREADS / HM_WAVE;
constexpr int ST_KMAX = 256;
constexpr int ST_MAX_WORDS = 16384;        // bitmap window: 64 KiB of LDS, 524288 items
constexpr int ST_RMAX = 1024;              // rated entries staged in LDS (12 KiB)
constexpr int ST_CBUF = 1024;              // candidate buffer: scored when a round may not fit
constexpr int ST_TKBUF = 1024;             // best-k list + survivors: sorted when a batch may not fit
constexpr int ST_AHEAD = 8;                // neighbours of a model row loaded together

// A product as a value of its own: nothing fuses across the (empty) asm statement.
__device__ __forceinline__ double st_rounded(double x) {
    asm volatile("" : "+v"(x));
    return x;
}

// Sorts s_key/s_item[0, n) best first (bitonic over the next power of two, the tail padded with
// the worst pair).  Every thread calls it with the same n <= ST_TKBUF.
__device__ __forceinline__ void st_sort(uint64_t* s_key, uint32_t* s_item, int n, int tid) {
    int n2 = 2;
    while (n2 < n) n2 <<= 1;
    for (int i = n + tid; i < n2; i += ST_THREADS) {
        s_key[i] = ST_WORST_KEY;
        s_item[i] = ST_WORST_ITEM;
    }
    __syncthreads();
    for (int size = 2; size <= n2; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < (n2 >> 1); t += ST_THREADS) {
                const int i = ((t & ~(stride - 1)) << 1) | (t & (stride - 1));
                const int j = i | stride;
                const uint64_t ki = s_key[i], kj = s_key[j];
                const uint32_t pi = s_item[i], pj = s_item[j];
                const bool up = (i & size) == 0;   // this run ends best first
                if (up ? st_better(kj, pj, ki, pi) : st_better(ki, pi, kj, pj)) {
                    s_key[i] = kj; s_item[i] = pj;
                    s_key[j] = ki; s_item[j] = pi;
                }
            }
            __syncthreads();
        }
    }
}

// score(u, i): model row i against the ascending rated slice rc / rv [0, nr).  rbits, when there
// is one, has a bit per item the user rated (n_bits of them): most neighbours are not rated, and
// one LDS read says so.
template <typename Index>
__device__ __forceinline__ double st_score(const int32_t* rc, const double* rv, Index nr,
                                           const uint32_t* rbits, uint32_t n_bits,
                                           const int32_t* __restrict__ mnn,
                                           const double* __restrict__ mw, int64_t q0, int64_t q1) {
    double acc = 0.0;
    Index from = 0;                                // every rated entry before it is below nn
    // The row is read ST_AHEAD neighbours at a time, the loads independent of each other: taken one
    // by one, every neighbour costs a trip to L2 on a chain nothing else hides (measured: the
    // lookups themselves did not show in the kernel's time).
    for (int64_t qb = q0; qb < q1 && from < nr; qb += ST_AHEAD) {
        int32_t ahead[ST_AHEAD];
#pragma unroll
        for (int j = 0; j < ST_AHEAD; ++j) ahead[j] = qb + j < q1 ? mnn[qb + j] : -1;
#pragma unroll
        for (int j = 0; j < ST_AHEAD; ++j) {
            const int32_t nn = ahead[j];
            if (nn < 0) continue;                  // past the row's end
            if (rbits && ((uint32_t)nn >= n_bits || !((rbits[nn >> 5] >> (nn & 31)) & 1u))) continue;
            Index lo = from, hi = nr;
            while (lo < hi) {
                const Index mid = lo + ((hi - lo) >> 1);
                if (rc[mid] < nn) lo = mid + 1;
                else hi = mid;
            }
            from = lo;
            if (lo < nr && rc[lo] == nn) acc = acc + st_rounded(mw[qb + j] * rv[lo]);
        }
    }
    return acc;
}

struct StTopk {
    uint64_t* key;
    uint32_t* item;
    int* cnt;
    uint64_t thr_key;                              // the list's k-th pair once it holds k
    uint32_t thr_item;
};

// Scores s_cand[0, n) and feeds the pairs that beat the threshold to the best-k list.  Every
// thread calls it with the same n <= ST_CBUF; ends behind a barrier.
__device__ __forceinline__ void st_score_all(
    const int32_t* s_cand, int n, const int32_t* s_rc, const double* s_rv,
    const int32_t* __restrict__ gcols, const double* __restrict__ gvals, int64_t nr, bool staged,
    const uint32_t* rbits, uint32_t n_bits, const int64_t* __restrict__ mptr, const int32_t* __restrict__ mnn,
    const double* __restrict__ mw, int k, StTopk& tk) {
    const int tid = threadIdx.x, lane = hm::lane_id();
    for (int b = 0; b < n; b += ST_THREADS) {
        // *tk.cnt <= ST_TKBUF - ST_THREADS here, so a batch of survivors stays inside the buffer
        const int c = b + tid;
        bool live = false;
        uint64_t key = ST_WORST_KEY;
        uint32_t item = ST_WORST_ITEM;
        if (c < n) {
            item = (uint32_t)s_cand[c];
            const int64_t q0 = mptr[item], q1 = mptr[item + 1];
            const double s =
                staged ? st_score<int>(s_rc, s_rv, (int)nr, rbits, n_bits, mnn, mw, q0, q1)
                       : st_score<int64_t>(gcols, gvals, nr, rbits, n_bits, mnn, mw, q0, q1);
            key = st_key(s);
            live = st_better(key, item, tk.thr_key, tk.thr_item);
        }
        const unsigned long long m = __ballot(live);
        if (m) {                                   // wave-uniform
            int at = 0;
            if (lane == 0) at = atomicAdd(tk.cnt, __popcll(m));
            at = __builtin_amdgcn_readfirstlane(at);
            if (live) {
                const int slot = at + __popcll(m & ((1ull << lane) - 1ull));
                tk.key[slot] = key;
                tk.item[slot] = item;
            }
        }
        __syncthreads();
        const int cnt = *tk.cnt;
        __syncthreads();                           // read by all before the next batch adds to it
        if (cnt > ST_TKBUF - ST_THREADS) {         // uniform: the next batch might not fit
            st_sort(tk.key, tk.item, cnt, tid);
            if (cnt >= k) {
                tk.thr_key = tk.key[k - 1];
                tk.thr_item = tk.item[k - 1];
            }
            __syncthreads();                       // everyone has read the threshold
            if (tid == 0) *tk.cnt = min(cnt, k);
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(ST_THREADS) void slim_topk_kernel(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ cols,
    const double* __restrict__ vals, const int64_t* __restrict__ mptr,
    const int32_t* __restrict__ mnn, const double* __restrict__ mw,
    const int64_t* __restrict__ tptr, const int32_t* __restrict__ ti, int I, int words, int rwords,
    int k, int exclude, int32_t* __restrict__ items, double* __restrict__ scores) {
    extern __shared__ uint32_t s_bits[];           // [words] candidates, then [rwords] rated items
    __shared__ double s_rv[ST_RMAX];
    __shared__ int32_t s_rc[ST_RMAX];
    __shared__ int32_t s_cand[ST_CBUF];
    __shared__ uint64_t s_key[ST_TKBUF];
    __shared__ uint32_t s_item[ST_TKBUF];
    __shared__ int s_cnt;                          // pairs in the top-k buffer, the list included
    __shared__ int s_wcnt[ST_WAVES];

    const int tid = threadIdx.x, lane = hm::lane_id(), wave = hm::wave_id();
    const int64_t u = blockIdx.x;
    const int64_t r0 = rowptr[u], r1 = rowptr[u + 1];
    const int64_t nr = r1 - r0;
    const bool staged = nr <= ST_RMAX;
    if (staged)
        for (int e = tid; e < (int)nr; e += ST_THREADS) {
            s_rc[e] = cols[r0 + e];
            s_rv[e] = vals[r0 + e];
        }
    if (tid == 0) s_cnt = 0;
    StTopk tk{s_key, s_item, &s_cnt, ST_WORST_KEY, ST_WORST_ITEM};
    // the rated items as a bitmap over all I items, where one window holds them all (rwords > 0)
    uint32_t* s_rbits = rwords ? s_bits + words : nullptr;
    const uint32_t n_bits = (uint32_t)I;           // rwords * 32 >= I
    if (rwords) {
        for (int w = tid; w < rwords; w += ST_THREADS) s_rbits[w] = 0u;
        __syncthreads();
        for (int64_t p = r0 + tid; p < r1; p += ST_THREADS) {
            const int32_t c = cols[p];
            if ((uint32_t)c < n_bits) atomicOr(&s_rbits[c >> 5], 1u << (c & 31));
        }
    }

    const int64_t bits = (int64_t)words * 32;
    int ncand = 0;                                 // entries of s_cand, the same in every thread
    for (int64_t base = 0; base < I && nr > 0; base += bits) {
        const int wbits = (int)min(bits, (int64_t)I - base);
        const int wwords = (wbits + 31) >> 5;
        for (int w = tid; w < wwords; w += ST_THREADS) s_bits[w] = 0u;
        __syncthreads();
        // 1. mark: wave per rated item, lanes over its transposed-model row
        for (int64_t p = r0 + wave; p < r1; p += ST_WAVES) {
            const int32_t c = cols[p];
            if ((uint32_t)c >= (uint32_t)I) continue;
            const int64_t t1 = tptr[c + 1];
            for (int64_t q = tptr[c] + lane; q < t1; q += HM_WAVE) {
                const int64_t d = (int64_t)ti[q] - base;
                if (d >= 0 && d < wbits) atomicOr(&s_bits[d >> 5], 1u << (d & 31));
            }
        }
        __syncthreads();
        if (exclude) {
            for (int64_t p = r0 + tid; p < r1; p += ST_THREADS) {
                const int64_t d = (int64_t)cols[p] - base;
                if (d >= 0 && d < wbits) atomicAnd(&s_bits[d >> 5], ~(1u << (d & 31)));
            }
            __syncthreads();
        }
        // 2. compact, 3. score when the buffer may not take another round
        for (int wb = 0; wb < wwords; wb += ST_THREADS / 32) {
            const int w = wb + (tid >> 5);
            const bool set = w < wwords && ((s_bits[w] >> (tid & 31)) & 1u);
            const unsigned long long m = __ballot(set);
            if (lane == 0) s_wcnt[wave] = __popcll(m);
            __syncthreads();
            int before = 0, total = 0;
#pragma unroll
            for (int x = 0; x < ST_WAVES; ++x) {
                const int n = s_wcnt[x];
                before += x < wave ? n : 0;
                total += n;
            }
            if (set)
                s_cand[ncand + before + __popcll(m & ((1ull << lane) - 1ull))] =
                    (int32_t)(base + (int64_t)w * 32 + (tid & 31));
            ncand += total;
            __syncthreads();                       // s_cand written, s_wcnt read
            if (ncand > ST_CBUF - ST_THREADS) {    // uniform
                st_score_all(s_cand, ncand, s_rc, s_rv, cols + r0, vals + r0, nr, staged, s_rbits,
                             n_bits, mptr, mnn, mw, k, tk);
                ncand = 0;
            }
        }
    }
    __syncthreads();                               // s_cnt = 0 and the staged slice, for a user without a window
    st_score_all(s_cand, ncand, s_rc, s_rv, cols + r0, vals + r0, nr, staged, s_rbits, n_bits, mptr, mnn,
                 mw, k, tk);

    const int cnt = s_cnt;
    st_sort(s_key, s_item, cnt, tid);
    const int n_out = min(cnt, k);
    for (int r = tid; r < k; r += ST_THREADS) {
        const bool in = r < n_out;
        items[u * k + r] = in ? (int32_t)s_item[r] : -1;
        scores[u * k + r] = in ? st_unkey(s_key[r]) : -__builtin_inf();
    }
}

}  // namespace

// Ratings as user-major CSR: rowptr int64 [U + 1], cols int32 ascending inside a row, vals fp64.
// The model as CSR over the I target items: mptr int64 [I + 1], mnn int32 ascending inside a row,
// mw fp64; and transposed: tptr int64 [I + 1], ti int32 = the targets of every neighbour.
// items int32 [U, k], scores fp64 [U, k]: the k best candidates of every user, best first, padded
// with -1 / -inf.  1 <= k <= 256.
HM_API int hm_slim_topk(const int64_t* rowptr, const int32_t* cols, const double* vals, int64_t U,
                        const int64_t* mptr, const int32_t* mnn, const double* mw,
                        const int64_t* tptr, const int32_t* ti, int I, int k, int exclude,
                        int32_t* items, double* scores, hipStream_t stream) {
    if (U <= 0) return 0;
    if (U > INT32_MAX || I < 0 || k < 1 || k > ST_KMAX) return (int)hipErrorInvalidValue;
    const int need = (int)(((int64_t)I + 31) / 32);
    const int words = need < 1 ? 1 : (need > ST_MAX_WORDS ? ST_MAX_WORDS : need);
    const int rwords = need <= ST_MAX_WORDS ? words : 0;
    // per launch, not once per process: the attribute belongs to the current device's copy of the
    // kernel, and a flag shared by threads would race.  It is a host-side setting, no stream work.
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&slim_topk_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize,
                                             2 * ST_MAX_WORDS * (int)sizeof(uint32_t));
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(slim_topk_kernel, dim3((unsigned)U), dim3(ST_THREADS),
                       (size_t)(words + rwords) * sizeof(uint32_t), stream, rowptr, cols, vals, mptr,
                       mnn, mw, tptr, ti, I, words, rwords, k, exclude, items, scores);
    HM_LAUNCH_RET();
}
