// Segmented top-k on gfx950: the engine behind each_top_k(k, group, score, cols...).
//
// The rows, sorted stably by group code, form G segments (segptr).  Inside a segment the order is
// total: the pair (key, p), key = the fp64 score mapped to a u64 that sorts best first, p = the
// row's position in the sorted order.  Smaller pair = better; no two rows share a pair, so the
// result is one integer array whatever the schedule.  Integer compares only.
//
//   hm_each_top_k        every segment of 1..ETK_WAVE_SEG_MAX rows: one wave per segment, a row's
//                        rank is the number of rows of its segment that beat it, rows of rank < k
//                        are stored at outptr[g] + rank.  Longer segments are left alone.
//   hm_each_top_k_items  a list of work items, one workgroup each.  An item streams a range of
//                        rows (level 0: scores, through perm) or of candidate pairs (a later
//                        level) and keeps its best k: a sorted list in LDS, the list's k-th pair
//                        as threshold in registers, survivors compacted behind the list by wave
//                        ballot, list + survivors sorted when the buffer may fill.  A final item
//                        (its range is a whole segment) writes rows; any other writes its best k
//                        as candidate pairs, which the wrapper feeds to the next level.
//
// The C++ twin is csrc/host/each_top_k_cpu.cpp.
#include "common.h"

namespace {

constexpr int ETK_THREADS = 256;
constexpr int ETK_WAVES = ETK_THREADS / HM_WAVE;
constexpr int ETK_KMAX = 128;              // cosine_knn's limit; the list is a quarter of a round
// One wave per segment, ETK_WAVE_SEG_MAX / 64 = 4 rows per lane: a 2 KiB key tile per wave, and
// len * 4 compares per lane.  Above it the counting loop (quadratic in len) loses to the
// streaming filter.
constexpr int ETK_WAVE_SEG_MAX = 256;
// A round is ETK_PER_THREAD rows per thread, loaded together (4 loads in flight per lane), and
// one barrier.  The sort buffer holds a full list-plus-survivors state (<= ETK_ROUND) and one
// round in which every row survives: 2048 pairs, 24 KiB of LDS, so six workgroups fit a CU.
constexpr int ETK_PER_THREAD = 4;
constexpr int ETK_ROUND = ETK_THREADS * ETK_PER_THREAD;    // 1024
constexpr int ETK_BUF = 2 * ETK_ROUND;                     // 2048
constexpr uint64_t ETK_WORST_KEY = ~0ull;  // no finite or infinite score maps here (a NaN would)
constexpr uint32_t ETK_WORST_POS = 0xffffffffu;

// fp64 -> u64, smaller = better.  -0.0 folds onto 0.0; the sign trick makes the bits sort like
// the value ascending; `flip` (all ones for largest-first) reverses that.
__device__ __forceinline__ uint64_t etk_key(double s, uint64_t flip) {
    uint64_t b = (uint64_t)__double_as_longlong(s);
    if ((b << 1) == 0) b = 0;
    const uint64_t u = b ^ ((b >> 63) ? ~0ull : 0x8000000000000000ull);
    return u ^ flip;
}

__device__ __forceinline__ bool etk_better(uint64_t k1, uint32_t p1, uint64_t k2, uint32_t p2) {
    return k1 < k2 || (k1 == k2 && p1 < p2);
}

// ------------------------------------------------------------------ short segments
template <int T>
__device__ __forceinline__ void etk_wave_rank(const uint64_t* __restrict__ tile, int len, int lane,
                                              const uint64_t (&key)[4], int (&rank)[4]) {
#pragma unroll
    for (int t = 0; t < T; ++t) rank[t] = 0;
    for (int j = 0; j < len; ++j) {
        const uint64_t kj = tile[j];               // one address per wave: a broadcast read
#pragma unroll
        for (int t = 0; t < T; ++t)
            rank[t] += (int)(kj < key[t] || (kj == key[t] && j < lane + HM_WAVE * t));
    }
}

__global__ __launch_bounds__(ETK_THREADS) void etk_wave_kernel(
    const double* __restrict__ score, const int32_t* __restrict__ perm,
    const int64_t* __restrict__ segptr, const int64_t* __restrict__ outptr, int G, int k,
    uint64_t flip, int32_t* __restrict__ rows) {
    __shared__ uint64_t s_tile[ETK_WAVES][ETK_WAVE_SEG_MAX];
    const int lane = hm::lane_id(), wave = hm::wave_id();
    const int64_t g = (int64_t)blockIdx.x * ETK_WAVES + wave;
    int64_t p0 = 0;
    int len = 0;
    if (g < G) {
        p0 = segptr[g];
        const int64_t l = segptr[g + 1] - p0;
        len = (l >= 1 && l <= ETK_WAVE_SEG_MAX) ? (int)l : 0;      // wave-uniform
    }
    uint64_t key[4];
    int32_t row[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int e = lane + HM_WAVE * t;
        key[t] = ETK_WORST_KEY;
        row[t] = 0;
        if (e < len) {
            row[t] = perm ? perm[p0 + e] : (int32_t)(p0 + e);
            key[t] = etk_key(score[row[t]], flip);
            s_tile[wave][e] = key[t];
        }
    }
    __syncthreads();
    if (len == 0) return;
    int rank[4] = {0, 0, 0, 0};
    const uint64_t* tile = s_tile[wave];
    if (len <= HM_WAVE) etk_wave_rank<1>(tile, len, lane, key, rank);
    else if (len <= 2 * HM_WAVE) etk_wave_rank<2>(tile, len, lane, key, rank);
    else if (len <= 3 * HM_WAVE) etk_wave_rank<3>(tile, len, lane, key, rank);
    else etk_wave_rank<4>(tile, len, lane, key, rank);
    const int64_t o0 = outptr[g];
#pragma unroll
    for (int t = 0; t < 4; ++t)
        if (lane + HM_WAVE * t < len && rank[t] < k) rows[o0 + rank[t]] = row[t];   // rank < min(k, len)
}

// ------------------------------------------------------------------ long segments
// Sorts s_key/s_pos[0, n) best first (bitonic over the next power of two, the tail padded with
// the worst pair).  Every thread calls it with the same n <= ETK_BUF.
__device__ __forceinline__ void etk_sort(uint64_t* s_key, uint32_t* s_pos, int n, int tid) {
    int n2 = 2;
    while (n2 < n) n2 <<= 1;
    for (int i = n + tid; i < n2; i += ETK_THREADS) {
        s_key[i] = ETK_WORST_KEY;
        s_pos[i] = ETK_WORST_POS;
    }
    __syncthreads();
    for (int size = 2; size <= n2; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < (n2 >> 1); t += ETK_THREADS) {
                const int i = ((t & ~(stride - 1)) << 1) | (t & (stride - 1));
                const int j = i | stride;
                const uint64_t ki = s_key[i], kj = s_key[j];
                const uint32_t pi = s_pos[i], pj = s_pos[j];
                const bool up = (i & size) == 0;   // this run ends best first
                if (up ? etk_better(kj, pj, ki, pi) : etk_better(ki, pi, kj, pj)) {
                    s_key[i] = kj; s_pos[i] = pj;
                    s_key[j] = ki; s_pos[j] = pi;
                }
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(ETK_THREADS) void etk_items_kernel(
    const double* __restrict__ score, const int32_t* __restrict__ perm,
    const uint64_t* __restrict__ ckey, const uint32_t* __restrict__ cpos,
    const int64_t* __restrict__ item_begin, const int64_t* __restrict__ item_end,
    const int64_t* __restrict__ item_dst, const int64_t* __restrict__ item_final, int k,
    uint64_t flip, uint64_t* __restrict__ okey, uint32_t* __restrict__ opos,
    int32_t* __restrict__ rows) {
    __shared__ uint64_t s_key[ETK_BUF];
    __shared__ uint32_t s_pos[ETK_BUF];
    __shared__ int s_cnt;                          // pairs in the buffer, the list included

    const int tid = threadIdx.x, lane = hm::lane_id();
    const int64_t w = blockIdx.x;
    const int64_t begin = item_begin[w], end = item_end[w];
    if (tid == 0) s_cnt = 0;
    __syncthreads();

    uint64_t thr_key = ETK_WORST_KEY;              // the list's k-th pair once it holds k
    uint32_t thr_pos = ETK_WORST_POS;
    for (int64_t base = begin; base < end; base += ETK_ROUND) {
        // s_cnt <= ETK_ROUND here, so a round of survivors stays inside the buffer
        uint64_t key[ETK_PER_THREAD];
        uint32_t pos[ETK_PER_THREAD];
#pragma unroll
        for (int t = 0; t < ETK_PER_THREAD; ++t) {
            const int64_t i = base + t * ETK_THREADS + tid;
            key[t] = ETK_WORST_KEY;
            pos[t] = ETK_WORST_POS;
            if (i < end) {
                if (ckey) {
                    key[t] = ckey[i];
                    pos[t] = cpos[i];
                } else {
                    key[t] = etk_key(score[perm ? perm[i] : (int32_t)i], flip);
                    pos[t] = (uint32_t)i;
                }
            }
        }
#pragma unroll
        for (int t = 0; t < ETK_PER_THREAD; ++t) {
            const bool in = base + t * ETK_THREADS + tid < end;
            const bool live = in && etk_better(key[t], pos[t], thr_key, thr_pos);
            const unsigned long long m = __ballot(live);
            if (m) {                               // wave-uniform
                int at = 0;
                if (lane == 0) at = atomicAdd(&s_cnt, __popcll(m));
                at = __builtin_amdgcn_readfirstlane(at);
                if (live) {
                    const int slot = at + __popcll(m & ((1ull << lane) - 1ull));
                    s_key[slot] = key[t];
                    s_pos[slot] = pos[t];
                }
            }
        }
        __syncthreads();
        const int cnt = s_cnt;
        __syncthreads();                           // read by all before the next round adds to it
        if (cnt > ETK_ROUND) {                     // uniform: the next round might not fit
            etk_sort(s_key, s_pos, cnt, tid);
            if (cnt >= k) {
                thr_key = s_key[k - 1];
                thr_pos = s_pos[k - 1];
            }
            __syncthreads();                       // everyone has read cnt and the threshold
            if (tid == 0) s_cnt = min(cnt, k);
            __syncthreads();
        }
    }
    const int cnt = s_cnt;
    etk_sort(s_key, s_pos, cnt, tid);
    const int n_out = min(cnt, k);
    const int64_t dst = item_dst[w];
    if (item_final[w]) {
        for (int r = tid; r < n_out; r += ETK_THREADS) {
            const uint32_t p = s_pos[r];
            rows[dst + r] = perm ? perm[p] : (int32_t)p;
        }
    } else {
        for (int r = tid; r < n_out; r += ETK_THREADS) {
            okey[dst + r] = s_key[r];
            opos[dst + r] = s_pos[r];
        }
    }
}

}  // namespace

// score fp64 [n]; perm int32 [n] = the rows sorted stably by group code, or NULL when the codes
// are non-decreasing already; segptr int64 [G + 1]; outptr int64 [G + 1] = running sum of
// min(k, len); rows int32 [outptr[G]].  Fills the output of every segment of
// 1..ETK_WAVE_SEG_MAX rows; 1 <= k <= 128.
HM_API int hm_each_top_k(const double* score, const int32_t* perm, const int64_t* segptr,
                         const int64_t* outptr, int G, int k, int largest, int32_t* rows,
                         hipStream_t stream) {
    if (G <= 0) return 0;
    if (k < 1 || k > ETK_KMAX) return (int)hipErrorInvalidValue;
    const unsigned grid = (unsigned)(((int64_t)G + ETK_WAVES - 1) / ETK_WAVES);
    hipLaunchKernelGGL(etk_wave_kernel, dim3(grid), dim3(ETK_THREADS), 0, stream, score, perm, segptr,
                       outptr, G, k, largest ? ~0ull : 0ull, rows);
    HM_LAUNCH_RET();
}

// W work items.  Item w selects the best min(k, end - begin) pairs of positions
// [item_begin[w], item_end[w]): of the sorted rows when ckey is NULL, of the candidate pairs
// (ckey u64, cpos u32) otherwise.  item_final[w] != 0: their row ids go to rows[item_dst[w] ...],
// best first; else the pairs go to (okey, opos)[item_dst[w] ...].
HM_API int hm_each_top_k_items(const double* score, const int32_t* perm, const uint64_t* ckey,
                               const uint32_t* cpos, const int64_t* item_begin,
                               const int64_t* item_end, const int64_t* item_dst,
                               const int64_t* item_final, int64_t W, int k, int largest,
                               uint64_t* okey, uint32_t* opos, int32_t* rows, hipStream_t stream) {
    if (W <= 0) return 0;
    if (W > INT32_MAX || k < 1 || k > ETK_KMAX) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(etk_items_kernel, dim3((unsigned)W), dim3(ETK_THREADS), 0, stream, score, perm,
                       ckey, cpos, item_begin, item_end, item_dst, item_final, k,
                       largest ? ~0ull : 0ull, okey, opos, rows);
    HM_LAUNCH_RET();
}
