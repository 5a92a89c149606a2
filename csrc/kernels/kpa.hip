// train_kpa on gfx950: PA-I on the explicit degree-2 polynomial expansion (models/recommend.py,
// KPA.fit / _kpa_score are the definition; docs/compat.md "KPA engine").
//
// Rows are CSR: ids int32 / vals fp64 in the row's entry order, ids distinct inside a training row,
// at most KPA_MAX_LEN entries.  A row of n entries has m = n (n - 1) / 2 ordered pairs (a, b),
// a < b, numbered in the learner's loop order (a outer, b inner); pair_base[r] is the number of pair
// occurrences before row r, so occurrence g = pair_base[r] + p is a global, sequential numbering of
// every pair the learner visits in its first epoch.  A pair's key is (id_a << 32) | id_b.
//
//   hm_kpa_table  whole chip, one thread an occurrence.  The key goes into an open-addressing table
//                 (64-bit compare-and-swap, linear probing), the slot's `first` takes the atomic min
//                 of g, and occ[g] = the table slot.  Where a key lands depends on who wins a race;
//                 `first` does not, and the host ranks the used slots by it: that compact, first-seen
//                 numbering is what the trainer and the model table use.  A workgroup finds the rows
//                 its occurrences span once (a wave-uniform search), each thread then searches only
//                 inside that window.
//   hm_kpa_train  ONE persistent 1024-thread workgroup walks the rows in order over all epochs.
//                 Thread i owns the pairs i, i + 1024, ... (at most 8) of every row; the last two
//                 waves own the singles.  While row t is gathered and reduced, every thread fetches
//                 its own slots of row t + 1 and decodes their (a, b) into registers and the last
//                 wave stages row t + 1's ids and values into the other half of a double LDS buffer,
//                 so the serial chain of a row is one dependent gather, one reduction, one scatter.
//                 Margin and |phi|^2 are reduced in a fixed tree (the thread's own terms in order,
//                 the DPP wave sum, 16 partials added in order by every thread): no atomics, two
//                 runs agree bit for bit.  Row t's stores reach row t + 1's loads through the
//                 workgroup-scope fences of the two barriers a row costs; one workgroup, one CU.
//   hm_kpa_score  whole chip, one wave a row.  Read-only probes of the finished table; a key or a
//                 name the model never saw (id < 0) takes weight 0.0.  The same reduction.
//
// The order of additions differs from the learner's sequential loop, nothing else does: fp64
// throughout.  x ** 4 and (xh xk) ** 2 are plain products here.  The C++ twin, which is the learner
// bit for bit, is csrc/host/kpa_cpu.cpp.
#include "common.h"

namespace {

constexpr int KPA_MAX_LEN = 128;                       // entries of a row
constexpr int KPA_THREADS = 1024;                      // the trainer's one workgroup
constexpr int KPA_WAVES = KPA_THREADS / HM_WAVE;
constexpr int KPA_PPT = KPA_MAX_LEN * (KPA_MAX_LEN - 1) / 2 / KPA_THREADS + 1;   // pairs a thread: 8
constexpr int KPA_SINGLES_AT = KPA_THREADS - KPA_MAX_LEN;                        // first thread of the singles
constexpr int KPA_TB = 256;                            // threads of a table / scoring workgroup
constexpr int KPA_ITEMS = 4;                           // occurrences a table thread
constexpr long long KPA_EMPTY = -1;

// Pair p of a row of n entries -> (a, b), a < b, in the order of `for a: for b in a+1..n-1`.
// Counted from the end the triangle's rows have 1, 2, 3, ... pairs: k = the largest integer with
// k (k + 1) / 2 <= q.  n <= 128, so 8 q + 1 <= 65017 is exact in fp32; the two loops mend the
// rounding of the root.
__device__ __forceinline__ void kpa_decode(int p, int n, int* a, int* b) {
    const int q = n * (n - 1) / 2 - 1 - p;
    int k = (int)((sqrtf((float)(8 * q + 1)) - 1.0f) * 0.5f);
    while (k * (k + 1) / 2 > q) --k;
    while ((k + 1) * (k + 2) / 2 <= q) ++k;
    *a = n - 2 - k;
    *b = n - 1 - (q - k * (k + 1) / 2);
}

__device__ __forceinline__ long long kpa_key(int ia, int ib) {
    return (long long)(((unsigned long long)(unsigned)ia << 32) | (unsigned)ib);
}

// The last r in lo..hi-1 with base[r] <= g (base ascending, base[lo] <= g).
__device__ __forceinline__ int64_t kpa_row_of(const int64_t* __restrict__ base, int64_t lo, int64_t hi, int64_t g) {
    while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (base[mid] <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}

// ------------------------------------------------------------------ A: the pair table
__global__ __launch_bounds__(KPA_TB) void kpa_table_kernel(
    const int64_t* __restrict__ ptr, const int32_t* __restrict__ ids, const int64_t* __restrict__ pair_base,
    int64_t row0, int64_t row1, long long* __restrict__ keys, unsigned long long* __restrict__ first,
    int64_t cap_mask, int32_t* __restrict__ occ, int* __restrict__ full) {
    const int64_t g_end = pair_base[row1];
    const int64_t b0 = pair_base[row0] + (int64_t)blockIdx.x * (KPA_TB * KPA_ITEMS);
    if (b0 >= g_end) return;
    const int64_t b1 = min(b0 + (int64_t)KPA_TB * KPA_ITEMS, g_end) - 1;
    // the rows this workgroup's occurrences span: block-uniform, scalar loads
    const int64_t r_lo = kpa_row_of(pair_base, row0, row1, b0);
    const int64_t r_hi = kpa_row_of(pair_base, r_lo, row1, b1) + 1;
#pragma unroll
    for (int it = 0; it < KPA_ITEMS; ++it) {
        const int64_t g = b0 + (int64_t)it * KPA_TB + threadIdx.x;
        if (g > b1) break;
        const int64_t r = kpa_row_of(pair_base, r_lo, r_hi, g);
        const int64_t e0 = ptr[r];
        const int n = (int)(ptr[r + 1] - e0);
        int a, b;
        kpa_decode((int)(g - pair_base[r]), n, &a, &b);
        const long long key = kpa_key(ids[e0 + a], ids[e0 + b]);
        int64_t h = (int64_t)(hm::mix64((uint64_t)key) & (uint64_t)cap_mask);
        int64_t at = -1;
        for (int64_t step = 0; step <= cap_mask; ++step) {
            long long cur = __hip_atomic_load(&keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == KPA_EMPTY)
                cur = (long long)atomicCAS((unsigned long long*)&keys[h], (unsigned long long)KPA_EMPTY,
                                           (unsigned long long)key);
            if (cur == KPA_EMPTY || cur == key) {
                at = h;
                break;
            }
            h = (h + 1) & cap_mask;
        }
        if (at < 0) {                              // every slot holds another key: the host raises
            atomicOr(full, 1);
            occ[g] = -1;
            continue;
        }
        atomicMin(&first[at], (unsigned long long)g);
        occ[g] = (int32_t)at;
    }
}

// ------------------------------------------------------------------ B: the sequential trainer
// What a thread holds of one row: its pairs' compact slots and packed (a | b << 8).
struct KpaMine {
    int32_t slot[KPA_PPT];
    int32_t ab[KPA_PPT];
    int n, m;
};

__device__ __forceinline__ void kpa_fetch(KpaMine& me, const int64_t* __restrict__ ptr,
                                          const int64_t* __restrict__ pair_base,
                                          const int32_t* __restrict__ occ, int64_t r) {
    me.n = (int)(ptr[r + 1] - ptr[r]);
    me.m = me.n * (me.n - 1) / 2;
    const int64_t base = pair_base[r];
#pragma unroll
    for (int j = 0; j < KPA_PPT; ++j) {
        const int p = (int)threadIdx.x + j * KPA_THREADS;
        me.slot[j] = 0;
        me.ab[j] = 0;
        if (p < me.m) {
            int a, b;
            kpa_decode(p, me.n, &a, &b);
            me.slot[j] = occ[base + p];
            me.ab[j] = a | (b << 8);
        }
    }
}

__global__ __launch_bounds__(KPA_THREADS) void kpa_train_kernel(
    const int64_t* __restrict__ ptr, const int32_t* __restrict__ ids, const double* __restrict__ vals,
    const double* __restrict__ y, const int64_t* __restrict__ pair_base, const int32_t* __restrict__ occ,
    int64_t n_rows, int iters, double c, double pkc, double s0, double s1, double s2,
    double* w0p, double* w1, double* w2, double* w3) {
    __shared__ double xs[2][KPA_MAX_LEN];
    __shared__ int32_t idl[2][KPA_MAX_LEN];
    __shared__ double red[2][KPA_WAVES][2];
    const int tid = threadIdx.x, lane = hm::lane_id(), wave = hm::wave_id();
    const bool stager = wave == KPA_WAVES - 1;     // the wave that stages the next row's entries
    const int single = tid - KPA_SINGLES_AT;       // >= 0: the entry this thread owns

    auto stage = [&](int buf, int64_t r) {
        const int64_t e0 = ptr[r];
        const int n = (int)(ptr[r + 1] - e0);
        for (int e = lane; e < n; e += HM_WAVE) {
            xs[buf][e] = vals[e0 + e];
            idl[buf][e] = ids[e0 + e];
        }
    };

    double w0 = w0p[0];
    const double sq0 = s0 * s0, pkc2 = 2.0 * pkc;
    KpaMine cur, nxt;
    kpa_fetch(cur, ptr, pair_base, occ, 0);
    if (stager) stage(0, 0);
    __syncthreads();

    const int64_t total = n_rows * (int64_t)iters;
    int64_t r = 0;
    for (int64_t t = 0; t < total; ++t) {
        const int buf = (int)(t & 1);
        const int64_t r_next = r + 1 == n_rows ? 0 : r + 1;
        const bool more = t + 1 < total;
        const double yy = y[r];

        // gather: the only loads of the row that depend on the previous row's stores
        double w[KPA_PPT];
        const int nj = (cur.m + KPA_THREADS - 1) / KPA_THREADS;
#pragma unroll
        for (int j = 0; j < KPA_PPT; ++j)
            if (j < nj && tid + j * KPA_THREADS < cur.m) w[j] = w3[cur.slot[j]];
        int id1 = 0;
        double x1 = 0.0, wa = 0.0, wb = 0.0;
        const bool has_single = single >= 0 && single < cur.n;
        if (has_single) {
            id1 = idl[buf][single];
            x1 = xs[buf][single];
            wa = w1[id1];
            wb = w2[id1];
        }
        // behind them, what row t + 1 needs and no weight changes
        if (more) {
            kpa_fetch(nxt, ptr, pair_base, occ, r_next);
            if (stager) stage(buf ^ 1, r_next);
        }

        double pm = 0.0, sq = 0.0;
#pragma unroll
        for (int j = 0; j < KPA_PPT; ++j)
            if (j < nj && tid + j * KPA_THREADS < cur.m) {
                const double xh = xs[buf][cur.ab[j] & 0xff], xk = xs[buf][cur.ab[j] >> 8];
                const double pr = xh * xk;
                pm += w[j] * s2 * xh * xk;
                sq += 2.0 * (pr * pr);
            }
        if (has_single) {
            const double x2 = x1 * x1;
            pm += wa * s1 * x1 + wb * x1 * x1;
            sq += pkc2 * x1 * x1 + x2 * x2;
        }
        pm = hm::wave_sum_uniform(pm);
        sq = hm::wave_sum_uniform(sq);
        if (lane == 0) {
            red[buf][wave][0] = pm;
            red[buf][wave][1] = sq;
        }
        __syncthreads();
        double p = w0 * s0, sqs = sq0;
#pragma unroll
        for (int v = 0; v < KPA_WAVES; ++v) {
            p += red[buf][v][0];
            sqs += red[buf][v][1];
        }
        const double loss = fmax(0.0, 1.0 - yy * p);
        if (!(loss <= 0.0)) {                      // the learner's test; uniform over the workgroup
            const double q = loss / sqs;
            const double eta = (q < c ? q : c) * yy;
            w0 += eta * s0;
#pragma unroll
            for (int j = 0; j < KPA_PPT; ++j)
                if (j < nj && tid + j * KPA_THREADS < cur.m) {
                    const double xh = xs[buf][cur.ab[j] & 0xff], xk = xs[buf][cur.ab[j] >> 8];
                    w3[cur.slot[j]] = w[j] + eta * s2 * xh * xk;
                }
            if (has_single) {
                w1[id1] = wa + eta * s1 * x1;
                w2[id1] = wb + eta * x1 * x1;
            }
        }
        // the row's stores and the staged entries, to every wave of the workgroup
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __syncthreads();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        if (more) cur = nxt;
        r = r_next;
    }
    if (tid == 0) w0p[0] = w0;
}

// ------------------------------------------------------------------ C: scoring
__global__ __launch_bounds__(KPA_TB) void kpa_score_kernel(
    const int64_t* __restrict__ ptr, const int32_t* __restrict__ ids, const double* __restrict__ vals,
    int64_t n_rows, const long long* __restrict__ keys, const int32_t* __restrict__ remap, int64_t cap_mask,
    const double* __restrict__ w0p, const double* __restrict__ w1, const double* __restrict__ w2,
    const double* __restrict__ w3, double s0, double s1, double s2, double* __restrict__ out) {
    const int lane = hm::lane_id();
    const int64_t r = (int64_t)blockIdx.x * (KPA_TB / HM_WAVE) + hm::wave_id();
    if (r >= n_rows) return;                       // wave-uniform
    const int64_t e0 = ptr[r];
    const int n = (int)(ptr[r + 1] - e0), m = n * (n - 1) / 2;
    double s = 0.0;
    for (int e = lane; e < n; e += HM_WAVE) {
        const int id = ids[e0 + e];
        const double x = vals[e0 + e];
        const double wa = id >= 0 ? w1[id] : 0.0, wb = id >= 0 ? w2[id] : 0.0;
        s += wa * s1 * x + wb * x * x;
    }
    for (int p = lane; p < m; p += HM_WAVE) {
        int a, b;
        kpa_decode(p, n, &a, &b);
        const int ia = ids[e0 + a], ib = ids[e0 + b];
        double w = 0.0;
        if (ia >= 0 && ib >= 0 && keys) {
            const long long key = kpa_key(ia, ib);
            int64_t h = (int64_t)(hm::mix64((uint64_t)key) & (uint64_t)cap_mask);
            for (int64_t step = 0; step <= cap_mask; ++step) {
                const long long cur = keys[h];
                if (cur == key) {
                    w = w3[remap[h]];
                    break;
                }
                if (cur == KPA_EMPTY) break;
                h = (h + 1) & cap_mask;
            }
        }
        s += w * s2 * vals[e0 + a] * vals[e0 + b];
    }
    // the loops above leave the lanes apart; the DPP sum needs them all
    __builtin_amdgcn_wave_barrier();
    s = hm::wave_sum_uniform(s);
    if (lane == 0) out[r] = w0p[0] * s0 + s;
}

}  // namespace

// Inserts the pair occurrences of rows row0..row1-1.  ptr int64 [rows + 1], ids int32 [nnz] (>= 0),
// pair_base int64 [rows + 1]; keys int64 [cap] (-1 = empty) and first uint64 [cap] (start: the
// largest value), cap = cap_mask + 1 a power of two; occ int32 [pair_base[rows]] takes the table
// slots; *full becomes 1 when a key found no slot.  Rows hold at most 128 entries (the caller checks).
HM_API int hm_kpa_table(const int64_t* ptr, const int32_t* ids, const int64_t* pair_base, int64_t row0,
                        int64_t row1, int64_t n_occ, long long* keys, unsigned long long* first,
                        int64_t cap_mask, int32_t* occ, int* full, hipStream_t stream) {
    if (row1 <= row0 || n_occ <= 0) return 0;
    if (cap_mask < 0 || (cap_mask & (cap_mask + 1)) != 0 || cap_mask >= ((int64_t)1 << 31))
        return (int)hipErrorInvalidValue;
    const int64_t per = (int64_t)KPA_TB * KPA_ITEMS;
    const int64_t grid = (n_occ + per - 1) / per;
    if (grid > INT32_MAX) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(kpa_table_kernel, dim3((unsigned)grid), dim3(KPA_TB), 0, stream, ptr, ids, pair_base, row0,
                       row1, keys, first, cap_mask, occ, full);
    HM_LAUNCH_RET();
}

// `iters` passes over the rows in order.  y fp64 [rows] in {-1, +1}; occ int32 the compact slot of
// every pair occurrence (0..slots-1); w0 fp64 [1], w1 / w2 fp64 [names], w3 fp64 [slots], updated
// in place.  hyper = c, pkc, s0 = pkc, s1 = sqrt(2 pkc), s2 = sqrt(2), from the host.
HM_API int hm_kpa_train(const int64_t* ptr, const int32_t* ids, const double* vals, const double* y,
                        const int64_t* pair_base, const int32_t* occ, int64_t n_rows, int iters, double c,
                        double pkc, double s0, double s1, double s2, double* w0, double* w1, double* w2,
                        double* w3, hipStream_t stream) {
    if (n_rows <= 0 || iters <= 0) return 0;
    hipLaunchKernelGGL(kpa_train_kernel, dim3(1), dim3(KPA_THREADS), 0, stream, ptr, ids, vals, y, pair_base, occ,
                       n_rows, iters, c, pkc, s0, s1, s2, w0, w1, w2, w3);
    HM_LAUNCH_RET();
}

// out[r] = the model's score of row r.  ids < 0 mark names the model never saw; keys / remap may be
// NULL when the model holds no pair (cap_mask is then ignored).
HM_API int hm_kpa_score(const int64_t* ptr, const int32_t* ids, const double* vals, int64_t n_rows,
                        const long long* keys, const int32_t* remap, int64_t cap_mask, const double* w0,
                        const double* w1, const double* w2, const double* w3, double s0, double s1, double s2,
                        double* out, hipStream_t stream) {
    if (n_rows <= 0) return 0;
    if (keys && (cap_mask < 0 || (cap_mask & (cap_mask + 1)) != 0)) return (int)hipErrorInvalidValue;
    const int64_t rows_per_block = KPA_TB / HM_WAVE;
    const int64_t grid = (n_rows + rows_per_block - 1) / rows_per_block;
    if (grid > INT32_MAX) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(kpa_score_kernel, dim3((unsigned)grid), dim3(KPA_TB), 0, stream, ptr, ids, vals, n_rows, keys,
                       remap, cap_mask, w0, w1, w2, w3, s0, s1, s2, out);
    HM_LAUNCH_RET();
}
