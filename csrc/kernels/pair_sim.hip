// Pairwise similarity primitives of sparse feature lists on gfx950: the engine behind
// knn.pair_similarity_batch / pairwise_similarity and the column forms of cosine_similarity,
// cosine_distance, angular_similarity, angular_distance, euclid_distance, euclid_similarity,
// manhattan_distance, jaccard_similarity and jaccard_distance.
//
// List l holds ids[ptr[l]..ptr[l + 1]) / vals[...] in entry order (distinct ids) and the same
// entries again sorted by id (sids / svals) for lookup.  For a pair (A, B) the four primitives
// are (docs/compat.md "Pair-similarity engine"):
//
//   DOT    over A's entries in entry order that also occur in B:  s = s + a * b
//   SQ     over A's entries in entry order: d = a - b (b = 0.0 on a miss), s = s + d * d; then over
//          B's entries in entry order that do not occur in A:  s = s + v * v
//   ABS    the walk of SQ with |d| and |v|
//   INTER  the number of common ids
//
//   hm_pair_sim     LPP lanes per pair (8, 16, 32 or 64, from the longest list), so a wave serves
//                   64 / LPP pairs.  A lane binary-searches its entry's id in the other list's
//                   sorted slice, held one entry a lane and read with lane reads when it has at most
//                   LPP entries, in memory otherwise; INTER comes from the ballot of the found lanes.  The ordered sums
//                   walk the set bits of the pair's lane mask from low to high and add that lane's
//                   own term, read with a lane read: never a tree, so the twin's sequential loop
//                   adds in the same order.  Lists longer than 64 go in chunks of 64 entries that
//                   carry the running sums.  M > 0 selects the cross form: pair p is
//                   (a_idx[p / M], b_idx[p % M]) and no pair arrays exist.
//   hm_pair_sim_sq  sq[l] = the left-to-right sum of v * v; one thread a list.
//
// The library is built with -ffp-contract=fast, which fuses in the backend whatever a contract
// pragma in the source says (measured: with the pragma alone the sq kernel came out as v_fmac_f64
// and differed from the twin in the last bit).  Every product here feeds an add that must round on
// its own, so each one passes through ps_rounded.  No atomics, no LDS, no scratch; every output
// element has one writer.
//
// The C++ twin is csrc/host/pair_sim_cpu.cpp.
#include "common.h"

namespace {

constexpr int PS_THREADS = 256;
constexpr int PS_WAVES = PS_THREADS / HM_WAVE;
enum { PS_DOT = 0, PS_SQ, PS_ABS, PS_INTER, PS_NPRIM };

// A product as a value of its own: nothing fuses across the (empty) asm statement.
__device__ __forceinline__ double ps_rounded(double x) {
    asm volatile("" : "+v"(x));
    return x;
}

// Lane `sub * LPP + b` of v.  LPP == 64: the wave is one pair and b is wave-uniform, so this is a
// scalar lane read (v_readlane_b32 x2) instead of a trip through the LDS crossbar.
template <int LPP>
__device__ __forceinline__ double ps_lane_read(double v, int sub, int b) {
    if constexpr (LPP == HM_WAVE) {
        const int sb = __builtin_amdgcn_readfirstlane(b);
        const long long bits = __double_as_longlong(v);
        const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)bits, sb);
        const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(bits >> 32), sb);
        return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
    } else {
        return __shfl(v, sub * LPP + b, HM_WAVE);
    }
}

// s = s + t[lane] over the lanes 0..cnt-1 in turn; cnt is wave-uniform.
__device__ __forceinline__ void ps_walk_first(double t, int cnt, double& s) {
    for (int b = 0; b < cnt; ++b) s = s + ps_lane_read<HM_WAVE>(t, 0, b);
}

// s = s + t[lane] over the set bits of the wave-uniform mask w, low to high.
__device__ __forceinline__ void ps_walk_bits(double t, unsigned long long w, double& s) {
    for (; w; w &= w - 1ull) s = s + ps_lane_read<HM_WAVE>(t, 0, __builtin_ctzll(w));
}

// Whether `id` is in the ascending slice keys[lo..hi); *at = its position.
__device__ __forceinline__ bool ps_find(const int32_t* __restrict__ keys, int64_t lo, int64_t hi,
                                        int32_t id, int64_t* at) {
    const int64_t end = hi;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < id) lo = mid + 1;
        else hi = mid;
    }
    *at = lo;
    return lo < end && keys[lo] == id;
}

// A sorted slice of at most LPP entries held one entry a lane: the pair's lane k holds entry k, the
// lanes past the end hold INT32_MAX (no id is that large).  find() is a branchless lower bound over
// the LPP lanes by lane reads, log2(LPP) + 2 of them and no memory access; every lane of the wave
// calls it, whatever its query.
template <int LPP>
struct PsSlice {
    int32_t key;
    double val;

    __device__ __forceinline__ void load(const int32_t* __restrict__ keys, const double* __restrict__ values,
                                         int64_t lo, int64_t n, int j) {
        const bool in = j < n;
        key = in ? keys[lo + j] : INT32_MAX;
        val = in && values ? values[lo + j] : 0.0;
    }
    __device__ __forceinline__ bool find(int sub, int32_t id, double* v) const {
        int pos = 0;                               // every entry before pos is below id
#pragma unroll
        for (int step = LPP / 2; step > 0; step >>= 1)
            if (__shfl(key, sub * LPP + pos + step - 1, HM_WAVE) < id) pos += step;
        *v = __shfl(val, sub * LPP + pos, HM_WAVE);
        return __shfl(key, sub * LPP + pos, HM_WAVE) == id;
    }
};

template <int LPP>
__global__ __launch_bounds__(PS_THREADS) void ps_kernel(
    const int64_t* __restrict__ ptr, const int32_t* __restrict__ ids, const double* __restrict__ vals,
    const int32_t* __restrict__ sids, const double* __restrict__ svals,
    const int32_t* __restrict__ ia, const int32_t* __restrict__ ib, int64_t P, int64_t M, int mask,
    double* __restrict__ out) {
    constexpr int PPW = HM_WAVE / LPP;             // pairs per wave
    const int lane = hm::lane_id();
    const int sub = lane / LPP, j = lane % LPP;
    const int64_t p = ((int64_t)blockIdx.x * PS_WAVES + hm::wave_id()) * PPW + sub;
    const bool live = p < P;                       // a tail wave holds fewer pairs than slots

    int64_t a0 = 0, a1 = 0, b0 = 0, b1 = 0;
    if (live) {
        int64_t pa = p, pb = p;                    // where the pair's lists stand in ia and ib
        if (M > 0) {
            if (P <= (int64_t)UINT32_MAX) {        // the 32-bit division is a fifth of the 64-bit one
                pa = (uint32_t)p / (uint32_t)M;
                pb = (uint32_t)p % (uint32_t)M;
            } else {
                pa = p / M;
                pb = p % M;
            }
        }
        const int64_t la = ia[pa], lb = ib[pb];
        a0 = ptr[la];
        a1 = ptr[la + 1];
        b0 = ptr[lb];
        b1 = ptr[lb + 1];
    }
    const bool want_dot = mask & (1 << PS_DOT), want_sq = mask & (1 << PS_SQ), want_abs = mask & (1 << PS_ABS);
    const bool want_walk = want_sq || want_abs;    // the sums that visit every entry
    // LPP < 64: the launcher chose LPP >= the longest list, one chunk serves every pair of the wave.
    // LPP == 64: the wave is one pair, so the trip counts are wave-uniform.
    const int64_t na = a1 - a0, nb = b1 - b0;
    const int chunks_a = LPP == HM_WAVE ? __builtin_amdgcn_readfirstlane((int)((na + HM_WAVE - 1) / HM_WAVE)) : 1;
    const int chunks_b = !want_walk ? 0
                         : LPP == HM_WAVE ? __builtin_amdgcn_readfirstlane((int)((nb + HM_WAVE - 1) / HM_WAVE)) : 1;

    // A list of at most LPP entries is searched in registers (always so below 64 lanes a pair, where
    // the launcher chose LPP >= the longest list), a longer one in memory.  Both tests are wave-uniform.
    const bool regs_a = LPP < HM_WAVE || na <= HM_WAVE, regs_b = LPP < HM_WAVE || nb <= HM_WAVE;
    PsSlice<LPP> slice_a, slice_b;
    slice_b.load(sids, svals, b0, regs_b ? nb : 0, j);
    if (want_walk) slice_a.load(sids, nullptr, a0, regs_a ? na : 0, j);

    int inter = 0;
    double s_dot = 0.0, s_sq = 0.0, s_abs = 0.0;
    // A's entries in entry order, looked up in B
    for (int c = 0; c < chunks_a; ++c) {
        const int64_t i = (int64_t)c * LPP + j;
        const bool valid = i < na;
        bool found = false;
        double t_dot = 0.0, t_sq = 0.0, t_abs = 0.0;     // the lane's own terms
        int32_t id = 0;
        double a = 0.0, b = 0.0;
        if (valid) {
            id = ids[a0 + i];
            a = vals[a0 + i];
        }
        if (regs_b) {
            double v;
            found = slice_b.find(sub, id, &v) && valid;
            if (found) b = v;
        } else if (valid) {
            int64_t at;
            found = ps_find(sids, b0, b1, id, &at);
            if (found) b = svals[at];
        }
        if (valid) {
            const double d = a - b;
            t_dot = ps_rounded(a * b);
            t_sq = ps_rounded(d * d);
            t_abs = fabs(d);
        }
        const unsigned long long bal_f = __ballot(found), bal_v = __ballot(valid);
        unsigned long long mf = bal_f, mv = bal_v;  // the pair's lanes only
        if constexpr (LPP < HM_WAVE) {
            mf = (bal_f >> (sub * LPP)) & ((1ull << LPP) - 1ull);
            mv = (bal_v >> (sub * LPP)) & ((1ull << LPP) - 1ull);
        }
        inter += __popcll(mf);
        if constexpr (LPP == HM_WAVE) {
            // The wave is one pair: the masks are wave-uniform and the walks run in scalar
            // registers, one plain loop per sum.  The valid lanes are 0..cnt-1.
            const int cnt = __popcll(mv);
            if (want_sq) ps_walk_first(t_sq, cnt, s_sq);
            if (want_abs) ps_walk_first(t_abs, cnt, s_abs);
            if (want_dot) ps_walk_bits(t_dot, mf, s_dot);
            continue;
        }
        // The set bits of the pair's mask, low to high.  The loop runs for the whole wave until the
        // pair with the most terms is done, so every lane is active at the lane reads.
        unsigned long long w = want_walk ? mv : want_dot ? mf : 0ull;
        while (__ballot(w != 0ull)) {
            const int b = w ? __builtin_ctzll(w) : 0;
            if (want_dot) {
                const double v = ps_lane_read<LPP>(t_dot, sub, b);
                if (w && ((mf >> b) & 1ull)) s_dot = s_dot + v;
            }
            if (want_sq) {
                const double v = ps_lane_read<LPP>(t_sq, sub, b);
                if (w) s_sq = s_sq + v;
            }
            if (want_abs) {
                const double v = ps_lane_read<LPP>(t_abs, sub, b);
                if (w) s_abs = s_abs + v;
            }
            w &= w - 1ull;
        }
    }
    // B's entries in entry order that A does not hold
    for (int c = 0; c < chunks_b; ++c) {
        const int64_t i = (int64_t)c * LPP + j;
        bool miss = false;
        double t_sq = 0.0, t_abs = 0.0;
        const bool valid = i < nb;
        const int32_t id = valid ? ids[b0 + i] : 0;
        if (regs_a) {
            double unused;
            miss = !slice_a.find(sub, id, &unused) && valid;
        } else if (valid) {
            int64_t at;
            miss = !ps_find(sids, a0, a1, id, &at);
        }
        if (miss) {
            const double v = vals[b0 + i];
            t_sq = ps_rounded(v * v);
            t_abs = fabs(v);
        }
        const unsigned long long bal = __ballot(miss);
        if constexpr (LPP == HM_WAVE) {
            if (want_sq) ps_walk_bits(t_sq, bal, s_sq);
            if (want_abs) ps_walk_bits(t_abs, bal, s_abs);
            continue;
        }
        const unsigned long long w0 = (bal >> (sub * LPP)) & ((1ull << (LPP & 63)) - 1ull);
        unsigned long long w = w0;
        while (__ballot(w != 0ull)) {
            const int b = w ? __builtin_ctzll(w) : 0;
            if (want_sq) {
                const double v = ps_lane_read<LPP>(t_sq, sub, b);
                if (w) s_sq = s_sq + v;
            }
            if (want_abs) {
                const double v = ps_lane_read<LPP>(t_abs, sub, b);
                if (w) s_abs = s_abs + v;
            }
            w &= w - 1ull;
        }
    }

    if (!live || j >= PS_NPRIM || !((mask >> j) & 1)) return;
    const double v = j == PS_DOT ? s_dot : j == PS_SQ ? s_sq : j == PS_ABS ? s_abs : (double)inter;
    out[(int64_t)j * P + p] = v;
}

__global__ __launch_bounds__(PS_THREADS) void ps_sq_kernel(const int64_t* __restrict__ ptr,
                                                           const double* __restrict__ vals, int64_t n,
                                                           double* __restrict__ sq) {
    const int64_t l = (int64_t)blockIdx.x * PS_THREADS + threadIdx.x;
    if (l >= n) return;
    double s = 0.0;
    for (int64_t e = ptr[l]; e < ptr[l + 1]; ++e) {
        const double v = vals[e];
        s = s + ps_rounded(v * v);
    }
    sq[l] = s;
}

}  // namespace

// ptr int64 [n + 1]; ids int32 / vals fp64 [nnz] in entry order, ids distinct inside a list; sids
// int32 / svals fp64 [nnz] the same entries ascending by id inside a list; max_len >= the longest
// list.  M == 0: ia, ib int32 [P] hold the pairs.  M > 0 (cross form): ia int32 [P / M], ib int32
// [M], pair p = (ia[p / M], ib[p % M]).  Every index is in 0..n-1 (the caller checks).  mask = bit
// mask of the planes of out fp64 [4, P] to fill.
HM_API int hm_pair_sim(const int64_t* ptr, const int32_t* ids, const double* vals, const int32_t* sids,
                       const double* svals, const int32_t* ia, const int32_t* ib, int64_t P, int64_t M,
                       int64_t max_len, int mask, double* out, hipStream_t stream) {
    if (P <= 0 || !(mask & ((1 << PS_NPRIM) - 1))) return 0;
    if (M < 0 || max_len < 0 || (M > 0 && P % M != 0)) return (int)hipErrorInvalidValue;
    const int lpp = max_len <= 8 ? 8 : max_len <= 16 ? 16 : max_len <= 32 ? 32 : 64;
    const int64_t pairs_per_block = (int64_t)PS_WAVES * (HM_WAVE / lpp);
    const int64_t grid = (P + pairs_per_block - 1) / pairs_per_block;
    if (grid > INT32_MAX) return (int)hipErrorInvalidValue;
#define PS_LAUNCH(LPP)                                                                              \
    hipLaunchKernelGGL(ps_kernel<LPP>, dim3((unsigned)grid), dim3(PS_THREADS), 0, stream, ptr, ids, vals, \
                       sids, svals, ia, ib, P, M, mask, out)
    if (lpp == 8) PS_LAUNCH(8);
    else if (lpp == 16) PS_LAUNCH(16);
    else if (lpp == 32) PS_LAUNCH(32);
    else PS_LAUNCH(64);
#undef PS_LAUNCH
    HM_LAUNCH_RET();
}

HM_API int hm_pair_sim_sq(const int64_t* ptr, const double* vals, int64_t n, double* sq, hipStream_t stream) {
    if (n <= 0) return 0;
    const int64_t grid = (n + PS_THREADS - 1) / PS_THREADS;
    if (grid > INT32_MAX) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(ps_sq_kernel, dim3((unsigned)grid), dim3(PS_THREADS), 0, stream, ptr, vals, n, sq);
    HM_LAUNCH_RET();
}
