// The front end of the kernels that hash a packed string column (hashing.hip, minhash.hip,
// sketch.hip): buf uint8 + off int64 [n + 1], string s = buf[off[s] .. off[s + 1]).
//
// A workgroup owns a run of consecutive strings, i.e. one contiguous span of bytes.  It copies
// the first BYTES of the span to LDS with aligned 16-B loads; the LDS image keeps the global
// address modulo 16 (byte i of the span is LDS byte lead + i), so the stores are aligned 16-B
// stores too.  A string is then read from the window through LdsWords, one aligned dword pair per
// 4-byte word, or through GlobalWords when it ends beyond the window.
//
// Precondition, for every caller: buf is readable in whole aligned 16-B chunks around every staged
// span (ops/_packed.py launch() pads it).
#pragma once
#include <stdint.h>

#include "hd.h"
#include "murmur3.h"

namespace hm {

// Word i of a string (little endian); the bytes past its end are unspecified (the caller masks).
struct LdsWords {
    const uint32_t* w;     // the aligned dword that holds the first byte
    int sh;                // 8 * (byte position of the first byte in it)
    HM_HD_MEMBER uint32_t operator()(int i) const {
        const uint64_t pair = ((uint64_t)w[i + 1] << 32) | w[i];
        return (uint32_t)(pair >> sh);
    }
};

struct GlobalWords {
    const uint8_t* q;
    int len;
    HM_HD_MEMBER uint32_t operator()(int i) const {
        uint32_t k = 0;
        for (int j = 0; j < 4; ++j)
            if (4 * i + j < len) k |= (uint32_t)q[4 * i + j] << (8 * j);
        return k;
    }
};

template <typename Words>
HM_HD uint32_t mm3(const Words& word, int len, uint32_t seed) {
    uint32_t h = seed;
    const int nw = len >> 2, r = len & 3;
    for (int i = 0; i < nw; ++i) h = mm_chain(h, mm_premix(word(i)));
    if (r) h ^= mm_premix(word(nw) & ((1u << (8 * r)) - 1u));
    return mm_fmix(h, (uint32_t)len);
}

#if defined(__HIPCC__)

// uint4s of the staging array of a BYTES window: the window, its lead of up to 15 bytes and the
// dword pair that LdsWords reads around the last byte.
constexpr int stage_vecs(int bytes) { return bytes / 16 + 2; }

// Copies the `staged` bytes at g0 to s_stage with the THREADS threads of the workgroup and returns
// lead = g0 mod 16.  The caller's barrier comes before the first read.
template <int THREADS>
__device__ __forceinline__ int stage_span(const uint8_t* g0, int staged, uint4* s_stage) {
    const int lead = (int)(reinterpret_cast<uintptr_t>(g0) & 15);
    const int nvec = (lead + staged + 15) >> 4;
    const uint4* gv = reinterpret_cast<const uint4*>(g0 - lead);
    for (int v = threadIdx.x; v < nvec; v += THREADS) s_stage[v] = gv[v];
    return lead;
}

// Calls op(s, words, len) once for every string s in 0..n-1, on the lane that owns it.  A
// workgroup of STRINGS threads takes STRINGS consecutive strings per step (grid stride) and stages
// the first BYTES of their span in s_stage (stage_vecs(BYTES) uint4s).  Ends with a barrier.
template <int STRINGS, int BYTES, typename Op>
__device__ __forceinline__ void sweep(const uint8_t* __restrict__ buf, const int64_t* __restrict__ off,
                                      int64_t n, uint4* s_stage, Op& op) {
    const int t = threadIdx.x;
    for (int64_t base = (int64_t)blockIdx.x * STRINGS; base < n; base += (int64_t)gridDim.x * STRINGS) {
        const int64_t last = n - base < STRINGS ? n : base + STRINGS;
        const int64_t span0 = off[base], span = off[last] - span0;
        const int staged = (int)(span < BYTES ? span : BYTES);
        const uint8_t* g0 = buf + span0;
        const int lead = stage_span<STRINGS>(g0, staged, s_stage);
        __syncthreads();
        const int64_t s = base + t;
        if (s < last) {
            const int64_t b = off[s] - span0, e = off[s + 1] - span0;
            const int len = (int)(e - b);
            if (e <= staged) {
                const int a = lead + (int)b;
                op(s, LdsWords{reinterpret_cast<const uint32_t*>(s_stage) + (a >> 2), 8 * (a & 3)}, len);
            } else {
                op(s, GlobalWords{g0 + b, len}, len);
            }
        }
        __syncthreads();                        // the next step overwrites the window
    }
}

#endif  // __HIPCC__

}  // namespace hm
