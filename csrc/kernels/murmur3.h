// MurmurHash3_x86_32 (bit-exact with upstream hivemall.utils.hashing.MurmurHash3): the project's
// only definition, compiled into the gfx950 kernels and into the host library alike.
//
// The hash of a byte string is h1 = seed; for every 4-byte little-endian word k1:
// h1 = mm_chain(h1, mm_premix(k1)); then h1 ^= mm_premix(tail word) for the 1-3 bytes left
// (mm_premix(0) == 0, so no tail changes nothing); then mm_fmix(h1, len).  murmur3 (byte loader)
// and murmur3_bytes (host pointer) run the whole of it; the minhash and sketch engines call the
// three steps from loops of their own, because the premix does not depend on the seed.
#pragma once
#include <stdint.h>
#include <string.h>

#include "hd.h"

namespace hm {

HM_HD uint32_t mm_rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }

// the seed-independent half of a word
HM_HD uint32_t mm_premix(uint32_t k1) {
    k1 *= 0xcc9e2d51u;
    k1 = mm_rotl32(k1, 15);
    return k1 * 0x1b873593u;
}

// one step of the h1 chain over a premixed word
HM_HD uint32_t mm_chain(uint32_t h1, uint32_t k) {
    h1 ^= k;
    h1 = mm_rotl32(h1, 13);
    return h1 * 5 + 0xe6546b64u;
}

HM_HD uint32_t mm_fmix(uint32_t h1, uint32_t len) {
    h1 ^= len;
    h1 ^= h1 >> 16; h1 *= 0x85ebca6bu; h1 ^= h1 >> 13; h1 *= 0xc2b2ae35u; h1 ^= h1 >> 16;
    return h1;
}

// the raw (not premixed) word of the r = len & 3 bytes after the last whole word; 0 for r = 0
HM_HD uint32_t mm_tail_word(const uint8_t* tp, int r) {
    uint32_t k1 = 0;
    switch (r) {
        case 3: k1 ^= (uint32_t)tp[2] << 16; [[fallthrough]];
        case 2: k1 ^= (uint32_t)tp[1] << 8; [[fallthrough]];
        case 1: k1 ^= (uint32_t)tp[0];
    }
    return k1;
}

// Device callers: at(i) loads byte i (global memory, LDS, a register image).
template <typename LoadByte>
HM_HD uint32_t murmur3(LoadByte at, int len, uint32_t seed) {
    uint32_t h1 = seed;
    const int nblocks = len >> 2;
    for (int i = 0; i < nblocks; ++i) {
        const uint32_t k1 = (uint32_t)at(4 * i) | ((uint32_t)at(4 * i + 1) << 8) |
                            ((uint32_t)at(4 * i + 2) << 16) | ((uint32_t)at(4 * i + 3) << 24);
        h1 = mm_chain(h1, mm_premix(k1));
    }
    uint32_t k1 = 0;
    const int t = nblocks * 4;
    switch (len & 3) {   // the premix stays inside case 1: hoisting it changes the kernels' code
        case 3: k1 ^= (uint32_t)at(t + 2) << 16; [[fallthrough]];
        case 2: k1 ^= (uint32_t)at(t + 1) << 8; [[fallthrough]];
        case 1: k1 ^= (uint32_t)at(t); h1 ^= mm_premix(k1);
    }
    return mm_fmix(h1, (uint32_t)len);
}

// Host callers: whole words with memcpy (little-endian host).  Not an overload of murmur3: a
// pointer would match its LoadByte as well.
HM_HD uint32_t murmur3_bytes(const uint8_t* data, int len, uint32_t seed) {
    uint32_t h1 = seed;
    const int nblocks = len >> 2;
    for (int i = 0; i < nblocks; ++i) {
        uint32_t k1;
        memcpy(&k1, data + 4 * i, 4);
        h1 = mm_chain(h1, mm_premix(k1));
    }
    const uint8_t* tail = data + nblocks * 4;
    uint32_t k1 = 0;
    switch (len & 3) {
        case 3: k1 ^= (uint32_t)tail[2] << 16; [[fallthrough]];
        case 2: k1 ^= (uint32_t)tail[1] << 8; [[fallthrough]];
        case 1: k1 ^= tail[0]; h1 ^= mm_premix(k1);
    }
    return mm_fmix(h1, (uint32_t)len);
}

// Java int % semantics, 1-based (Hivemall mhash)
HM_HD int32_t mhash_reduce(uint32_t h, int32_t num_features) {
    int32_t r = (int32_t)h % num_features;
    if (r < 0) r += num_features;
    return r + 1;
}

// ---------------------------------------------------------------- sketches
// the two seeds of the 64-bit hash of sketch.hip / sketch_cpu.cpp:
// h64 = (murmur3(s, SKETCH_SEED_HI) << 32) | murmur3(s, SKETCH_SEED_LO)
constexpr uint32_t SKETCH_SEED_HI = 0x9747B28Cu, SKETCH_SEED_LO = 0x5BD1E995u;

}  // namespace hm
