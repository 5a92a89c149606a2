// The order of the SLIM recommendation engine (docs/compat.md "SLIM recommendation"), one text
// for the gfx950 kernel (slim_topk.hip) and the host twin (hm_slim_topk_cpu in slim_cpu.cpp).
//
//   key     the fp64 score as a u64 that sorts best first: the bits made to order as the value
//           does (sign bit set on a positive value, all bits flipped on a negative one), then
//           inverted.  A score is a sum that starts at +0.0, so it is never -0.0 and the map is one
//           to one; st_unkey gives the score's bits back.  No finite or infinite score maps to
//           ST_WORST_KEY.
//   better  the total order of (key, item) pairs: smaller key, then smaller item index.
#pragma once
#include <stdint.h>
#include <string.h>

#include "hd.h"

#define ST_WORST_KEY (~0ull)
#define ST_WORST_ITEM 0xffffffffu

HM_HD uint64_t st_key(double s) {
    uint64_t b;
    memcpy(&b, &s, 8);
    return ~(b ^ ((b >> 63) ? ~0ull : 0x8000000000000000ull));
}

HM_HD double st_unkey(uint64_t key) {
    const uint64_t u = ~key;
    const uint64_t b = (u >> 63) ? (u ^ 0x8000000000000000ull) : ~u;
    double s;
    memcpy(&s, &b, 8);
    return s;
}

HM_HD bool st_better(uint64_t k1, uint32_t i1, uint64_t k2, uint32_t i2) {
    return k1 < k2 || (k1 == k2 && i1 < i2);
}
