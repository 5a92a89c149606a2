// The row rules of the AUC engine (docs/compat.md "AUC engine"), one text for the gfx950 prepare
// kernel (auc.hip) and the host twin (auc_cpu.cpp).
//
//   key    an int64 that orders as the fp64 score does: -0.0 becomes 0.0, a negative value has its
//          63 magnitude bits flipped, a positive one is its own bits.  It is the unsigned key
//          "negatives bit-flipped, positives with the sign bit set" with the top bit flipped, so
//          that a signed compare (and torch.sort on int64) applies.  +-inf are ordinary values.
//   class  AUC_NEG / AUC_POS / AUC_ABSENT: a row with a NaN score or a NaN label is absent, a
//          label > 0 is positive.
#pragma once
#include <stdint.h>
#include <string.h>

#include "hd.h"

enum { AUC_NEG = 0, AUC_POS = 1, AUC_ABSENT = 2 };
// how the caller's columns are stored
enum { AUC_F64 = 0, AUC_F32 = 1, AUC_I64 = 2, AUC_I32 = 3 };

HM_HD int64_t auc_key(double s) {
    int64_t b;
    memcpy(&b, &s, 8);
    if (((uint64_t)b << 1) == 0) return 0;         // -0.0 == 0.0
    return b < 0 ? b ^ INT64_MAX : b;
}

HM_HD double auc_score_at(const void* p, int kind, int64_t i) {
    return kind == AUC_F64 ? ((const double*)p)[i] : (double)((const float*)p)[i];
}

// the class a label gives a row whose score is not NaN
HM_HD int auc_label_class(const void* p, int kind, int64_t i) {
    switch (kind) {
    case AUC_F64: {
        const double y = ((const double*)p)[i];
        return y != y ? AUC_ABSENT : y > 0.0 ? AUC_POS : AUC_NEG;
    }
    case AUC_F32: {
        const float y = ((const float*)p)[i];
        return y != y ? AUC_ABSENT : y > 0.f ? AUC_POS : AUC_NEG;
    }
    case AUC_I64:
        return ((const int64_t*)p)[i] > 0 ? AUC_POS : AUC_NEG;
    default:
        return ((const int32_t*)p)[i] > 0 ? AUC_POS : AUC_NEG;
    }
}

// Row `src` of the caller's columns (n rows) as (key, class); a `src` outside 0..n-1 is absent.
HM_HD int auc_row(const void* scores, int score_kind, const void* labels, int label_kind, int64_t n,
                  int64_t src, int64_t* key) {
    *key = 0;
    if (src < 0 || src >= n) return AUC_ABSENT;
    const double s = auc_score_at(scores, score_kind, src);
    if (s != s) return AUC_ABSENT;
    *key = auc_key(s);
    return auc_label_class(labels, label_kind, src);
}
