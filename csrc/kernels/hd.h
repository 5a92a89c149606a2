// HM_HD marks a function of a header that is compiled both into the gfx950 kernels and into the
// host library or a host test (linear_rules.h, murmur3.h, parse.h, strspan.h): one text, the same
// numbers on both sides.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HM_HD __host__ __device__ __forceinline__
#define HM_HD_MEMBER HM_HD
#else
#define HM_HD static inline __attribute__((always_inline))   // as on the device: these must inline into the caller's loop
#define HM_HD_MEMBER inline __attribute__((always_inline))   // a member function takes no `static`
#endif
