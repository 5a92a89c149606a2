// MurmurHash3_x86_32 / mhash over packed UTF-8 strings on gfx950 (SURVEY.md §2.3.10, K1;
// upstream core/src/main/java/hivemall/utils/hashing/MurmurHash3.java,
// ftvec/hashing/{MurmurHash3UDF,FeatureHashingUDF}.java).
//
// Input: one byte buffer + int64 offsets (string s = buf[off[s] .. off[s+1])), read through
// hm::sweep of strspan.h (which states what it asks of buf): 256 strings and a 16 KB window per
// 256-thread block and step (the span is usually < 8 KB for feature names), every lane hashes its
// own string.  Output = raw hash (uint32) or mhash ((int)h % num_features, negatives fixed up, +1)
// — bit-exact with the Java/C++ versions.
#include "common.h"
#include "murmur3.h"
#include "strspan.h"

namespace {

constexpr int HASH_STRINGS = 256;
constexpr int HASH_LDS = 16 * 1024;

struct MhashOp {
    uint32_t seed;
    int32_t num_features;
    int32_t* out;
    template <typename Words>
    __device__ __forceinline__ void operator()(int64_t s, const Words& word, int len) const {
        const uint32_t h = hm::mm3(word, len, seed);
        out[s] = num_features > 0 ? hm::mhash_reduce(h, num_features) : (int32_t)h;
    }
};

__global__ __launch_bounds__(HASH_STRINGS) void mhash_kernel(const uint8_t* __restrict__ buf,
                                                             const int64_t* __restrict__ off, int64_t n,
                                                             uint32_t seed, int32_t num_features,
                                                             int32_t* __restrict__ out) {
    __shared__ uint4 s_stage[hm::stage_vecs(HASH_LDS)];
    MhashOp op{seed, num_features, out};
    hm::sweep<HASH_STRINGS, HASH_LDS>(buf, off, n, s_stage, op);
}

}  // namespace

// num_features <= 0: raw 32-bit hash; else mhash in [1, num_features].
HM_API int hm_mhash(const uint8_t* buf, const int64_t* off, int64_t n, uint32_t seed,
                    int32_t num_features, int32_t* out, hipStream_t stream) {
    if (n <= 0) return 0;
    int64_t blocks = (n + HASH_STRINGS - 1) / HASH_STRINGS;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(mhash_kernel, dim3((int)blocks), dim3(HASH_STRINGS), 0, stream, buf, off, n, seed,
                       num_features, out);
    HM_LAUNCH_RET();
}
