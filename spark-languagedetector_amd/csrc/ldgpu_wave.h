// ldgpu_wave.h -- wave-level (64 lanes) selection primitives shared by the
// top-k kernel (ldgpu_topk.hip) and the segment kernels (ldgpu_segments.hip):
// the order-preserving key of a score and the exact first-maximum pick.
#pragma once

#include "ldgpu_common.h"

namespace ldgpu {

__device__ __forceinline__ uint32_t rdlane(uint32_t v, int l) {
    return (uint32_t)__builtin_amdgcn_readlane((int)v, l);
}
__device__ __forceinline__ double rdlaned(double v, int l) {
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    return __longlong_as_double(
        (long long)((uint64_t)rdlane((uint32_t)b, l) | ((uint64_t)rdlane((uint32_t)(b >> 32), l) << 32)));
}

// wave maximum by DPP row shifts / broadcasts (lanes without a source keep 0,
// the identity); the result is read from lane 63 and is wave-uniform
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false));  // row_shr:1
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false));  // row_shr:2
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false));  // row_shr:4
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false));  // row_shr:8
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false));  // row_bcast:15
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false));  // row_bcast:31
    return rdlane(v, 63);
}
// u64: the high words' maximum, then the low words' among the lanes holding it
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
    const uint32_t hi = wave_max_u32((uint32_t)(v >> 32));
    const uint32_t lo = wave_max_u32((uint32_t)(v >> 32) == hi ? (uint32_t)v : 0u);
    return ((uint64_t)hi << 32) | lo;
}

// Order-preserving key of language l's score: greater key = earlier; equal
// keys = equal in the order (then the smaller index wins).  0 is no element
// (retired, or l >= L), 1 a NaN beyond index 0 -- below -inf's key 2^52 - 1.
__device__ __forceinline__ uint64_t topk_key(double v, int l) {
    if (v != v) return l == 0 ? ~0ull : 1ull;
    uint64_t b = (uint64_t)__double_as_longlong(v);
    if ((b << 1) == 0ull) b = 0ull;  // -0.0 equals +0.0
    return (b >> 63) ? ~b : b | (1ull << 63);
}

struct Pick {
    uint64_t key;
    int idx;
};

// the wave's next element: the maximal key, the smallest index holding it
__device__ __forceinline__ Pick wave_pick(uint64_t bk, int bi) {
    const uint64_t M = wave_max_u64(bk);
    const int w = (int)(0xffffffffu - wave_max_u32(bk == M ? 0xffffffffu - (uint32_t)bi : 0u));
    return Pick{M, w};
}

}  // namespace ldgpu
