// The counter-based generator of every Bernoulli mask (sat_rng_fill, include/sat_abi.h): the one
// copy shared by the fill kernels (rng.hip) and the kernels that draw their own words
// (decode_persistent.hip).
#pragma once
#include "sat_common.h"

namespace sat {

// Philox-4x32-10 (Salmon et al., SC'11): 4 x 32-bit outputs per (counter, key).
__device__ __forceinline__ uint4 philox(uint4 ctr, uint2 key) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(M0, ctr.x), lo0 = M0 * ctr.x;
    const uint32_t hi1 = __umulhi(M1, ctr.z), lo1 = M1 * ctr.z;
    ctr = make_uint4(hi1 ^ ctr.y ^ key.x, lo1, hi0 ^ ctr.w ^ key.y, lo0);
    key.x += W0;
    key.y += W1;
  }
  return ctr;
}

// u = (float)v * 2^-32 < keep.  (float)v rounds the 129 largest words up to 2^32, so u can be
// exactly 1.0: keep >= 1 (a rate-0 mask) keeps every element outright instead of dropping those.
// No draw with keep < 1 is affected.
__device__ __forceinline__ bool rng_keep(uint32_t v, float keep) {
  return keep >= 1.f || (float)v * 2.3283064365386963e-10f /* 2^-32 */ < keep;
}

// The mask value sat_rng_fill writes at element i of a tensor drawn on `stream_id` with `key`
// (= the seed's two halves): word i % 4 of Philox(counter = {i / 4, stream_id}, key).
__device__ __forceinline__ float rng_mask_value(uint64_t i, uint64_t stream_id, uint2 key,
                                                float keep, float on) {
  const uint64_t g = i >> 2;
  const uint4 r = philox(make_uint4((uint32_t)g, (uint32_t)(g >> 32), (uint32_t)stream_id,
                                    (uint32_t)(stream_id >> 32)), key);
  const uint32_t j = (uint32_t)i & 3u;
  const uint32_t v = j == 0 ? r.x : j == 1 ? r.y : j == 2 ? r.z : r.w;
  return rng_keep(v, keep) ? on : 0.f;
}

}  // namespace sat
