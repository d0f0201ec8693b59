// Device digest of an arena (sat_amd/checkpoint.py): a position-dependent 64-bit checksum and a
// count of non-finite fp32 bit patterns over a buffer read as 32-bit words, accumulated into two
// uint64 words the caller zeroed.
//   out[0] += sum_i mix(base_index + i, w[i])   (mod 2^64)
//   out[1] += #{ i : (w[i] & 0x7F800000) == 0x7F800000 }        when count_nonfinite != 0
//   mix(p, w) = splitmix64 finaliser of ((p + 1) * 0x9E3779B97F4A7C15) ^ w  (include/sat_abi.h)
// The sum is an integer sum, so the result is exact whatever the grid, the block order or the
// shape of the reduction: one 64-bit integer atomic add per block (and one more only when the
// block saw a non-finite word).  16-byte loads in a grid-stride loop over the 16-byte-aligned
// body, a scalar head and tail (block 0) for a base that is only 4-byte aligned and a word count
// that is no multiple of 4.  (p + 1) * G advances by additions, so a word costs two 64-bit
// products; those, not memory, bound the kernel: measured 0.35-0.38 of the HBM read rate
// (31-34 us for 75 MB).
#include "sat_common.h"

namespace sat {
namespace {

constexpr unsigned long long kGolden = 0x9E3779B97F4A7C15ull;
constexpr int kDigestBlocks = 2048;

__device__ __forceinline__ unsigned long long mix_pos(unsigned long long pos_g, uint32_t w) {
  unsigned long long z = pos_g ^ (unsigned long long)w;   // pos_g = (p + 1) * kGolden
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__device__ __forceinline__ unsigned nonfinite(uint32_t w) {
  return (w & 0x7F800000u) == 0x7F800000u ? 1u : 0u;
}

// w: the buffer; head words before the first 16-byte boundary, then n4 uint4, then tail words
__global__ void __launch_bounds__(256) digest_kernel(const uint32_t* __restrict__ w, int head,
                                                     int64_t n4, int tail,
                                                     unsigned long long base, int count,
                                                     unsigned long long* __restrict__ out) {
  __shared__ unsigned long long sh_d[4];
  __shared__ unsigned sh_c[4];
  unsigned long long acc = 0ull;
  unsigned cnt = 0u;
  const uint4* __restrict__ body = reinterpret_cast<const uint4*>(w + head);
  const unsigned long long body_base = base + (unsigned long long)head + 1ull;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  unsigned long long pg = (body_base + 4ull * (unsigned long long)i) * kGolden;
  const unsigned long long pg_step = 4ull * (unsigned long long)stride * kGolden;
  for (; i < n4; i += stride, pg += pg_step) {
    const uint4 v = body[i];
    acc += mix_pos(pg, v.x) + mix_pos(pg + kGolden, v.y) + mix_pos(pg + 2ull * kGolden, v.z) +
           mix_pos(pg + 3ull * kGolden, v.w);
    cnt += nonfinite(v.x) + nonfinite(v.y) + nonfinite(v.z) + nonfinite(v.w);
  }
  if (blockIdx.x == 0) {
    const int t = threadIdx.x;           // head < 4 and tail < 4: one word per thread
    if (t < head) {
      const uint32_t x = w[t];
      acc += mix_pos((base + (unsigned long long)t + 1ull) * kGolden, x);
      cnt += nonfinite(x);
    }
    if (t < tail) {
      const int64_t k = (int64_t)head + 4 * n4 + t;
      const uint32_t x = w[k];
      acc += mix_pos((base + (unsigned long long)k + 1ull) * kGolden, x);
      cnt += nonfinite(x);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    acc += __shfl_xor(acc, o, 64);
    cnt += __shfl_xor(cnt, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    sh_d[threadIdx.x >> 6] = acc;
    sh_c[threadIdx.x >> 6] = cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long d = sh_d[0] + sh_d[1] + sh_d[2] + sh_d[3];
    const unsigned c = sh_c[0] + sh_c[1] + sh_c[2] + sh_c[3];
    atomicAdd(out, d);
    if (count && c != 0u) atomicAdd(out + 1, (unsigned long long)c);
  }
}

}  // namespace
}  // namespace sat

using namespace sat;

extern "C" int sat_arena_digest(const void* buf, int64_t n_words, int64_t base_index,
                                int32_t count_nonfinite, uint64_t* out, void* stream) {
  SAT_CHECK_ARG(n_words >= 0 && base_index >= 0 && out &&
                    (reinterpret_cast<uintptr_t>(out) & 7) == 0,
                "sat_arena_digest: n_words >= 0, base_index >= 0, out = two 8-byte-aligned words");
  if (n_words == 0) return SAT_OK;
  SAT_CHECK_ARG(buf && (reinterpret_cast<uintptr_t>(buf) & 3) == 0,
                "sat_arena_digest: buf must be a 4-byte-aligned device pointer");
  const int64_t to_boundary = (int64_t)((16 - (reinterpret_cast<uintptr_t>(buf) & 15)) & 15) / 4;
  const int head = (int)std::min<int64_t>(to_boundary, n_words);
  const int64_t n4 = (n_words - head) >> 2;
  const int tail = (int)((n_words - head) & 3);
  const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>((n4 + 255) / 256, kDigestBlocks));
  hipLaunchKernelGGL(digest_kernel, dim3(blocks), dim3(256), 0, as_stream(stream),
                     reinterpret_cast<const uint32_t*>(buf), head, n4, tail,
                     (unsigned long long)base_index, (int)count_nonfinite,
                     reinterpret_cast<unsigned long long*>(out));
  SAT_LAUNCH_CHECK("sat_arena_digest");
  return SAT_OK;
}
