// VQ-code targets (include/sat_abi.h "VQ-code batches"): the fork's targets are one-hot code frames
// (datasets/codes/dataset.py), stored and fed by the reference as dense float32 [T, C].  Here a batch
// travels as its code indices and is expanded on the device.
//
//   codes_batch_kernel<VEC4>, one launch: a grid-stride loop over the B * T_pad * (C / 4) float4s
//     (VEC4, C % 4 == 0: consecutive lanes store consecutive 16 bytes, so at C = 256 a wave writes
//     one whole 1 KB row) or over the B * T_pad * C floats (any C >= 1) of `codes`.  The unit at
//     column 0 of a row also writes that row's two loss-mask entries, its `done` entry (rows whose
//     t is a multiple of r) and, at t = 0, target_length[b]: every output element has exactly one
//     writer, nothing is cleared beforehand.  All lanes of a row read the same idx entry (one
//     cache line, broadcast).  An index outside 0..C-1 is never used as an address: the row is
//     written as zeros and the error word is raised by a 64-bit atomic max of ~((b << 32) | t),
//     so the word names the lowest (utterance, position) whatever the order of the waves.
//   codes_argmax_kernel: a group of G lanes per row (G = 64 above 32 columns, else the smallest
//     power of two >= C, so a wave holds 64 / G rows).  Lane j scans columns j, j + G, .. in
//     ascending order keeping the first maximum, then a butterfly over the group merges
//     (value, index) pairs by "larger value, then lower index": a fixed order, no atomics, ties to
//     the lowest index, NaN ranked above every number (numpy's argmax).
#include "sat_common.h"

using namespace sat;

namespace {

struct CodesBatchP {
  const int32_t* idx; const int64_t* offsets;
  float* codes; float* done; float* cmask; float* bmask; int64_t* target_length;
  unsigned long long* err;
  int64_t n_idx, rows, units;        // rows = B * T_pad, units = rows * cw
  int B, C, cw, T_pad, r, steps;     // cw = units per row (C / 4 or C), steps = T_pad / r
};

// I: the type the flat unit index is divided in -- uint32_t wherever the unit count fits (a
// 64-bit division is several times the instructions, twice per unit), int64_t above that
template <bool VEC4, typename I>
__global__ void __launch_bounds__(256) codes_batch_kernel(CodesBatchP p) {
  const I stride = (I)gridDim.x * 256, units = (I)p.units;
  for (I e = (I)blockIdx.x * 256 + threadIdx.x; e < units; e += stride) {
    const I row = e / (I)p.cw;
    const int q = (int)(e - row * (I)p.cw);
    const int b = (int)(row / (I)p.T_pad);
    const int t = (int)(row - (I)b * (I)p.T_pad);
    const int64_t o0 = p.offsets[b];
    // a device length the entry would have refused is clamped to what the buffers hold
    int64_t Tb = p.offsets[b + 1] - o0;
    Tb = Tb < 0 ? 0 : (Tb > p.T_pad ? p.T_pad : Tb);
    const bool inside = t < Tb && o0 >= 0 && o0 + t < p.n_idx;
    int k = -1;
    if (inside) {
      k = p.idx[o0 + t];
      if ((unsigned)k >= (unsigned)p.C) {
        if (q == 0) atomicMax(p.err, ~(((unsigned long long)(unsigned)b << 32) | (unsigned)t));
        k = -1;
      }
    }
    if (VEC4) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (k >= 0 && (k >> 2) == q) {
        const int c = k & 3;
        v.x = c == 0 ? 1.f : 0.f;
        v.y = c == 1 ? 1.f : 0.f;
        v.z = c == 2 ? 1.f : 0.f;
        v.w = c == 3 ? 1.f : 0.f;
      }
      reinterpret_cast<float4*>(p.codes)[e] = v;
    } else {
      p.codes[e] = k == q ? 1.f : 0.f;
    }
    if (q == 0) {
      const float m = t < Tb ? 1.f : 0.f;
      p.cmask[row] = m;
      p.bmask[row] = m;
      if (t % p.r == 0) {
        const int s = t / p.r;
        p.done[(int64_t)b * p.steps + s] = s == (int)(Tb / p.r) - 1 ? 1.f : 0.f;
      }
      if (t == 0) p.target_length[b] = Tb;
    }
  }
}

struct CodesArgmaxP {
  const float* x; int32_t* out; float* onehot;
  int64_t ldx, ldo;
  int R, C, G, shift;                // G lanes per row, shift = log2(G)
};

// (ov, oi) ranks before (v, i): NaN above every number, then the larger value, then the lower index
__device__ __forceinline__ bool ranks_before(float ov, int oi, float v, int i) {
  const bool on = ov != ov, vn = v != v;
  if (on || vn) return on && (!vn || oi < i);
  return ov > v || (ov == v && oi < i);
}

__global__ void __launch_bounds__(256) codes_argmax_kernel(CodesArgmaxP p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int per_wave = 64 >> p.shift;
  const int j = lane & (p.G - 1);
  const int64_t row = ((int64_t)blockIdx.x * 4 + wave) * per_wave + (lane >> p.shift);
  const bool live = row < p.R;
  float v = -INFINITY;
  int i = INT32_MAX;
  if (live) {
    const float* x = p.x + row * p.ldx;
    for (int c = j; c < p.C; c += p.G) {
      const float w = x[c];
      if (ranks_before(w, c, v, i)) { v = w; i = c; }
    }
  }
  // every lane of the wave takes part in the butterfly, live or not
  for (int o = p.G >> 1; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(i, o, 64);
    if (ranks_before(ov, oi, v, i)) { v = ov; i = oi; }
  }
  if (!live) return;
  if (j == 0) p.out[row] = i;
  if (p.onehot) {
    float* oh = p.onehot + row * p.ldo;
    for (int c = j; c < p.C; c += p.G) oh[c] = c == i ? 1.f : 0.f;
  }
}

inline bool aligned_to(const void* ptr, uintptr_t a) {
  return (reinterpret_cast<uintptr_t>(ptr) & (a - 1)) == 0;
}

}  // namespace

extern "C" int sat_codes_batch(const int32_t* idx, int64_t n_idx, const int64_t* offsets,
                               const int64_t* offsets_host, int32_t B, int32_t C, int32_t T_pad,
                               int32_t r, float* codes, float* done, float* code_loss_mask,
                               float* binary_loss_mask, int64_t* target_length, uint64_t* err,
                               void* stream) {
  SAT_CHECK_ARG(B >= 0, "sat_codes_batch: B %d < 0", B);
  SAT_CHECK_ARG(C >= 1, "sat_codes_batch: C %d < 1", C);
  SAT_CHECK_ARG(r >= 1, "sat_codes_batch: r %d < 1", r);
  SAT_CHECK_ARG(T_pad >= 1, "sat_codes_batch: T_pad %d < 1", T_pad);
  SAT_CHECK_ARG(T_pad % r == 0, "sat_codes_batch: T_pad %d is not a multiple of r %d", T_pad, r);
  SAT_CHECK_ARG(n_idx >= 0, "sat_codes_batch: n_idx %lld < 0", (long long)n_idx);
  if (B == 0) return SAT_OK;
  SAT_CHECK_ARG(idx && offsets && offsets_host && codes && done && code_loss_mask &&
                binary_loss_mask && target_length && err, "sat_codes_batch: null pointer");
  SAT_CHECK_ARG(offsets_host[0] == 0, "sat_codes_batch: offsets[0] = %lld, not 0",
                (long long)offsets_host[0]);
  for (int b = 0; b < B; ++b) {
    const int64_t Tb = offsets_host[b + 1] - offsets_host[b];
    SAT_CHECK_ARG(Tb >= 1, "sat_codes_batch: utterance %d has %lld codes (< 1)", b, (long long)Tb);
    SAT_CHECK_ARG(Tb <= T_pad, "sat_codes_batch: T_pad %d < utterance %d's %lld codes", T_pad, b,
                  (long long)Tb);
  }
  SAT_CHECK_ARG(offsets_host[B] == n_idx, "sat_codes_batch: offsets[B] = %lld but idx holds %lld "
                "entries", (long long)offsets_host[B], (long long)n_idx);
  const bool vec4 = C % 4 == 0;
  SAT_CHECK_ARG(aligned_to(codes, vec4 ? 16 : 4), "sat_codes_batch: codes is not %d-byte aligned",
                vec4 ? 16 : 4);
  SAT_CHECK_ARG(aligned_to(idx, 4) && aligned_to(done, 4) && aligned_to(code_loss_mask, 4) &&
                aligned_to(binary_loss_mask, 4), "sat_codes_batch: idx, done or a mask is not "
                "4-byte aligned");
  SAT_CHECK_ARG(aligned_to(offsets, 8) && aligned_to(target_length, 8) && aligned_to(err, 8),
                "sat_codes_batch: offsets, target_length or err is not 8-byte aligned");
  CodesBatchP p{};
  p.idx = idx; p.offsets = offsets; p.codes = codes; p.done = done; p.cmask = code_loss_mask;
  p.bmask = binary_loss_mask; p.target_length = target_length;
  p.err = reinterpret_cast<unsigned long long*>(err);
  p.n_idx = n_idx; p.B = B; p.C = C; p.T_pad = T_pad; p.r = r; p.steps = T_pad / r;
  p.cw = vec4 ? C / 4 : C;
  p.rows = (int64_t)B * T_pad;
  p.units = p.rows * p.cw;
  const int blocks = (int)std::min<int64_t>((p.units + 255) / 256, 4096);
  // e + stride must not wrap in 32 bits: stride <= 4096 * 256 = 2^20
  const bool small = p.units < (int64_t)0xFFFFFFFF - (4096 * 256);
  auto kernel = vec4 ? (small ? codes_batch_kernel<true, uint32_t> : codes_batch_kernel<true, int64_t>)
                     : (small ? codes_batch_kernel<false, uint32_t>
                              : codes_batch_kernel<false, int64_t>);
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, as_stream(stream), p);
  SAT_LAUNCH_CHECK("sat_codes_batch");
  return SAT_OK;
}

extern "C" int sat_codes_argmax(const float* x, int64_t ldx, int32_t R, int32_t C, int32_t* out,
                                float* onehot, int64_t ld_onehot, void* stream) {
  SAT_CHECK_ARG(R >= 0, "sat_codes_argmax: R %d < 0", R);
  SAT_CHECK_ARG(C >= 1, "sat_codes_argmax: C %d < 1", C);
  SAT_CHECK_ARG(ldx >= C, "sat_codes_argmax: row stride %lld < C %d", (long long)ldx, C);
  SAT_CHECK_ARG(!onehot || ld_onehot >= C, "sat_codes_argmax: one-hot row stride %lld < C %d",
                (long long)ld_onehot, C);
  if (R == 0) return SAT_OK;
  SAT_CHECK_ARG(x && out, "sat_codes_argmax: null pointer");
  SAT_CHECK_ARG(aligned_to(x, 4) && aligned_to(out, 4) && aligned_to(onehot, 4),
                "sat_codes_argmax: a pointer is not 4-byte aligned");
  CodesArgmaxP p{};
  p.x = x; p.out = out; p.onehot = onehot; p.ldx = ldx; p.ldo = ld_onehot; p.R = R; p.C = C;
  p.shift = 6;
  if (C <= 32) {
    p.shift = 0;
    while ((1 << p.shift) < C) ++p.shift;
  }
  p.G = 1 << p.shift;
  const int rows_per_block = 4 * (64 >> p.shift);
  hipLaunchKernelGGL(codes_argmax_kernel, dim3(ceil_div(R, rows_per_block)), dim3(256), 0,
                     as_stream(stream), p);
  SAT_LAUNCH_CHECK("sat_codes_argmax");
  return SAT_OK;
}
