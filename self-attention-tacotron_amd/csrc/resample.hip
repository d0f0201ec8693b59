// Sample-rate conversion by band-limited interpolation: librosa.core.load(path, sr=...) of
// utils/audio.py:30-31 for a batch of utterances in one launch (include/sat_abi.h "resampling").
//
// The caller's table holds, for each of the L phases of the reduced ratio L / M, the `taps`
// filter values one output needs; output n of utterance b is
//   scale * sum_j table[(n M) mod L][j] * x_b[floor(n M / L) + offset + j],   x_b zero outside the
// utterance.
//
// resample_kernel, grid (ceil(stride_out / 256), B), 256 threads: a workgroup owns 256
// consecutive outputs of one utterance.  It stages the input samples they read --
// ceil(255 M / L) + taps of them, zeros where the index falls outside [0, length) -- in LDS, so
// the halo at the utterance's edges never touches the neighbouring row.  Each of the four waves
// then takes every fourth output: its lanes spread over the taps (lane l adds taps l, l + 64, ..
// in that order with fused multiply-adds, so both the table row and the LDS reads are
// contiguous), a butterfly over the lanes forms the sum, and the result goes to LDS.  The tile is
// written out in one coalesced pass, zeros past the utterance's output length.  Every sum has an
// order fixed by the sizes alone: no atomics, bit-identical runs.
#include "sat_common.h"

using namespace sat;

namespace {

constexpr int kTile = 256;                  // outputs per workgroup
constexpr int64_t kMaxLds = 64 * 1024;      // bytes of LDS a workgroup may ask for

struct ResampleP {
  const float* wav; const int32_t* lengths; const float* table; float* out;
  int stride_in, stride_out, L, M, taps, offset, span;
  float scale;
};

__global__ void __launch_bounds__(256) resample_kernel(ResampleP p) {
  extern __shared__ __align__(16) float xs[];           // span inputs, then kTile results
  float* ys = xs + p.span;
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t n0 = (int64_t)blockIdx.x * kTile;
  int64_t len = p.lengths[b];
  if (len < 0 || len > p.stride_in) len = 0;            // a length the entry would have refused
  int64_t n_out = (len * p.L + p.M - 1) / p.M;
  n_out = n_out < p.stride_out ? n_out : p.stride_out;
  float* o = p.out + (int64_t)b * p.stride_out;
  const int nt = (int)(p.stride_out - n0 < kTile ? p.stride_out - n0 : kTile);
  if (n0 >= n_out) {                                    // wholly past the utterance
    if (tid < nt) o[n0 + tid] = 0.f;
    return;
  }
  const int64_t first = n0 * p.M / p.L;                 // floor: the tile's first input period
  const int64_t k0 = first + p.offset;                  // input index of xs[0]; may be negative
  const float* x = p.wav + (int64_t)b * p.stride_in;
  for (int i = tid; i < p.span; i += 256) {
    const int64_t k = k0 + i;
    xs[i] = (k >= 0 && k < len) ? x[k] : 0.f;
  }
  __syncthreads();
  const int nv = (int)(n_out - n0 < nt ? n_out - n0 : nt);
  for (int t = wave; t < nv; t += 4) {
    const int64_t nm = (n0 + t) * p.M, i0 = nm / p.L;
    const float* row = p.table + (nm - i0 * p.L) * p.taps;
    const float* xt = xs + (i0 - first);                // (i0 - first) + taps <= span
    float acc = 0.f;
    for (int j = lane; j < p.taps; j += 64) acc = fmaf(row[j], xt[j], acc);
    acc = wave_sum(acc);
    if (lane == 0) ys[t] = acc * p.scale;
  }
  __syncthreads();
  if (tid < nt) o[n0 + tid] = tid < nv ? ys[tid] : 0.f;
}

inline bool aligned4(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 3) == 0; }

}  // namespace

extern "C" int sat_resample(const float* wav, const int32_t* lengths,
                            const int32_t* lengths_host, int32_t B, int32_t stride_in,
                            const float* table, int32_t L, int32_t M, int32_t taps,
                            int32_t offset, float scale, float* out, int32_t stride_out,
                            void* stream) {
  SAT_CHECK_ARG(B >= 0 && B <= 65535, "sat_resample: B %d outside 0..65535", B);
  SAT_CHECK_ARG(L >= 1 && M >= 1 && taps >= 1, "sat_resample: L %d, M %d, taps %d: each must be "
                ">= 1", L, M, taps);
  SAT_CHECK_ARG(stride_in >= 0 && stride_out >= 0, "sat_resample: bad sizes");
  SAT_CHECK_ARG(std::isfinite(scale), "sat_resample: scale is not finite");
  if (B == 0) return SAT_OK;
  SAT_CHECK_ARG(wav && lengths && lengths_host && table && out, "sat_resample: null pointer");
  SAT_CHECK_ARG(aligned4(wav) && aligned4(lengths) && aligned4(table) && aligned4(out),
                "sat_resample: a pointer is not 4-byte aligned");
  int64_t max_len = 0;
  for (int b = 0; b < B; ++b) {
    const int len = lengths_host[b];
    SAT_CHECK_ARG(len >= 0 && len <= stride_in, "sat_resample: lengths[%d] = %d outside 0.."
                  "stride_in %d", b, len, stride_in);
    max_len = std::max<int64_t>(max_len, len);
  }
  const int64_t need = (max_len * L + M - 1) / M;
  SAT_CHECK_ARG(stride_out >= need, "sat_resample: stride_out %d < the longest output %lld "
                "(%lld samples at %d / %d)", stride_out, (long long)need, (long long)max_len, L, M);
  if (stride_out == 0) return SAT_OK;
  const int64_t span = ((int64_t)(kTile - 1) * M + L - 1) / L + taps;
  if ((span + kTile) * (int64_t)sizeof(float) > kMaxLds) {
    set_error("sat_resample: %d taps at %d / %d need %lld bytes of LDS per tile, more than %lld",
              taps, L, M, (long long)((span + kTile) * sizeof(float)), (long long)kMaxLds);
    return SAT_ERR_UNSUPPORTED;
  }
  ResampleP p{wav, lengths, table, out, stride_in, stride_out, L, M, taps, offset, (int)span,
              scale};
  const int tiles = ceil_div(stride_out, kTile);
  hipLaunchKernelGGL(resample_kernel, dim3(tiles, B), dim3(256),
                     sizeof(float) * (size_t)(span + kTile), as_stream(stream), p);
  SAT_LAUNCH_CHECK("sat_resample");
  return SAT_OK;
}
