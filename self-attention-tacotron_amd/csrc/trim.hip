// Silence trim bounds: Audio.trim (utils/audio.py:40-49) with librosa 0.6 effects.trim semantics,
// for a batch of utterances in one entry call (include/sat_abi.h "silence trim").
//
// Two launches on the caller's stream:
//   trim_energy_kernel, grid (frame tiles of 64, B), 256 threads: ms[b][f] = the mean square of
//     frame f of the utterance reflect-padded by frame_length/2 (taken by index, as sat_melspec).
//     Where frame_length = R * hop the tile first forms the 64 + R - 1 per-hop partial sums it
//     needs in LDS -- one wave per hop chunk, lane j adds samples j, j + 64, .. in that order, then
//     a butterfly over the lanes -- and frame f is partial[f] + .. + partial[f + R - 1] added left
//     to right, so a sample is read from memory once per tile (64 + R - 1 chunks for 64 frames)
//     instead of R times.  Any other (frame_length, hop) takes one wave per frame over the
//     frame's own samples.  Either way every sum is fp32 in an order fixed by the sizes alone.
//   trim_bounds_kernel, grid (B), 256 threads: the largest ms of the utterance, the first and the
//     last frame with max(amin, ms) > max(amin, msmax) * 10^(-top_db / 10), and the two bounds.
//     max / min over integers and floats: no order dependence, no atomics.
#include "sat_common.h"

using namespace sat;

namespace {

constexpr int kTileFrames = 64;
constexpr int kMaxHopRatio = 1024;      // R above this: the per-frame path (LDS stays under 5 KB)
constexpr float kAmin = 1e-10f;         // librosa.power_to_db's amin

struct TrimP {
  const float* wav; const int32_t* lengths; float* ms; int32_t* bounds;
  int B, wav_stride, frame_length, hop, ratio, ms_stride, pad_samples;
  float factor;
};

// frames of an utterance of L samples, 0 for a length the entry would have refused
__device__ __forceinline__ int trim_frames(const TrimP& p, int L) {
  const int half = p.frame_length >> 1;
  if (L <= half || L > p.wav_stride) return 0;
  const int64_t f = 1 + ((int64_t)L + 2 * half - p.frame_length) / p.hop;
  return (int)(f < p.ms_stride ? f : p.ms_stride);
}

// sample i of the padded utterance (i counted from the first padding sample), squared
// (not stft.h's reflect_index: a 64-bit index about the trim's own half-width; keep it apart)
__device__ __forceinline__ float padded_square(const float* y, int64_t i, int half, int L) {
  i -= half;
  if (i < 0) i = -i;
  if (i >= L) i = 2 * (int64_t)(L - 1) - i;
  const float v = y[i];
  return v * v;
}

__global__ void __launch_bounds__(256) trim_energy_kernel(TrimP p) {
  extern __shared__ __align__(16) float partial[];
  const int b = blockIdx.y, f0 = blockIdx.x * kTileFrames;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int L = p.lengths[b];
  const int frames = trim_frames(p, L);
  if (f0 >= frames) return;
  const int half = p.frame_length >> 1;
  const float* y = p.wav + (int64_t)b * p.wav_stride;
  float* out = p.ms + (int64_t)b * p.ms_stride;
  const int nf = frames - f0 < kTileFrames ? frames - f0 : kTileFrames;
  const float inv = 1.0f / (float)p.frame_length;

  if (p.ratio > 0) {
    // chunk c of the tile = padded samples [(f0 + c) * hop, + hop); the last frame of the
    // utterance ends at frames - 1 + ratio chunks, inside the padded utterance
    const int nc = nf + p.ratio - 1;
    for (int c = wave; c < nc; c += 4) {
      const int64_t base = (int64_t)(f0 + c) * p.hop;
      float s = 0.f;
      for (int j = lane; j < p.hop; j += 64) s += padded_square(y, base + j, half, L);
      s = wave_sum(s);
      if (lane == 0) partial[c] = s;
    }
    __syncthreads();
    if ((int)threadIdx.x < nf) {
      float s = 0.f;
      for (int r = 0; r < p.ratio; ++r) s += partial[threadIdx.x + r];
      out[f0 + threadIdx.x] = s * inv;
    }
  } else {
    for (int t = wave; t < nf; t += 4) {
      const int64_t base = (int64_t)(f0 + t) * p.hop;
      float s = 0.f;
      for (int j = lane; j < p.frame_length; j += 64) s += padded_square(y, base + j, half, L);
      s = wave_sum(s);
      if (lane == 0) out[f0 + t] = s * inv;
    }
  }
}

__global__ void __launch_bounds__(256) trim_bounds_kernel(TrimP p) {
  __shared__ float smax[4];
  __shared__ int sfirst[4], slast[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int L = p.lengths[b];
  const int frames = trim_frames(p, L);
  const float* ms = p.ms + (int64_t)b * p.ms_stride;

  float mx = 0.f;                                       // mean squares are >= 0
  for (int f = tid; f < frames; f += 256) mx = fmaxf(mx, ms[f]);
  mx = block_max(mx, smax);
  const float thr = fmaxf(kAmin, mx) * p.factor;

  int first = INT32_MAX, last = -1;
  for (int f = tid; f < frames; f += 256)
    if (fmaxf(kAmin, ms[f]) > thr) {
      first = f < first ? f : first;
      last = f;
    }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int of = __shfl_xor(first, o, 64), ol = __shfl_xor(last, o, 64);
    first = of < first ? of : first;
    last = ol > last ? ol : last;
  }
  if (lane == 0) { sfirst[wave] = first; slast[wave] = last; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w) {
      first = sfirst[w] < first ? sfirst[w] : first;
      last = slast[w] > last ? slast[w] : last;
    }
    int64_t i0 = 0, i1 = 0;
    if (last >= 0) {
      i0 = (int64_t)first * p.hop;
      i1 = (int64_t)(last + 1) * p.hop;
      i1 = i1 < L ? i1 : L;
    }
    const int64_t Lc = frames > 0 ? L : 0;             // a refused length: (0, 0)
    int64_t start = i0 - p.pad_samples, stop = i1 + p.pad_samples;
    start = start > 0 ? start : 0;
    stop = stop < Lc ? stop : Lc;
    p.bounds[2 * b] = (int32_t)start;
    p.bounds[2 * b + 1] = (int32_t)stop;
  }
}

}  // namespace

extern "C" int sat_trim_bounds(const float* wav, const int32_t* lengths,
                               const int32_t* lengths_host, int32_t B, int32_t wav_stride,
                               int32_t frame_length, int32_t hop, float top_db,
                               int32_t pad_samples, int32_t* bounds, float* frame_ms,
                               int32_t ms_stride, void* stream) {
  SAT_CHECK_ARG(B >= 0 && B <= 65535, "sat_trim_bounds: B %d outside 0..65535", B);
  SAT_CHECK_ARG(hop >= 1, "sat_trim_bounds: hop %d < 1", hop);
  SAT_CHECK_ARG(frame_length >= 2, "sat_trim_bounds: frame_length %d < 2", frame_length);
  SAT_CHECK_ARG(std::isfinite(top_db) && top_db >= 0.f,
                "sat_trim_bounds: top_db %g is not a finite value >= 0", (double)top_db);
  SAT_CHECK_ARG(pad_samples >= 0, "sat_trim_bounds: pad_samples %d < 0", pad_samples);
  SAT_CHECK_ARG(wav_stride >= 0 && ms_stride >= 0, "sat_trim_bounds: bad sizes");
  if (B == 0) return SAT_OK;
  SAT_CHECK_ARG(wav && lengths && lengths_host && bounds && frame_ms,
                "sat_trim_bounds: null pointer");
  const int half = frame_length / 2;
  int64_t max_frames = 0;
  for (int b = 0; b < B; ++b) {
    const int L = lengths_host[b];
    SAT_CHECK_ARG(L > half, "sat_trim_bounds: lengths[%d] = %d <= frame_length/2 = %d (the "
                  "reflection would run past the utterance)", b, L, half);
    SAT_CHECK_ARG(L <= wav_stride, "sat_trim_bounds: lengths[%d] = %d > wav_stride %d", b, L,
                  wav_stride);
    max_frames = std::max(max_frames, 1 + ((int64_t)L + 2 * half - frame_length) / hop);
  }
  SAT_CHECK_ARG(ms_stride >= max_frames, "sat_trim_bounds: ms_stride %d < the largest frame "
                "count %lld", ms_stride, (long long)max_frames);
  const int ratio = (frame_length % hop == 0 && frame_length / hop <= kMaxHopRatio)
                        ? frame_length / hop : 0;
  TrimP p{wav, lengths, frame_ms, bounds, B, wav_stride, frame_length, hop, ratio, ms_stride,
          pad_samples, (float)std::pow(10.0, -(double)top_db / 10.0)};
  const int tiles = (int)((max_frames + kTileFrames - 1) / kTileFrames);
  const size_t lds = ratio > 0 ? sizeof(float) * (kTileFrames + ratio - 1) : 0;
  hipLaunchKernelGGL(trim_energy_kernel, dim3(tiles, B), dim3(256), lds, as_stream(stream), p);
  SAT_LAUNCH_CHECK("sat_trim_bounds");
  hipLaunchKernelGGL(trim_bounds_kernel, dim3(B), dim3(256), 0, as_stream(stream), p);
  SAT_LAUNCH_CHECK("sat_trim_bounds");
  return SAT_OK;
}
