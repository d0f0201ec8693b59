// The one STFT core of the audio kernels (audio.hip, vocoder.hip): librosa 0.6 stft / istft
// semantics, the padded periodic Hann window, the (cos, -sin) twiddle table of n_fft/2 entries, one
// workgroup of 256 threads per PAIR of frames.  The two windowed frames x0, x1 are the real and
// imaginary part of one complex n_fft-point FFT z = x0 + i x1 in LDS (radix-2 decimation in time:
// the gather writes bit-reversed, log2(n_fft) butterfly passes follow); the spectra separate as
// X0[k] = (Z[k] + conj Z[n-k]) / 2, X1[k] = (Z[k] - conj Z[n-k]) / 2i at no further twiddle.  The
// inverse runs the same passes with the table's sine negated.
#pragma once
#include "sat_common.h"

namespace sat {
namespace {

// LDS: z [n_fft] float2 + n_fft/2 float2 twiddles; 24 KB at 2048 (6 workgroups per CU), 48 at 4096
constexpr size_t stft_lds_bytes(int n_fft) { return (size_t)12 * n_fft; }

// sample j of frame f of the utterance reflect-padded by n_fft/2 on both sides, by index on the
// unpadded row: i = f*hop + j - n_fft/2, mirrored about 0 (i -> -i) or about L-1 (i -> 2(L-1)-i).
// With n_fft/2 < L and f <= L/hop one mirror always lands inside [0, L).
__device__ __forceinline__ int reflect_index(int f, int j, int hop, int half_n, int L) {
  int i = f * hop + j - half_n;
  if (i < 0) i = -i;
  if (i >= L) i = 2 * (L - 1) - i;
  return i;
}

// frames f0 and f1 (when have1) of the row y of L samples, windowed, into z bit-reversed and the
// twiddles into tw; ends in the barrier.  A zero of the window (its padding) reads no sample.
__device__ __forceinline__ void stft_gather_pair(float2* z, float2* tw, const float* y, int L,
                                                 int f0, int f1, bool have1, const float* window,
                                                 const float2* twiddle, int n, int log2n, int hop,
                                                 int tid) {
  const int half_n = n >> 1, shift = 32 - log2n;
  for (int j = tid; j < n; j += 256) {
    const float w = window[j];
    float v0 = 0.f, v1 = 0.f;
    if (w != 0.f) {
      v0 = w * y[reflect_index(f0, j, hop, half_n, L)];
      if (have1) v1 = w * y[reflect_index(f1, j, hop, half_n, L)];
    }
    z[__brev((unsigned)j) >> shift] = make_float2(v0, v1);
  }
  for (int j = tid; j < half_n; j += 256) tw[j] = twiddle[j];
  __syncthreads();
}

template <bool kInverse>
__device__ __forceinline__ void fft_passes(float2* z, const float2* tw, int log2n, int half_n,
                                           int tid) {
  for (int s = 0; s < log2n; ++s) {
    const int half = 1 << s, tshift = log2n - 1 - s;
    for (int j = tid; j < half_n; j += 256) {
      const int pos = j & (half - 1);
      const int i0 = ((j >> s) << (s + 1)) + pos, i1 = i0 + half;
      float2 w = tw[pos << tshift];
      if (kInverse) w.y = -w.y;
      const float2 a = z[i0], c = z[i1];
      const float tr = c.x * w.x - c.y * w.y, ti = c.x * w.y + c.y * w.x;
      z[i0] = make_float2(a.x + tr, a.y + ti);
      z[i1] = make_float2(a.x - tr, a.y - ti);
    }
    __syncthreads();
  }
}

// bin k of the two frames' spectra X0 = r0 + i i0, X1 = r1 + i i1 out of Z, in fp64; computed on
// demand, so that a caller's `if (have1)` keeps the second frame's arithmetic inside its branch
struct BinPair {
  float2 a, c;                  // Z[k], Z[n-k]
  __device__ __forceinline__ double r0() const { return 0.5 * ((double)a.x + c.x); }
  __device__ __forceinline__ double i0() const { return 0.5 * ((double)a.y - c.y); }
  __device__ __forceinline__ double r1() const { return 0.5 * ((double)a.y + c.y); }
  __device__ __forceinline__ double i1() const { return 0.5 * ((double)c.x - a.x); }
};
__device__ __forceinline__ BinPair separate_bin(const float2* z, int k, int n) {
  return {z[k], z[(n - k) & (n - 1)]};
}

// ------------------------------------------------------------------ host side
inline int ilog2(int n) {
  int l = 0;
  while ((1 << l) < n) ++l;
  return l;
}

// the configuration every STFT entry accepts; returns SAT_OK or the refusal's code
inline int check_stft_config(const char* who, int n, int hop, int win, int num_freq) {
  if (n < 64 || n > 4096 || (n & (n - 1)) != 0) {
    set_error("%s: n_fft %d is not a power of two in 64..4096", who, n);
    return SAT_ERR_UNSUPPORTED;
  }
  SAT_CHECK_ARG(win >= 1 && win <= n, "%s: win %d outside 1..n_fft %d", who, win, n);
  SAT_CHECK_ARG(hop >= 1, "%s: hop %d < 1", who, hop);
  SAT_CHECK_ARG(num_freq == n / 2 + 1, "%s: num_freq %d != n_fft/2 + 1 = %d", who, num_freq,
                n / 2 + 1);
  return SAT_OK;
}

}  // namespace
}  // namespace sat
