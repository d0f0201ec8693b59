// Audio front end: waveform -> log-mel targets (utils/audio.py:51-73 with librosa 0.6 stft
// semantics) and the per-utterance mel statistics of preprocess/ljspeech.py:119-131.
//
// sat_melspec: one workgroup per PAIR of frames of one utterance, on the STFT core of csrc/stft.h
// (gather, butterfly passes, separation of the two spectra).  Magnitudes replace the twiddle table
// in LDS (8 bytes longer), the band sums read them there, and only num_mels floats per frame leave
// the chip.
// The separation, the magnitude, the band sum and the logarithm are done in fp64 (a few hundred
// operations per frame beside the 11 k butterflies), so the FFT's own fp32 rounding is the only
// error of the result -- DESIGN.md "Audio front end".  With SatMelSpec.offsets an utterance is a
// segment of its row (the silence trim's bounds, csrc/trim.hip): the row pointer moves by the
// offset and everything else, the reflection at the segment's ends included, is as before.
#include "stft.h"

using namespace sat;

namespace {

struct MelSpecP {
  const float* wav; const int32_t* lengths; const int32_t* offsets;
  const float* window; const float2* twiddle;
  const float* basis; const int32_t* band_lo; const int32_t* band_hi;
  float* out; float* mag_out;
  int B, wav_stride, n_fft, log2n, hop, num_mels, num_freq, F_max;
  float ref_level_db, amp_floor;
};

__device__ __forceinline__ float magnitude(double re, double im) {
  return (float)sqrt(re * re + im * im);
}

__global__ void __launch_bounds__(256) melspec_kernel(MelSpecP p) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int n = p.n_fft, half_n = n >> 1, nf = p.num_freq, tid = threadIdx.x;
  float2* z = reinterpret_cast<float2*>(smem_raw);
  float2* tw = z + n;                                   // half_n twiddles
  float* mag = reinterpret_cast<float*>(tw);            // later: 2 x nf magnitudes
  const int b = blockIdx.y, f0 = 2 * blockIdx.x, f1 = f0 + 1;

  // a length or an offset the entry would have refused (device copy out of step with the host's)
  // reads nothing
  const int L = p.lengths[b], off = p.offsets ? p.offsets[b] : 0;
  int frames = (L > half_n && off >= 0 && (int64_t)off + L <= p.wav_stride) ? 1 + L / p.hop : 0;
  if (frames > p.F_max) frames = p.F_max;
  float* out0 = p.out + ((int64_t)b * p.F_max + f0) * p.num_mels;
  float* mag0 = p.mag_out ? p.mag_out + ((int64_t)b * p.F_max + f0) * nf : nullptr;
  const bool row1 = f1 < p.F_max;                       // the pair's second row exists at all

  if (f0 >= frames) {                                   // both rows are padding: zeros
    const int rows = row1 ? 2 : 1;
    for (int i = tid; i < rows * p.num_mels; i += 256) out0[i] = 0.f;
    if (mag0)
      for (int i = tid; i < rows * nf; i += 256) mag0[i] = 0.f;
    return;
  }
  const bool have1 = f1 < frames;

  const float* y = p.wav + (int64_t)b * p.wav_stride + off;
  stft_gather_pair(z, tw, y, L, f0, f1, have1, p.window, p.twiddle, n, p.log2n, p.hop, tid);
  fft_passes<false>(z, tw, p.log2n, half_n, tid);

  // the last pass's barrier also released the twiddles: magnitudes take their place
  for (int k = tid; k < nf; k += 256) {
    const BinPair x = separate_bin(z, k, n);
    const float m0 = magnitude(x.r0(), x.i0());
    const float m1 = have1 ? magnitude(x.r1(), x.i1()) : 0.f;
    mag[k] = m0;
    mag[nf + k] = m1;
    if (mag0) {
      mag0[k] = m0;
      if (row1) mag0[nf + k] = m1;
    }
  }
  __syncthreads();

  for (int t = tid; t < 2 * p.num_mels; t += 256) {
    const int fr = t >= p.num_mels, m = t - fr * p.num_mels;
    if (fr && !row1) continue;
    float v = 0.f;
    if (!fr || have1) {
      int lo = p.band_lo[m], hi = p.band_hi[m];
      lo = lo < 0 ? 0 : lo;
      hi = hi > nf ? nf : hi;
      const float* wrow = p.basis + (int64_t)m * nf;
      const float* mg = mag + fr * nf;
      double acc = 0.0;
      for (int k = lo; k < hi; ++k) acc += (double)wrow[k] * (double)mg[k];
      const double fl = (double)p.amp_floor;
      v = (float)(20.0 * log10(acc > fl ? acc : fl) - (double)p.ref_level_db);
    }
    out0[fr * p.num_mels + m] = v;
  }
}

struct MelStatsP {
  const float* mel; const int32_t* frames; double* out;
  int B, F_max, M;
};

// One block per (utterance, 16 mel bins): 16 frame slices x 16 bins.  Each slice folds its frames
// f = slice, slice + 16, .. (sums in fp64), one thread per bin then folds the 16 slices in a fixed
// order: no atomics, the same bits on every run.
__global__ void __launch_bounds__(256) mel_stats_kernel(MelStatsP p) {
  __shared__ double part[16][16][4];
  const int b = blockIdx.y;
  const int cg = threadIdx.x & 15, slice = threadIdx.x >> 4;
  const int m = blockIdx.x * 16 + cg;
  int rows = p.frames[b];
  rows = rows < 0 ? 0 : (rows > p.F_max ? p.F_max : rows);
  double mn = INFINITY, mx = -INFINITY, s1 = 0.0, s2 = 0.0;
  if (m < p.M) {
    const float* base = p.mel + (int64_t)b * p.F_max * p.M + m;
    for (int f = slice; f < rows; f += 16) {
      const double v = base[(int64_t)f * p.M];
      mn = v < mn ? v : mn;
      mx = v > mx ? v : mx;
      s1 += v;
      s2 += v * v;
    }
  }
  part[slice][cg][0] = mn; part[slice][cg][1] = mx;
  part[slice][cg][2] = s1; part[slice][cg][3] = s2;
  __syncthreads();
  if (slice == 0 && m < p.M) {
    for (int k = 1; k < 16; ++k) {
      mn = part[k][cg][0] < mn ? part[k][cg][0] : mn;
      mx = part[k][cg][1] > mx ? part[k][cg][1] : mx;
      s1 += part[k][cg][2];
      s2 += part[k][cg][3];
    }
    double* o = p.out + (int64_t)b * 4 * p.M + m;
    o[0] = mn; o[p.M] = mx; o[2 * p.M] = s1; o[3 * p.M] = s2;
  }
}

}  // namespace

extern "C" int sat_melspec(const SatMelSpec* d, void* stream) {
  SAT_CHECK_ARG(d, "sat_melspec: null descriptor");
  const int n = d->n_fft;
  if (const int rc = check_stft_config("sat_melspec", n, d->hop, d->win, d->num_freq)) return rc;
  SAT_CHECK_ARG(d->B >= 0 && d->B <= 65535 && d->num_mels >= 1 && d->wav_stride >= 0 &&
                d->F_max >= 0, "sat_melspec: bad sizes");
  if (d->B == 0) return SAT_OK;
  SAT_CHECK_ARG(d->wav && d->lengths && d->lengths_host && d->window && d->twiddle && d->basis &&
                d->band_lo && d->band_hi && d->out, "sat_melspec: null pointer");
  SAT_CHECK_ARG(!d->offsets == !d->offsets_host,
                "sat_melspec: offsets and offsets_host go together (both or neither)");
  SAT_CHECK_ARG((reinterpret_cast<uintptr_t>(d->twiddle) & 7) == 0,
                "sat_melspec: twiddle table must be 8-byte aligned");
  int max_frames = 0;
  for (int b = 0; b < d->B; ++b) {
    const int L = d->lengths_host[b];
    SAT_CHECK_ARG(L > n / 2, "sat_melspec: lengths[%d] = %d <= n_fft/2 = %d (the reflection would "
                  "run past the utterance)", b, L, n / 2);
    SAT_CHECK_ARG(L <= d->wav_stride, "sat_melspec: lengths[%d] = %d > wav_stride %d", b, L,
                  d->wav_stride);
    if (d->offsets) {
      const int off = d->offsets_host[b];
      SAT_CHECK_ARG(off >= 0 && (int64_t)off + L <= d->wav_stride, "sat_melspec: segment %d = "
                    "[%d, %d + %d) leaves the row of %d samples", b, off, off, L, d->wav_stride);
    }
    max_frames = std::max(max_frames, 1 + L / d->hop);
  }
  SAT_CHECK_ARG(d->F_max >= max_frames, "sat_melspec: F_max %d < the largest frame count %d",
                d->F_max, max_frames);
  MelSpecP p{d->wav, d->lengths, d->offsets, d->window, reinterpret_cast<const float2*>(d->twiddle), d->basis,
             d->band_lo, d->band_hi, d->out, d->mag_out, d->B, d->wav_stride, n, ilog2(n), d->hop,
             d->num_mels, d->num_freq, d->F_max, d->ref_level_db, d->amp_floor};
  // + 8: 2 x (n/2 + 1) magnitudes take the place of the n/2 float2 twiddles
  hipLaunchKernelGGL(melspec_kernel, dim3((d->F_max + 1) / 2, d->B), dim3(256),
                     stft_lds_bytes(n) + 8, as_stream(stream), p);
  SAT_LAUNCH_CHECK("sat_melspec");
  return SAT_OK;
}

extern "C" int sat_mel_stats(const float* mel, const int32_t* frames, int32_t B, int32_t F_max,
                             int32_t M, double* out, void* stream) {
  SAT_CHECK_ARG(B >= 0 && B <= 65535 && F_max >= 0 && M >= 1, "sat_mel_stats: bad sizes");
  if (B == 0) return SAT_OK;
  SAT_CHECK_ARG(frames && out && (mel || F_max == 0), "sat_mel_stats: null pointer");
  SAT_CHECK_ARG((reinterpret_cast<uintptr_t>(out) & 7) == 0, "sat_mel_stats: out must be 8-byte aligned");
  MelStatsP p{mel, frames, out, B, F_max, M};
  hipLaunchKernelGGL(mel_stats_kernel, dim3((M + 15) / 16, B), dim3(256), 0, as_stream(stream), p);
  SAT_LAUNCH_CHECK("sat_mel_stats");
  return SAT_OK;
}
