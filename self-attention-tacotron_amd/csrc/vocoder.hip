// Vocoder: normalised mel -> linear magnitudes -> waveform by Griffin-Lim, the inverse of the audio
// front end (csrc/audio.hip) on the same STFT core (csrc/stft.h: conventions, FFT in LDS, size).
//
// sat_mel_to_linear: one workgroup per frame; the frame's num_mels amplitudes 10^(dB / 20) go to
//   LDS as doubles, thread k forms lin[k] = max(1e-10, inv_basis[k] . amp)^power in fp64.
// sat_istft: the two launches every synthesis step is made of --
//   inverse_kernel, one workgroup of 256 threads per PAIR of frames: the two half spectra X0, X1
//     are extended by conjugate symmetry and combined as Z = X0 + i X1, one complex inverse FFT
//     gives frame 0 in the real and frame 1 in the imaginary part; times window / n_fft they go to
//     the frame buffer, and only over the window's support [(n_fft - win) / 2, + win): the
//     zero-padded rest of a frame adds nothing.
//   overlap_add_kernel, one thread per output sample: a GATHER over the few frames whose window
//     support covers the sample, added in ascending frame order in fp64 together with the window's
//     squares, divided where that sum exceeds FLT_MIN.  No atomics: the same bits on every run.
// sat_griffin_lim: init_kernel (angles = exp(i init_phase), prev = 0; the only sincos), then per
//   iteration inverse_kernel (spectrum = mag * angles), overlap_add_kernel into the intermediate
//   waveform and analysis_kernel: the core's forward FFT of frame pairs of the reflect-padded
//   intermediate waveform, whose separated spectra give t = reb - c prev, prev = reb and the new
//   unit phasors t / (|t| + 1e-16) in fp64 around the fp32 butterflies.  A last inverse +
//   overlap-add writes the caller's waveform.  Everything is queued on the caller's stream; nothing
//   is read back.
// The overlap-add is its own kernel rather than part of the analysis kernel's gather: a sample is
// read by n_fft / hop analysis frames, so folding the sum in would repeat it that many times, and
// the last synthesis needs the stand-alone kernel anyway.
#include <cfloat>

#include "stft.h"

using namespace sat;

namespace {

constexpr double kLinFloor = 1e-10;     // the clamp under the power of sat_mel_to_linear
constexpr double kPhaseEps = 1e-16;     // librosa's griffinlim: angles = t / (|t| + 1e-16)

inline int64_t align256(int64_t n) { return (n + 255) / 256 * 256; }

// frames of utterance b as the kernels use them: 0 for a count the entry would have refused
// (a device copy out of step with the host's), so that nothing is read or written out of bounds
__device__ __forceinline__ int valid_frames(int F, int F_max, int hop, int half_n, int stride) {
  if (F < 1 || F > F_max) return 0;
  const int64_t L = (int64_t)hop * (F - 1);
  return (L > half_n && L <= stride) ? F : 0;
}

// ------------------------------------------------------------------ mel -> linear
struct MelLinP {
  const float* mel; const int32_t* frames; const float* inv_basis;
  const float* average; const float* stddev; float* out;
  int B, F_max, M, num_freq;
  float ref_level_db, power;
};

__global__ void __launch_bounds__(256) mel_to_linear_kernel(MelLinP p) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  double* amp = reinterpret_cast<double*>(smem_raw);
  const int b = blockIdx.y, f = blockIdx.x, tid = threadIdx.x;
  int F = p.frames[b];
  F = F < 0 ? 0 : (F > p.F_max ? p.F_max : F);
  float* out = p.out + ((int64_t)b * p.F_max + f) * p.num_freq;
  if (f >= F) {
    for (int k = tid; k < p.num_freq; k += 256) out[k] = 0.f;
    return;
  }
  const float* mel = p.mel + ((int64_t)b * p.F_max + f) * p.M;
  for (int m = tid; m < p.M; m += 256) {
    const double db = (double)mel[m] * (double)p.stddev[m] + (double)p.average[m] +
                      (double)p.ref_level_db;
    amp[m] = pow(10.0, db * 0.05);
  }
  __syncthreads();
  for (int k = tid; k < p.num_freq; k += 256) {
    const float* row = p.inv_basis + (int64_t)k * p.M;
    double acc = 0.0;
    for (int m = 0; m < p.M; ++m) acc += (double)row[m] * amp[m];
    out[k] = (float)pow(acc > kLinFloor ? acc : kLinFloor, (double)p.power);
  }
}

// ------------------------------------------------------------------ synthesis
struct SynthP {
  const float2* spec;           // [B][F_max][nf] complex, read when mag == nullptr
  const float* mag;             // [B][F_max][nf] with ang: spectrum = mag * ang
  const float2* ang;
  const int32_t* frames; const float* window; const float2* twiddle;
  float* fb;                    // frame buffer [B][F_max][n_fft], window support only
  float* wav;                   // [B][wav_stride]
  int B, F_max, n_fft, log2n, hop, win_lo, win, num_freq, wav_stride;
};

__device__ __forceinline__ float2 load_bin(const SynthP& p, int64_t row, int k, int half_n) {
  const int64_t i = row * p.num_freq + k;
  float2 v;
  if (p.mag) {
    const float m = p.mag[i];
    const float2 a = p.ang[i];
    v = make_float2(m * a.x, m * a.y);
  } else {
    v = p.spec[i];
  }
  // a real signal's spectrum is real at 0 and at n_fft/2: an inverse real FFT ignores what is not
  if (k == 0 || k == half_n) v.y = 0.f;
  return v;
}

__global__ void __launch_bounds__(256) inverse_kernel(SynthP p) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int n = p.n_fft, half_n = n >> 1, tid = threadIdx.x;
  float2* z = reinterpret_cast<float2*>(smem_raw);
  float2* tw = z + n;
  const int b = blockIdx.y, f0 = 2 * blockIdx.x, f1 = f0 + 1;
  const int F = valid_frames(p.frames[b], p.F_max, p.hop, half_n, p.wav_stride);
  if (f0 >= F) return;
  const bool have1 = f1 < F;
  const int64_t row0 = (int64_t)b * p.F_max + f0;
  const int shift = 32 - p.log2n;

  for (int k = tid; k <= half_n; k += 256) {
    const float2 x0 = load_bin(p, row0, k, half_n);
    const float2 x1 = have1 ? load_bin(p, row0 + 1, k, half_n) : make_float2(0.f, 0.f);
    // Z[k] = X0[k] + i X1[k];  Z[n-k] = conj X0[k] + i conj X1[k]
    z[__brev((unsigned)k) >> shift] = make_float2(x0.x - x1.y, x0.y + x1.x);
    if (k > 0 && k < half_n)
      z[__brev((unsigned)(n - k)) >> shift] = make_float2(x0.x + x1.y, x1.x - x0.y);
  }
  for (int j = tid; j < half_n; j += 256) tw[j] = p.twiddle[j];
  __syncthreads();

  fft_passes<true>(z, tw, p.log2n, half_n, tid);

  const float inv_n = 1.0f / (float)n;                  // a power of two: exact
  float* fb0 = p.fb + row0 * n;
  for (int j = p.win_lo + tid; j < p.win_lo + p.win; j += 256) {
    const float w = p.window[j] * inv_n;
    const float2 v = z[j];
    fb0[j] = w * v.x;
    if (have1) fb0[n + j] = w * v.y;
  }
}

// sample i of utterance b sits at p = i + n_fft/2 of the padded signal; frame f covers it with
// window sample j = p - f*hop, inside the support for win_lo <= j < win_lo + win
__global__ void __launch_bounds__(256) overlap_add_kernel(SynthP p) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= p.wav_stride) return;
  const int half_n = p.n_fft >> 1;
  const int F = valid_frames(p.frames[b], p.F_max, p.hop, half_n, p.wav_stride);
  float v = 0.f;
  if (F > 0 && i < p.hop * (F - 1)) {
    const int q = i + half_n - p.win_lo;                // q - f*hop in [0, win)
    int f_hi = q / p.hop;                               // q >= 0: win_lo <= n_fft/2
    int f_lo = q - p.win + 1 <= 0 ? 0 : (q - p.win + p.hop) / p.hop;
    if (f_hi > F - 1) f_hi = F - 1;
    const float* fb = p.fb + (int64_t)b * p.F_max * p.n_fft;
    double acc = 0.0, wss = 0.0;
    for (int f = f_lo; f <= f_hi; ++f) {
      const int j = p.win_lo + q - f * p.hop;
      const double w = (double)p.window[j];
      acc += (double)fb[(int64_t)f * p.n_fft + j];
      wss += w * w;
    }
    v = (float)(wss > (double)FLT_MIN ? acc / wss : acc);
  }
  p.wav[(int64_t)b * p.wav_stride + i] = v;
}

// ------------------------------------------------------------------ Griffin-Lim
struct GlP {
  const float* x;               // intermediate waveform [B][x_stride]
  const int32_t* frames; const float* window; const float2* twiddle;
  const float* init_phase;
  float2* ang; float2* prev;    // [B][F_max][nf]; prev nullptr: momentum 0
  int B, F_max, n_fft, log2n, hop, num_freq, x_stride;
  double c;                     // momentum / (1 + momentum)
};

__global__ void __launch_bounds__(256) init_kernel(GlP p, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  double s, c;
  sincos((double)p.init_phase[i], &s, &c);
  p.ang[i] = make_float2((float)c, (float)s);
  if (p.prev) p.prev[i] = make_float2(0.f, 0.f);
}

__device__ __forceinline__ void update_phase(const GlP& p, int64_t i, double re, double im) {
  double tr = re, ti = im;
  if (p.prev) {
    const float2 pv = p.prev[i];
    tr -= p.c * (double)pv.x;
    ti -= p.c * (double)pv.y;
    p.prev[i] = make_float2((float)re, (float)im);
  }
  const double m = sqrt(tr * tr + ti * ti) + kPhaseEps;
  p.ang[i] = make_float2((float)(tr / m), (float)(ti / m));
}

__global__ void __launch_bounds__(256) analysis_kernel(GlP p) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int n = p.n_fft, half_n = n >> 1, nf = p.num_freq, tid = threadIdx.x;
  float2* z = reinterpret_cast<float2*>(smem_raw);
  float2* tw = z + n;
  const int b = blockIdx.y, f0 = 2 * blockIdx.x, f1 = f0 + 1;
  const int F = valid_frames(p.frames[b], p.F_max, p.hop, half_n, p.x_stride);
  if (f0 >= F) return;
  const bool have1 = f1 < F;
  const int L = p.hop * (F - 1);                        // frames of it: 1 + L / hop = F again
  const float* y = p.x + (int64_t)b * p.x_stride;
  stft_gather_pair(z, tw, y, L, f0, f1, have1, p.window, p.twiddle, n, p.log2n, p.hop, tid);
  fft_passes<false>(z, tw, p.log2n, half_n, tid);

  const int64_t row0 = ((int64_t)b * p.F_max + f0) * nf;
  for (int k = tid; k < nf; k += 256) {
    const BinPair x = separate_bin(z, k, n);
    update_phase(p, row0 + k, x.r0(), x.i0());
    if (have1) update_phase(p, row0 + nf + k, x.r1(), x.i1());
  }
}

// ------------------------------------------------------------------ host side
struct Stft {
  int B, F_max, n_fft, hop, win, num_freq, wav_stride;
  const int32_t* frames; const int32_t* frames_host;
};

// the checks the synthesis entries share; returns SAT_OK or the refusal's code
int check_stft(const char* who, const Stft& s) {
  const int n = s.n_fft;
  if (const int rc = check_stft_config(who, n, s.hop, s.win, s.num_freq)) return rc;
  SAT_CHECK_ARG(s.B >= 0 && s.B <= 65535 && s.F_max >= 0 && s.wav_stride >= 0, "%s: bad sizes",
                who);
  SAT_CHECK_ARG(s.B == 0 || (s.frames && s.frames_host), "%s: null pointer (frames)", who);
  for (int b = 0; b < s.B; ++b) {
    const int F = s.frames_host[b];
    SAT_CHECK_ARG(F <= s.F_max, "%s: frames[%d] = %d > F_max %d", who, b, F, s.F_max);
    const int64_t L = (int64_t)s.hop * ((int64_t)F - 1);
    SAT_CHECK_ARG(F >= 1 && L > n / 2, "%s: frames[%d] = %d gives %lld samples <= n_fft/2 = %d "
                  "(the reflection would run past the utterance)", who, b, F, (long long)L, n / 2);
    SAT_CHECK_ARG(L <= s.wav_stride, "%s: wav_stride %d < the %lld samples of utterance %d", who,
                  s.wav_stride, (long long)L, b);
  }
  return SAT_OK;
}

// inverse FFT of every pair of frames into fb, then the gather into wav
int launch_synthesis(const char* who, SynthP p, void* stream) {
  hipLaunchKernelGGL(inverse_kernel, dim3((p.F_max + 1) / 2, p.B), dim3(256),
                     stft_lds_bytes(p.n_fft), as_stream(stream), p);
  SAT_LAUNCH_CHECK(who);
  hipLaunchKernelGGL(overlap_add_kernel, dim3((p.wav_stride + 255) / 256, p.B), dim3(256), 0,
                     as_stream(stream), p);
  SAT_LAUNCH_CHECK(who);
  return SAT_OK;
}

}  // namespace

extern "C" int sat_mel_to_linear(const float* mel, const int32_t* frames,
                                 const int32_t* frames_host, int32_t B, int32_t F_max, int32_t M,
                                 int32_t num_freq, const float* inv_basis, const float* average,
                                 const float* stddev, float ref_level_db, float power, float* out,
                                 void* stream) {
  SAT_CHECK_ARG(B >= 0 && B <= 65535 && F_max >= 0 && F_max <= 65535 * 32 && M >= 1 && M <= 4096 &&
                num_freq >= 1, "sat_mel_to_linear: bad sizes");
  SAT_CHECK_ARG(std::isfinite(power) && power > 0.f, "sat_mel_to_linear: power %g is not a finite "
                "value > 0", (double)power);
  if (B == 0 || F_max == 0) return SAT_OK;
  SAT_CHECK_ARG(mel && frames && frames_host && inv_basis && average && stddev && out,
                "sat_mel_to_linear: null pointer");
  for (int b = 0; b < B; ++b)
    SAT_CHECK_ARG(frames_host[b] >= 0 && frames_host[b] <= F_max, "sat_mel_to_linear: frames[%d] = "
                  "%d outside 0..F_max %d", b, frames_host[b], F_max);
  MelLinP p{mel, frames, inv_basis, average, stddev, out, B, F_max, M, num_freq, ref_level_db,
            power};
  hipLaunchKernelGGL(mel_to_linear_kernel, dim3(F_max, B), dim3(256), sizeof(double) * M,
                     as_stream(stream), p);
  SAT_LAUNCH_CHECK("sat_mel_to_linear");
  return SAT_OK;
}

extern "C" int64_t sat_istft_scratch_bytes(int32_t B, int32_t F_max, int32_t n_fft) {
  if (B < 0 || F_max < 0 || n_fft < 0) return SAT_ERR_ARGUMENT;
  return align256((int64_t)sizeof(float) * B * F_max * n_fft);
}

extern "C" int64_t sat_griffin_lim_scratch_bytes(int32_t B, int32_t F_max, int32_t n_fft,
                                                 int32_t hop, int32_t momentum_on) {
  if (B < 0 || F_max < 0 || n_fft < 0 || hop < 0) return SAT_ERR_ARGUMENT;
  const int64_t rows = (int64_t)B * F_max, nf = n_fft / 2 + 1;
  const int64_t x_stride = F_max > 1 ? (int64_t)hop * (F_max - 1) : 0;
  return sat_istft_scratch_bytes(B, F_max, n_fft) +
         (momentum_on ? 2 : 1) * align256((int64_t)sizeof(float2) * rows * nf) +
         align256((int64_t)sizeof(float) * B * x_stride);
}

extern "C" int sat_istft(const float* spec, const int32_t* frames, const int32_t* frames_host,
                         int32_t B, int32_t F_max, int32_t n_fft, int32_t hop, int32_t win,
                         int32_t num_freq, const float* window, const float* twiddle, float* wav,
                         int32_t wav_stride, void* scratch, int64_t scratch_bytes, void* stream) {
  const Stft s{B, F_max, n_fft, hop, win, num_freq, wav_stride, frames, frames_host};
  if (const int rc = check_stft("sat_istft", s)) return rc;
  if (B == 0) return SAT_OK;
  SAT_CHECK_ARG(spec && window && twiddle && wav && scratch, "sat_istft: null pointer");
  SAT_CHECK_ARG((reinterpret_cast<uintptr_t>(spec) & 7) == 0 &&
                (reinterpret_cast<uintptr_t>(twiddle) & 7) == 0 &&
                (reinterpret_cast<uintptr_t>(scratch) & 15) == 0,
                "sat_istft: spec and twiddle must be 8-byte, scratch 16-byte aligned");
  const int64_t need = sat_istft_scratch_bytes(B, F_max, n_fft);
  SAT_CHECK_ARG(scratch_bytes >= need, "sat_istft: scratch of %lld bytes, %lld needed "
                "(sat_istft_scratch_bytes)", (long long)scratch_bytes, (long long)need);
  SynthP p{reinterpret_cast<const float2*>(spec), nullptr, nullptr, frames, window,
           reinterpret_cast<const float2*>(twiddle), static_cast<float*>(scratch), wav, B, F_max,
           n_fft, ilog2(n_fft), hop, (n_fft - win) / 2, win, num_freq, wav_stride};
  return launch_synthesis("sat_istft", p, stream);
}

extern "C" int sat_griffin_lim(const SatGriffinLim* d, void* stream) {
  SAT_CHECK_ARG(d, "sat_griffin_lim: null descriptor");
  const Stft s{d->B, d->F_max, d->n_fft, d->hop, d->win, d->num_freq, d->wav_stride, d->frames,
               d->frames_host};
  if (const int rc = check_stft("sat_griffin_lim", s)) return rc;
  SAT_CHECK_ARG(d->n_iter >= 0, "sat_griffin_lim: n_iter %d < 0", d->n_iter);
  SAT_CHECK_ARG(std::isfinite(d->momentum) && d->momentum >= 0.f && d->momentum < 1.f,
                "sat_griffin_lim: momentum %g outside [0, 1)", (double)d->momentum);
  if (d->B == 0) return SAT_OK;
  SAT_CHECK_ARG(d->mag && d->init_phase && d->window && d->twiddle && d->wav && d->scratch,
                "sat_griffin_lim: null pointer");
  SAT_CHECK_ARG((reinterpret_cast<uintptr_t>(d->twiddle) & 7) == 0 &&
                (reinterpret_cast<uintptr_t>(d->scratch) & 15) == 0,
                "sat_griffin_lim: twiddle must be 8-byte, scratch 16-byte aligned");
  const int64_t total = (int64_t)d->B * d->F_max * d->num_freq;
  SAT_CHECK_ARG((int64_t)d->hop * (d->F_max - 1) <= INT32_MAX && total / 256 < INT32_MAX,
                "sat_griffin_lim: hop %d x F_max %d rows of %d utterances exceed the index range",
                d->hop, d->F_max, d->B);
  const bool mom = d->momentum > 0.f;
  const int64_t need = sat_griffin_lim_scratch_bytes(d->B, d->F_max, d->n_fft, d->hop, mom);
  SAT_CHECK_ARG(d->scratch_bytes >= need, "sat_griffin_lim: scratch of %lld bytes, %lld needed "
                "(sat_griffin_lim_scratch_bytes)", (long long)d->scratch_bytes, (long long)need);

  const int n = d->n_fft, log2n = ilog2(n);
  const int x_stride = d->hop * (d->F_max - 1);         // > n_fft/2: F_max >= every frames[b]
  char* base = static_cast<char*>(d->scratch);
  float* fb = reinterpret_cast<float*>(base);
  base += sat_istft_scratch_bytes(d->B, d->F_max, n);
  float2* ang = reinterpret_cast<float2*>(base);
  base += align256((int64_t)sizeof(float2) * total);
  float2* prev = nullptr;
  if (mom) {
    prev = reinterpret_cast<float2*>(base);
    base += align256((int64_t)sizeof(float2) * total);
  }
  float* x = reinterpret_cast<float*>(base);

  const float2* tw = reinterpret_cast<const float2*>(d->twiddle);
  GlP g{x, d->frames, d->window, tw, d->init_phase, ang, prev, d->B, d->F_max, n, log2n, d->hop,
        d->num_freq, x_stride, (double)d->momentum / (1.0 + (double)d->momentum)};
  SynthP p{nullptr, d->mag, ang, d->frames, d->window, tw, fb, x, d->B, d->F_max, n, log2n,
           d->hop, (n - d->win) / 2, d->win, d->num_freq, x_stride};

  hipLaunchKernelGGL(init_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     as_stream(stream), g, total);
  SAT_LAUNCH_CHECK("sat_griffin_lim");
  for (int it = 0; it < d->n_iter; ++it) {
    if (const int rc = launch_synthesis("sat_griffin_lim", p, stream)) return rc;
    hipLaunchKernelGGL(analysis_kernel, dim3((d->F_max + 1) / 2, d->B), dim3(256),
                       stft_lds_bytes(n), as_stream(stream), g);
    SAT_LAUNCH_CHECK("sat_griffin_lim");
  }
  p.wav = d->wav;
  p.wav_stride = d->wav_stride;
  return launch_synthesis("sat_griffin_lim", p, stream);
}
