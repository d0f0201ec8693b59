"""Time of the vocoder on the shape of one predicted batch: B=32 utterances of 1000 frames
(n_fft 2048, hop 275: 274 725 samples, about 12.5 s each).

  * sat_griffin_lim at 60, 10 and 0 iterations (device events around the entry call, tables,
    magnitudes and start phases already resident; the scratch comes from torch's caching
    allocator, so after the warm-up no call allocates): the time per iteration is the slope
    between 10 and 60, the 0-iteration call is the start phasors plus one synthesis;
  * sat_mel_to_linear at the same shape;
  * the sat_melspec launch at the same shape, as the yardstick: one forward FFT per frame, where an
    iteration does a forward and an inverse one and moves the frame buffer once each way;
  * the bytes an iteration moves by design (counted below), as a fraction of HBM bandwidth.

Numbers from one machine and one run of this script; medians over the repetitions.

Usage: python tools/probes/griffin_lim_time.py [reps]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import _sat_path  # noqa: E402

_sat_path.load()
import numpy as np  # noqa: E402
import torch  # noqa: E402

from sat_amd import audio as A, hparams as H, kernels as K  # noqa: E402

HBM_PEAK = 8.0e12           # bytes/s, MI355X
B, FRAMES = 32, 1000
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20

hp = H.ljspeech_hparams()
dev = torch.device("cuda:0")
a = A.Audio(hp, device=dev)
n_fft, hop, win = a._stft_parameters()
nf = n_fft // 2 + 1
samples = hop * (FRAMES - 1)
frames = [FRAMES] * B

gen = torch.Generator(device=dev)
gen.manual_seed(0)
wav0 = torch.empty(B, samples, device=dev).normal_(0.0, 0.1, generator=gen)
_, _, mag = a.melspectrogram_batch(list(wav0), return_magnitudes=True)
assert mag.shape == (B, FRAMES, nf)
phase = torch.empty_like(mag).uniform_(-np.pi, np.pi, generator=gen)


def median_us(fn, n):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    ev = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        ev.append((e0, e1))
    torch.cuda.synchronize()
    us = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev)
    return us[len(us) // 2], us[0], us[-1]


t = {}
for n_iter in (0, 10, 60):
    t[n_iter] = median_us(lambda: a.griffin_lim_batch(mag, frames, n_iter=n_iter, momentum=0.99,
                                                      init_phase=phase), reps)
    print(f"sat_griffin_lim B={B} x {FRAMES} frames (n_fft {n_fft}), {n_iter} iterations, "
          f"momentum 0.99: median {t[n_iter][0] / 1e3:.2f} ms over {reps} calls (min "
          f"{t[n_iter][1] / 1e3:.2f}, max {t[n_iter][2] / 1e3:.2f})", flush=True)
per_iter = (t[60][0] - t[10][0]) / 50.0
t0 = median_us(lambda: a.griffin_lim_batch(mag, frames, n_iter=10, momentum=0.0,
                                           init_phase=phase), reps)[0]
t1 = median_us(lambda: a.griffin_lim_batch(mag, frames, n_iter=60, momentum=0.0,
                                           init_phase=phase), reps)[0]
per_iter0 = (t1 - t0) / 50.0

# bytes of one iteration: synthesis reads mag (4) and the phasors (8) per bin and writes the
# window support of every frame; the gather reads that and writes the waveform; the analysis
# reads the waveform once (its n_fft / hop re-reads hit the cache), reads and writes prev
# (momentum only) and writes the phasors
rows = B * FRAMES
it_bytes = rows * nf * 12 + 2 * rows * win * 4 + 2 * B * samples * 4 + rows * nf * 8
mom_bytes = it_bytes + rows * nf * 16
print(f"per iteration: {per_iter:.1f} us with momentum ({mom_bytes / 1e6:.0f} MB by design = "
      f"{100 * mom_bytes / (per_iter * 1e-6) / HBM_PEAK:.1f} % of {HBM_PEAK / 1e12:.0f} TB/s), "
      f"{per_iter0:.1f} us without ({it_bytes / 1e6:.0f} MB = "
      f"{100 * it_bytes / (per_iter0 * 1e-6) / HBM_PEAK:.1f} %); 3 launches each", flush=True)

mel = torch.zeros(B, FRAMES, hp.num_mels, device=dev)
ml = median_us(lambda: a.mel_to_linear_batch(mel, frames), reps)
print(f"sat_mel_to_linear at the same shape: median {ml[0]:.1f} us", flush=True)

plan = a._plan(dev)
lengths = [samples] * B
dl = torch.tensor(lengths, dtype=torch.int32, device=dev)
out = torch.empty(B, FRAMES, hp.num_mels, device=dev)
ms = median_us(lambda: K.melspec(wav0, dl, lengths, n_fft=n_fft, hop=hop, win=win,
                                 window=plan["window"], twiddle=plan["twiddle"],
                                 basis=plan["basis"], band_lo=plan["band_lo"],
                                 band_hi=plan["band_hi"], ref_level_db=hp.ref_level_db,
                                 amp_floor=A.AMP_FLOOR, out=out), 10 * reps)
print(f"sat_melspec at the same shape: median {ms[0]:.1f} us; one Griffin-Lim iteration = "
      f"{per_iter / ms[0]:.2f} x that launch, 60 iterations = {t[60][0] / 1e3:.2f} ms", flush=True)
