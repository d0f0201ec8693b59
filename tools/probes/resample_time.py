"""Time of the resampler's launch at a preprocessing batch's size, beside the mel launch it feeds.

One sat_resample launch over B = 32 utterances of 10 s at 48 kHz brought to 22 050 Hz (147 / 320,
282 taps), device events around the entry call, beside what it must do by design: every input
sample read once and every output written once, as a fraction of HBM bandwidth, and
outputs x taps fused multiply-adds, as a fraction of the fp32 vector rate.  Then the sat_melspec
launch of the LJSpeech configuration on that output, timed the same way.

Numbers from one machine and one run of this script; medians over the repetitions.  Nothing here
says what bounds the resampler's time: that needs a counter run of its own.

Usage: python tools/probes/resample_time.py [reps]
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
FMA_PEAK = 157.3e12 / 2     # fp32 vector fused multiply-adds/s, MI355X
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
dev = torch.device("cuda:0")


def median_us(fn, n):
    for _ in range(5):
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


B, ORIG, TARGET, SECONDS = 32, 48000, 22050, 10
hp = H.ljspeech_hparams()
audio = A.Audio(hp, device=dev)
f = A.resample_filter(ORIG, TARGET)
n_in = ORIG * SECONDS
n_out = A.resampled_length(n_in, f.L, f.M)
gen = torch.Generator(device=dev)
gen.manual_seed(0)
wav = torch.empty(B, n_in, device=dev).uniform_(-0.5, 0.5, generator=gen)
lengths = [n_in] * B
dlen = torch.tensor(lengths, dtype=torch.int32, device=dev)
table = torch.from_numpy(np.array(f.table)).to(dev)
out = torch.empty(B, n_out, device=dev)
scale = min(1.0, f.L / f.M)
run = lambda: K.resample(wav, dlen, lengths, table=table, L=f.L, M=f.M, offset=f.offset,  # noqa: E731
                         scale=scale, out=out)
nbytes = 4 * B * (n_in + n_out)
fma = B * n_out * f.taps
print(f"B {B} x {SECONDS} s: {ORIG} -> {TARGET} Hz = {f.L}/{f.M}, {f.taps} taps, table "
      f"{f.table.nbytes / 1e3:.0f} kB; {n_in} -> {n_out} samples per utterance", flush=True)
t = median_us(run, reps)
print(f"sat_resample: median {t[0]:.1f} us over {reps} calls (min {t[1]:.1f}, max {t[2]:.1f}); "
      f"{nbytes / 1e6:.1f} MB by design = {100 * nbytes / (t[0] * 1e-6) / HBM_PEAK:.1f} % of "
      f"{HBM_PEAK / 1e12:.0f} TB/s; {fma / 1e9:.2f} G fused multiply-adds = "
      f"{100 * fma / (t[0] * 1e-6) / FMA_PEAK:.1f} % of {FMA_PEAK / 1e12:.1f} T/s", flush=True)
rows = [out[b] for b in range(B)]
audio.melspectrogram_batch(rows)                    # tables built and uploaded before the timing
n_fft, hop, win = audio._stft_parameters()
plan = audio._plan(dev)
olen = [n_out] * B
meta = torch.tensor([olen, [1 + n // hop for n in olen]], dtype=torch.int32, device=dev)
mel = torch.empty(B, 1 + n_out // hop, hp.num_mels, device=dev)
t = median_us(lambda: K.melspec(out, meta[0], olen, n_fft=n_fft, hop=hop, win=win,
                                window=plan["window"], twiddle=plan["twiddle"],
                                basis=plan["basis"], band_lo=plan["band_lo"],
                                band_hi=plan["band_hi"], ref_level_db=hp.ref_level_db,
                                amp_floor=A.AMP_FLOOR, out=mel), reps)
print(f"sat_melspec on its output (n_fft {n_fft}, hop {hop}, {mel.shape[1]} frames per "
      f"utterance): median {t[0]:.1f} us over {reps} calls (min {t[1]:.1f}, max {t[2]:.1f})",
      flush=True)
