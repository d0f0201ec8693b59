"""Time of the VCTK front end on one batch: B=32 utterances of 192 000 samples at 48 kHz (4 s:
0.5 s of floor noise, 3 s of a modulated tone, 0.5 s of floor noise).

  * sat_trim_bounds alone (device events around the entry's two launches, waveforms resident),
    and its achieved fraction of HBM bandwidth counted as one read of the waveform;
  * sat_melspec over the trimmed segments (offsets) alone;
  * trim_batch + melspectrogram_batch(wav, bounds=...) as a caller sees it (upload, trim launch,
    read-back of the bounds, mel launch; host clock around a device synchronise).

Numbers from one machine and one run of this script; medians over the repetitions.

Usage: python tools/probes/trim_time.py [reps]
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import _sat_path  # noqa: E402

_sat_path.load()
import numpy as np  # noqa: E402
import torch  # noqa: E402

from sat_amd import audio as A, hparams as H, kernels as K  # noqa: E402

HBM_PEAK = 8.0e12           # bytes/s, MI355X
B, SAMPLES, SR = 32, 192000, 48000
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200

hp = H.vctk_hparams()
dev = torch.device("cuda:0")
a = A.Audio(hp, device=dev)
n_fft, hop, win = a._stft_parameters()
t = np.arange(SAMPLES) / SR
wavs = []
for b in range(B):
    y = 1e-3 * np.random.default_rng(b).standard_normal(SAMPLES)
    y[SR // 2:SAMPLES - SR // 2] += (0.5 * np.sin(2 * np.pi * 220 * t)
                                     * (0.8 + 0.2 * np.sin(2 * np.pi * 3 * t)))[SR // 2:-SR // 2]
    wavs.append(y.astype(np.float32))

# as a caller sees it
for _ in range(3):
    wav, bounds = a.trim_batch(wavs)
    mel, fr = a.melspectrogram_batch(wav, bounds=bounds)
torch.cuda.synchronize()
ts = []
for _ in range(20):
    t0 = time.perf_counter()
    wav, bounds = a.trim_batch(wavs)
    mel, fr = a.melspectrogram_batch(wav, bounds=bounds)
    torch.cuda.synchronize()
    ts.append(time.perf_counter() - t0)
call_ms = 1e3 * sorted(ts)[len(ts) // 2]
bh = bounds.cpu().numpy()

# the launches alone
lengths = [SAMPLES] * B
dl = torch.tensor(lengths, dtype=torch.int32, device=dev)
fl, th = int(hp.trim_frame_length), int(hp.trim_hop_length)
ms = torch.empty(B, 1 + SAMPLES // th, device=dev)
out_b = torch.empty(B, 2, dtype=torch.int32, device=dev)
plan = a._plan(dev)
seg = [int(e - s) for s, e in bh]
off = [int(s) for s, _ in bh]
dseg = torch.tensor(seg, dtype=torch.int32, device=dev)
doff = torch.tensor(off, dtype=torch.int32, device=dev)
out = torch.empty_like(mel)


def trim():
    K.trim_bounds(wav, dl, lengths, frame_length=fl, hop=th, top_db=hp.trim_top_db,
                  pad_samples=0, bounds=out_b, frame_ms=ms)


def melspec():
    K.melspec(wav, dseg, seg, n_fft=n_fft, hop=hop, win=win, window=plan["window"],
              twiddle=plan["twiddle"], basis=plan["basis"], band_lo=plan["band_lo"],
              band_hi=plan["band_hi"], ref_level_db=hp.ref_level_db, amp_floor=A.AMP_FLOOR,
              out=out, offsets=doff, offsets_host=off)


def timed(fn):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    ev = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        ev.append((e0, e1))
    torch.cuda.synchronize()
    us = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev)
    return us[len(us) // 2], us[0], us[-1]


tm, tlo, thi = timed(trim)
mm, mlo, mhi = timed(melspec)
assert torch.equal(out_b, bounds) and torch.equal(out, mel)
nbytes = 4 * B * SAMPLES
print(f"bounds of utterance 0: {tuple(bh[0])} of {SAMPLES} samples", flush=True)
print(f"sat_trim_bounds B={B} x {SAMPLES} samples (frames of {fl} every {th}): median {tm:.1f} us "
      f"over {reps} calls (min {tlo:.1f}, max {thi:.1f}); one read of the waveform "
      f"{nbytes / 1e6:.2f} MB = {nbytes / tm / 1e6:.3f} TB/s = "
      f"{100 * nbytes / (tm * 1e-6) / HBM_PEAK:.2f} % of {HBM_PEAK / 1e12:.0f} TB/s", flush=True)
print(f"sat_melspec over the trimmed segments (n_fft {n_fft}, {int(fr.max())} frames at most): "
      f"median {mm:.1f} us over {reps} launches (min {mlo:.1f}, max {mhi:.1f})", flush=True)
print(f"trim_batch + melspectrogram_batch(bounds) (upload, trim, read-back, mel): median "
      f"{call_ms:.2f} ms over 20 calls", flush=True)
