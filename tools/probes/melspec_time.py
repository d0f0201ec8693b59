"""Time of the audio front end on an LJSpeech-sized batch: B=32 utterances of 143 000 samples
(about 6.5 s, 521 frames each).

  * sat_melspec alone (device events around the launch, tables and waveforms already resident),
    its achieved fraction of HBM bandwidth counted as waveform read + num_mels floats per frame
    written, and Audio.melspectrogram_batch as a caller sees it (upload + launch, host clock
    around a device synchronise);
  * the float32 CPU pipeline (torch.stft, matmul, log10) on the same batch with 16 threads.

Numbers from one machine and one run of this script; medians over the repetitions.

Usage: python tools/probes/melspec_time.py [reps] [cpu_reps]
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
B, SAMPLES = 32, 143000
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
cpu_reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5

hp = H.ljspeech_hparams()
dev = torch.device("cuda:0")
a = A.Audio(hp, device=dev)
n_fft, hop, win = a._stft_parameters()
rng = np.random.default_rng(0)
wavs = [(0.1 * rng.standard_normal(SAMPLES)).astype(np.float32) for _ in range(B)]
frames = 1 + SAMPLES // hop

# as a caller sees it: upload + launch
for _ in range(3):
    mel, fr = a.melspectrogram_batch(wavs)
torch.cuda.synchronize()
ts = []
for _ in range(20):
    t0 = time.perf_counter()
    mel, fr = a.melspectrogram_batch(wavs)
    torch.cuda.synchronize()
    ts.append(time.perf_counter() - t0)
call_ms = 1e3 * sorted(ts)[len(ts) // 2]

# the launch alone
plan = a._plan(dev)
wav = torch.from_numpy(np.stack(wavs)).to(dev)
lengths = [SAMPLES] * B
dl = torch.tensor(lengths, dtype=torch.int32, device=dev)
out = torch.empty(B, frames, hp.num_mels, device=dev)


def launch():
    K.melspec(wav, dl, lengths, n_fft=n_fft, hop=hop, win=win, window=plan["window"],
              twiddle=plan["twiddle"], basis=plan["basis"], band_lo=plan["band_lo"],
              band_hi=plan["band_hi"], ref_level_db=hp.ref_level_db, amp_floor=A.AMP_FLOOR,
              out=out)


for _ in range(10):
    launch()
torch.cuda.synchronize()
ev = []
for _ in range(reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    launch()
    e1.record()
    ev.append((e0, e1))
torch.cuda.synchronize()
us = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev)
med = us[len(us) // 2]
assert torch.equal(out, mel)
nbytes = 4 * (B * SAMPLES + B * frames * hp.num_mels)
print(f"sat_melspec B={B} x {SAMPLES} samples ({frames} frames, n_fft {n_fft}): median "
      f"{med:.1f} us over {reps} launches (min {us[0]:.1f}, max {us[-1]:.1f}); "
      f"{nbytes / 1e6:.2f} MB moved = {nbytes / med / 1e6:.3f} TB/s = "
      f"{100 * nbytes / (med * 1e-6) / HBM_PEAK:.2f} % of {HBM_PEAK / 1e12:.0f} TB/s", flush=True)
print(f"Audio.melspectrogram_batch (upload + launch): median {call_ms:.2f} ms over 20 calls",
      flush=True)

# float32 CPU pipeline, 16 threads
torch.set_num_threads(16)
basis = torch.from_numpy(a._mel_basis)
w = torch.hann_window(win, periodic=True)
cw = torch.from_numpy(np.stack(wavs))


def cpu():
    X = torch.stft(cw, n_fft, hop_length=hop, win_length=win, window=w, center=True,
                   pad_mode="reflect", return_complex=True)
    S = torch.matmul(basis, X.abs())
    return (20.0 * torch.log10(torch.clamp(S, min=A.AMP_FLOOR)) - hp.ref_level_db).transpose(1, 2)


ref = cpu()
ts = []
for _ in range(cpu_reps):
    t0 = time.perf_counter()
    cpu()
    ts.append(time.perf_counter() - t0)
cpu_ms = 1e3 * sorted(ts)[len(ts) // 2]
diff = float((mel.cpu() - ref).abs().max())
print(f"CPU float32 torch.stft pipeline, 16 threads: median {cpu_ms:.1f} ms over {cpu_reps} runs "
      f"({cpu_ms * 1e3 / med:.0f} x the launch); largest |GPU - CPU| {diff:.2e} dB", flush=True)
