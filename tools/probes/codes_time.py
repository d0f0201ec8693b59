"""What a batch of VQ-code targets costs to build, at B=32, T=1000, C=256 (the benchmark's shape).

(a) the route a code batch would take without the device kernel: every utterance a dense float32
    one-hot [T_b, C] on the host (as the reference's records hold it), padded into [B, T, C] with
    the masks as datasets.padded_batch pads mel targets, uploaded through the model's pinned
    stager;
(b) the index route: the int32 indices and int64 offsets through the same stager, then ONE
    sat_codes_batch launch that writes codes, done, both masks and target_length.

Both are host wall-clock times from the utterance list to device tensors that are complete
(a synchronisation closes each repetition), because (a) is mostly host work.  The kernel alone is
timed with device events, warm (its outputs just written, so partly resident in the caches) and
after a 512 MB fill, beside the bytes it writes as a fraction of HBM bandwidth.

Numbers from one machine and one run of this script; medians over the repetitions.

Usage: python tools/probes/codes_time.py [reps]
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import _sat_path  # noqa: E402

_sat_path.load()
import numpy as np  # noqa: E402
import torch  # noqa: E402

from sat_amd import kernels as K  # noqa: E402
from sat_amd.models import _PinnedStager  # noqa: E402

HBM_PEAK = 8.0e12           # bytes/s, MI355X
B, T, C = 32, 1000, 256
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
dev = torch.device("cuda:0")
rng = np.random.default_rng(0)
lengths = rng.integers(T // 2, T + 1, B)
lengths[0] = T
seqs = [rng.integers(0, C, n).astype(np.int32) for n in lengths]
dense = []                                      # what the reference's records decode to
for s in seqs:
    d = np.zeros((len(s), C), np.float32)
    d[np.arange(len(s)), s] = 1.0
    dense.append(d)
stager = _PinnedStager()
f32, i64 = torch.float32, torch.int64


def pad(arrays, value):
    out = np.full((B, T) + arrays[0].shape[1:], value, np.float32)
    for i, a in enumerate(arrays):
        out[i, :a.shape[0]] = a
    return out


def route_host():
    ones = [np.ones(len(s), np.float32) for s in seqs]
    done = [np.concatenate([np.zeros(len(s) - 1, np.float32), np.ones(1, np.float32)])
            for s in seqs]
    arrays = {"mel": pad(dense, 0.0), "mel_mask": pad(ones, 0.0), "done": pad(done, 1.0),
              "done_mask": pad(ones, 0.0), "target_length": lengths.astype(np.int64)}
    return stager.upload(arrays, dev, {k: i64 if k == "target_length" else f32 for k in arrays})


def route_index():
    offsets = np.zeros(B + 1, np.int64)
    np.cumsum(lengths, out=offsets[1:])
    up = stager.upload({"code_index": np.concatenate(seqs), "offsets": offsets}, dev,
                       {"code_index": torch.int32, "offsets": i64})
    return K.codes_batch(up["code_index"], up["offsets"], offsets, C=C, T_pad=T, check=False)


def wall_ms(fn, n):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]


def event_us(fn, n, before=None):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    ev = []
    for _ in range(n):
        if before is not None:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        ev.append((e0, e1))
    torch.cuda.synchronize()
    us = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    return us[len(us) // 2], us[0], us[-1]


a = route_host()
b = route_index()
torch.cuda.synchronize()
assert torch.equal(a["mel"], b["codes"]) and torch.equal(a["mel_mask"], b["code_loss_mask"])
print(f"B={B} T={T} C={C}: {int(lengths.sum())} code frames; dense batch "
      f"{B * T * C * 4 / 1e6:.1f} MB, indices + offsets "
      f"{(int(lengths.sum()) * 4 + (B + 1) * 8) / 1e3:.1f} KB", flush=True)
for name, fn in (("(a) host one-hot, pad, upload", route_host),
                 ("(b) index upload + sat_codes_batch", route_index)):
    t = wall_ms(fn, reps)
    print(f"{name}: median {t[0]:.3f} ms over {reps} batches (min {t[1]:.3f}, max {t[2]:.3f})",
          flush=True)

offsets = np.zeros(B + 1, np.int64)
np.cumsum(lengths, out=offsets[1:])
idx, off = torch.tensor(np.concatenate(seqs), device=dev), torch.tensor(offsets, device=dev)
outs = {k: v for k, v in route_index().items() if k != "err"}
nbytes = sum(v.numel() * v.element_size() for v in outs.values())
scrub = torch.empty(512 << 20, dtype=torch.uint8, device=dev)


def kernel():
    K.codes_batch(idx, off, offsets, C=C, T_pad=T, check=False, **outs)


for name, before in (("warm", None), ("after a 512 MB fill", lambda: scrub.fill_(1))):
    t = event_us(kernel, reps, before)
    print(f"sat_codes_batch alone, {name}: median {t[0]:.1f} us over {reps} launches (min "
          f"{t[1]:.1f}, max {t[2]:.1f}); {nbytes / 1e6:.1f} MB written = "
          f"{100 * nbytes / (t[0] * 1e-6) / HBM_PEAK:.1f} % of {HBM_PEAK / 1e12:.0f} TB/s",
          flush=True)
