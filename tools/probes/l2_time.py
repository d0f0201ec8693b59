"""Time of the L2 regulariser's kernel at the LJSpeech config's real arena size.

sat_l2_regularize alone (its two launches: the pass over the regularised ranges of the parameter
and gradient arenas, and the one-workgroup finish), device events around the entry call, beside
the bytes it must move -- the regularised parameters read once, their gradients read and written
once -- as a fraction of HBM bandwidth; the loss-only form (parameters read once); and the same
call after a 512 MB fill, so that neither arena is resident in a cache.

Numbers from one machine and one run of this script; medians over the repetitions.

Usage: python tools/probes/l2_time.py [reps]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import _sat_path  # noqa: E402

_sat_path.load()
import torch  # noqa: E402

from sat_amd import hparams as H, kernels as K, params as PR  # noqa: E402

HBM_PEAK = 8.0e12           # bytes/s, MI355X
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
dev = torch.device("cuda:0")


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


hp = H.ljspeech_hparams()
lay = PR.Layout(PR.param_specs(hp))
params = torch.from_numpy(lay.pack(PR.init_params(hp, seed=1234))).to(dev)
grads = torch.zeros_like(params)
segs = PR.l2_segments(lay.specs, lay)
table = K.l2_table(segs, lay.total, dev)
n_sel = sum(n for _, n in segs)
out = torch.zeros(1, device=dev)
print(f"arena {lay.total} floats ({lay.total * 4 / 1e6:.1f} MB), regularised "
      f"{n_sel} floats in {len(segs)} ranges (largest {max(n for _, n in segs)})", flush=True)
for what, gr, nbytes in (("loss + gradient", grads, 12 * n_sel), ("loss only", None, 4 * n_sel)):
    t = median_us(lambda: K.l2_regularize(params, gr, table, 1e-7, 1e-7, out), reps)
    print(f"sat_l2_regularize, {what}: median {t[0]:.1f} us over {reps} calls (min {t[1]:.1f}, "
          f"max {t[2]:.1f}); {nbytes / 1e6:.1f} MB by design = "
          f"{100 * nbytes / (t[0] * 1e-6) / HBM_PEAK:.1f} % of {HBM_PEAK / 1e12:.0f} TB/s",
          flush=True)
# the same pass with the arenas resident in no cache: a 512 MB fill between calls
big = torch.empty(128 << 20, device=dev)
cold = []
for _ in range(20):
    big.fill_(1.0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    K.l2_regularize(params, grads, table, 1e-7, 1e-7, out)
    e1.record()
    cold.append((e0, e1))
torch.cuda.synchronize()
us = sorted(a.elapsed_time(b) * 1e3 for a, b in cold)
print(f"sat_l2_regularize, loss + gradient, after a 512 MB fill (cold caches): median "
      f"{us[len(us) // 2]:.1f} us = {100 * 12 * n_sel / (us[len(us) // 2] * 1e-6) / HBM_PEAK:.1f} % "
      f"of peak", flush=True)
