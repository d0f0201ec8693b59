"""What the plot figures of a synthesised batch cost, at B = 32 figures of 5 panels (two alignments
over N = 200 x T' = 500, one decoder self-attention head T' x T', the true and the predicted mel of
1000 frames x 80), boxes of Hp x Wp = 160 x 1000 pixels.

(a) the host route: the sources copied to the host, then tests/figure_ref.py (the NumPy statement
    of the kernel) composing the canvases;
(b) the device route: sat_image_minmax per source tensor + ONE sat_figure_render + the copy of the
    canvases to the host (plots.render_figures(...).cpu());
(c) sat_figure_render alone, device events, median of the launches, warm and after a 512 MB fill,
    beside the canvas bytes it writes as a fraction of HBM write bandwidth.

(a) and (b) are host wall-clock times closed by a synchronisation.  Numbers from one machine and
one run of this script.

Usage: python tools/probes/figure_time.py [reps]
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _sat_path  # noqa: E402

_sat_path.load()
import numpy as np  # noqa: E402
import torch  # noqa: E402

import figure_ref as R  # noqa: E402
from sat_amd import kernels as K, plots  # noqa: E402
from sat_amd.plots import Panel  # noqa: E402

HBM_PEAK = 8.0e12           # bytes/s, MI355X
B, N, Tp, H, T, M = 32, 200, 500, 2, 1000, 80
GEO = dict(Hp=160, Wp=1000, margin=16, cbar=24)
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
dev = torch.device("cuda:0")
g = torch.Generator(device="cpu").manual_seed(0)
rng = np.random.default_rng(0)
n_src = rng.integers(N // 2, N + 1, B)
steps = rng.integers(Tp // 2, Tp + 1, B)
n_src[0], steps[0] = N, Tp
al1 = torch.rand(Tp, B, N, generator=g).to(dev)             # [t][b][n]: rows n, stride B * N
al2 = torch.rand(Tp, B, N, generator=g).to(dev)
sa = torch.rand(B, H, Tp, Tp, generator=g).to(dev)          # [b][h][q][k]: rows k, stride T'
mel_true = torch.randn(B, T, M, generator=g).to(dev)        # [b][t][m]: rows m, stride M
mel_pred = torch.randn(B, T, M, generator=g).to(dev)
tables = plots.default_tables()


def figures(a1, a2, s, mt, mp):
    return [[Panel(a1, b * N, int(n_src[b]), int(steps[b]), B * N, plots.JET),
             Panel(a2, b * N, int(n_src[b]), int(steps[b]), B * N, plots.JET),
             Panel(s, b * H * Tp * Tp, int(steps[b]), int(steps[b]), Tp, plots.JET),
             Panel(mt, b * T * M, M, 2 * int(steps[b]), M, plots.MAGMA),
             Panel(mp, b * T * M, M, 2 * int(steps[b]), M, plots.MAGMA)] for b in range(B)]


dev_figs = figures(al1, al2, sa, mel_true, mel_pred)


def route_host():
    return R.render(figures(*(x.cpu().numpy() for x in (al1, al2, sa, mel_true, mel_pred))),
                    tables, GEO["Hp"], GEO["Wp"], GEO["margin"], GEO["cbar"])


def route_device():
    return plots.render_figures(dev_figs, tables, **GEO).cpu()


def wall_ms(fn, n, warm):
    for _ in range(warm):
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


want = route_host()
got = route_device().numpy()
assert (got == want).all()
src_mb = sum(x.numel() * 4 for x in (al1, al2, sa, mel_true, mel_pred)) / 1e6
print(f"B={B} figures x 5 panels, boxes {GEO['Hp']} x {GEO['Wp']}: canvases {want.shape} = "
      f"{want.nbytes / 1e6:.1f} MB, sources {src_mb:.1f} MB; device and host canvases equal",
      flush=True)
for name, fn, n, warm in (("(a) sources to the host + figure_ref", route_host, 3, 0),
                          ("(b) minmax + sat_figure_render + canvases to the host", route_device,
                           max(reps // 5, 3), 2)):
    t = wall_ms(fn, n, warm)
    print(f"{name}: median {t[0]:.1f} ms over {n} batches (min {t[1]:.1f}, max {t[2]:.1f})",
          flush=True)

# the kernel alone: descriptors and min / max pairs made once
flat = [p for fig in dev_figs for p in fig]
mm = torch.empty(len(flat), 2, device=dev)
bad = torch.empty(len(flat), dtype=torch.int32, device=dev)
for i, p in enumerate(flat):
    K.image_minmax(p.src, torch.tensor([p.base], dtype=torch.int64, device=dev),
                   torch.tensor([p.rows], dtype=torch.int32, device=dev),
                   torch.tensor([p.cols], dtype=torch.int32, device=dev), p.col_stride, p.rows,
                   p.cols, mm[i:i + 1], bad[i:i + 1], [p.rows], [p.cols])
host = K.figure_panels([(p.src, p.base, p.rows, p.cols, p.col_stride, p.table, mm[i])
                        for i, p in enumerate(flat)])
table_dev = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(dev)
lut = torch.from_numpy(tables).to(dev)
canvas = torch.empty(want.shape, dtype=torch.uint8, device=dev)
scrub = torch.empty(512 << 20, dtype=torch.uint8, device=dev)


def kernel():
    K.figure_render(host, table_dev, lut, canvas, GEO["Hp"], GEO["Wp"], GEO["margin"], GEO["cbar"])


kernel()
torch.cuda.synchronize()
assert (canvas.cpu().numpy() == want).all()
nbytes = canvas.numel()
for name, before in (("warm", None), ("after a 512 MB fill", lambda: scrub.fill_(1))):
    t = event_us(kernel, reps, before)
    print(f"sat_figure_render alone, {name}: median {t[0]:.1f} us over {reps} launches (min "
          f"{t[1]:.1f}, max {t[2]:.1f}); {nbytes / 1e6:.1f} MB written = "
          f"{nbytes / (t[0] * 1e-6) / 1e9:.0f} GB/s = "
          f"{100 * nbytes / (t[0] * 1e-6) / HBM_PEAK:.1f} % of {HBM_PEAK / 1e12:.0f} TB/s",
          flush=True)
