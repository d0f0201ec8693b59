"""Time of the two score kernels at the lengths a test list is scored at.

sat_dtw_distortion (width 80) and sat_edit_distance (256 symbols) at Tp = Tt = 1000, for 32 pairs
(fewer workgroups than compute units) and 512 pairs (more): device events around the entry call
alone -- arguments, offsets and scratch are made once -- medians over the repetitions.  Beside
them the time of tests/score_ref.py's vectorised (anti-diagonal numpy) form on the first
``cpu_pairs`` of the same pairs on this machine's CPU, per pair, and the agreement of the two on
those pairs.

Numbers from one machine and one run of this script.

Usage: python tools/probes/score_time.py [reps] [cpu_pairs]
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

import score_ref as R  # noqa: E402
from sat_amd import _lib, kernels as K  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
cpu_pairs = int(sys.argv[2]) if len(sys.argv) > 2 else 8
dev = torch.device("cuda:0")
T, WIDTH, SYMBOLS = 1000, 80, 256


def median_us(fn, n):
    for _ in range(3):
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


lib = _lib.load()
stream = torch.cuda.current_stream().cuda_stream
err = torch.zeros(1, dtype=torch.int32, device=dev)
cells = T * T
for pairs in (32, 512):
    rng = np.random.default_rng(pairs)
    off = torch.arange(pairs + 1, dtype=torch.int64, device=dev) * T
    nbytes = int(lib.sat_score_scratch_bytes(pairs, T))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    p_host = rng.standard_normal((pairs * T, WIDTH)).astype(np.float32)
    t_host = (p_host + 0.5 * rng.standard_normal((pairs * T, WIDTH))).astype(np.float32)
    p, t = torch.from_numpy(p_host).to(dev), torch.from_numpy(t_host).to(dev)
    cost = torch.empty(pairs, dtype=torch.float64, device=dev)
    plen = torch.empty(pairs, dtype=torch.int32, device=dev)

    def dtw():
        _lib.call("sat_dtw_distortion", p.data_ptr(), pairs * T, off.data_ptr(), t.data_ptr(),
                  pairs * T, off.data_ptr(), WIDTH, pairs, T, cost.data_ptr(), plen.data_ptr(),
                  err.data_ptr(), scratch.data_ptr(), nbytes, stream)

    m = median_us(dtw, reps)
    print(f"sat_dtw_distortion, {pairs} pairs of {T} x {T} frames, width {WIDTH}: median "
          f"{m[0]:.0f} us over {reps} calls (min {m[1]:.0f}, max {m[2]:.0f}) = "
          f"{m[0] / pairs:.1f} us per pair, {pairs * cells / m[0] / 1e3:.2f} G cells/s", flush=True)

    a_host = rng.integers(0, SYMBOLS, pairs * T).astype(np.int32)
    b_host = np.where(rng.random(pairs * T) < 0.3, rng.integers(0, SYMBOLS, pairs * T),
                      a_host).astype(np.int32)
    a, b = torch.from_numpy(a_host).to(dev), torch.from_numpy(b_host).to(dev)
    dist = torch.empty(pairs, dtype=torch.int32, device=dev)

    def edit():
        _lib.call("sat_edit_distance", a.data_ptr(), pairs * T, off.data_ptr(), b.data_ptr(),
                  pairs * T, off.data_ptr(), pairs, T, dist.data_ptr(), err.data_ptr(),
                  scratch.data_ptr(), nbytes, stream)

    m = median_us(edit, reps)
    print(f"sat_edit_distance, {pairs} pairs of {T} x {T} symbols: median {m[0]:.0f} us over "
          f"{reps} calls (min {m[1]:.0f}, max {m[2]:.0f}) = {m[0] / pairs:.1f} us per pair, "
          f"{pairs * cells / m[0] / 1e3:.2f} G cells/s", flush=True)
    assert int(err.item()) == 0

    if pairs == 32:
        n = min(cpu_pairs, pairs)
        gc, gl, gd = cost.cpu().numpy(), plen.cpu().numpy(), dist.cpu().numpy()
        t0 = time.perf_counter()
        ref = [R.dtw(p_host[k * T:(k + 1) * T], t_host[k * T:(k + 1) * T]) for k in range(n)]
        t1 = time.perf_counter()
        red = [R.edit_distance(a_host[k * T:(k + 1) * T], b_host[k * T:(k + 1) * T])
               for k in range(n)]
        t2 = time.perf_counter()
        worst = max(abs(gc[k] - ref[k][0]) / ref[k][0] for k in range(n))
        same = sum(int(gl[k] == ref[k][1]) for k in range(n))
        print(f"score_ref.dtw (numpy, anti-diagonals, CPU), the first {n} of those pairs: "
              f"{(t1 - t0) / n * 1e3:.0f} ms per pair; kernel cost within {worst:.2e} relative, "
              f"path length equal on {same} of {n}", flush=True)
        print(f"score_ref.edit_distance (numpy, anti-diagonals, CPU), the first {n} of those "
              f"pairs: {(t2 - t1) / n * 1e3:.0f} ms per pair; kernel distance equal on "
              f"{sum(int(gd[k] == red[k]) for k in range(n))} of {n}", flush=True)
