"""Cost of apply_dropout_on_inference at the C5 shape (LJSpeech, batch 8, 500 decoder steps).

The decode is timed as bench.py's c5_free_running times it (wall clock around run(), after one
warm-up run that builds the plan, median of the repetitions), with the switch off and on:
* the one-launch decode (sat_decode_persistent without / with its dropout option), where the
  mask words are drawn inside the kernel;
* the per-step launch path with captured step graphs, where one sat_rng_fill_segments launch per
  decode fills the masks of all steps -- that launch is also timed alone with device events.

Numbers from one machine and one run of this script.

Usage: python tools/probes/infer_dropout_time.py [reps] [chars]
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import _sat_path  # noqa: E402

_sat_path.load()
import torch  # noqa: E402

from sat_amd import data, engine, hparams, kernels as K  # noqa: E402
from sat_amd.inference import FreeRunningDecoder  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
chars = int(sys.argv[2]) if len(sys.argv) > 2 else 200
B, steps = 8, 500


def decode_ms(dec, batch):
    dec.run(batch)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        dec.run(batch)
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


for persistent in (True, False):
    for drop in (False, True, False, True):
        hp = hparams.ljspeech_hparams()
        hp.set_hparam("apply_dropout_on_inference", drop)
        m = engine.Tacotron(hp, "cuda", seed=1234)
        b = data.synthetic_batch(hp, B, N=chars, T=1000, shape="max", seed=55)
        batch = {k: torch.tensor(v).cuda() for k, v in b.items()}
        dec = FreeRunningDecoder(m, max_iters=steps, min_iters=steps, check_every=25,
                                 graphs=True, persistent=persistent, seed=7)
        med, lo, hi = decode_ms(dec, batch)
        path = dec.last_path
        print(f"{path:10s} switch {'on ' if drop else 'off'}: decode median {med:.2f} ms "
              f"(min {lo:.2f}, max {hi:.2f}) over {reps} runs = {1e3 * med / steps:.2f} us per "
              f"decoder step", flush=True)
        if drop and not persistent:
            pl = next(iter(dec._plans.values()))
            ev = []
            for _ in range(50):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                K.rng_fill_segments(pl.drop_arena, pl.drop_segs, dec.seed)
                e1.record()
                ev.append((e0, e1))
            torch.cuda.synchronize()
            us = sorted(a.elapsed_time(c) * 1e3 for a, c in ev)
            print(f"           the fill launch alone ({pl.drop_arena.numel()} floats, one per "
                  f"decode): median {us[len(us) // 2]:.1f} us", flush=True)
        del dec, m
        torch.cuda.empty_cache()
