"""The one-launch decode of the multi-speaker (VCTK) model at the C5 shape (batch 8, 200
characters, 500 decoder steps) beside what that model decoded with before and beside the
single-speaker kernel.

The decode is timed as bench.py's c5_free_running times it (wall clock around run(), after one
warm-up run that builds the plan, median of the repetitions):
* (a) VCTK on the per-step launch path -- eager, which is what model_fn PREDICT / predict() /
  synthesize ran for this model before the multi-speaker kernels, and with captured step graphs
  (graphs=True, check_every=25), the faster form of that path;
* (b) VCTK in one launch (sat_decode_persistent with its speaker option);
* (c) LJSpeech in one launch (sat_decode_persistent), the floor: (b) - (c) is the cost of the
  extra dense phase and its hand-off;
* (d) (a) and (b) with apply_dropout_on_inference on (the speaker and dropout options).
The whole list is measured twice in one session so that the run-to-run spread shows.

Numbers from one machine and one run of this script.

Usage: python tools/probes/decode_spk_time.py [reps] [chars]
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import _sat_path  # noqa: E402

_sat_path.load()
import torch  # noqa: E402

from sat_amd import data, engine, hparams  # noqa: E402
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


# (label, preset, switch, persistent, graphs)
CASES = [("(a) vctk launches eager", "vctk", False, False, False),
         ("(a) vctk launches graphs", "vctk", False, False, True),
         ("(b) vctk one launch", "vctk", False, True, False),
         ("(c) ljspeech one launch", "ljspeech", False, True, False),
         ("(d) vctk launches eager, switch on", "vctk", True, False, False),
         ("(d) vctk launches graphs, switch on", "vctk", True, False, True),
         ("(d) vctk one launch, switch on", "vctk", True, True, False)]

for rnd in (1, 2):
    for label, preset, drop, persistent, graphs in CASES:
        hp = getattr(hparams, f"{preset}_hparams")()
        hp.set_hparam("apply_dropout_on_inference", drop)
        m = engine.Tacotron(hp, "cuda", seed=1234)
        b = data.synthetic_batch(hp, B, N=chars, T=1000, shape="max", seed=55)
        batch = {k: torch.tensor(v).cuda() for k, v in b.items()}
        dec = FreeRunningDecoder(m, max_iters=steps, min_iters=steps, check_every=25,
                                 graphs=graphs, persistent=persistent, seed=7)
        med, lo, hi = decode_ms(dec, batch)
        assert dec.last_path == ("persistent" if persistent else "launches")
        print(f"round {rnd} {label:36s}: decode median {med:8.2f} ms (min {lo:.2f}, max {hi:.2f}) "
              f"over {reps} runs = {1e3 * med / steps:7.2f} us per decoder step", flush=True)
        del dec, m
        torch.cuda.empty_cache()
