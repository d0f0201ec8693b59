"""The free-running decode of a VQ-code model (num_mels = num_codes, r = 1, multi-speaker as
the corpus is) at the preset's length: batch 8, 128 characters, 450 decoder steps (max_iters),
num_codes 256 and 1025, on the per-step launch path -- what these models ran on before the history
kernels -- and in one launch (sat_decode_persistent with its history and speaker options + the
projection of the z history).

Timed with device events around run() (encoder, memories, weight packing, the decode and the
output copies: everything a caller waits for), after one warm-up run that builds the plan; median
of the repetitions.  The projection's share is the device-event time of
FreeRunningDecoder._project_history alone on the same plan.  The whole list is measured twice in
one session so that the run-to-run spread shows.

Numbers from one machine and one run of this script.

Usage: python tools/probes/decode_codes_time.py [reps] [chars]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import _sat_path  # noqa: E402

_sat_path.load()
import torch  # noqa: E402

from sat_amd import data, engine, hparams  # noqa: E402
from sat_amd.inference import FreeRunningDecoder  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
chars = int(sys.argv[2]) if len(sys.argv) > 2 else 128
B, steps = 8, 450


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def median_ms(fn):
    fn()
    torch.cuda.synchronize()
    ts = sorted(event_ms(fn) for _ in range(reps))
    return ts[len(ts) // 2], ts[0], ts[-1]


# (label, persistent, graphs)
CASES = [("launches eager", False, False), ("launches graphs", False, True),
         ("one launch", True, False)]

for rnd in (1, 2):
    for C in (256, 1025):
        hp = hparams.codes_hparams(C, use_speaker_embedding=True)
        assert hp.max_iters == steps
        m = engine.Tacotron(hp, "cuda", seed=1234)
        b = data.synthetic_batch(hp, B, N=chars, T=20, shape="max", seed=55)
        batch = {k: torch.tensor(v).cuda() for k, v in b.items()}
        for label, persistent, graphs in CASES:
            dec = FreeRunningDecoder(m, max_iters=steps, min_iters=steps, check_every=25,
                                     graphs=graphs, persistent=persistent)
            med, lo, hi = median_ms(lambda: dec.run(batch))
            assert dec.last_path == ("persistent" if persistent else "launches")
            line = (f"round {rnd} C={C:4d} {label:15s}: run() median {med:8.2f} ms (min {lo:.2f}, "
                    f"max {hi:.2f}) over {reps} runs = {1e3 * med / steps:7.2f} us per decoder step")
            if persistent:
                pl = dec._plans[(B, chars, steps)]
                pm, plo, phi = median_ms(lambda: dec._project_history(pl, steps))
                line += (f"; projection {1e3 * pm:.1f} us (min {1e3 * plo:.1f}, max "
                         f"{1e3 * phi:.1f}) = {100 * pm / med:.2f} % of run()")
            print(line, flush=True)
            del dec
        del m
        torch.cuda.empty_cache()
