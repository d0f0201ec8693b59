"""``bench.py`` plain run with ``--dump-outputs``: the result line carries the headline fields
only (nothing of ``--full``), ``--steps`` sets the number of timed steps, and the last timed
step's outputs land as float32 ``<name>.npy`` files (large arrays as a fixed sample)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_plain_run_dumps_last_step_outputs(cuda, tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                        "--steps", "3", "--warmup", "1", "--batch", "2", "--chars", "13",
                        "--frames", "16", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0
    assert d["unit"] == "frames/s" and d["higher_is_better"] is True and d["dtype"] == "fp32"
    assert d["value"] == pytest.approx(2 * 16 * 1e3 / d["ms_per_step"], rel=1e-2)
    for k in ("roofline", "roofline_bptt", "cpu_baseline", "cpu_baseline_c2", "c4_vctk_training",
              "c5_free_running", "drop_in_ragged_ljs", "fallback_b64_per_step_path"):
        assert k not in d, k
    arrays = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
    assert {"loss", "mel", "stop", "alignment1", "alignment2", "params", "grads"} <= set(arrays)
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    assert arrays["mel"].shape == (2, 16, 80) and arrays["stop"].shape[:2] == (2, 8)
    # 6,227,928 parameters: written as the fixed 2^20-element sample
    assert arrays["params"].shape == arrays["grads"].shape == (1 << 20,)
    assert np.abs(arrays["grads"]).max() > 0
    # the dump is of the last timed step
    assert round(float(arrays["loss"][0]), 5) == pytest.approx(d["loss_last"], abs=1.1e-5)
