"""``sat_amd.score`` over files: ``Scorer`` and the CLI on a directory of ``.preds.txt`` /
``.truth.txt`` files and on prediction records, and the opt-in ``scores`` switch of
``predict_code.write_code_predictions``.  The truths are the sequences of tests/golden/codes, the
predictions hand-perturbed copies; every expected number comes from tests/score_ref.py and plain
arithmetic on its integers."""
import csv
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import codes_ref as CR
import score_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "codes")
C = 16


def _perturbed():
    """[(key, prediction, truth)] in record order: a substitution, a deletion, an insertion,
    two edits, an exact copy, a truncation, ... by hand, cycling over the corpus."""
    out = []
    for k, (key, _, _, truth) in enumerate(CR.read_corpus(GOLDEN)):
        t = [int(c) for c in truth]
        p = list(t)
        kind = k % 5
        if kind == 0:
            p[1] = (p[1] + 1) % C                     # one substitution
        elif kind == 1:
            del p[2]                                  # one deletion
        elif kind == 2:
            p.insert(3, (p[3] + 5) % C)               # one insertion
        elif kind == 3:
            p = p[:len(p) // 2]                       # the second half is missing
        out.append((key, np.array(p, np.int64), np.array(t, np.int64)))
    assert len(out) >= 5
    return out


def _expected_codes(rows):
    d = [R.edit_distance(p, t) for _, p, t in rows]
    tt, tp = [len(t) for _, _, t in rows], [len(p) for _, p, _ in rows]
    summary = {"code_error_rate": sum(d) / sum(tt),
               "mean_error_rate": sum(x / y for x, y in zip(d, tt)) / len(d),
               "mean_length_ratio": sum(x / y for x, y in zip(tp, tt)) / len(d)}
    return d, tt, tp, summary


def _check_code_files(out_dir, rows):
    d, tt, tp, summary = _expected_codes(rows)
    with open(os.path.join(out_dir, "scores.csv"), newline="") as f:
        got = list(csv.DictReader(f))
    assert [g["key"] for g in got] == [key for key, _, _ in rows]            # order kept
    assert [int(g["distance"]) for g in got] == d
    assert [int(g["truth_length"]) for g in got] == tt
    assert [int(g["predicted_length"]) for g in got] == tp
    for g, x, y, z in zip(got, d, tt, tp):
        assert abs(float(g["error_rate"]) - x / y) <= 1e-12
        assert abs(float(g["length_ratio"]) - z / y) <= 1e-12
    with open(os.path.join(out_dir, "scores.json")) as f:
        doc = json.load(f)
    assert doc["kind"] == "codes" and doc["utterances"] == len(rows)
    assert set(doc["summary"]) == set(summary)
    for name, want in summary.items():
        assert abs(doc["summary"][name] - want) <= 1e-12, name
    assert any(x > 0 for x in d) and any(x == 0 for x in d)


def _line(seq):
    return " ".join(str(int(c)) for c in seq) + "\n"


def test_scorer_and_cli_over_code_files(cuda, tmp_path):
    from sat_amd import score
    rows = sorted(_perturbed())                    # the CLI reads the keys in sorted order
    d = tmp_path / "pred"
    d.mkdir()
    for key, p, t in rows:
        (d / f"{key}.preds.txt").write_text(_line(p))
        (d / f"{key}.truth.txt").write_text(_line(t))
    (d / "stray.preds.txt").write_text("1 2 3\n")   # no truth beside it: not a pair
    s = score.Scorer("codes")
    s.add([r[0] for r in rows[:3]], [r[1] for r in rows[:3]], [r[2] for r in rows[:3]])
    s.add([r[0] for r in rows[3:]], [r[1] for r in rows[3:]], [r[2] for r in rows[3:]])
    s.write(str(tmp_path / "a"))
    _check_code_files(tmp_path / "a", rows)
    assert score.main(["--predictions-dir", str(d), "--kind", "codes", "--output-dir",
                       str(tmp_path / "b")]) == 0
    _check_code_files(tmp_path / "b", rows)
    for name in ("scores.csv", "scores.json"):
        assert (tmp_path / "a" / name).read_bytes() == (tmp_path / "b" / name).read_bytes()
    # in a fresh process, into the predictions directory itself (the default)
    r = subprocess.run([sys.executable, "-m", "sat_amd.score", "--predictions-dir", str(d)],
                       cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert (d / "scores.json").read_bytes() == (tmp_path / "a" / "scores.json").read_bytes()
    assert json.loads(r.stdout.strip().splitlines()[-1])["utterances"] == len(rows)


def test_scorer_and_cli_over_prediction_records(cuda, tmp_path):
    """kind = mel: every <key>.tfrecord holds the prediction and the ground truth."""
    from sat_amd import score, tfrecord
    rng = np.random.default_rng(11)
    d = tmp_path / "rec"
    d.mkdir()
    rows = []
    for k, (n, m) in enumerate([(17, 23), (40, 31), (9, 9), (70, 66)]):
        amp = np.exp(rng.standard_normal((n + m, 1)))
        x = (amp * rng.standard_normal((n + m, 20))).astype(np.float32)
        p, t = x[:n], x[n:]
        key = f"utt{k:02d}"
        tfrecord.write_prediction_result(k, key, p, t, "text", np.arange(5), str(d / f"{key}.tfrecord"))
        rows.append((key, p, t, R.dtw(p, t)))
    assert score.main(["--predictions-dir", str(d), "--kind", "mel", "--output-dir",
                       str(tmp_path / "o")]) == 0
    s = score.Scorer("mel")
    s.add([r[0] for r in rows], [r[1] for r in rows], [torch.tensor(r[2], device=cuda) for r in rows])
    s.write(str(tmp_path / "s"))
    for out in ("o", "s"):
        with open(tmp_path / out / "scores.csv", newline="") as f:
            got = list(csv.DictReader(f))
        assert [g["key"] for g in got] == [r[0] for r in rows]
        bound = 24 * 2.0 ** -23
        for g, (_, p, t, (cost, cells, margin, mean)) in zip(got, rows):
            assert margin > 1e-3 * mean
            assert int(g["path_length"]) == cells
            assert (int(g["predicted_length"]), int(g["truth_length"])) == (len(p), len(t))
            assert abs(float(g["cost"]) - cost) <= bound * cost
            assert abs(float(g["distortion"]) - float(g["cost"]) / cells) <= 1e-12
            assert abs(float(g["length_ratio"]) - len(p) / len(t)) <= 1e-12
        with open(tmp_path / out / "scores.json") as f:
            doc = json.load(f)
        assert doc["kind"] == "mel" and doc["utterances"] == len(rows)
        costs = [float(g["cost"]) for g in got]
        cells = [r[3][1] for r in rows]
        want = {"mean_distortion": sum(c / k for c, k in zip(costs, cells)) / len(rows),
                "pooled_distortion": sum(costs) / sum(cells),
                "mean_length_ratio": sum(len(r[1]) / len(r[2]) for r in rows) / len(rows)}
        assert set(doc["summary"]) == set(want)
        for name, v in want.items():
            assert abs(doc["summary"][name] - v) <= 1e-12 * max(1.0, abs(v)), name
    assert (tmp_path / "o" / "scores.csv").read_bytes() == (tmp_path / "s" / "scores.csv").read_bytes()


def _pairs(rows, dev, batch=3):
    """Hand-made (predictions, features) pairs as model.predict yields them beside its batches:
    the raw outputs are the one-hot of the predicted indices, padded; the stop logit fires at
    each utterance's last frame."""
    out = []
    for b0 in range(0, len(rows), batch):
        part = rows[b0:b0 + batch]
        B, T = len(part), max(len(p) for _, p, _ in part) + 2
        raw = np.zeros((B, T, C), np.float32)
        stop = np.full((B, T), -1.0, np.float32)
        for b, (_, p, _) in enumerate(part):
            raw[b, np.arange(len(p)), p] = 1.0
            raw[b, len(p):, 0] = 1.0
            stop[b, len(p) - 1] = 1.0
        truth = [t.astype(np.int32) for _, _, t in part]
        offsets = np.zeros(B + 1, np.int64)
        np.cumsum([len(t) for t in truth], out=offsets[1:])
        p = {"mel": torch.tensor(raw, device=dev), "stop_token": torch.tensor(stop),
             "key": np.array([k.encode() for k, _, _ in part]), "id": np.arange(b0, b0 + B),
             "text": np.array([b"text"] * B, dtype=object)}
        features = types.SimpleNamespace(code_index=np.concatenate(truth), offsets=offsets,
                                         source=np.zeros((B, 4), np.int64),
                                         source_length=np.full(B, 4, np.int64))
        out.append((p, features))
    return out


def test_write_code_predictions_scores_switch(cuda, tmp_path):
    from sat_amd import predict_code
    rows = _perturbed()
    hp = types.SimpleNamespace(num_mels=C, outputs_per_step=1)
    on, off = tmp_path / "on", tmp_path / "off"
    keys = predict_code.write_code_predictions(_pairs(rows, cuda), str(on), hp, min_iters=0,
                                               scores=True)
    assert keys == [r[0] for r in rows]
    _check_code_files(on, rows)
    assert predict_code.write_code_predictions(_pairs(rows, cuda), str(off), hp,
                                               min_iters=0) == keys
    names = sorted(os.listdir(off))
    assert "scores.csv" not in names and "scores.json" not in names
    assert sorted(os.listdir(on)) == sorted(names + ["scores.csv", "scores.json"])
    for name in names:                                 # every other file byte for byte
        assert (on / name).read_bytes() == (off / name).read_bytes(), name
    # --limit: the scores cover what was written, no more
    lim = tmp_path / "lim"
    assert predict_code.write_code_predictions(_pairs(rows, cuda), str(lim), hp, min_iters=0,
                                               limit=4, scores=True) == keys[:4]
    _check_code_files_subset(lim, rows[:4])
    # the written directory can be scored again without decoding
    from sat_amd import score
    assert score.main(["--predictions-dir", str(off), "--output-dir", str(tmp_path / "re")]) == 0
    _check_code_files(tmp_path / "re", sorted(rows))


def test_write_predictions_scores_switch(cuda, tmp_path):
    """synthesize.write_predictions(scores=True): the predicted mel cut at its stop step against
    the ground-truth mel cut at its own length."""
    from sat_amd import synthesize
    rng = np.random.default_rng(12)
    B, T, M = 3, 40, 8
    frames, n_truth = [25, 40, 12], [30, 33, 12]
    amp = np.exp(rng.standard_normal((2, B, T, 1)))
    mel, truth = (amp * rng.standard_normal((2, B, T, M))).astype(np.float32)
    stop = np.full((B, T), -1.0, np.float32)
    for b, n in enumerate(frames):
        stop[b, n - 1:] = 1.0
    keys = ["k0", "k1", "k2"]

    def preds():
        return [{"mel": torch.tensor(mel, device=cuda), "stop_token": torch.tensor(stop),
                 "key": np.array([k.encode() for k in keys]),
                 "ground_truth_mel": truth, "ground_truth_mel_length": np.array(n_truth)}]

    hp = types.SimpleNamespace(num_mels=M, outputs_per_step=1, predicted_mel_extension="mfbsp",
                               use_postnet_v2=False)
    on, off = tmp_path / "on", tmp_path / "off"
    assert synthesize.write_predictions(preds(), str(on), hp, wav=False, scores=True) == keys
    assert synthesize.write_predictions(preds(), str(off), hp, wav=False) == keys
    names = sorted(os.listdir(off))
    assert sorted(os.listdir(on)) == sorted(names + ["scores.csv", "scores.json"])
    for name in names:
        assert (on / name).read_bytes() == (off / name).read_bytes(), name
    with open(on / "scores.csv", newline="") as f:
        got = list(csv.DictReader(f))
    assert [g["key"] for g in got] == keys
    for b, g in enumerate(got):
        cost, cells, margin, mean = R.dtw(mel[b, :frames[b]], truth[b, :n_truth[b]])
        assert margin > 1e-3 * mean
        assert int(g["path_length"]) == cells
        assert (int(g["predicted_length"]), int(g["truth_length"])) == (frames[b], n_truth[b])
        assert abs(float(g["cost"]) - cost) <= 12 * 2.0 ** -23 * cost
    with open(on / "scores.json") as f:
        doc = json.load(f)
    assert doc["kind"] == "mel" and doc["utterances"] == B
    with pytest.raises(ValueError, match="ground_truth_mel"):
        synthesize.write_predictions([{k: v for k, v in preds()[0].items()
                                       if k != "ground_truth_mel"}], str(tmp_path / "x"), hp,
                                     wav=False, scores=True)


def _check_code_files_subset(out_dir, rows):
    d, tt, tp, summary = _expected_codes(rows)
    with open(os.path.join(out_dir, "scores.csv"), newline="") as f:
        got = list(csv.DictReader(f))
    assert [g["key"] for g in got] == [r[0] for r in rows]
    assert [int(g["distance"]) for g in got] == d
    with open(os.path.join(out_dir, "scores.json")) as f:
        doc = json.load(f)
    assert doc["utterances"] == len(rows)
    assert abs(doc["summary"]["code_error_rate"] - summary["code_error_rate"]) <= 1e-12


CHILD = """
import sys, types
import numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import _sat_path; _sat_path.load()
import torch
import test_score_files_gpu as T
from sat_amd import predict_code
hp = types.SimpleNamespace(num_mels=T.C, outputs_per_step=1)
predict_code.write_code_predictions(T._pairs(T._perturbed(), torch.device("cuda:0")), {out!r}, hp,
                                    min_iters=0)
assert "sat_amd.predict_code" in sys.modules
print("score imported:", "sat_amd.score" in sys.modules)
"""


def test_scores_off_never_imports_the_score_module(cuda, tmp_path):
    code = CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), out=str(tmp_path / "o"))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "score imported: False" in r.stdout
    assert not (tmp_path / "o" / "scores.csv").exists()
