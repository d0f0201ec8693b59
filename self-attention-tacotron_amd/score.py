"""Objective scores of a free-running decode.

The fork ends its post-processing (postprocess_vqcodes.py:99-111,
tsu_postprocess_vqcodes_validation.py:104-116) by writing corpus-wide hypothesis / true lists for
an external sequence-error tool.  Here the two numbers are computed in the program, on the GPU
(csrc/score.hip, one workgroup per utterance):

* VQ-code models: the code error rate -- the Levenshtein distance between the predicted and the
  true code sequence over the true length (``score_codes``);
* mel models: the distortion along the dynamic-time-warping path between the predicted and the
  true mel, as stored (normalised log-mel): path cost over path length (``score_mels``).

``Scorer(kind)`` accumulates batches (``add(keys, pred, truth)``: one ragged upload and one launch
per batch) and ``write(output_dir)`` leaves

* ``scores.csv``: one row per key in the order added;
* ``scores.json``: ``{"kind", "utterances", "summary"}``.

CLI: ``python -m sat_amd.score --predictions-dir D [--kind codes|mel] [--output-dir D]`` scores a
directory an earlier ``predict_code`` (``codes``: every ``<key>.preds.txt`` / ``<key>.truth.txt``
pair) or ``synthesize --records`` (``mel``: every ``<key>.tfrecord`` prediction record, which
holds the prediction and the ground truth) run has written, without decoding again, at most
``GROUP`` = 256 pairs per launch.  ``--output-dir`` defaults to the predictions directory.
"""

from __future__ import annotations

import argparse
import csv
import json
import math
import os
from typing import List, Sequence

import numpy as np
import torch

from . import kernels as K

GROUP = 256                 # pairs per launch of the CLI
KINDS = ("codes", "mel")
COLUMNS = {"codes": ("key", "distance", "truth_length", "predicted_length", "error_rate",
                     "length_ratio"),
           "mel": ("key", "cost", "path_length", "distortion", "predicted_length",
                   "truth_length", "length_ratio")}


def _device(device):
    return torch.device("cuda" if device is None else device)


def _offsets(lengths, device):
    off = np.zeros(len(lengths) + 1, np.int64)
    np.cumsum(lengths, out=off[1:])
    return torch.from_numpy(off).to(device)


def _pack_codes(seqs, device):
    arrays = [np.asarray(s).reshape(-1) for s in seqs]
    for a in arrays:
        if a.size and a.dtype.kind not in "iu":
            raise ValueError(f"score_codes: code sequences must be integers, not {a.dtype}")
    lengths = [a.size for a in arrays]
    flat = (np.concatenate(arrays) if arrays else np.zeros(0)).astype(np.int32)
    return torch.from_numpy(flat).to(device), _offsets(lengths, device), lengths


def _pack_frames(seqs, device):
    rows = []
    for s in seqs:
        t = s if isinstance(s, torch.Tensor) else torch.from_numpy(np.array(s, np.float32))
        if t.dim() != 2:
            raise ValueError(f"score_mels: frames must be [T, width], not {tuple(t.shape)}")
        rows.append(t.to(device=device, dtype=torch.float32))
    lengths = [int(t.shape[0]) for t in rows]
    return torch.cat(rows).contiguous(), _offsets(lengths, device), lengths


def codes_summary(distance, truth_length, predicted_length) -> dict:
    """The summary of ``score_codes`` from per-utterance integers."""
    d, tt, tp = (np.asarray(x, np.int64) for x in (distance, truth_length, predicted_length))
    return {"code_error_rate": int(d.sum()) / int(tt.sum()),
            "mean_error_rate": math.fsum(int(x) / int(y) for x, y in zip(d, tt)) / len(d),
            "mean_length_ratio": math.fsum(int(x) / int(y) for x, y in zip(tp, tt)) / len(d)}


def mels_summary(cost, path_length, predicted_length, truth_length) -> dict:
    """The summary of ``score_mels`` from per-utterance costs and counts."""
    n = len(cost)
    return {"mean_distortion": math.fsum(float(c) / int(k) for c, k in zip(cost, path_length)) / n,
            "pooled_distortion": math.fsum(float(c) for c in cost) /
            int(np.asarray(path_length, np.int64).sum()),
            "mean_length_ratio": math.fsum(int(x) / int(y) for x, y in
                                           zip(predicted_length, truth_length)) / n}


def score_codes(pred: Sequence, truth: Sequence, device=None) -> dict:
    """``pred`` / ``truth``: equally many 1-D integer code sequences.  One launch.  Returns the
    per-utterance ``distance``, ``truth_length``, ``predicted_length`` (int64), ``error_rate`` =
    distance / truth_length and ``length_ratio`` = Tp / Tt (float64), and ``summary``:
    ``code_error_rate`` = sum distance / sum truth_length, ``mean_error_rate``,
    ``mean_length_ratio``.  A truth must not be empty (it has no rate); a prediction may be."""
    if len(pred) != len(truth) or not len(pred):
        raise ValueError(f"score_codes: {len(pred)} predictions for {len(truth)} truths")
    dev = _device(device)
    a, a_off, la = _pack_codes(pred, dev)
    b, b_off, lb = _pack_codes(truth, dev)
    if min(lb) < 1:
        raise ValueError(f"score_codes: truth {lb.index(0)} is empty")
    d = K.edit_distance(a, a_off, b, b_off).cpu().numpy().astype(np.int64)
    tt, tp = np.asarray(lb, np.int64), np.asarray(la, np.int64)
    return {"distance": d, "truth_length": tt, "predicted_length": tp,
            "error_rate": d / tt, "length_ratio": tp / tt, "summary": codes_summary(d, tt, tp)}


def score_mels(pred: Sequence, truth: Sequence, device=None) -> dict:
    """``pred`` / ``truth``: equally many [T, width] float arrays or device tensors, T >= 1,
    scored as stored.  One launch.  Returns the per-utterance ``cost`` (float64), ``path_length``,
    ``predicted_length``, ``truth_length`` (int64), ``distortion`` = cost / path_length and
    ``length_ratio`` = Tp / Tt, and ``summary``: ``mean_distortion`` over utterances, the pooled
    ``pooled_distortion`` = sum cost / sum path_length, ``mean_length_ratio``."""
    if len(pred) != len(truth) or not len(pred):
        raise ValueError(f"score_mels: {len(pred)} predictions for {len(truth)} truths")
    dev = _device(device)
    p, p_off, lp = _pack_frames(pred, dev)
    t, t_off, lt = _pack_frames(truth, dev)
    cost, n = K.dtw_distortion(p, p_off, t, t_off)
    cost, n = cost.cpu().numpy(), n.cpu().numpy().astype(np.int64)
    tp, tt = np.asarray(lp, np.int64), np.asarray(lt, np.int64)
    return {"cost": cost, "path_length": n, "predicted_length": tp, "truth_length": tt,
            "distortion": cost / n, "length_ratio": tp / tt,
            "summary": mels_summary(cost, n, tp, tt)}


class Scorer:
    """Accumulates the scores of a run: ``add`` per batch, ``write`` at the end."""

    def __init__(self, kind: str, device=None):
        if kind not in KINDS:
            raise ValueError(f"Scorer: kind {kind!r} is not one of {KINDS}")
        self.kind, self.device = kind, device
        self.rows: List[tuple] = []

    def add(self, keys: Sequence[str], pred: Sequence, truth: Sequence) -> dict:
        """Scores one batch (one upload, one launch) and keeps its rows; returns the batch's
        ``score_codes`` / ``score_mels`` result."""
        if len(keys) != len(pred):
            raise ValueError(f"Scorer.add: {len(keys)} keys for {len(pred)} predictions")
        if self.kind == "codes":
            s = score_codes(pred, truth, self.device)
            cols = (s["distance"], s["truth_length"], s["predicted_length"], s["error_rate"],
                    s["length_ratio"])
        else:
            s = score_mels(pred, truth, self.device)
            cols = (s["cost"], s["path_length"], s["distortion"], s["predicted_length"],
                    s["truth_length"], s["length_ratio"])
        for i, key in enumerate(keys):
            self.rows.append((str(key),) + tuple(c[i].item() for c in cols))
        return s

    def summary(self) -> dict:
        if not self.rows:
            raise ValueError("Scorer: nothing was added")
        col = {name: [r[i] for r in self.rows] for i, name in enumerate(COLUMNS[self.kind])}
        if self.kind == "codes":
            return codes_summary(col["distance"], col["truth_length"], col["predicted_length"])
        return mels_summary(col["cost"], col["path_length"], col["predicted_length"],
                            col["truth_length"])

    def write(self, output_dir: str) -> dict:
        """``scores.csv`` and ``scores.json`` in ``output_dir``; returns the json's content.
        Floats are written by ``repr``: they read back as the same float64."""
        doc = {"kind": self.kind, "utterances": len(self.rows), "summary": self.summary()}
        os.makedirs(output_dir, exist_ok=True)
        with open(os.path.join(output_dir, "scores.csv"), "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(COLUMNS[self.kind])
            for r in self.rows:
                w.writerow([repr(v) if isinstance(v, float) else v for v in r])
        with open(os.path.join(output_dir, "scores.json"), "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")
        return doc


def _read_codes(path: str) -> np.ndarray:
    with open(path) as f:
        return np.asarray([int(x) for x in f.read().split()], np.int64)


def score_directory(predictions_dir: str, kind: str = "codes", output_dir=None,
                    device=None) -> dict:
    """Scores what a decode wrote into ``predictions_dir`` (see the module docstring), keys in
    sorted order, and writes the two files into ``output_dir`` (default: the same directory)."""
    from . import tfrecord
    names = sorted(os.listdir(predictions_dir))
    if kind == "codes":
        keys = [n[:-len(".preds.txt")] for n in names if n.endswith(".preds.txt")
                and os.path.exists(os.path.join(predictions_dir,
                                                n[:-len(".preds.txt")] + ".truth.txt"))]
    else:
        keys = [n[:-len(".tfrecord")] for n in names if n.endswith(".tfrecord")]
    if not keys:
        wanted = ("<key>.preds.txt / <key>.truth.txt pairs" if kind == "codes"
                  else "<key>.tfrecord prediction records")
        raise FileNotFoundError(f"{predictions_dir}: no {wanted}")
    scorer = Scorer(kind, device)
    for g in range(0, len(keys), GROUP):
        group = keys[g:g + GROUP]
        pred, truth = [], []
        for key in group:
            base = os.path.join(predictions_dir, key)
            if kind == "codes":
                pred.append(_read_codes(base + ".preds.txt"))
                truth.append(_read_codes(base + ".truth.txt"))
            else:
                rec = tfrecord.parse_prediction_result(
                    next(iter(tfrecord.read_tfrecords(base + ".tfrecord"))))
                pred.append(rec.codes)
                truth.append(rec.ground_truth_codes)
        scorer.add(group, pred, truth)
    return scorer.write(output_dir or predictions_dir)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m sat_amd.score",
                                 description="Code error rate or DTW mel distortion of the "
                                             "utterances a decode has written")
    ap.add_argument("--predictions-dir", required=True,
                    help="output directory of predict_code, or of synthesize --records")
    ap.add_argument("--kind", choices=KINDS, default="codes")
    ap.add_argument("--output-dir", default=None, help="default: the predictions directory")
    args = ap.parse_args(argv)
    doc = score_directory(args.predictions_dir, args.kind, args.output_dir)
    print(json.dumps(doc, sort_keys=True))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
