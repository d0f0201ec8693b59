"""Code prediction: ``predict_code.py`` followed by ``postprocess_vqcodes.py``.

``write_code_predictions(pairs, output_dir, hparams)`` consumes ``(predictions, features)`` pairs
-- what ``model.predict`` yields per batch beside the batch it was predicted from -- and writes
per utterance

* ``<key>.mfbsp``: the predicted one-hot frames as raw little-endian float32 [T, C]
  (predict_code.py:55-59, ``codes.tofile``);
* ``<key>.tfrecord``: ``tfrecord.write_prediction_result`` (utils/tfrecord.py:144-157): ``id, key,
  codes, codes_length, codes_width, ground_truth_codes, ground_truth_codes_length, text, source,
  source_length``;
* ``<key>.txt`` (the text), ``<key>.preds.txt`` and ``<key>.truth.txt`` (blank-joined code indices
  and a newline): what postprocess_vqcodes.py:81-97 derives from that record;
* ``<key>.png`` (``plots=True``, ``--plots``; off by default): the two alignments, the decoder
  self-attention heads, the true and the predicted one-hot frames as one colour figure
  (``sat_amd.plots``, composed on the GPU by csrc/figure.hip);
* ``scores.csv`` and ``scores.json`` (``scores=True``, ``--scores``; off by default): the edit
  distance and the code error rate of every utterance written, from the indices already on the
  host, cut at each utterance's stop frame (``sat_amd.score``, csrc/score.hip).

The indices and the one-hot frames of a batch come from ONE ``sat_codes_argmax`` launch over the
decoder's raw outputs (``predictions["mel"]``; ties to the lowest index, as ``tf.argmax``).  The
decode of a batch ends when every utterance has stopped, so each utterance is cut at its own stop
step by ``synthesize.stop_frames``.  The ground truth is the target record's own indices.

Not carried over: the reference's ``sys.exit()`` after ten utterances (debugging; ``--limit N``
stops after N where that is wanted) and the corpus-wide list files postprocess_vqcodes.py writes
to fixed paths of its author's machine (``--scores``, or ``python -m sat_amd.score`` over the
output directory, gives the numbers those lists were made for).

CLI: ``python -m sat_amd.predict_code --source-data-root D --target-data-root D --checkpoint-dir D
--selected-list-dir D --output-dir D [--checkpoint P] [--selected-list-filename test.csv]
[--hparams S] [--hparam-json-file F] [--limit N] [--batch-size 1] [--seed 1234] [--plots]
[--scores]`` (``--seed``: the prenet dropout masks under ``--hparams apply_dropout_on_inference=True``).
"""

from __future__ import annotations

import argparse
import os
from typing import Iterable, List, Optional

import numpy as np

from . import tfrecord
from .synthesize import MIN_ITERS, _host, _key, load_key_list, predict_input_fn, stop_frames


def _text(t) -> str:
    if isinstance(t, np.ndarray):
        t = t.item()
    return t.decode("utf-8") if isinstance(t, (bytes, bytearray)) else str(t)


def _codes_line(index) -> str:
    return " ".join(str(int(c)) for c in index) + "\n"


def write_code_predictions(pairs: Iterable, output_dir: str, hparams,
                           limit: Optional[int] = None, min_iters: int = MIN_ITERS,
                           plots: bool = False, plot_options: Optional[dict] = None,
                           scores: bool = False) -> List[str]:
    """Writes the files of every predicted batch (see the module docstring) and returns the keys
    in the order written; stops after ``limit`` utterances when given.  ``plots``: also
    ``<key>.png`` (``plots.write_plots``; ``plot_options`` its geometry).  ``scores``: also
    ``scores.csv`` / ``scores.json`` over the utterances written."""
    from . import kernels as K
    os.makedirs(output_dir, exist_ok=True)
    scorer = None
    if scores:
        from .score import Scorer
        scorer = Scorer("codes")
    C, r = int(hparams.num_mels), int(hparams.outputs_per_step)
    written: List[str] = []
    for p, features in pairs:
        raw = p["mel"]
        if getattr(raw, "ndim", 0) != 3 or raw.shape[2] != C:
            raise ValueError(f"predicted codes {tuple(raw.shape)}, expected [B, frames, {C}]")
        B, T = int(raw.shape[0]), int(raw.shape[1])
        keys = [_key(k) for k in np.asarray(p["key"]).reshape(-1)]
        if len(keys) != B:
            raise ValueError(f"{len(keys)} keys for {B} predicted utterances")
        frames = stop_frames(p["stop_token"], r, T, min_iters)
        index, onehot = K.codes_argmax(raw.contiguous(), onehot=True)
        truth_index, offsets = np.asarray(features.code_index), np.asarray(features.offsets)
        if plots and (limit is None or len(written) < limit):
            from . import plots as P
            n_truth = np.diff(offsets[:B + 1]).astype(np.int64)
            dense = np.zeros((B, max(int(n_truth.max()), 1), C), np.float32)
            for b in range(B):
                dense[b, :n_truth[b]] = tfrecord.index_to_one_hot(
                    truth_index[int(offsets[b]):int(offsets[b + 1])], C)
            P.write_plots(dict(p, source_length=features.source_length, ground_truth_mel=dense,
                               ground_truth_mel_length=n_truth), output_dir, hparams,
                          frames=frames, mel=onehot, **(plot_options or {}))
        index, onehot = _host(index), _host(onehot)
        ids = np.asarray(p["id"]).reshape(-1)
        texts = np.asarray(p["text"], dtype=object).reshape(-1)
        source, source_length = _host(features.source), _host(features.source_length)
        first = len(written)
        for b, key in enumerate(keys):
            if limit is not None and len(written) >= limit:
                break
            codes = np.ascontiguousarray(onehot[b, :frames[b]]).astype("<f4")
            truth = truth_index[int(offsets[b]):int(offsets[b + 1])]
            text = _text(texts[b])
            base = os.path.join(output_dir, key)
            with open(base + ".mfbsp", "wb") as f:
                f.write(codes.tobytes())
            tfrecord.write_prediction_result(int(ids[b]), key, codes,
                                             tfrecord.index_to_one_hot(truth, C), text,
                                             source[b, :int(source_length[b])],
                                             base + ".tfrecord")
            with open(base + ".txt", "w", encoding="utf-8") as f:
                f.write(text)
            with open(base + ".preds.txt", "w") as f:
                f.write(_codes_line(index[b, :frames[b]]))
            with open(base + ".truth.txt", "w") as f:
                f.write(_codes_line(truth))
            print(key, codes.shape[0], len(truth), text)
            written.append(key)
        n = len(written) - first
        if scorer is not None and n:
            scorer.add(keys[:n], [index[b, :frames[b]] for b in range(n)],
                       [truth_index[int(offsets[b]):int(offsets[b + 1])] for b in range(n)])
        if limit is not None and len(written) >= limit:
            break
    if scorer is not None and written:
        scorer.write(output_dir)
    return written


def predict_codes(model, input_fn, output_dir: str, hparams, checkpoint_path=None,
                  limit: Optional[int] = None, plots: bool = False,
                  plot_options: Optional[dict] = None, scores: bool = False) -> List[str]:
    """``model.predict`` over ``input_fn`` beside a second pass over the same batches (the
    ground truth and the unpadded sources), into ``write_code_predictions``."""
    pairs = ((p, features) for p, (features, _) in
             zip(model.predict(input_fn, checkpoint_path=checkpoint_path), input_fn()))
    return write_code_predictions(pairs, output_dir, hparams, limit=limit, plots=plots,
                                  plot_options=plot_options, scores=scores)


def main(argv=None) -> int:
    from .hparams import create_hparams, hparams_debug_string
    from .models import tacotron_model_factory
    ap = argparse.ArgumentParser(prog="python -m sat_amd.predict_code",
                                 description="Predicted code frames and code sequences of the "
                                             "listed utterances")
    ap.add_argument("--source-data-root", required=True, help="preprocessed source records")
    ap.add_argument("--target-data-root", required=True, help="preprocessed target records")
    ap.add_argument("--checkpoint-dir", required=True, help="the model_dir of the training")
    ap.add_argument("--checkpoint", default=None, help="a checkpoint file (default: the newest)")
    ap.add_argument("--selected-list-dir", required=True, help="directory of the key list")
    ap.add_argument("--selected-list-filename", default="test.csv")
    ap.add_argument("--output-dir", required=True)
    ap.add_argument("--hparams", default="", help="ad-hoc overrides, k=v,...")
    ap.add_argument("--hparam-json-file", default=None, help="JSON file of hyper-parameters")
    ap.add_argument("--limit", type=int, default=None, help="stop after this many utterances")
    ap.add_argument("--batch-size", type=int, default=1, help="utterances per predicted batch")
    ap.add_argument("--seed", type=int, default=1234,
                    help="seed of the prenet dropout masks (apply_dropout_on_inference=True)")
    ap.add_argument("--plots", action="store_true",
                    help="also <key>.png: alignments, true and predicted codes as one figure")
    ap.add_argument("--scores", action="store_true",
                    help="also scores.csv / scores.json: edit distance and code error rate")
    args = ap.parse_args(argv)
    hp = create_hparams(args.hparam_json_file, args.hparams)
    print(hparams_debug_string(hp))
    keys = load_key_list(args.selected_list_filename, args.selected_list_dir)
    if args.limit is not None:
        keys = keys[:max(args.limit, 0)]
    print(f"{len(keys)} keys from "
          f"{os.path.join(args.selected_list_dir, args.selected_list_filename)}")
    src = [os.path.join(args.source_data_root, f"{k}.{hp.source_file_extension}") for k in keys]
    tgt = [os.path.join(args.target_data_root, f"{k}.{hp.target_file_extension}") for k in keys]
    model = tacotron_model_factory(hp, args.checkpoint_dir, None, seed=args.seed)
    done = predict_codes(model, predict_input_fn(hp, src, tgt, args.batch_size), args.output_dir,
                         hp, checkpoint_path=args.checkpoint, limit=args.limit,
                         plots=args.plots, scores=args.scores)
    print(f"{len(done)} utterances written to {args.output_dir}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
