"""Synthesis: ``predict_mel.py`` ("synthesize waveform") with a waveform at the end.

``write_predictions(predictions, output_dir, hparams)`` consumes what ``model.predict`` yields --
one predictions dict per batch -- and writes per utterance

* ``<key>.<predicted_mel_extension>``: the predicted mel as raw little-endian float32
  [frames, num_mels], exactly predict_mel.py:58-62;
* ``<key>.wav`` (unless ``wav=False``): 16-bit PCM by ``Audio.inv_melspectrogram_batch`` --
  denormalise, inverse mel basis, Griffin-Lim on the GPU (csrc/vocoder.hip) -- where the reference
  stops at the mel file for an external WaveNet.

The decode of a batch ends when EVERY utterance has stopped, so each utterance is cut at its own
stop step by the rule of the device-side finished flag (inference.py): the first decoder step
``t > min_iters`` with ``sigmoid(stop_t) > 0.5``; it keeps ``(t + 1) * outputs_per_step`` frames, an
utterance that never stops all of them.  The waveforms of one batch are one
``inv_melspectrogram_batch`` call.  An utterance too short to invert (``hop * (frames - 1) <=
n_fft / 2``: the analysis could not reflect-pad it) is written as a mel file only, with a warning,
as preprocessing skips what it cannot frame.

Opt-in, the rest of predict_mel.py:63-74:

* ``<key>.png`` (``plots=True``, ``--plots``): the alignments, the decoder self-attention heads,
  the ground-truth and the predicted mel as one colour figure, composed on the GPU
  (csrc/figure.hip, ``sat_amd.plots``), each alignment cut at the utterance's own source length and
  stop step; ``key`` and ``text`` are ``tEXt`` chunks of the file, no text is drawn;
* ``<key>.tfrecord`` (``records=True``, ``--records``): ``tfrecord.write_prediction_result`` with
  the fields of utils/tfrecord.py:144-157 -- ``codes`` is the mel as written to the mel file,
  ``ground_truth_codes`` the target mel up to its own length (no rows where the batch has none).
  ``tfrecord.parse_prediction_result`` reads it back;
* ``scores.csv`` and ``scores.json`` (``scores=True``, ``--scores``): the distortion along the
  dynamic-time-warping path between each predicted mel, cut at its stop step, and the ground-truth
  mel, cut at its own length -- the ground truth ``--plots`` draws (``sat_amd.score``,
  csrc/score.hip).

CLI: ``python -m sat_amd.synthesize --source-data-root D --target-data-root D --checkpoint-dir D
--selected-list-dir D --output-dir D [--checkpoint P] [--selected-list-filename test.csv]
[--hparams S] [--hparam-json-file F] [--no-wav] [--griffin-lim-iters 60] [--power 1.5]
[--batch-size 1] [--seed 1234] [--plots] [--records] [--scores]``.  ``--seed`` seeds the prenet dropout masks
of a decode under ``--hparams apply_dropout_on_inference=True`` (inference.py); the weights come
from the checkpoint.
"""

from __future__ import annotations

import argparse
import os
import sys
import warnings
from typing import Iterable, List, Optional

import numpy as np

MIN_ITERS = 10              # FreeRunningDecoder's default, which model.predict decodes with


def _host(x) -> np.ndarray:
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def _key(k) -> str:
    if isinstance(k, np.ndarray):
        k = k.item()
    return k.decode("utf-8") if isinstance(k, (bytes, bytearray)) else str(k)


def stop_frames(stop, outputs_per_step: int, total_frames: int, min_iters: int = MIN_ITERS):
    """Frames each utterance keeps: ``stop`` [B, steps] are the stop-token logits;
    sigmoid(x) > 0.5 is x > 0."""
    stop = _host(stop)
    if stop.ndim == 1:
        stop = stop[None, :]
    fired = stop > 0
    fired[:, :min_iters + 1] = False                     # t > min_iters
    first = np.where(fired.any(axis=1), fired.argmax(axis=1), stop.shape[1] - 1)
    return [min(int(t + 1) * int(outputs_per_step), int(total_frames)) for t in first]


def _write_records(p: dict, keys, frames, host, output_dir: str) -> None:
    """``<key>.tfrecord`` of one predicted batch (predict_mel.py:71-74)."""
    from . import tfrecord
    B, M = host.shape[0], host.shape[2]
    ids = np.asarray(p["id"]).reshape(-1)
    texts = (np.asarray(p["text"], dtype=object).reshape(-1) if p.get("text") is not None
             else [""] * B)
    source = _host(p["source"])
    n_src = (_host(p["source_length"]).reshape(-1) if p.get("source_length") is not None
             else [source.shape[1]] * B)
    truth = _host(p["ground_truth_mel"]) if p.get("ground_truth_mel") is not None else None
    n_truth = (_host(p["ground_truth_mel_length"]).reshape(-1)
               if truth is not None and p.get("ground_truth_mel_length") is not None else None)
    for b, key in enumerate(keys):
        if truth is None:
            t = np.zeros((0, M), np.float32)
        else:
            t = truth[b, :int(n_truth[b])] if n_truth is not None else truth[b]
        tfrecord.write_prediction_result(int(ids[b]), key, host[b, :frames[b]], t, _key(texts[b]),
                                         source[b, :int(n_src[b])],
                                         os.path.join(output_dir, f"{key}.tfrecord"))


def write_predictions(predictions: Iterable[dict], output_dir: str, hparams, wav: bool = True,
                      audio=None, min_iters: int = MIN_ITERS, plots: bool = False,
                      records: bool = False, plot_options: Optional[dict] = None,
                      scores: bool = False, **gl) -> List[str]:
    """Writes the files of every predicted batch (see the module docstring) and returns the keys
    in the order written.  ``gl``: options of ``Audio.inv_melspectrogram_batch`` (``power``,
    ``n_iter``, ``momentum``, ``seed``); ``audio``: the ``Audio`` to use (built on first need);
    ``plots`` / ``records``: also ``<key>.png`` / ``<key>.tfrecord``; ``plot_options``: the
    geometry of ``plots.write_plots`` (``Hp, Wp, margin, cbar, background``); ``scores``: also
    ``scores.csv`` / ``scores.json`` over every utterance (the predictions must carry
    ``ground_truth_mel`` and ``ground_truth_mel_length``)."""
    os.makedirs(output_dir, exist_ok=True)
    r, M = int(hparams.outputs_per_step), int(hparams.num_mels)
    keys_written = []
    scorer = None
    if scores:
        from .score import Scorer
        scorer = Scorer("mel")
    for p in predictions:
        mel = p.get("mel_postnet") if getattr(hparams, "use_postnet_v2", False) else p["mel"]
        if getattr(mel, "ndim", 0) != 3 or mel.shape[2] != M:
            raise ValueError(f"predicted mel {tuple(mel.shape)}, expected [B, frames, {M}]")
        B, T = int(mel.shape[0]), int(mel.shape[1])
        keys = [_key(k) for k in np.asarray(p["key"]).reshape(-1)]
        if len(keys) != B:
            raise ValueError(f"{len(keys)} keys for {B} predicted utterances")
        frames = stop_frames(p["stop_token"], r, T, min_iters)
        host = _host(mel)
        for b, key in enumerate(keys):
            path = os.path.join(output_dir, f"{key}.{hparams.predicted_mel_extension}")
            with open(path, "wb") as f:
                f.write(np.ascontiguousarray(host[b, :frames[b]]).astype("<f4").tobytes())
        keys_written.extend(keys)
        if plots:
            from . import plots as P
            P.write_plots(p, output_dir, hparams, frames=frames, mel=mel, **(plot_options or {}))
        if records:
            _write_records(p, keys, frames, host, output_dir)
        if scorer is not None:
            if p.get("ground_truth_mel") is None or p.get("ground_truth_mel_length") is None:
                raise ValueError("scores: the predictions carry no ground_truth_mel / "
                                 "ground_truth_mel_length")
            truth, n_truth = p["ground_truth_mel"], _host(p["ground_truth_mel_length"]).reshape(-1)
            scorer.add(keys, [mel[b, :frames[b]] for b in range(B)],
                       [truth[b, :int(n_truth[b])] for b in range(B)])
        if not wav:
            continue
        if audio is None:
            from .audio import Audio
            audio = Audio(hparams, device=mel.device if hasattr(mel, "device") else None)
        n_fft, hop, _ = audio._stft_parameters()
        rows = [b for b in range(B) if hop * (frames[b] - 1) > n_fft // 2]
        for b in sorted(set(range(B)) - set(rows)):
            warnings.warn(f"{keys[b]}: {frames[b]} predicted frames are too few to invert "
                          f"(hop {hop}, n_fft {n_fft}); no wav written", RuntimeWarning)
        if not rows:
            continue
        if getattr(mel, "is_cuda", False):           # stays on the device: one gather of the rows
            kept = [frames[b] for b in rows]
            padded = mel[rows, :max(kept)].contiguous()
            out, lengths = audio.inv_melspectrogram_batch(padded, frames=kept, **gl)
        else:
            out, lengths = audio.inv_melspectrogram_batch([host[b, :frames[b]] for b in rows],
                                                          **gl)
        out, lengths = _host(out), _host(lengths)
        for i, b in enumerate(rows):
            audio.save_wav(out[i, :int(lengths[i])], os.path.join(output_dir, f"{keys[b]}.wav"))
    if scorer is not None and keys_written:
        scorer.write(output_dir)
    return keys_written


def load_key_list(filename: str, in_dir: str):
    """predict_mel.py:77-81."""
    with open(os.path.join(in_dir, filename), mode="r", encoding="utf-8") as f:
        return [l.rstrip("\n") for l in f if l.rstrip("\n")]


def predict_input_fn(hparams, source_files, target_files, batch_size: int = 1):
    """predict_mel.py:39-45: the listed records in order, batched, targets merged into the
    sources."""
    from . import datasets

    def input_fn():
        ds = datasets.create_from_tfrecord_files(source_files, target_files, hparams,
                                                 cycle_length=1)
        return iter(ds.prepare_and_zip().group_by_batch(batch_size=batch_size)
                    .merge_target_to_source().dataset)
    return input_fn


def main(argv=None) -> int:
    from .hparams import create_hparams, hparams_debug_string
    from .models import tacotron_model_factory
    ap = argparse.ArgumentParser(prog="python -m sat_amd.synthesize",
                                 description="Predicted mel files and Griffin-Lim waveforms of "
                                             "the listed utterances")
    ap.add_argument("--source-data-root", required=True, help="preprocessed source records")
    ap.add_argument("--target-data-root", required=True, help="preprocessed target records")
    ap.add_argument("--checkpoint-dir", required=True, help="the model_dir of the training")
    ap.add_argument("--checkpoint", default=None, help="a checkpoint file (default: the newest)")
    ap.add_argument("--selected-list-dir", required=True, help="directory of the key list")
    ap.add_argument("--selected-list-filename", default="test.csv")
    ap.add_argument("--output-dir", required=True)
    ap.add_argument("--hparams", default="", help="ad-hoc overrides, k=v,...")
    ap.add_argument("--hparam-json-file", default=None, help="JSON file of hyper-parameters")
    ap.add_argument("--no-wav", action="store_true", help="mel files only")
    ap.add_argument("--griffin-lim-iters", type=int, default=60)
    ap.add_argument("--power", type=float, default=1.5,
                    help="exponent on the linear magnitudes before Griffin-Lim")
    ap.add_argument("--batch-size", type=int, default=1, help="utterances per predicted batch")
    ap.add_argument("--seed", type=int, default=1234,
                    help="seed of the prenet dropout masks (apply_dropout_on_inference=True): "
                         "the same seed and key list give the same files")
    ap.add_argument("--plots", action="store_true",
                    help="also <key>.png: alignments and mels as one colour figure")
    ap.add_argument("--records", action="store_true",
                    help="also <key>.tfrecord: the prediction record (codes = the predicted mel)")
    ap.add_argument("--scores", action="store_true",
                    help="also scores.csv / scores.json: DTW distortion against the target mel")
    args = ap.parse_args(argv)
    hp = create_hparams(args.hparam_json_file, args.hparams)
    print(hparams_debug_string(hp))
    keys = load_key_list(args.selected_list_filename, args.selected_list_dir)
    listed = os.path.join(args.selected_list_dir, args.selected_list_filename)
    print(f"{len(keys)} keys from {listed}")
    src = [os.path.join(args.source_data_root, f"{k}.{hp.source_file_extension}") for k in keys]
    tgt = [os.path.join(args.target_data_root, f"{k}.{hp.target_file_extension}") for k in keys]
    model = tacotron_model_factory(hp, args.checkpoint_dir, None, seed=args.seed)
    preds = model.predict(predict_input_fn(hp, src, tgt, args.batch_size),
                          checkpoint_path=args.checkpoint)
    done = write_predictions(preds, args.output_dir, hp, wav=not args.no_wav,
                             plots=args.plots, records=args.records, scores=args.scores,
                             n_iter=args.griffin_lim_iters, power=args.power)
    print(f"{len(done)} utterances written to {args.output_dir}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
