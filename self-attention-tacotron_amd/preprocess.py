"""LJSpeech preprocessing: ``preprocess_ljspeech.py`` + ``preprocess/ljspeech.py`` +
``preprocess/text.py`` without TensorFlow, pyspark or librosa.

``LJSpeech(in_dir, out_dir, hparams)`` reads ``metadata.csv`` (``key|raw|normalised``; the third
field is the text, the line index the record id) and ``wavs/<key>.wav``, and writes per utterance
``<key>.source.tfrecord`` and ``<key>.target.tfrecord`` with the record writers of
``sat_amd.tfrecord`` -- the files ``sat_amd.datasets`` reads.  The mel is stored unnormalised as
float32 [frames, num_mels].  At the end ``hparams.json`` carries the keys of
``preprocess_ljspeech.py:69-80`` (corpus mean, standard deviation and minimum per mel bin) and
``list.csv`` the keys (:83-86).

Utterances go to the GPU in batches of up to 32, sorted by length inside a window of 8 batches so
that padding stays small (``Audio.melspectrogram_batch``: one upload, one launch).  The
per-utterance statistics come from ``sat_mel_stats``; corpus totals are float64 on the host.
Record files are written by one writer thread, so the GPU does not wait for the disk.

The shipped cleaner is ``basic_cleaners`` (lowercase, collapse whitespace).  The reference's
``english_cleaners`` also expands numbers and abbreviations and transliterates to ASCII with
``inflect`` / ``unidecode``; that is out of scope here, and the cleaner is an argument.

CLI: ``python -m sat_amd.preprocess ljspeech <in_dir> <out_dir> [--hparam-json-file F]
[--hparams S] [--source-only | --target-only]``.
"""

from __future__ import annotations

import argparse
import csv
import json
import os
import queue
import re
import threading
from collections import namedtuple
from typing import Callable, List, Optional, Tuple

import numpy as np

from . import tfrecord

# preprocess/text.py:21-28 -- ids 1..70, 0 reserved
_characters = 'ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz!\'\"()[],-.:;?` %<>'
symbols = list(_characters)
_symbol_to_id = {s: i + 1 for i, s in enumerate(symbols)}
_id_to_symbol = {i + 1: s for i, s in enumerate(symbols)}

_whitespace_re = re.compile(r"\s+")


def basic_cleaners(text: str) -> str:
    """Lowercase and collapse whitespace."""
    return re.sub(_whitespace_re, " ", text.lower())


def text_to_sequence(text: str, cleaner: Callable[[str], str] = basic_cleaners):
    """``(ids, clean_text)`` (preprocess/text.py:31-42: no leading or trailing silence symbol)."""
    clean_text = cleaner(text)
    sequence = []
    for ch in clean_text:
        if ch not in _symbol_to_id:
            raise ValueError(f"character {ch!r} (U+{ord(ch):04X}) is not in the symbol table; "
                             f"text: {clean_text!r}")
        sequence.append(_symbol_to_id[ch])
    return sequence, clean_text


def sequence_to_text(sequence) -> str:
    return "".join(_id_to_symbol[int(i)] for i in sequence)


class TextAndPath(namedtuple("TextAndPath", ["id", "key", "wav_path", "labels_path", "text"])):
    pass


class MelStatistics(namedtuple("MelStatistics",
                               ["id", "key", "max", "min", "sum", "length", "moment2"])):
    pass


HPARAMS_JSON_KEYS = ("num_mels", "num_freq", "sample_rate", "frame_length_ms", "frame_shift_ms",
                     "average_mel_level_db", "stddev_mel_level_db", "min_mel_level_db")


class _Writer:
    """One thread that runs queued write jobs in order; errors surface in ``close``."""

    def __init__(self, depth: int = 256):
        self._q: "queue.Queue" = queue.Queue(maxsize=depth)
        self._error: Optional[BaseException] = None
        self._thread = threading.Thread(target=self._work, daemon=True)
        self._thread.start()

    def _work(self):
        while True:
            job = self._q.get()
            if job is None:
                return
            if self._error is None:
                try:
                    job[0](*job[1:])
                except BaseException as ex:
                    self._error = ex

    def put(self, fn, *args):
        if self._error is not None:
            self.close()
        self._q.put((fn,) + args)

    def close(self):
        self._q.put(None)
        self._thread.join()
        if self._error is not None:
            raise self._error


class LJSpeech:
    BATCH = 32              # utterances per launch
    WINDOW = 8              # batches read ahead and sorted by length together

    def __init__(self, in_dir, out_dir, hparams, cleaner: Callable[[str], str] = basic_cleaners,
                 device=None):
        from .audio import Audio
        self.in_dir = in_dir
        self.out_dir = out_dir
        self.hparams = hparams
        self.cleaner = cleaner
        self.audio = Audio(hparams, device=device)

    def _extract_text_and_path(self, line, index):
        parts = line.strip().split('|')
        key = parts[0]
        text = parts[2]
        wav_path = os.path.join(self.in_dir, 'wavs', '%s.wav' % key)
        return TextAndPath(index, key, wav_path, None, text)

    def _extract_all_text_and_path(self):
        with open(os.path.join(self.in_dir, 'metadata.csv'), mode='r', encoding='utf-8') as f:
            for index, line in enumerate(f):
                if line.strip():
                    yield self._extract_text_and_path(line, index)

    def _text_to_sequence(self, text):
        sequence, clean_text = text_to_sequence(text, self.cleaner)
        return np.array(sequence, dtype=np.int64), clean_text

    def source_path(self, key):
        return os.path.join(self.out_dir, f"{key}.source.tfrecord")

    def target_path(self, key):
        return os.path.join(self.out_dir, f"{key}.target.tfrecord")

    def process_sources(self, records=None) -> List[str]:
        writer = _Writer()
        keys = []
        try:
            for r in (records if records is not None else self._extract_all_text_and_path()):
                sequence, clean_text = self._text_to_sequence(r.text)
                writer.put(tfrecord.write_preprocessed_source_data, r.id, r.key, sequence,
                           clean_text, self.source_path(r.key))
                keys.append(r.key)
        finally:
            writer.close()
        return keys

    def _batches(self, records):
        """Windows of BATCH * WINDOW utterances, loaded, sorted by length, cut into batches."""
        window: List[Tuple[TextAndPath, np.ndarray]] = []

        def flush():
            window.sort(key=lambda e: len(e[1]))
            for i in range(0, len(window), self.BATCH):
                yield window[i:i + self.BATCH]
            window.clear()
        for r in records:
            window.append((r, self.audio.load_wav(r.wav_path)))
            if len(window) == self.BATCH * self.WINDOW:
                yield from flush()
        yield from flush()

    def process_targets(self, records=None) -> List[MelStatistics]:
        """Writes every target record; returns the per-utterance statistics in record order."""
        writer = _Writer()
        stats: List[MelStatistics] = []
        try:
            for batch in self._batches(records if records is not None
                                       else self._extract_all_text_and_path()):
                mel, frames = self.audio.melspectrogram_batch([w for _, w in batch])
                st = self.audio.mel_statistics(mel, frames).cpu().numpy()
                mel_h, frames_h = mel.cpu().numpy(), frames.cpu().numpy()
                for b, (r, _) in enumerate(batch):
                    n = int(frames_h[b])
                    writer.put(tfrecord.write_preprocessed_target_data, r.id, r.key,
                               mel_h[b, :n], self.target_path(r.key))
                    stats.append(MelStatistics(id=r.id, key=r.key, min=st[b, 0], max=st[b, 1],
                                               sum=st[b, 2], length=n, moment2=st[b, 3]))
        finally:
            writer.close()
        stats.sort(key=lambda s: s.id)
        return stats

    @staticmethod
    def corpus_statistics(stats: List[MelStatistics]):
        """(average, stddev, min) per mel bin over all frames, float64
        (preprocess_ljspeech.py:65-67: stddev = sqrt(moment2 - average^2))."""
        total = float(sum(s.length for s in stats))
        average = np.sum([s.sum for s in stats], axis=0, dtype=np.float64) / total
        moment2 = np.sum([s.moment2 for s in stats], axis=0, dtype=np.float64) / total
        stddev = np.sqrt(moment2 - np.square(average))
        return average, stddev, np.min([s.min for s in stats], axis=0)

    def run(self, process_source: bool = True, process_target: bool = True) -> List[str]:
        os.makedirs(self.out_dir, exist_ok=True)
        records = list(self._extract_all_text_and_path())
        keys = [r.key for r in records]
        if process_source:
            self.process_sources(records)
        if process_target:
            average, stddev, min_db = self.corpus_statistics(self.process_targets(records))
            hp = self.hparams
            hparams_obj = {
                "num_mels": hp.num_mels,
                "num_freq": hp.num_freq,
                "sample_rate": hp.sample_rate,
                "frame_length_ms": hp.frame_length_ms,
                "frame_shift_ms": hp.frame_shift_ms,
                "average_mel_level_db": average.tolist(),
                "stddev_mel_level_db": stddev.tolist(),
                "min_mel_level_db": min_db.tolist(),
            }
            with open(os.path.join(self.out_dir, 'hparams.json'), 'w') as f:
                json.dump(hparams_obj, f, indent=4)
        with open(os.path.join(self.out_dir, 'list.csv'), 'w', newline='') as csvfile:
            w = csv.writer(csvfile)
            for key in keys:
                w.writerow([key])
        return keys


def main(argv=None) -> int:
    from .hparams import create_hparams, hparams_debug_string
    ap = argparse.ArgumentParser(prog="python -m sat_amd.preprocess",
                                 description="Waveforms and transcripts to TFRecord training data")
    sub = ap.add_subparsers(dest="dataset", required=True)
    lj = sub.add_parser("ljspeech", help="LJSpeech-1.1 layout: metadata.csv and wavs/")
    lj.add_argument("in_dir")
    lj.add_argument("out_dir")
    lj.add_argument("--hparam-json-file", default=None, help="JSON file of hyper-parameters")
    lj.add_argument("--hparams", default="", help="ad-hoc overrides, k=v,...")
    only = lj.add_mutually_exclusive_group()
    only.add_argument("--source-only", action="store_true")
    only.add_argument("--target-only", action="store_true")
    args = ap.parse_args(argv)
    hp = create_hparams(args.hparam_json_file, args.hparams)
    print(hparams_debug_string(hp))
    LJSpeech(args.in_dir, args.out_dir, hp).run(process_source=not args.target_only,
                                                 process_target=not args.source_only)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
