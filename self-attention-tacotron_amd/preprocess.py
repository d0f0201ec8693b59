"""LJSpeech and VCTK preprocessing: ``preprocess_ljspeech.py`` + ``preprocess/ljspeech.py``,
``preprocess_vctk.py`` + ``preprocess/vctk.py`` and ``preprocess/text.py`` without TensorFlow,
pyspark or librosa.

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

``VCTK(in_dir, out_dir, hparams)`` reads the VCTK 0.8 layout (preprocess/vctk.py:91-127):
``speaker-info.txt`` (header skipped; id, age, gender with ``F`` -> 0 and anything else -> 1;
speaker 315 left out), ``wav48/p<id>/*.wav`` and ``txt/p<id>/*.txt`` sorted and paired by key, ids
in enumeration order.  Each batch is uploaded once, trimmed on the GPU (``Audio.trim_batch``) and
its mel taken from the trimmed segments in place (``melspectrogram_batch(wav, bounds=...)``).
Source records carry ``speaker_id, age, gender`` and the first line of the txt file.  An utterance
whose trimmed length is <= n_fft/2 cannot be framed: it is skipped with a warning and left out of
``list.csv``.  Both corpora share the batching, the writer thread, the statistics and the two
output files.

``Codes(in_dir, out_dir, hparams, num_codes, version)`` reads the VQ-code corpus of
preprocess/codes.py: the speaker table as VCTK's, per speaker the files ``p<id>*.txt`` of
``in_dir``, each holding ``text<TAB>codes`` on its first line.  ``version`` 0 keeps all codes, 1 or
2 every second one starting at ``version - 1``.  The source record has the VCTK fields plus the
phone fields (empty: there is no flite here, so ``hparams.phoneme`` must be ``none``) and ``lang``;
the target record holds the one-hot frames dense, as the reference, or as int32 indices
(``--compact``).  A first line without a tab is skipped with a warning and left out of
``list.csv``.  CLI: ``python -m sat_amd.preprocess codes <in_dir> <out_dir> --num-codes C
[--version V] [--speaker-info F] [--compact]`` plus the shared options below (no ``--resample``).

CLI: ``python -m sat_amd.preprocess {ljspeech | vctk} <in_dir> <out_dir> [--hparam-json-file F]
[--hparams S] [--source-only | --target-only] [--resample]``; ``vctk`` also takes
``--version 0.8``.

``--resample`` (``resample=True``) accepts wavs at any rate: ``_batches`` keeps ``(wav, rate)`` as
read, and ``_mel_batch`` first brings the batch to ``hparams.sample_rate`` on the GPU
(``Audio.resample_batch``, one launch per distinct source rate); the trim, the mel launch and the
too-short rule then see the resampled utterances, which stay on the device.  Without it a file at
another rate raises ``load_wav``'s ``ValueError``, as before.
"""

from __future__ import annotations

import argparse
import csv
import json
import os
import queue
import re
import sys
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


class SpeakerInfo(namedtuple("SpeakerInfo", ["id", "age", "gender"])):
    pass


class TxtWavRecord(namedtuple("TxtWavRecord",
                              ["id", "key", "txt_path", "wav_path", "speaker_info"])):
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


class _Corpus:
    """What the corpora share: length-sorted batches, the writer thread, the statistics,
    ``hparams.json`` and ``list.csv``.  A corpus lists its records (``_records``; each has ``id``,
    ``key`` and ``wav_path``), queues one source record (``_put_source``) and turns a batch of
    loaded waveforms into mels (``_mel_batch``)."""
    BATCH = 32              # utterances per launch
    WINDOW = 8              # batches read ahead and sorted by length together

    def __init__(self, in_dir, out_dir, hparams, cleaner: Callable[[str], str] = basic_cleaners,
                 device=None, resample: bool = False):
        from .audio import Audio
        self.in_dir = in_dir
        self.out_dir = out_dir
        self.hparams = hparams
        self.cleaner = cleaner
        self.audio = Audio(hparams, device=device)
        self.resample = resample            # wavs at any rate, brought to hparams.sample_rate
        self.skipped: List[str] = []        # keys _mel_batch left out

    def _records(self):
        raise NotImplementedError("_records")

    def _put_source(self, writer, r):
        raise NotImplementedError("_put_source")

    def _mel_batch(self, batch):
        """``(kept, mel, frames)``: the batch's entries that have a mel, in the row order of
        ``mel`` [len(kept), F_max, num_mels] and ``frames`` (both on the device)."""
        batch = self._resampled(batch)
        mel, frames = self.audio.melspectrogram_batch([w for _, w in batch])
        return batch, mel, frames

    def _resampled(self, batch):
        """With ``resample`` the batch's ``(wav, rate)`` entries become device tensors at
        hparams.sample_rate (``Audio.resample_batch``); without it the batch is returned as it
        is."""
        if not self.resample:
            return batch
        wavs, _ = self.audio.resample_batch([w for _, (w, _) in batch],
                                            [rate for _, (_, rate) in batch])
        return [(r, w) for (r, _), w in zip(batch, wavs)]

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
            for r in (records if records is not None else self._records()):
                self._put_source(writer, r)
                keys.append(r.key)
        finally:
            writer.close()
        return keys

    def _batches(self, records):
        """Windows of BATCH * WINDOW utterances, loaded, sorted by length, cut into batches.
        With ``resample`` an entry's waveform is ``read_wav``'s ``(wav, rate)`` and the order is
        by duration."""
        window: List[Tuple[TextAndPath, np.ndarray]] = []
        if self.resample:
            load, length = self.audio.read_wav, lambda e: len(e[1][0]) / e[1][1]
        else:
            load, length = self.audio.load_wav, lambda e: len(e[1])

        def flush():
            window.sort(key=length)
            for i in range(0, len(window), self.BATCH):
                yield window[i:i + self.BATCH]
            window.clear()
        for r in records:
            window.append((r, load(r.wav_path)))
            if len(window) == self.BATCH * self.WINDOW:
                yield from flush()
        yield from flush()

    def process_targets(self, records=None) -> List[MelStatistics]:
        """Writes every target record; returns the per-utterance statistics in record order."""
        writer = _Writer()
        stats: List[MelStatistics] = []
        try:
            for batch in self._batches(records if records is not None else self._records()):
                batch, mel, frames = self._mel_batch(batch)
                if not batch:
                    continue
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
        records = list(self._records())
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
        # sources after the targets: an utterance _mel_batch left out gets no record at all
        records = [r for r in records if r.key not in set(self.skipped)]
        keys = [r.key for r in records]
        if process_source:
            self.process_sources(records)
        with open(os.path.join(self.out_dir, 'list.csv'), 'w', newline='') as csvfile:
            w = csv.writer(csvfile)
            for key in keys:
                w.writerow([key])
        return keys


class LJSpeech(_Corpus):
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

    _records = _extract_all_text_and_path

    def _put_source(self, writer, r):
        sequence, clean_text = self._text_to_sequence(r.text)
        writer.put(tfrecord.write_preprocessed_source_data, r.id, r.key, sequence, clean_text,
                   self.source_path(r.key))


class VCTK(_Corpus):
    """preprocess/vctk.py:83-152, VCTK-Corpus 0.8."""

    def __init__(self, in_dir, out_dir, hparams, speaker_info_filename='speaker-info.txt',
                 cleaner: Callable[[str], str] = basic_cleaners, device=None,
                 version: str = "0.8", resample: bool = False):
        if str(version) != "0.8":
            raise ValueError(f"VCTK version {version}: only the 0.8 layout is read (0.91 needs "
                             "flite phone labels, which are not built here)")
        super().__init__(in_dir, out_dir, hparams, cleaner, device, resample)
        self.speaker_info_filename = speaker_info_filename

    def _load_speaker_info(self):
        with open(os.path.join(self.in_dir, self.speaker_info_filename), mode='r',
                  encoding='utf8') as f:
            for line in f.readlines()[1:]:
                si = line.split()
                if not si or si[0] == "315":      # the corpus ships no transcripts for p315
                    continue
                yield SpeakerInfo(int(si[0]), int(si[1]), 0 if si[2] == 'F' else 1)

    def list_files(self) -> List[TxtWavRecord]:
        def files(sub, si, ext):
            d = os.path.join(self.in_dir, sub, f"p{si.id}")
            return [os.path.join(d, f) for f in sorted(os.listdir(d)) if f.endswith(ext)]

        out: List[TxtWavRecord] = []
        for si in self._load_speaker_info():
            txts, wavs = files("txt", si, ".txt"), files("wav48", si, ".wav")
            if len(txts) != len(wavs):
                raise ValueError(f"speaker p{si.id}: {len(txts)} txt files, {len(wavs)} wav files")
            for txt_f, wav_f in zip(txts, wavs):
                key1 = os.path.splitext(os.path.basename(wav_f))[0]
                key2 = os.path.splitext(os.path.basename(txt_f))[0]
                if key1 != key2:
                    raise ValueError(f"speaker p{si.id}: {wav_f} is paired with {txt_f}")
                out.append(TxtWavRecord(len(out), key1, txt_f, wav_f, si))
        return out

    _records = list_files

    def _put_source(self, writer, r):
        with open(r.txt_path, mode='r', encoding='utf8') as f:
            txt = f.readline().rstrip("\n")
        sequence, clean_text = self._text_to_sequence(txt)
        si = r.speaker_info
        writer.put(tfrecord.write_preprocessed_vctk_source_data, r.id, r.key, sequence,
                   clean_text, si.id, si.age, si.gender, self.source_path(r.key))

    def _skip(self, r, why):
        print(f"warning: skipping {r.key}: {why}", file=sys.stderr)
        self.skipped.append(r.key)

    def _mel_batch(self, batch):
        """One upload, the trim launch, one read-back of the bounds, one mel launch over the
        trimmed segments in place."""
        import torch
        n_fft = self.audio._stft_parameters()[0]
        half_trim = int(self.hparams.trim_frame_length) // 2
        batch = self._resampled(batch)
        kept = []
        for r, w in batch:
            if len(w) <= half_trim:
                self._skip(r, f"{len(w)} samples, at most half a trim frame ({half_trim})")
            else:
                kept.append((r, w))
        if not kept:
            return [], None, None
        wav, bounds = self.audio.trim_batch([w for _, w in kept])
        bounds = bounds.cpu().numpy()
        rows = []
        for b, (r, _) in enumerate(kept):
            n = int(bounds[b, 1] - bounds[b, 0])
            if n <= n_fft // 2:
                self._skip(r, f"{n} samples after the trim, at most n_fft/2 = {n_fft // 2}: "
                              "no frame can be formed")
            else:
                rows.append(b)
        if not rows:
            return [], None, None
        if len(rows) < len(kept):
            wav = wav[torch.tensor(rows, device=wav.device)]
            bounds, kept = bounds[rows], [kept[b] for b in rows]
        mel, frames = self.audio.melspectrogram_batch(wav, bounds=bounds)
        return kept, mel, frames


class TxtCodeRecord(namedtuple("TxtCodeRecord",
                               ["id", "key", "txt_path", "code_path", "speaker_info"])):
    pass


class Codes:
    """preprocess/codes.py:90-176 + preprocess_vqcodes.py: a folder of ``p<id>_*.txt`` files whose
    first line is ``text<TAB>codes`` (codes separated by blanks) becomes source and target
    records.  No audio and no device work: a target is ``num_codes``-wide one-hot frames, written
    dense as the reference does or, with ``compact``, as int32 indices."""

    def __init__(self, in_dir, out_dir, hparams, num_codes, version=0,
                 speaker_info_filename=None, cleaner: Callable[[str], str] = basic_cleaners,
                 compact: bool = False):
        if hparams.phoneme != "none":
            raise ValueError(f"phoneme={hparams.phoneme!r}: phone labels need flite, which is not "
                             "built here; preprocess with phoneme=none (the records then hold "
                             "empty phone fields and train with source='char')")
        if int(version) not in (0, 1, 2):
            raise ValueError(f"codes version {version}: 0 (all codes), 1 or 2 (every second one)")
        if int(num_codes) < 1:
            raise ValueError(f"num_codes {num_codes} < 1")
        self.in_dir, self.out_dir, self.hparams = in_dir, out_dir, hparams
        self.num_codes, self.version = int(num_codes), int(version)
        self.speaker_info_filename = (speaker_info_filename if speaker_info_filename is not None
                                      else os.path.join(in_dir, "speaker-info.txt"))
        self.cleaner, self.compact = cleaner, bool(compact)
        self.skipped: List[str] = []

    def _load_speaker_info(self):
        with open(self.speaker_info_filename, mode='r', encoding='utf8') as f:
            for line in f.readlines()[1:]:
                si = line.split()
                if not si or si[0] == "315":
                    continue
                yield SpeakerInfo(int(si[0]), int(si[1]), 0 if si[2] == 'F' else 1)

    def list_files(self) -> List[TxtCodeRecord]:
        """:100-124.  The key is the file name without its extension (``os.path.splitext``); the
        reference's ``strip('.txt')`` also eats trailing ``t`` and ``x`` characters of the key."""
        names = sorted(os.listdir(self.in_dir))
        out: List[TxtCodeRecord] = []
        for si in self._load_speaker_info():
            for name in names:
                if name.endswith('.txt') and name.startswith(f"p{si.id}"):
                    path = os.path.join(self.in_dir, name)
                    out.append(TxtCodeRecord(len(out), os.path.splitext(name)[0], path, path, si))
        return out

    def read_record(self, r: TxtCodeRecord):
        """``(text, code indices)`` of a file's first line (:140-151, :165-167); None for a line
        that is not ``text<TAB>codes``."""
        with open(r.code_path, mode='r', encoding='utf8') as f:
            parts = f.readline().rstrip("\n").split("\t")
        if len(parts) != 2:
            return None
        codes = [int(c) for c in parts[1].split(" ") if c != ""]
        if self.version >= 1:
            codes = codes[self.version - 1::2]
        return parts[0], np.array(codes, dtype=np.int32)

    def source_path(self, key):
        return os.path.join(self.out_dir, f"{key}.source.tfrecord")

    def target_path(self, key):
        return os.path.join(self.out_dir, f"{key}.target.tfrecord")

    def _skip(self, r, why):
        print(f"warning: skipping {r.key}: {why}", file=sys.stderr)
        self.skipped.append(r.key)

    def run(self, process_source: bool = True, process_target: bool = True) -> List[str]:
        os.makedirs(self.out_dir, exist_ok=True)
        keys = []
        for r in self.list_files():
            rec = self.read_record(r)
            if rec is None:
                self._skip(r, "the first line is not text<TAB>codes")
                continue
            text, codes = rec
            if codes.size == 0:
                self._skip(r, "no codes")
                continue
            if codes.min() < 0 or codes.max() >= self.num_codes:
                raise ValueError(f"{r.code_path}: a code outside 0..{self.num_codes - 1}")
            if process_source:
                sequence, clean_text = text_to_sequence(text, self.cleaner)
                si = r.speaker_info
                tfrecord.write_preprocessed_codes_source_data(
                    r.id, r.key, np.array(sequence, dtype=np.int64), clean_text, si.id, si.age,
                    si.gender, self.source_path(r.key))
            if process_target:
                tfrecord.write_preprocessed_code_data(r.id, r.key, codes, self.num_codes,
                                                      self.target_path(r.key), self.compact)
            keys.append(r.key)
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
    vc = sub.add_parser("vctk", help="VCTK-Corpus 0.8 layout: speaker-info.txt, wav48/, txt/")
    vc.add_argument("--version", default="0.8", help="corpus version (only 0.8)")
    cd = sub.add_parser("codes", help="VQ-code corpus: speaker-info.txt and p<id>_*.txt files "
                                      "holding text<TAB>codes")
    cd.add_argument("--num-codes", type=int, required=True, help="code values (one-hot width)")
    cd.add_argument("--version", type=int, default=0,
                    help="0: all codes; 1 or 2: every second code from the first / second")
    cd.add_argument("--speaker-info", default=None,
                    help="speaker table (default <in_dir>/speaker-info.txt)")
    cd.add_argument("--compact", action="store_true",
                    help="targets as int32 code indices instead of dense one-hot rows")
    for p in (lj, vc, cd):
        p.add_argument("in_dir")
        p.add_argument("out_dir")
        p.add_argument("--hparam-json-file", default=None, help="JSON file of hyper-parameters")
        p.add_argument("--hparams", default="", help="ad-hoc overrides, k=v,...")
        only = p.add_mutually_exclusive_group()
        only.add_argument("--source-only", action="store_true")
        only.add_argument("--target-only", action="store_true")
    for p in (lj, vc):
        p.add_argument("--resample", action="store_true",
                       help="bring wavs at another rate to hparams.sample_rate on the GPU "
                            "(default: such a file is an error)")
    args = ap.parse_args(argv)
    hp = create_hparams(args.hparam_json_file, args.hparams)
    print(hparams_debug_string(hp))
    if args.dataset == "codes":
        corpus = Codes(args.in_dir, args.out_dir, hp, args.num_codes, version=args.version,
                       speaker_info_filename=args.speaker_info, compact=args.compact)
    elif args.dataset == "vctk":
        corpus = VCTK(args.in_dir, args.out_dir, hp, version=args.version,
                      resample=args.resample)
    else:
        corpus = LJSpeech(args.in_dir, args.out_dir, hp, resample=args.resample)
    corpus.run(process_source=not args.target_only, process_target=not args.source_only)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
