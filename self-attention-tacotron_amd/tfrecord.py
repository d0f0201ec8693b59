"""TFRecord files and ``tf.train.Example`` records of the dataset path, without TensorFlow.

Restates what the reference's data path reads and writes:
* framing (``tf.data.TFRecordDataset`` / ``tf.python_io.TFRecordWriter``, used by
  datasets/ljspeech/dataset.py:96-112 and utils/tfrecord.py:46-49): ``uint64 length |
  uint32 masked_crc32c(length) | payload | uint32 masked_crc32c(payload)``.  Framing, CRC-32C and
  record indexing run in libsat_hip's host entries (``sat_tfrecord_frame`` /
  ``sat_tfrecord_index``, csrc/records.hip);
* the ``tf.train.Example`` protobuf wire format (``Example{features=1}``, ``Features{map<string,
  Feature> feature=1}``, ``Feature{bytes_list=1 | float_list=2 | int64_list=3}``, each list a
  repeated field 1, packed or not), encoded and decoded here;
* the LJSpeech record types of preprocess/ljspeech.py:23-45: source records ``id, key,
  source (int64 bytes), source_length, text`` and target records ``id, key, mel (float32
  bytes), target_length, mel_width``; parsed as ``parse_preprocessed_source_data`` /
  ``decode_preprocessed_source_data`` (datasets/ljspeech/dataset.py:53-73) and the mel
  analogues the dataset imports from utils.tfrecord (``PreprocessedMelData``);
* the VCTK source record of preprocess/vctk.py:31-44, which adds ``speaker_id, age, gender``, and
  its parser (datasets/vctk/dataset.py:64-96), which also takes the ``phone, phone_length,
  phone_txt`` fields of the phone front end when a record carries them (None otherwise).  VCTK
  target records are the LJSpeech ones;
* the VQ-code records of preprocess/codes.py:20-49: the source record with the phone fields and
  ``lang``, the target record ``id, key, lang, codes (float32 one-hot bytes), codes_length,
  codes_width`` -- or, compact, ``code_index`` (int32 bytes) in place of ``codes`` -- parsed to
  indices either way, and the prediction record of utils/tfrecord.py:144-157.
"""

from __future__ import annotations

import ctypes
import struct
from collections import namedtuple
from typing import Dict, Iterable, Iterator, List, Tuple, Union

import numpy as np

from . import _lib


class PreprocessedSourceData(namedtuple("PreprocessedSourceData",
                                        ["id", "key", "source", "source_length", "text"])):
    pass


class PreprocessedVCTKSourceData(namedtuple("PreprocessedVCTKSourceData",
                                            ["id", "key", "source", "source_length",
                                             "speaker_id", "age", "gender", "text", "phone",
                                             "phone_length", "phone_txt"])):
    pass


class PreprocessedMelData(namedtuple("PreprocessedMelData",
                                     ["id", "key", "mel", "target_length", "mel_width"])):
    pass


class PreprocessedCodeData(namedtuple("PreprocessedCodeData",
                                      ["id", "key", "lang", "code_index", "codes_length",
                                       "codes_width"])):
    """A code target as indices: ``code_index`` int32 [codes_length], each in 0..codes_width-1
    (utils/tfrecord.py:21-23 holds the dense ``codes`` instead)."""


class CodePredictionResult(namedtuple("CodePredictionResult",
                                      ["id", "key", "codes", "codes_length", "codes_width",
                                       "ground_truth_codes", "ground_truth_codes_length", "text",
                                       "source", "source_length"])):
    pass


Feature = Tuple[str, list]          # ("int64" | "bytes" | "float", values)


# ---------------------------------------------------------------- framing (libsat_hip host)
def frame_record(payload: bytes) -> bytes:
    out = ctypes.create_string_buffer(len(payload) + 16)
    n = _lib.load().sat_tfrecord_frame(payload, len(payload), out)
    return out.raw[:n]


def split_records(buf: bytes, verify: bool = True) -> List[bytes]:
    """Payloads of a buffer of concatenated TFRecords (checksums verified by default)."""
    L = _lib.load()
    cap = max(1, len(buf) // 16)
    spans = (ctypes.c_int64 * (2 * cap))()
    n = L.sat_tfrecord_index(buf, len(buf), int(verify), spans, cap)
    if n < 0:
        raise ValueError("corrupt TFRecord data: " + L.sat_last_error_string().decode(errors="replace"))
    return [buf[spans[2 * i]: spans[2 * i] + spans[2 * i + 1]] for i in range(n)]


def write_tfrecords(records: Iterable[bytes], filename: str) -> None:
    with open(filename, "wb") as f:
        for r in records:
            f.write(frame_record(r))


def read_tfrecords(filename: str, verify: bool = True) -> Iterator[bytes]:
    with open(filename, "rb") as f:
        buf = f.read()
    yield from split_records(buf, verify)


# ---------------------------------------------------------------- protobuf wire format
def _varint(v: int) -> bytes:
    v &= (1 << 64) - 1                 # int64 two's complement, as protobuf
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        if v:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def _read_varint(b: bytes, i: int) -> Tuple[int, int]:
    shift = v = 0
    while True:
        if i >= len(b):
            raise ValueError("truncated varint")
        c = b[i]
        i += 1
        v |= (c & 0x7F) << shift
        if not c & 0x80:
            return v, i
        shift += 7
        if shift > 63:
            raise ValueError("varint too long")


def _ld(field: int, payload: bytes) -> bytes:
    return _varint(field << 3 | 2) + _varint(len(payload)) + payload


def _fields(b: bytes) -> Iterator[Tuple[int, int, Union[int, bytes]]]:
    i = 0
    while i < len(b):
        key, i = _read_varint(b, i)
        field, wt = key >> 3, key & 7
        if wt == 0:
            v, i = _read_varint(b, i)
        elif wt == 2:
            n, i = _read_varint(b, i)
            if i + n > len(b):
                raise ValueError("truncated length-delimited field")
            v, i = b[i:i + n], i + n
        elif wt == 5:
            v, i = b[i:i + 4], i + 4
        elif wt == 1:
            v, i = b[i:i + 8], i + 8
        else:
            raise ValueError(f"unsupported wire type {wt}")
        yield field, wt, v


def encode_example(features: Dict[str, Feature]) -> bytes:
    """``tf.train.Example(features=tf.train.Features(feature=...)).SerializeToString()``;
    map entries in the given order, numeric lists packed (proto3)."""
    entries = b""
    for name, (kind, values) in features.items():
        if kind == "bytes":
            lst = b"".join(_ld(1, bytes(v)) for v in values)
            feat = _ld(1, lst)
        elif kind == "float":
            feat = _ld(2, _ld(1, np.asarray(values, "<f4").tobytes()) if len(values) else b"")
        elif kind == "int64":
            feat = _ld(3, _ld(1, b"".join(_varint(int(v)) for v in values)) if len(values) else b"")
        else:
            raise ValueError(f"unknown feature kind {kind!r}")
        entries += _ld(1, _ld(1, name.encode("utf-8")) + _ld(2, feat))
    return _ld(1, entries)


def decode_example(buf: bytes) -> Dict[str, Feature]:
    out: Dict[str, Feature] = {}
    for f, wt, feats in _fields(buf):
        if f != 1 or wt != 2:
            continue
        for f2, wt2, entry in _fields(feats):
            if f2 != 1 or wt2 != 2:
                continue
            name, feat = "", b""
            for f3, _, v in _fields(entry):
                if f3 == 1:
                    name = v.decode("utf-8")
                elif f3 == 2:
                    feat = v
            kind, values = "bytes", []
            for f4, _, lst in _fields(feat):
                if f4 == 1:
                    kind, values = "bytes", [v for f5, _, v in _fields(lst) if f5 == 1]
                elif f4 == 2:
                    kind, values = "float", []
                    for f5, wt5, v in _fields(lst):
                        if f5 == 1:
                            values.extend(np.frombuffer(v, "<f4").tolist() if wt5 == 2
                                          else [struct.unpack("<f", v)[0]])
                elif f4 == 3:
                    kind, values = "int64", []
                    for f5, wt5, v in _fields(lst):
                        if f5 != 1:
                            continue
                        if wt5 == 2:
                            j = 0
                            while j < len(v):
                                x, j = _read_varint(v, j)
                                values.append(x - (1 << 64) if x >> 63 else x)
                        else:
                            values.append(v - (1 << 64) if v >> 63 else v)
            out[name] = (kind, values)
    return out


def _scalar(ex: Dict[str, Feature], name: str, kind: str):
    """tf.FixedLenFeature((), kind): exactly one value, else InvalidArgumentError (ValueError)."""
    if name not in ex:
        raise ValueError(f"Feature: {name} (data type: {kind}) is required but could not be found")
    k, v = ex[name]
    if k != kind or len(v) != 1:
        raise ValueError(f"Key: {name}.  Can't parse serialized Example: expected one {kind}")
    return v[0]


# ---------------------------------------------------------------- LJSpeech record types
def source_example(_id: int, key: str, source: np.ndarray, text: str) -> bytes:
    """preprocess/ljspeech.py:35-45 (write_preprocessed_source_data's Example)."""
    source = np.ascontiguousarray(source, dtype="<i8")
    return encode_example({"id": ("int64", [_id]), "key": ("bytes", [key.encode("utf-8")]),
                           "source": ("bytes", [source.tobytes()]),
                           "source_length": ("int64", [len(source)]),
                           "text": ("bytes", [text.encode("utf-8")])})


def target_example(_id: int, key: str, mel: np.ndarray) -> bytes:
    """preprocess/ljspeech.py:23-32 (write_preprocessed_target_data's Example)."""
    mel = np.ascontiguousarray(mel, dtype="<f4")
    return encode_example({"id": ("int64", [_id]), "key": ("bytes", [key.encode("utf-8")]),
                           "mel": ("bytes", [mel.tobytes()]),
                           "target_length": ("int64", [len(mel)]),
                           "mel_width": ("int64", [mel.shape[1]])})


def write_preprocessed_source_data(_id: int, key: str, source: np.ndarray, text: str,
                                   filename: str) -> None:
    write_tfrecords([source_example(_id, key, source, text)], filename)


def write_preprocessed_target_data(_id: int, key: str, mel: np.ndarray, filename: str) -> None:
    write_tfrecords([target_example(_id, key, mel)], filename)


def parse_preprocessed_source_data(record: bytes) -> PreprocessedSourceData:
    """parse_preprocessed_source_data + decode_preprocessed_source_data
    (datasets/ljspeech/dataset.py:53-73): source = decode_raw(int64)."""
    ex = decode_example(record)
    return PreprocessedSourceData(
        id=_scalar(ex, "id", "int64"), key=_scalar(ex, "key", "bytes"),
        source=np.frombuffer(_scalar(ex, "source", "bytes"), "<i8").astype(np.int64),
        source_length=_scalar(ex, "source_length", "int64"), text=_scalar(ex, "text", "bytes"))


def parse_preprocessed_mel_data(record: bytes) -> PreprocessedMelData:
    """The mel target record (preprocess/ljspeech.py:23-32): mel = decode_raw(float32)
    reshaped [target_length, mel_width]."""
    ex = decode_example(record)
    width = _scalar(ex, "mel_width", "int64")
    mel = np.frombuffer(_scalar(ex, "mel", "bytes"), "<f4").astype(np.float32)
    if width <= 0 or mel.size % width:
        raise ValueError(f"mel record: {mel.size} floats do not fill rows of width {width}")
    return PreprocessedMelData(id=_scalar(ex, "id", "int64"), key=_scalar(ex, "key", "bytes"),
                               mel=mel.reshape(-1, width),
                               target_length=_scalar(ex, "target_length", "int64"),
                               mel_width=width)


# ---------------------------------------------------------------- VCTK source records
def vctk_source_example(_id: int, key: str, source: np.ndarray, text: str, speaker_id: int,
                        age: int, gender: int, phone: np.ndarray = None,
                        phone_txt: str = None) -> bytes:
    """preprocess/vctk.py:31-44 (write_preprocessed_source_data's Example); with ``phone`` also
    the three phone fields datasets/vctk/dataset.py:74-76 reads."""
    source = np.ascontiguousarray(source, dtype="<i8")
    feats = {"id": ("int64", [_id]), "key": ("bytes", [key.encode("utf-8")]),
             "source": ("bytes", [source.tobytes()]),
             "source_length": ("int64", [len(source)]),
             "text": ("bytes", [text.encode("utf-8")]),
             "speaker_id": ("int64", [speaker_id]), "age": ("int64", [age]),
             "gender": ("int64", [gender])}
    if phone is not None:
        phone = np.ascontiguousarray(phone, dtype="<i8")
        feats.update({"phone": ("bytes", [phone.tobytes()]),
                      "phone_length": ("int64", [len(phone)]),
                      "phone_txt": ("bytes", [(phone_txt or "").encode("utf-8")])})
    return encode_example(feats)


def write_preprocessed_vctk_source_data(_id: int, key: str, source: np.ndarray, text: str,
                                        speaker_id: int, age: int, gender: int,
                                        filename: str) -> None:
    write_tfrecords([vctk_source_example(_id, key, source, text, speaker_id, age, gender)],
                    filename)


def parse_preprocessed_vctk_source_data(record: bytes) -> PreprocessedVCTKSourceData:
    """parse_preprocessed_source_data + decode_preprocessed_source_data
    (datasets/vctk/dataset.py:64-96).  ``speaker_id``, ``age`` and ``gender`` are required; the
    phone fields are read when the record has any of them (then all three are required) and are
    None otherwise."""
    ex = decode_example(record)
    phone = phone_length = phone_txt = None
    if any(n in ex for n in ("phone", "phone_length", "phone_txt")):
        phone = np.frombuffer(_scalar(ex, "phone", "bytes"), "<i8").astype(np.int64)
        phone_length = _scalar(ex, "phone_length", "int64")
        phone_txt = _scalar(ex, "phone_txt", "bytes")
    return PreprocessedVCTKSourceData(
        id=_scalar(ex, "id", "int64"), key=_scalar(ex, "key", "bytes"),
        source=np.frombuffer(_scalar(ex, "source", "bytes"), "<i8").astype(np.int64),
        source_length=_scalar(ex, "source_length", "int64"),
        speaker_id=_scalar(ex, "speaker_id", "int64"), age=_scalar(ex, "age", "int64"),
        gender=_scalar(ex, "gender", "int64"), text=_scalar(ex, "text", "bytes"),
        phone=phone, phone_length=phone_length, phone_txt=phone_txt)


# ---------------------------------------------------------------- VQ-code records
def codes_source_example(_id: int, key: str, source: np.ndarray, text: str, speaker_id: int,
                         age: int, gender: int, phone: np.ndarray = None, phone_txt: str = "",
                         lang: str = "EN") -> bytes:
    """preprocess/codes.py:33-49: the VCTK source fields, the three phone fields (always present;
    empty without a phone front end) and ``lang``."""
    phone = np.zeros(0, np.int64) if phone is None else phone
    ex = decode_example(vctk_source_example(_id, key, source, text, speaker_id, age, gender,
                                            phone, phone_txt))
    ex["lang"] = ("bytes", [lang.encode("utf-8")])
    return encode_example(ex)


def write_preprocessed_codes_source_data(_id, key, source, text, speaker_id, age, gender,
                                         filename, phone=None, phone_txt="", lang="EN") -> None:
    write_tfrecords([codes_source_example(_id, key, source, text, speaker_id, age, gender, phone,
                                          phone_txt, lang)], filename)


def parse_preprocessed_codes_source_data(record: bytes) -> PreprocessedVCTKSourceData:
    """datasets/codes/dataset.py:66-97: every field is required, the phone fields included."""
    ex = decode_example(record)
    for name, kind in (("phone", "bytes"), ("phone_length", "int64"), ("phone_txt", "bytes")):
        _scalar(ex, name, kind)
    return parse_preprocessed_vctk_source_data(record)


def one_hot_to_index(codes: np.ndarray, key="") -> np.ndarray:
    """int32 indices of dense one-hot rows [T, C]; a row that is not exactly one 1.0 among zeros
    is a ``ValueError`` naming ``key`` and the row."""
    codes = np.asarray(codes)
    if codes.ndim != 2 or codes.shape[1] < 1:
        raise ValueError(f"code record {key!r}: codes must be [codes_length, codes_width]")
    ok = ((codes == 1).sum(axis=1) == 1) & ((codes != 0).sum(axis=1) == 1)
    if not ok.all():
        raise ValueError(f"code record {key!r}: row {int(np.argmin(ok))} is not one-hot")
    return codes.argmax(axis=1).astype(np.int32)


def index_to_one_hot(index: np.ndarray, width: int) -> np.ndarray:
    """float32 [len(index), width] one-hot rows (preprocess/codes.py:154-157)."""
    index = np.asarray(index, np.int64)
    if index.size and (index.min() < 0 or index.max() >= width):
        bad = int(np.argmax((index < 0) | (index >= width)))
        raise ValueError(f"code {int(index[bad])} at position {bad} is outside 0..{width - 1}")
    out = np.zeros((index.size, int(width)), np.float32)
    out[np.arange(index.size), index] = 1.0
    return out


def code_target_example(_id: int, key: str, code_index: np.ndarray, codes_width: int,
                        compact: bool = False, lang: str = "EN") -> bytes:
    """The code target record.  Dense (preprocess/codes.py:20-30): ``codes`` = raw float32
    [codes_length, codes_width] one-hot bytes; compact: ``code_index`` = raw int32 [codes_length]
    instead.  Both carry ``id, key, lang, codes_length, codes_width``."""
    code_index = np.ascontiguousarray(code_index, dtype="<i4")
    dense = index_to_one_hot(code_index, codes_width)        # also the range check
    feats = {"id": ("int64", [_id]), "key": ("bytes", [key.encode("utf-8")]),
             "lang": ("bytes", [lang.encode("utf-8")])}
    if compact:
        feats["code_index"] = ("bytes", [code_index.tobytes()])
    else:
        feats["codes"] = ("bytes", [dense.astype("<f4").tobytes()])
    feats["codes_length"] = ("int64", [len(code_index)])
    feats["codes_width"] = ("int64", [int(codes_width)])
    return encode_example(feats)


def write_preprocessed_code_data(_id: int, key: str, code_index: np.ndarray, codes_width: int,
                                 filename: str, compact: bool = False, lang: str = "EN") -> None:
    write_tfrecords([code_target_example(_id, key, code_index, codes_width, compact, lang)],
                    filename)


def parse_preprocessed_code_data(record: bytes) -> PreprocessedCodeData:
    """parse_preprocessed_code_data + decode_preprocessed_code_data (utils/tfrecord.py:89-113) for
    both layouts; a dense record is reduced to indices here, on the host."""
    ex = decode_example(record)
    key = _scalar(ex, "key", "bytes")
    name = key.decode("utf-8", errors="replace")
    length = _scalar(ex, "codes_length", "int64")
    width = _scalar(ex, "codes_width", "int64")
    if width < 1 or length < 0:
        raise ValueError(f"code record {name!r}: codes_length {length}, codes_width {width}")
    if "code_index" in ex:
        index = np.frombuffer(_scalar(ex, "code_index", "bytes"), "<i4").astype(np.int32)
        if index.size != length:
            raise ValueError(f"code record {name!r}: {index.size} indices, codes_length {length}")
        if index.size and (index.min() < 0 or index.max() >= width):
            bad = int(np.argmax((index < 0) | (index >= width)))
            raise ValueError(f"code record {name!r}: code {int(index[bad])} at position {bad} is "
                             f"outside 0..{width - 1}")
    else:
        dense = np.frombuffer(_scalar(ex, "codes", "bytes"), "<f4")
        if dense.size != length * width:
            raise ValueError(f"code record {name!r}: {dense.size} floats do not fill "
                             f"[{length}, {width}]")
        index = one_hot_to_index(dense.reshape(length, width), name)
    lang = ex["lang"][1][0] if "lang" in ex and ex["lang"][1] else b""
    return PreprocessedCodeData(id=_scalar(ex, "id", "int64"), key=key, lang=lang,
                                code_index=index, codes_length=length, codes_width=width)


def prediction_result_example(_id: int, key: str, codes: np.ndarray,
                              ground_truth_codes: np.ndarray, text: str,
                              source: np.ndarray) -> bytes:
    """utils/tfrecord.py:144-157 (write_prediction_result's Example; its ``alignments`` and
    ``accent_type`` arguments are not written there either)."""
    codes = np.ascontiguousarray(codes, dtype="<f4")
    truth = np.ascontiguousarray(ground_truth_codes, dtype="<f4")
    source = np.ascontiguousarray(source, dtype="<i8")
    return encode_example({
        "id": ("int64", [_id]), "key": ("bytes", [key.encode("utf-8")]),
        "codes": ("bytes", [codes.tobytes()]),
        "codes_length": ("int64", [codes.shape[0]]),
        "codes_width": ("int64", [codes.shape[1]]),
        "ground_truth_codes": ("bytes", [truth.tobytes()]),
        "ground_truth_codes_length": ("int64", [truth.shape[0]]),
        "text": ("bytes", [text.encode("utf-8")]),
        "source": ("bytes", [source.tobytes()]),
        "source_length": ("int64", [source.shape[0]])})


def write_prediction_result(_id, key, codes, ground_truth_codes, text, source, filename) -> None:
    write_tfrecords([prediction_result_example(_id, key, codes, ground_truth_codes, text,
                                               source)], filename)


def parse_prediction_result(record: bytes) -> CodePredictionResult:
    """postprocess_vqcodes.py:15-49, with the code rows read as the float32 they were written
    as (the script reads them as int32 words, which has the same argmax)."""
    ex = decode_example(record)
    n, w = _scalar(ex, "codes_length", "int64"), _scalar(ex, "codes_width", "int64")
    gn = _scalar(ex, "ground_truth_codes_length", "int64")
    return CodePredictionResult(
        id=_scalar(ex, "id", "int64"), key=_scalar(ex, "key", "bytes"),
        codes=np.frombuffer(_scalar(ex, "codes", "bytes"), "<f4").reshape(n, w),
        codes_length=n, codes_width=w,
        ground_truth_codes=np.frombuffer(_scalar(ex, "ground_truth_codes", "bytes"),
                                         "<f4").reshape(gn, w),
        ground_truth_codes_length=gn, text=_scalar(ex, "text", "bytes"),
        source=np.frombuffer(_scalar(ex, "source", "bytes"), "<i8").astype(np.int64),
        source_length=_scalar(ex, "source_length", "int64"))
