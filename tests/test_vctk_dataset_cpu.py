"""The VCTK data path without a GPU: the source record of preprocess/vctk.py:31-44 and its parser
(datasets/vctk/dataset.py:64-96), the VCTK DatasetSource through the shared zipped / batched
classes (:136-150, 261-318, 341-357), the factory names, and the corpus listing of
preprocess/vctk.py:91-127."""
import numpy as np
import pytest

import _sat_path

_sat_path.load()
from sat_amd import datasets as D  # noqa: E402
from sat_amd import hparams  # noqa: E402
from sat_amd import tfrecord as R  # noqa: E402

# (key, text ids, speaker, age, gender, frames)
UTTS = [("p225_001", [3, 4, 5], 225, 23, 0, 7), ("p225_002", [9], 225, 23, 0, 4),
        ("p226_001", [1, 2, 3, 4, 5, 6], 226, 22, 1, 9), ("p226_002", [7, 7], 226, 22, 1, 5),
        ("p227_001", [8, 9, 10, 11], 227, 38, 1, 6), ("p228_001", [12, 13], 228, 22, 0, 8)]


def _hp(**extra):
    return hparams.vctk_hparams(num_mels=3, average_mel_level_db=[1.0, 2.0, 3.0],
                                stddev_mel_level_db=[2.0, 4.0, 8.0], source="char", **extra)


def _mel(i, frames):
    return (np.arange(frames * 3, dtype=np.float32).reshape(frames, 3) - 5.0) * (i + 1)


def _write(tmp_path, phone=False):
    src, tgt = [], []
    for i, (key, ids, spk, age, gender, frames) in enumerate(UTTS):
        s, t = str(tmp_path / f"{key}.source.tfrecord"), str(tmp_path / f"{key}.target.tfrecord")
        if phone:
            ex = R.vctk_source_example(i, key, np.array(ids), "text %d" % i, spk, age, gender,
                                       phone=np.array(ids[::-1] + [40]), phone_txt="ph %d" % i)
            R.write_tfrecords([ex], s)
        else:
            R.write_preprocessed_vctk_source_data(i, key, np.array(ids), "text %d" % i, spk, age,
                                                  gender, s)
        R.write_preprocessed_target_data(i, key, _mel(i, frames), t)
        src.append(s)
        tgt.append(t)
    return src, tgt


def test_source_record_round_trip():
    ex = R.vctk_source_example(5, "p225_001", np.array([3, 1, 2]), "abc", 225, 23, 0)
    assert list(R.decode_example(ex)) == ["id", "key", "source", "source_length", "text",
                                          "speaker_id", "age", "gender"]
    s = R.parse_preprocessed_vctk_source_data(ex)
    assert (s.id, s.key, s.text, s.source_length) == (5, b"p225_001", b"abc", 3)
    assert s.source.dtype == np.int64 and s.source.tolist() == [3, 1, 2]
    assert (s.speaker_id, s.age, s.gender) == (225, 23, 0)
    assert s.phone is None and s.phone_length is None and s.phone_txt is None
    ex = R.vctk_source_example(5, "p225_001", np.array([3, 1, 2]), "abc", 225, 23, 1,
                               phone=np.array([9, 8]), phone_txt="ax b")
    s = R.parse_preprocessed_vctk_source_data(ex)
    assert s.phone.tolist() == [9, 8] and (s.phone_length, s.phone_txt) == (2, b"ax b")
    assert s.gender == 1 and s.source.tolist() == [3, 1, 2]


def test_record_without_speaker_id_raises():
    """An LJSpeech source record is no VCTK one: speaker_id is a required feature."""
    lj = R.source_example(0, "LJ001-0001", np.array([1, 2]), "ab")
    with pytest.raises(ValueError, match="speaker_id"):
        R.parse_preprocessed_vctk_source_data(lj)
    # and the LJSpeech parser still reads what it read
    assert R.parse_preprocessed_source_data(lj).text == b"ab"
    # a record with only some of the phone fields is malformed
    ex = R.encode_example(dict(R.decode_example(
        R.vctk_source_example(0, "k", np.array([1]), "a", 225, 23, 0)), phone=("bytes", [b""])))
    with pytest.raises(ValueError, match="phone_length"):
        R.parse_preprocessed_vctk_source_data(ex)


def test_factory_names():
    hp = _hp()
    assert hp.dataset == "vctk.dataset.DatasetSource"
    for name in ("vctk.dataset.DatasetSource", "datasets.vctk.dataset.DatasetSource"):
        hp.dataset = name
        assert type(D.dataset_factory([], [], hp)) is D.VCTKDatasetSource
        assert type(D.create_from_tfrecord_files([], [], hp)) is D.VCTKDatasetSource
    assert D.vctk.DatasetSource is D.VCTKDatasetSource
    assert D.vctk.SourceData._fields == ("id", "key", "source", "source_length", "speaker_id",
                                         "age", "gender", "text")
    assert D.vctk.SourceDataForPrediction._fields == D.vctk.SourceData._fields + (
        "mel", "mel_width", "target_length")
    hp.dataset = "ljspeech.dataset.DatasetSource"
    assert type(D.dataset_factory([], [], hp)) is D.DatasetSource
    hp.dataset = "codes.dataset.DatasetSource"
    for make in (D.dataset_factory, D.create_from_tfrecord_files):
        with pytest.raises(ValueError, match="Unknown dataset"):
            make([], [], hp)


def test_six_utterances_in_batches_of_four(tmp_path):
    hp = _hp()
    src, tgt = _write(tmp_path)
    ds = D.create_from_tfrecord_files(src, tgt, hp, cycle_length=1)
    batches = list(ds.prepare_and_zip().group_by_batch(4))
    assert [len(s.id) for s, _ in batches] == [4, 2]
    r = hp.outputs_per_step
    row = 0
    for s, t in batches:
        assert isinstance(s, D.VCTKSourceData) and isinstance(t, D.MelData)
        n = len(s.id)
        utts = UTTS[row:row + n]
        assert s.id.tolist() == list(range(row, row + n)) and t.id.tolist() == s.id.tolist()
        assert list(s.key) == [u[0].encode() for u in utts]
        assert s.speaker_id.tolist() == [u[2] for u in utts]
        assert s.age.tolist() == [u[3] for u in utts]
        assert s.gender.tolist() == [u[4] for u in utts]
        for a in (s.speaker_id, s.age, s.gender, s.source, s.source_length):
            assert a.dtype == np.int64
        assert s.source_length.tolist() == [len(u[1]) for u in utts]
        width = max(len(u[1]) for u in utts)
        assert s.source.shape == (n, width)
        for b, u in enumerate(utts):
            assert s.source[b].tolist() == u[1] + [0] * (width - len(u[1]))
            assert s.text[b] == b"text %d" % (row + b)
            # the shared target preparation: normalised mel between r silence frames
            want = (_mel(row + b, u[5]) - np.float32([1, 2, 3])) / np.float32([2, 4, 8])
            assert np.array_equal(t.mel[b, r:r + u[5]], want)
            L = u[5] + 2 * r
            assert t.target_length[b] == (L if L % r == 0 else (L // r + 1) * r)
        row += n


def test_merge_target_to_source(tmp_path):
    hp = _hp()
    src, tgt = _write(tmp_path)
    ds = D.create_from_tfrecord_files(src, tgt, hp, cycle_length=1)
    batched = ds.prepare_and_zip().group_by_batch(4)
    plain = list(batched)
    merged = list(batched.merge_target_to_source())
    assert len(merged) == 2
    for (f, t), (s, t0) in zip(merged, plain):
        assert isinstance(f, D.VCTKSourceDataForPrediction)
        assert f._fields == D.VCTKSourceData._fields + ("mel", "mel_width", "target_length")
        for name in D.VCTKSourceData._fields:
            assert np.array_equal(getattr(f, name), getattr(s, name))
        assert np.array_equal(f.mel, t0.mel) and np.array_equal(f.target_length, t0.target_length)
        assert np.array_equal(f.mel_width, t0.mel_width) and np.array_equal(t.mel, t0.mel)


def test_ljspeech_batches_keep_their_types(tmp_path):
    """The shared batching still gives LJSpeech its own record types."""
    hp = hparams.ljspeech_hparams(num_mels=3, average_mel_level_db=[0.0] * 3,
                                  stddev_mel_level_db=[1.0] * 3)
    s, t = str(tmp_path / "a.source.tfrecord"), str(tmp_path / "a.target.tfrecord")
    R.write_preprocessed_source_data(0, "a", np.array([1, 2]), "ab", s)
    R.write_preprocessed_target_data(0, "a", _mel(0, 4), t)
    batched = D.create_from_tfrecord_files([s], [t], hp).prepare_and_zip().group_by_batch(2)
    (f, _), = list(batched)
    assert type(f) is D.SourceData and not hasattr(f, "speaker_id")
    (p, _), = list(batched.merge_target_to_source())
    assert type(p) is D.SourceDataForPrediction


def test_phone_source_selects_the_phone_fields(tmp_path):
    src, tgt = _write(tmp_path, phone=True)
    hp = _hp()
    hp.source = "phone"
    (s, _), _ = list(D.create_from_tfrecord_files(src, tgt, hp, cycle_length=1)
                     .prepare_and_zip().group_by_batch(4))
    assert s.source[0].tolist()[:4] == [5, 4, 3, 40] and s.source_length.tolist() == [4, 2, 7, 3]
    assert s.text[1] == b"ph 1" and s.speaker_id.tolist() == [225, 225, 226, 226]
    hp.source = "char"                                  # any other value: the characters
    (s, _), _ = list(D.create_from_tfrecord_files(src, tgt, hp, cycle_length=1)
                     .prepare_and_zip().group_by_batch(4))
    assert s.source[0].tolist()[:3] == [3, 4, 5] and s.text[1] == b"text 1"


def test_phone_source_without_phone_fields_names_the_field(tmp_path):
    src, tgt = _write(tmp_path)
    hp = _hp()
    hp.source = "phone"
    ds = D.create_from_tfrecord_files(src, tgt, hp, cycle_length=1)
    with pytest.raises(ValueError, match="'phone'"):
        list(ds.prepare_and_zip())


# ---------------------------------------------------------------- corpus listing
def _tree(root, speakers, files):
    root.mkdir(parents=True, exist_ok=True)
    (root / "speaker-info.txt").write_text(
        "ID  AGE  GENDER  ACCENTS  REGION\n" + "".join(
            f"{i}  {age}  {g}    English    Somewhere\n" for i, age, g in speakers))
    for sub, name in files:
        p = root / sub / name[:4] / name
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_text("Please call Stella.\nsecond line\n")


def test_vctk_listing(tmp_path):
    from sat_amd import preprocess as P
    _tree(tmp_path, [(226, 22, "M"), (225, 23, "F"), (315, 18, "M")],
          [("wav48", "p225_002.wav"), ("wav48", "p225_001.wav"), ("wav48", "p226_001.wav"),
           ("txt", "p225_001.txt"), ("txt", "p225_002.txt"), ("txt", "p226_001.txt"),
           ("txt", "p226_notes.md")])
    v = P.VCTK(str(tmp_path), str(tmp_path / "out"), hparams.vctk_hparams())
    infos = list(v._load_speaker_info())
    assert infos == [P.SpeakerInfo(226, 22, 1), P.SpeakerInfo(225, 23, 0)]     # 315 is left out
    recs = v.list_files()
    # ids in enumeration order: speakers as listed, files sorted
    assert [(r.id, r.key) for r in recs] == [(0, "p226_001"), (1, "p225_001"), (2, "p225_002")]
    assert recs[1].speaker_info == P.SpeakerInfo(225, 23, 0)
    assert recs[2].wav_path.endswith("wav48/p225/p225_002.wav")
    assert recs[2].txt_path.endswith("txt/p225/p225_002.txt")


def test_vctk_listing_mismatch_is_an_error(tmp_path):
    from sat_amd import preprocess as P
    _tree(tmp_path, [(225, 23, "F")],
          [("wav48", "p225_001.wav"), ("wav48", "p225_003.wav"),
           ("txt", "p225_001.txt"), ("txt", "p225_002.txt")])
    with pytest.raises(ValueError, match="p225_003"):
        P.VCTK(str(tmp_path), str(tmp_path / "out"), hparams.vctk_hparams()).list_files()


def test_vctk_091_is_refused():
    from sat_amd import preprocess as P
    with pytest.raises(ValueError, match="flite"):
        P.VCTK("in", "out", hparams.vctk_hparams(), version="0.91")


def test_vctk_source_only_writes_speaker_fields(tmp_path):
    """--source-only needs no GPU: first line of the txt file, cleaned, with the speaker info."""
    from sat_amd import preprocess as P
    _tree(tmp_path / "in", [(225, 23, "F"), (226, 22, "M")],
          [("wav48", "p225_001.wav"), ("wav48", "p226_001.wav"),
           ("txt", "p225_001.txt"), ("txt", "p226_001.txt")])
    out = tmp_path / "out"
    keys = P.VCTK(str(tmp_path / "in"), str(out), hparams.vctk_hparams()).run(process_target=False)
    assert keys == ["p225_001", "p226_001"] and (out / "list.csv").read_text().split() == keys
    assert not (out / "hparams.json").exists()
    rec, = list(R.read_tfrecords(str(out / "p226_001.source.tfrecord")))
    s = R.parse_preprocessed_vctk_source_data(rec)
    assert (s.id, s.key, s.text) == (1, b"p226_001", b"please call stella.")
    assert (s.speaker_id, s.age, s.gender) == (226, 22, 1)
    assert P.sequence_to_text(s.source) == "please call stella."
