"""The VQ-code corpus on the host: preprocess codes -> records -> codes dataset, against the numpy
restatement (codes_ref.py) over the hand-written corpus under tests/golden/codes.  Everything
here is integers, zeros and ones: comparisons are exact."""
import os

import numpy as np
import pytest

import codes_ref as CR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "codes")
C = 16
NAMES = ("codes.dataset.DatasetSource", "datasets.codes.dataset.DatasetSource")


def _hp(**kw):
    from sat_amd import hparams
    return hparams.codes_hparams(C, **dict(dict(source="char", phoneme="none"), **kw))


def _preprocess(out, version=0, compact=False):
    from sat_amd import preprocess
    corpus = preprocess.Codes(GOLDEN, str(out), _hp(), C, version=version, compact=compact)
    return corpus, corpus.run()


def _files(out, keys, ext):
    return [os.path.join(str(out), f"{k}.{ext}.tfrecord") for k in keys]


@pytest.mark.parametrize("name", NAMES)
def test_factory_accepts_the_codes_names(name):
    from sat_amd import datasets as D
    hp = _hp(dataset=name)
    assert isinstance(D.dataset_factory([], [], hp), D.CodesDatasetSource)
    assert isinstance(D.create_from_tfrecord_files([], [], hp), D.CodesDatasetSource)


def test_reference_default_dataset_is_accepted():
    from sat_amd import datasets as D, hparams
    hp = hparams.create_hparams()                 # hparams.py's own default names the codes corpus
    assert hp.dataset == NAMES[0] and hp.outputs_per_step == 1
    assert isinstance(D.dataset_factory([], [], hp), D.CodesDatasetSource)


def test_codes_hparams():
    from sat_amd import hparams
    hp = hparams.codes_hparams(256)
    assert (hp.dataset, hp.num_mels, hp.outputs_per_step, hp.n_feed_frame) == (NAMES[0], 256, 1, 1)
    assert hparams.codes_hparams(8, max_iters=20).max_iters == 20
    assert hparams.ljspeech_hparams().dataset == "ljspeech.dataset.DatasetSource"
    assert hparams.vctk_hparams().dataset == "vctk.dataset.DatasetSource"


@pytest.mark.parametrize("r", (2, 3))
def test_outputs_per_step_other_than_one_is_refused(r):
    from sat_amd import datasets as D
    with pytest.raises(ValueError, match="outputs_per_step"):
        D.dataset_factory([], [], _hp(outputs_per_step=r))


@pytest.mark.parametrize("compact", (False, True))
@pytest.mark.parametrize("version", (0, 1, 2))
def test_preprocess_records_parse_back(tmp_path, version, compact):
    from sat_amd import tfrecord as R
    want = CR.read_corpus(GOLDEN, version)
    corpus, keys = _preprocess(tmp_path, version, compact)
    assert keys == [w[0] for w in want]
    with open(tmp_path / "list.csv") as f:
        assert [l.strip() for l in f if l.strip()] == keys
    for i, (key, spk, text, index) in enumerate(want):
        (rec,) = R.read_tfrecords(_files(tmp_path, [key], "target")[0])
        ex = R.decode_example(rec)
        assert ("code_index" in ex, "codes" in ex) == (compact, not compact)
        if not compact:              # the reference's layout: raw float32 [length, width] one-hot
            dense = np.frombuffer(ex["codes"][1][0], "<f4").reshape(len(index), C)
            assert np.array_equal(dense, CR.one_hot(index, C))
        t = R.parse_preprocessed_code_data(rec)
        assert t.key.decode() == key and (t.codes_length, t.codes_width) == (len(index), C)
        assert t.code_index.dtype == np.int32 and np.array_equal(t.code_index, index)
        assert t.lang == b"EN"
        (rec,) = R.read_tfrecords(_files(tmp_path, [key], "source")[0])
        s = R.parse_preprocessed_codes_source_data(rec)
        assert (s.key.decode(), s.speaker_id, s.text.decode()) == (key, spk, text.lower())
        assert s.id == t.id and s.source_length == len(text) and s.phone_length == 0
        assert s.gender == (0 if spk == 225 else 1) and s.age == (23 if spk == 225 else 22)
    # version 0 reaches both ends of the code range
    if version == 0:
        allc = np.concatenate([w[3] for w in want])
        assert allc.min() == 0 and allc.max() == C - 1


def test_tabless_line_is_skipped_and_key_ending_in_t_survives(tmp_path, capsys):
    corpus, keys = _preprocess(tmp_path)
    assert "p226_001" not in keys and corpus.skipped == ["p226_001"]
    assert "p226_001" in capsys.readouterr().err
    assert not os.path.exists(tmp_path / "p226_001.target.tfrecord")
    assert not os.path.exists(tmp_path / "p226_001.source.tfrecord")
    assert "p225_test" in keys and "p225_test".strip(".txt") != "p225_test"
    assert not any(k.startswith("p315") for k in keys)


def test_only_flags_and_refusals(tmp_path):
    from sat_amd import hparams, preprocess
    rc = preprocess.main(["codes", GOLDEN, str(tmp_path), "--num-codes", str(C), "--compact",
                          "--target-only", "--hparams", "phoneme=none"])
    assert rc == 0
    assert os.path.exists(tmp_path / "p225_001.target.tfrecord")
    assert not os.path.exists(tmp_path / "p225_001.source.tfrecord")
    with pytest.raises(ValueError, match="flite"):
        preprocess.Codes(GOLDEN, str(tmp_path), hparams.codes_hparams(C), C)
    with pytest.raises(ValueError, match="version"):
        preprocess.Codes(GOLDEN, str(tmp_path), _hp(), C, version=3)
    with pytest.raises(ValueError, match="outside"):
        preprocess.Codes(GOLDEN, str(tmp_path), _hp(), 15).run()


def test_dense_record_with_a_row_that_is_not_one_hot_is_refused():
    from sat_amd import tfrecord as R
    good = CR.one_hot(np.array([1, 0, 3]), 4)
    for row in ([0, 0, 0, 0], [0, 1, 1, 0], [0, 0.5, 0, 0], [0, 1, 0, 1e-3], [2, 0, 0, 0]):
        dense = good.copy()
        dense[1] = row
        rec = R.encode_example({"id": ("int64", [7]), "key": ("bytes", [b"p225_bad"]),
                                "lang": ("bytes", [b"EN"]),
                                "codes": ("bytes", [dense.astype("<f4").tobytes()]),
                                "codes_length": ("int64", [3]), "codes_width": ("int64", [4])})
        with pytest.raises(ValueError, match="p225_bad.*row 1"):
            R.parse_preprocessed_code_data(rec)
    with pytest.raises(ValueError, match="p225_bad.*position 2"):
        R.parse_preprocessed_code_data(R.encode_example({
            "id": ("int64", [7]), "key": ("bytes", [b"p225_bad"]),
            "code_index": ("bytes", [np.array([0, 3, 4], "<i4").tobytes()]),
            "codes_length": ("int64", [3]), "codes_width": ("int64", [4])}))


@pytest.mark.parametrize("compact", (False, True))
def test_dataset_batches(tmp_path, compact):
    from sat_amd import datasets as D
    want = CR.read_corpus(GOLDEN)
    _, keys = _preprocess(tmp_path, compact=compact)
    hp = _hp(use_speaker_embedding=True)
    ds = D.create_from_tfrecord_files(_files(tmp_path, keys, "source"),
                                      _files(tmp_path, keys, "target"), hp, cycle_length=1)
    batches = list(ds.prepare_and_zip().filter_by_max_output_length().group_by_batch(2))
    assert [len(s.id) for s, _ in batches] == [2, 2, 1]
    n = 0
    for s, t in batches:
        assert isinstance(s, D.VCTKSourceData) and isinstance(t, D.CodeBatch)
        B = len(s.id)
        assert t.code_index.dtype == np.int32 and t.offsets.dtype == np.int64
        assert t.offsets[0] == 0 and t.offsets[-1] == len(t.code_index) and t.codes_width == C
        for b in range(B):
            key, spk, text, index = want[n]
            assert s.key[b].decode() == key and s.speaker_id[b] == spk
            assert s.source_length[b] == len(text) and np.all(s.source[b, len(text):] == 0)
            assert np.array_equal(t.code_index[t.offsets[b]:t.offsets[b + 1]], index)
            assert t.target_length[b] == len(index) == t.codes_length[b]
            n += 1
    assert n == len(want)
    # filter_by_max_output_length: target_length <= max_iters (r = 1)
    hp.set_hparam("max_iters", 10)
    kept = list(ds.prepare_and_zip().filter_by_max_output_length())
    assert [e[0].key.decode() for e in kept] == [w[0] for w in want if len(w[3]) <= 10]
    # merge_target_to_source carries the indices for prediction
    f, t = next(iter(ds.prepare_and_zip().group_by_batch(1).merge_target_to_source()))
    assert np.array_equal(f.code_index, want[0][3]) and f.speaker_id[0] == 225
    # repeat / shuffle / prefetch keep the element set
    it = iter(ds.prepare_and_zip().repeat(2).shuffle(3, seed=1).group_by_batch(2).prefetch(2))
    assert sum(len(s.id) for s, _ in it) == 2 * len(want)


def test_phone_source_needs_phones(tmp_path):
    from sat_amd import datasets as D
    _, keys = _preprocess(tmp_path)
    ds = D.create_from_tfrecord_files(_files(tmp_path, keys, "source"),
                                      _files(tmp_path, keys, "target"), _hp(source="phone"))
    with pytest.raises(ValueError, match="source='char'"):
        next(iter(ds.prepare_and_zip()))


def test_prediction_record_round_trip():
    from sat_amd import tfrecord as R
    codes, truth = CR.one_hot(np.array([3, 0, 2]), 4), CR.one_hot(np.array([1, 3]), 4)
    rec = R.prediction_result_example(5, "p225_001", codes, truth, "hi.", np.array([8, 9, 1]))
    ex = R.decode_example(rec)
    assert list(ex) == ["id", "key", "codes", "codes_length", "codes_width",
                        "ground_truth_codes", "ground_truth_codes_length", "text", "source",
                        "source_length"]
    p = R.parse_prediction_result(rec)
    assert np.array_equal(p.codes, codes) and np.array_equal(p.ground_truth_codes, truth)
    assert (p.id, p.key, p.text, p.source_length) == (5, b"p225_001", b"hi.", 3)
    assert np.array_equal(p.source, [8, 9, 1])


def test_header_and_binding_agree_with_the_codes_entries():
    from sat_amd import _lib
    assert _lib.header_symbols() == _lib.bound_symbols()
    assert {"sat_codes_batch", "sat_codes_argmax"} <= _lib.header_symbols()
