"""LJSpeech preprocessing end to end on the GPU: three synthetic wavs and a metadata.csv ->
source / target TFRecords + hparams.json -> the existing dataset pipeline."""
import json
import wave

import numpy as np
import pytest

import audio_ref as R

pytestmark = pytest.mark.gpu

SR = 22050
KEYS = ["LJ001-0001", "LJ001-0002", "LJ001-0003"]
TEXTS = ["Printing, in the only sense", "With which we are  at present concerned", "Differs (from) most"]
SECONDS = [0.5, 0.3, 0.4]


@pytest.fixture(scope="module")
def corpus(tmp_path_factory, cuda):
    from sat_amd import hparams as H, preprocess as P
    root = tmp_path_factory.mktemp("ljs")
    in_dir, out_dir = root / "in", root / "out"
    (in_dir / "wavs").mkdir(parents=True)
    pcm = []
    for i, (key, sec) in enumerate(zip(KEYS, SECONDS)):
        y = R.make_signal(int(sec * SR), SR, seed=10 + i)
        q = np.clip(np.rint(y.astype(np.float64) * 32768.0), -32768, 32767).astype("<i2")
        with wave.open(str(in_dir / "wavs" / f"{key}.wav"), "wb") as f:
            f.setnchannels(1)
            f.setsampwidth(2)
            f.setframerate(SR)
            f.writeframes(q.tobytes())
        pcm.append(q.astype(np.float32) / np.float32(32768.0))
    (in_dir / "metadata.csv").write_text(
        "".join(f"{k}|raw {t}|{t}\n" for k, t in zip(KEYS, TEXTS)), encoding="utf-8")
    hp = H.ljspeech_hparams()
    keys = P.LJSpeech(str(in_dir), str(out_dir), hp, device=cuda).run()
    return dict(out_dir=out_dir, pcm=pcm, keys=keys, hp=hp)


def _targets(corpus):
    from sat_amd import tfrecord as T
    out = []
    for key in KEYS:
        rec, = list(T.read_tfrecords(str(corpus["out_dir"] / f"{key}.target.tfrecord")))
        out.append(T.parse_preprocessed_mel_data(rec))
    return out


def test_source_records(corpus):
    from sat_amd import preprocess as P, tfrecord as T
    assert corpus["keys"] == KEYS
    assert (corpus["out_dir"] / "list.csv").read_text().split() == KEYS
    for i, (key, text) in enumerate(zip(KEYS, TEXTS)):
        rec, = list(T.read_tfrecords(str(corpus["out_dir"] / f"{key}.source.tfrecord")))
        s = T.parse_preprocessed_source_data(rec)
        clean = " ".join(text.lower().split())
        assert (s.id, s.key, s.text) == (i, key.encode(), clean.encode())
        assert s.source_length == len(clean) and s.source.dtype == np.int64
        assert P.sequence_to_text(s.source) == clean
        assert s.source.min() >= 1 and s.source.max() <= 70


def test_target_records_against_float64(corpus):
    basis = R.cached_basis(SR, 2048, 80)
    for i, (t, y) in enumerate(zip(_targets(corpus), corpus["pcm"])):
        frames = 1 + len(y) // 275
        assert (t.id, t.key, t.target_length, t.mel_width) == (i, KEYS[i].encode(), frames, 80)
        assert t.mel.shape == (frames, 80) and t.mel.dtype == np.float32
        db64, mag64 = R.melspectrogram(y, 2048, 275, 1102, basis)
        assert R.band_values(mag64, basis).min() >= 1e-3        # clear of the amplitude floor
        db32, _ = R.pipeline32(y, 2048, 275, 1102, basis)
        e32 = float(np.abs(db32 - db64).max())
        err = float(np.abs(t.mel - db64).max())
        print(f"utterance {i}: |err| {err:.3e} dB, e32 {e32:.3e} dB, ratio {err / e32:.2f}")
        assert err <= 8 * e32


def test_hparams_json_statistics(corpus):
    from sat_amd import hparams as H, preprocess as P
    text = (corpus["out_dir"] / "hparams.json").read_text()
    obj = json.loads(text)
    assert tuple(obj) == P.HPARAMS_JSON_KEYS
    assert (obj["num_mels"], obj["num_freq"], obj["sample_rate"]) == (80, 1025, SR)
    assert (obj["frame_length_ms"], obj["frame_shift_ms"]) == (50.0, 12.5)
    allm = np.concatenate([t.mel for t in _targets(corpus)]).astype(np.float64)
    assert np.allclose(obj["average_mel_level_db"], allm.mean(0), rtol=1e-5, atol=0)
    assert np.allclose(obj["stddev_mel_level_db"], allm.std(0), rtol=1e-5, atol=0)
    assert np.array_equal(np.array(obj["min_mel_level_db"]), allm.min(0))
    H.HParams(**H.default_values()).parse_json(text)


def test_dataset_pipeline_reads_the_directory(corpus):
    """hparams.parse_json of the written file, then sat_amd.datasets as it is: one batch's mel is
    (stored mel - average) / stddev between the silence frames."""
    from sat_amd import datasets as D, hparams as H
    hp = H.ljspeech_hparams().parse_json((corpus["out_dir"] / "hparams.json").read_text())
    src = [str(corpus["out_dir"] / f"{k}.source.tfrecord") for k in KEYS]
    tgt = [str(corpus["out_dir"] / f"{k}.target.tfrecord") for k in KEYS]
    ds = D.create_from_tfrecord_files(src, tgt, hp, cycle_length=1)
    (s, t), = list(ds.prepare_and_zip().group_by_batch(batch_size=3))
    assert list(s.key) == [k.encode() for k in KEYS] and list(t.id) == [0, 1, 2]
    avg = np.asarray(hp.average_mel_level_db, np.float32)
    std = np.asarray(hp.stddev_mel_level_db, np.float32)
    r = hp.outputs_per_step
    for b, ref in enumerate(_targets(corpus)):
        want = (ref.mel - avg) / std
        assert np.array_equal(t.mel[b, r:r + len(want)], want)
        assert abs(float(want.mean())) < 3.0 and np.isfinite(want).all()
