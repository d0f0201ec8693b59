"""VCTK preprocessing end to end on the GPU: a synthetic VCTK 0.8 tree (two speakers, three
utterances that survive the trim, one that does not, and a speaker-info entry for the absent
speaker 315) -> trim + mel in place -> source / target TFRecords, hparams.json, list.csv -> the
VCTK dataset pipeline -> one model_fn TRAIN step.

Each target record is held to the float64 mel (tests/audio_ref.py) of the waveform trimmed by the
float64 restatement (tests/trim_ref.py), within 8 x e32 -- the rule of
tests/test_audio_gpu.py::test_melspec_against_float64."""
import contextlib
import io
import json
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

import audio_ref as R
import trim_ref as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 48000
N_FFT, HOP, WIN = 4096, 600, 2400
TRIM = (1024, 256, 10)                      # vctk_hparams: trim_top_db 10, frames of 1024 / 256
# key -> (speaker, signal, first line of the transcript)
UTTS = {"p225_001": (225, (24000, 6000, 18000, 5), "Please call Stella."),
        "p225_002": (225, (5000, 1000, 1300, 4), "Too short to frame."),      # 1024 after the trim
        "p225_003": (225, (20001, 0, 9000, 6), "Ask her to bring  these things"),
        "p226_001": (226, (30000, 12000, 30000, 7), "Six spoons of fresh snow peas")}
KEPT = ["p225_001", "p225_003", "p226_001"]
IDS = {"p225_001": 0, "p225_003": 2, "p226_001": 3}                            # enumeration order
SPEAKERS = {225: (23, 0), 226: (22, 1)}

_SIG = {}


def _signal(case):
    """trim_ref's signal over a 4e-3 N(0, 1) floor (on 16-bit steps), so that every mel band of
    the trimmed utterances stays 100 x clear of the amplitude floor and the clamp decides
    nothing in the comparison."""
    if case not in _SIG:
        y = T.signal(case).astype(np.float64)
        y = y + 4e-3 * np.random.default_rng(100 + case[3]).standard_normal(case[0])
        _SIG[case] = (np.rint(y * 32768.0) / 32768.0).astype(np.float32)
    return _SIG[case]


@pytest.fixture(scope="module")
def corpus(tmp_path_factory, cuda):
    from sat_amd import hparams as H, preprocess as P
    root = tmp_path_factory.mktemp("vctk")
    in_dir, out_dir = root / "in", root / "out"
    in_dir.mkdir()
    (in_dir / "speaker-info.txt").write_text(
        "ID  AGE  GENDER  ACCENTS  REGION\n225  23  F    English    Southern  England\n"
        "226  22  M    English    Surrey\n315  18  M    American  New  England\n")
    pcm = {}
    for key, (spk, case, text) in UTTS.items():
        for sub in ("wav48", "txt"):
            (in_dir / sub / f"p{spk}").mkdir(parents=True, exist_ok=True)
        y = _signal(case)                                    # already on 16-bit steps
        q = np.rint(y.astype(np.float64) * 32768.0).astype("<i2")
        with wave.open(str(in_dir / "wav48" / f"p{spk}" / f"{key}.wav"), "wb") as f:
            f.setnchannels(1)
            f.setsampwidth(2)
            f.setframerate(SR)
            f.writeframes(q.tobytes())
        (in_dir / "txt" / f"p{spk}" / f"{key}.txt").write_text(text + "\nnot read\n")
        pcm[key] = q.astype(np.float32) / np.float32(32768.0)
    hp = H.vctk_hparams()
    err = io.StringIO()
    with contextlib.redirect_stderr(err):
        keys = P.VCTK(str(in_dir), str(out_dir), hp, device=cuda).run()
    return dict(in_dir=in_dir, out_dir=out_dir, root=root, pcm=pcm, keys=keys, hp=hp,
                stderr=err.getvalue())


def _targets(out_dir):
    from sat_amd import tfrecord as TF
    out = {}
    for key in KEPT:
        rec, = list(TF.read_tfrecords(str(out_dir / f"{key}.target.tfrecord")))
        out[key] = TF.parse_preprocessed_mel_data(rec)
    return out


def test_too_short_utterance_is_skipped_with_a_warning(corpus):
    assert T.trim_bounds(_signal(UTTS["p225_002"][1]), *TRIM) == (768, 1792)   # 1024 <= 2048
    assert corpus["keys"] == KEPT
    assert (corpus["out_dir"] / "list.csv").read_text().split() == KEPT
    assert "p225_002" in corpus["stderr"] and "warning" in corpus["stderr"]
    assert not any(k in corpus["stderr"] for k in KEPT)
    written = sorted(p.name for p in corpus["out_dir"].iterdir())
    assert written == sorted([f"{k}.{s}.tfrecord" for k in KEPT for s in ("source", "target")]
                             + ["hparams.json", "list.csv"])


def test_source_records_carry_the_speaker(corpus):
    from sat_amd import preprocess as P, tfrecord as TF
    for key in KEPT:
        spk, _, text = UTTS[key]
        rec, = list(TF.read_tfrecords(str(corpus["out_dir"] / f"{key}.source.tfrecord")))
        s = TF.parse_preprocessed_vctk_source_data(rec)
        clean = " ".join(text.lower().split())
        assert (s.id, s.key, s.text) == (IDS[key], key.encode(), clean.encode())
        assert (s.speaker_id, s.age, s.gender) == (spk,) + SPEAKERS[spk]
        assert s.source_length == len(clean) and P.sequence_to_text(s.source) == clean
        assert s.phone is None


def test_target_records_against_float64_of_the_reference_trim(corpus):
    basis = R.cached_basis(SR, N_FFT, 80)
    for key, t in _targets(corpus["out_dir"]).items():
        y = corpus["pcm"][key]
        assert np.array_equal(y, _signal(UTTS[key][1]))
        assert T.margin_db(y, *TRIM) >= T.GUARD_DB          # the exact trim is a fair demand
        s, e = T.trim_bounds(y, *TRIM)
        assert e - s > N_FFT // 2
        frames = 1 + (e - s) // HOP
        assert (t.id, t.key, t.target_length, t.mel_width) == (IDS[key], key.encode(), frames, 80)
        assert t.mel.shape == (frames, 80) and t.mel.dtype == np.float32
        db64, mag64 = R.melspectrogram(y[s:e], N_FFT, HOP, WIN, basis)
        assert R.band_values(mag64, basis).min() >= 100 * R.AMP_FLOOR   # clear of the clamp
        db32, _ = R.pipeline32(y[s:e], N_FFT, HOP, WIN, basis)
        e32 = float(np.abs(db32 - db64).max())
        err = float(np.abs(t.mel - db64).max())
        print(f"{key}: trim ({s}, {e}), |err| {err:.3e} dB, e32 {e32:.3e} dB, "
              f"ratio {err / e32:.2f}")
        assert err <= 8 * e32


def test_hparams_json_statistics(corpus):
    from sat_amd import hparams as H, preprocess as P
    text = (corpus["out_dir"] / "hparams.json").read_text()
    obj = json.loads(text)
    assert tuple(obj) == P.HPARAMS_JSON_KEYS
    assert (obj["num_mels"], obj["num_freq"], obj["sample_rate"]) == (80, 2049, SR)
    assert (obj["frame_length_ms"], obj["frame_shift_ms"]) == (50.0, 12.5)
    allm = np.concatenate([t.mel for t in _targets(corpus["out_dir"]).values()]).astype(np.float64)
    assert np.allclose(obj["average_mel_level_db"], allm.mean(0), rtol=1e-5, atol=0)
    assert np.allclose(obj["stddev_mel_level_db"], allm.std(0), rtol=1e-5, atol=0)
    assert np.array_equal(np.array(obj["min_mel_level_db"]), allm.min(0))
    H.HParams(**H.default_values()).parse_json(text)


def test_cli_in_a_fresh_process_writes_the_same_files(corpus):
    out2 = corpus["root"] / "out_cli"
    r = subprocess.run([sys.executable, "-m", "sat_amd.preprocess", "vctk", str(corpus["in_dir"]),
                        str(out2), "--version", "0.8", "--hparams",
                        "num_mels=80,num_freq=2049,sample_rate=48000,trim_top_db=10"],
                       cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "p225_002" in r.stderr
    for p in sorted(corpus["out_dir"].iterdir()):
        assert (out2 / p.name).read_bytes() == p.read_bytes(), p.name
    assert sorted(p.name for p in out2.iterdir()) == sorted(
        p.name for p in corpus["out_dir"].iterdir())
    r = subprocess.run([sys.executable, "-m", "sat_amd.preprocess", "vctk", str(corpus["in_dir"]),
                        str(out2), "--version", "0.91", "--source-only"],
                       cwd=ROOT, capture_output=True, text=True)
    assert r.returncode != 0 and "flite" in r.stderr


def test_batch_runs_one_train_step(corpus, cuda):
    """hparams.json + the records through the VCTK dataset into model_fn TRAIN as they are."""
    from sat_amd import datasets as D, hparams as H, models as M
    hp = H.vctk_hparams(source="char").parse_json(
        (corpus["out_dir"] / "hparams.json").read_text())
    src = [str(corpus["out_dir"] / f"{k}.source.tfrecord") for k in KEPT]
    tgt = [str(corpus["out_dir"] / f"{k}.target.tfrecord") for k in KEPT]
    ds = D.create_from_tfrecord_files(src, tgt, hp, cycle_length=1)
    (feats, labels), = list(ds.prepare_and_zip().group_by_batch(batch_size=3))
    assert isinstance(feats, D.VCTKSourceData)
    assert feats.speaker_id.tolist() == [225, 225, 226] and feats.gender.tolist() == [0, 0, 1]
    assert feats.age.tolist() == [23, 23, 22] and list(feats.key) == [k.encode() for k in KEPT]
    model = M.tacotron_model_factory(hp, None, None, device=cuda, seed=3)
    spec = model.model_fn(feats, labels, M.ModeKeys.TRAIN, hp)
    assert np.isfinite(float(spec.loss.item())) and int(spec.train_op.item()) == 1
