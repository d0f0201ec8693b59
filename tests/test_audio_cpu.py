"""Audio front end and preprocessing, the parts that need no GPU: the float64 restatement
(tests/audio_ref.py) against CPU torch.stft, the mel basis, the host surface of ``Audio``, the
text front end, and the condition the GPU tolerances rest on (no test band value near the
amplitude floor)."""
import json
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

import audio_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CONFIGS = {"ljspeech": (22050, 2048, 80), "vctk": (48000, 4096, 80)}


def _write_wav(path, y, rate, channels=1):
    pcm = np.clip(np.rint(np.asarray(y, np.float64) * 32768.0), -32768, 32767).astype("<i2")
    with wave.open(str(path), "wb") as f:
        f.setnchannels(channels)
        f.setsampwidth(2)
        f.setframerate(rate)
        f.writeframes(pcm.tobytes())
    return pcm


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_restatement_matches_torch_stft(name):
    """float64 torch.stft(center=True, pad_mode='reflect') with the periodic Hann: the restatement
    agrees to float64 rounding (1e-12 of the largest magnitude), and the frame count is
    1 + len // hop."""
    c = R.CASES[name]
    for r in R.case_reference(name):
        y = torch.from_numpy(r["y"].astype(np.float64))
        w = torch.hann_window(c["win"], periodic=True, dtype=torch.float64)
        X = torch.stft(y, c["n_fft"], hop_length=c["hop"], win_length=c["win"], window=w,
                       center=True, pad_mode="reflect", return_complex=True)
        want = X.abs().t().numpy()
        assert r["mag64"].shape == (1 + len(r["y"]) // c["hop"], c["n_fft"] // 2 + 1)
        assert want.shape == r["mag64"].shape
        assert np.abs(want - r["mag64"]).max() <= 1e-12 * want.max()
        # and the float32 pipeline is close, but not equal: e32 is a real rounding error
        e32, e32_mag = R.case_e32(name)
        assert 0 < e32 < 1e-4 and 0 < e32_mag < 2e-6


def test_zero_waveform_is_exactly_the_floor():
    c = R.CASES["a"]
    basis = R.cached_basis(c["sr"], c["n_fft"], c["num_mels"])
    db, mag = R.melspectrogram(np.zeros(3000, np.float32), c["n_fft"], c["hop"], c["win"], basis)
    assert (mag == 0).all() and (db == -120.0).all()


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_band_values_clear_of_the_floor(name):
    """Every band value of the float64 reference on every test input is >= 1e-3 = 100 x the
    amplitude floor, so no GPU comparison is decided by the clamp."""
    c = R.CASES[name]
    basis = R.cached_basis(c["sr"], c["n_fft"], c["num_mels"])
    smallest = min(float(R.band_values(r["mag64"], basis).min()) for r in R.case_reference(name))
    print(f"case {name}: smallest band value {smallest:.3e}")
    assert smallest >= 1e-3


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_mel_basis(config):
    from sat_amd import audio as A
    sr, n_fft, n_mels = CONFIGS[config]
    basis = A.mel_filterbank(sr, n_fft, n_mels)
    assert basis.shape == (n_mels, n_fft // 2 + 1) and basis.dtype == np.float32
    assert (basis >= 0).all()
    lo, hi = A.band_limits(basis)
    assert lo.dtype == np.int32 and hi.dtype == np.int32
    for m in range(n_mels):
        nz = np.flatnonzero(basis[m])
        assert nz.size > 0, f"band {m} is empty"
        assert (np.diff(nz) == 1).all(), f"band {m} support is not contiguous"
        assert lo[m] == nz[0] and hi[m] == nz[-1] + 1
    # the element-by-element restatement agrees to a rounding of float32
    want = R.cached_basis(sr, n_fft, n_mels)
    assert np.abs(basis.astype(np.float64) - want).max() <= 2.0 ** -23 * want.max()
    # Slaney area normalisation: interior triangles integrate to ~1 over frequency
    df = (sr / 2.0) / (n_fft // 2)
    area = basis.astype(np.float64).sum(axis=1) * df
    assert np.abs(area[n_mels // 2:] - 1.0).max() < 0.05


def test_band_limits_of_an_empty_row():
    from sat_amd import audio as A
    b = np.zeros((3, 9), np.float32)
    b[0, 2:5] = 1.0
    b[2, 8] = 1.0
    lo, hi = A.band_limits(b)
    assert list(lo) == [2, 0, 8] and list(hi) == [5, 0, 9]


def test_stft_parameters():
    from sat_amd import audio as A, hparams as H
    assert A.Audio(H.ljspeech_hparams())._stft_parameters() == (2048, 275, 1102)
    assert A.Audio(H.vctk_hparams())._stft_parameters() == (4096, 600, 2400)
    for name, c in R.CASES.items():
        assert A.Audio(R.case_hparams(name))._stft_parameters() == (c["n_fft"], c["hop"], c["win"])


def test_window_and_twiddles():
    from sat_amd import audio as A
    for win, n_fft in ((1102, 2048), (101, 256), (2400, 4096), (64, 64)):
        w = A.hann_window(win, n_fft)
        assert w.dtype == np.float32 and w.shape == (n_fft,)
        assert np.abs(w - R.window(win, n_fft)).max() <= 2.0 ** -24
        off = (n_fft - win) // 2
        assert not w[:off].any() and not w[off + win:].any()
        t = A.twiddle_table(n_fft)
        assert t.dtype == np.float32 and t.shape == (n_fft // 2, 2)
        k = np.arange(n_fft // 2)
        want = np.exp(-2j * np.pi * k / n_fft)
        assert np.abs(t[:, 0] + 1j * t[:, 1] - want).max() <= 2.0 ** -24
        assert tuple(t[0]) == (1.0, 0.0) and tuple(t[n_fft // 4]) == (0.0, -1.0)


def test_host_helpers_follow_the_reference_formulas():
    from sat_amd import audio as A, hparams as H
    hp = H.ljspeech_hparams(average_mel_level_db=[-50.0] * 80, stddev_mel_level_db=[10.0] * 80)
    a = A.Audio(hp)
    S = np.full((80, 3), -40.0, np.float32)
    assert np.allclose(a.normalize_mel(S.T), 1.0)
    assert np.allclose(a._amp_to_db(np.array([0.0, 1e-5, 1.0, 10.0])), [-100, -100, 0, 20])
    mag = np.abs(np.random.default_rng(0).standard_normal((1025, 4)))
    assert np.allclose(a._linear_to_mel(mag), a._mel_basis @ mag)


def test_text_to_sequence_round_trip_and_rejection():
    from sat_amd import preprocess as P
    assert len(P.symbols) == 70
    table = "".join(P.symbols)
    ids, clean = P.text_to_sequence(table, cleaner=lambda s: s)
    assert ids == list(range(1, 71)) and clean == table
    assert P.sequence_to_text(ids) == table
    ids, clean = P.text_to_sequence("Hello,   World!\n")
    assert clean == "hello, world! " and P.sequence_to_text(ids) == clean
    with pytest.raises(ValueError, match="é"):
        P.text_to_sequence("café")


def test_load_wav_and_save_wav(tmp_path):
    from sat_amd import audio as A, hparams as H
    a = A.Audio(H.ljspeech_hparams())
    y = R.make_signal(500, 22050)
    pcm = _write_wav(tmp_path / "ok.wav", y, 22050)
    got = a.load_wav(str(tmp_path / "ok.wav"))
    assert got.dtype == np.float32 and np.array_equal(got, pcm.astype(np.float32) / 32768.0)
    a.save_wav(got, str(tmp_path / "again.wav"))
    assert np.array_equal(a.load_wav(str(tmp_path / "again.wav")), got)
    stereo = np.stack([y, -y], axis=1).reshape(-1)
    _write_wav(tmp_path / "stereo.wav", stereo, 22050, channels=2)
    assert np.abs(a.load_wav(str(tmp_path / "stereo.wav"))).max() <= 1.0 / 32768.0
    _write_wav(tmp_path / "slow.wav", y, 16000)
    with pytest.raises(ValueError, match="16000.*22050"):
        a.load_wav(str(tmp_path / "slow.wav"))


def _tiny_corpus(tmp_path):
    in_dir = tmp_path / "in"
    (in_dir / "wavs").mkdir(parents=True)
    (in_dir / "metadata.csv").write_text(
        "LJ001-0001|Raw ONE|Printing, in the only sense\n"
        "LJ001-0002|Raw TWO|With which we are at present concerned\n", encoding="utf-8")
    return in_dir


def test_source_records_and_cli(tmp_path):
    """--source-only needs no GPU: the CLI (as a fresh process, from the repository root) writes
    the source records and list.csv, and no hparams.json."""
    from sat_amd import preprocess as P, tfrecord as T
    in_dir, out_dir = _tiny_corpus(tmp_path), tmp_path / "out"
    r = subprocess.run([sys.executable, "-m", "sat_amd.preprocess", "ljspeech", str(in_dir),
                        str(out_dir), "--source-only", "--hparams", "num_mels=80,num_freq=1025"],
                       cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert (out_dir / "list.csv").read_text().split() == ["LJ001-0001", "LJ001-0002"]
    assert not (out_dir / "hparams.json").exists()
    rec, = list(T.read_tfrecords(str(out_dir / "LJ001-0002.source.tfrecord")))
    s = T.parse_preprocessed_source_data(rec)
    text = "with which we are at present concerned"
    assert (s.id, s.key, s.text) == (1, b"LJ001-0002", text.encode())
    assert s.source_length == len(text) and P.sequence_to_text(s.source) == text


def test_hparams_json_keys_and_corpus_statistics(tmp_path):
    """corpus_statistics follows preprocess_ljspeech.py:65-67, and the hparams.json keys are the
    reference's and load through hparams.parse_json."""
    from sat_amd import preprocess as P, hparams as H
    rng = np.random.default_rng(1)
    mels = [rng.standard_normal((n, 5)) * 7.0 - 40.0 for n in (3, 8)]
    stats = [P.MelStatistics(id=i, key=str(i), max=m.max(0), min=m.min(0), sum=m.sum(0),
                             length=len(m), moment2=np.square(m).sum(0))
             for i, m in enumerate(mels)]
    avg, std, mn = P.LJSpeech.corpus_statistics(stats)
    allm = np.concatenate(mels)
    assert np.allclose(avg, allm.mean(0), rtol=1e-12)
    assert np.allclose(std, allm.std(0), rtol=1e-9)
    assert np.array_equal(mn, allm.min(0))
    assert P.HPARAMS_JSON_KEYS == ("num_mels", "num_freq", "sample_rate", "frame_length_ms",
                                   "frame_shift_ms", "average_mel_level_db",
                                   "stddev_mel_level_db", "min_mel_level_db")
    obj = dict(num_mels=5, num_freq=1025, sample_rate=22050, frame_length_ms=50,
               frame_shift_ms=12.5, average_mel_level_db=avg.tolist(),
               stddev_mel_level_db=std.tolist(), min_mel_level_db=mn.tolist())
    assert tuple(obj) == P.HPARAMS_JSON_KEYS
    hp = H.HParams(**H.default_values()).parse_json(json.dumps(obj))
    assert hp.average_mel_level_db == avg.tolist() and hp.frame_length_ms == 50.0
