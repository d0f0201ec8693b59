"""The resampler without a GPU: the ratio and length arithmetic, the polyphase table against the
filter function, the float64 oracle (tests/resample_ref.py) as a resampler in its own right, and
the opt-in surface (``load_wav``'s default, the CLI flag)."""
import wave

import numpy as np
import pytest

import resample_ref as R


def _audio_module():
    from sat_amd import audio as A
    return A


@pytest.mark.parametrize("orig,target,want", [(48000, 22050, (147, 320)),
                                              (16000, 22050, (441, 320)),
                                              (44100, 22050, (1, 2)),
                                              (22050, 22050, (1, 1))])
def test_ratio_reduction(orig, target, want):
    A = _audio_module()
    assert A.resample_ratio(orig, target) == want == R.ratio(orig, target)
    f = A.resample_filter(orig, target)
    assert (f.L, f.M) == want and f.table.shape == (f.L, f.taps) and f.table.dtype == np.float32
    assert f.taps == 2 * R.half_width(*want) + 2 and f.offset == -R.half_width(*want)
    assert A.resample_filter(orig, target) is f                     # cached


def test_unrelated_rates_are_refused():
    A = _audio_module()
    with pytest.raises(ValueError) as e:
        A.resample_filter(44101, 22050)
    assert "44101" in str(e.value) and "22050" in str(e.value) and "22050/44101" in str(e.value)


def test_downsampling_filter_has_282_taps():
    f = _audio_module().resample_filter(48000, 22050)
    assert (f.taps, f.offset) == (282, -140)


@pytest.mark.parametrize("n", [1, 319, 320, 321, 6000])
def test_output_lengths(n):
    A = _audio_module()
    want = int(np.ceil(n * 147 / 320))
    assert A.resampled_length(n, 147, 320) == want == R.out_length(n, 147, 320)
    assert len(R.oracle(np.zeros(n), 48000, 22050)) == want


@pytest.mark.parametrize("orig,target", R.RATES)
def test_table_against_h(orig, target):
    """Every entry is h in float64 at its tap position, rounded once.  The position is worked out
    from an output index of that phase, (n M - k L) / max(L, M) with k = floor(n M / L) + offset
    + j, not from the table's own layout."""
    f = _audio_module().resample_filter(orig, target)
    L, M = f.L, f.M
    n = np.arange(L, dtype=np.int64)                                # one output per phase
    phase = n * M % L
    assert sorted(phase) == list(range(L))
    k = (n * M // L)[:, None] + f.offset + np.arange(f.taps, dtype=np.int64)[None, :]
    want = R.h((n[:, None] * M - k * L).astype(np.float64) / max(L, M)).astype(np.float32)
    assert np.array_equal(f.table[phase], want)
    # the taps cover h's support: one more on either side would be zero
    for dk in (-1, f.taps):
        edge = (n * M - ((n * M // L) + f.offset + dk) * L).astype(np.float64) / max(L, M)
        assert (np.abs(edge) > R.Z).all()
    # phase p mirrors phase (L - p) mod L
    for p in range(1, L):
        assert np.array_equal(f.table[p], f.table[L - p][::-1])
    assert np.array_equal(f.table[0, :-1], f.table[0, :-1][::-1]) and f.table[0, -1] == 0.0
    assert np.array_equal(f.table, R.table32(orig, target)[0])


def test_h_is_the_stated_function():
    A = _audio_module()
    assert (A.RESAMPLE_ZEROS, A.RESAMPLE_BETA, A.RESAMPLE_ROLLOFF) == (R.Z, R.BETA, R.ROLLOFF)
    t = np.linspace(-70.0, 70.0, 2801)
    assert np.array_equal(A.resample_kernel_function(t), R.h(t))
    assert R.h(0.0) == R.ROLLOFF and R.h(64.5) == 0.0 and R.h(-64.0) != 0.0


# rates, tone in Hz: the oracle alone, against the analytic sine at the new rate
TONES = [(48000, 22050, 3000.0), (48000, 22050, 9000.0), (16000, 22050, 5000.0),
         (44100, 22050, 7000.0)]


@pytest.mark.parametrize("orig,target,freq", TONES)
def test_oracle_is_a_resampler(orig, target, freq):
    n = 6000
    y = R.oracle(R.sine(n, orig, freq), orig, target)
    sl = R.interior(n, orig, target)
    assert sl.stop - sl.start > 1000
    err = float(np.abs(y - R.sine(len(y), target, freq))[sl].max())
    print(f"{orig} -> {target}, {freq:.0f} Hz: interior |err| {err:.2e}")
    assert err < 1e-6


def test_oracle_rejects_an_alias():
    """14 kHz lies above the new Nyquist frequency (11 025 Hz): it must not fold back."""
    n = 6000
    y = R.oracle(R.sine(n, 48000, 14000.0), 48000, 22050)
    rms = float(np.sqrt(np.mean(np.square(y[R.interior(n, 48000, 22050)]))))
    print(f"14 kHz through 48000 -> 22050: interior rms {rms:.2e}")
    assert rms < 1e-6


def test_pipeline32_follows_the_oracle():
    """The float32 pipeline's error is rounding, not a different filter."""
    for orig, target in R.RATES:
        refs = R.reference(orig, target)
        assert [len(r["y32"]) for r in refs] == [len(r["y64"]) for r in refs]
        assert 0.0 < R.e32(refs) < 1e-5


def _write_wav(path, y, rate):
    q = np.clip(np.rint(np.asarray(y, np.float64) * 32768.0), -32768, 32767).astype("<i2")
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(rate)
        f.writeframes(q.tobytes())
    return q.astype(np.float32) / np.float32(32768.0)


def test_load_wav_default_still_raises(tmp_path):
    from sat_amd import hparams as H
    A = _audio_module()
    a = A.Audio(H.ljspeech_hparams())
    pcm = _write_wav(tmp_path / "a.wav", 0.5 * R.signal(800, 3), 16000)
    with pytest.raises(ValueError) as e:
        a.load_wav(str(tmp_path / "a.wav"))
    assert "16000" in str(e.value) and "22050" in str(e.value)
    y, rate = a.read_wav(str(tmp_path / "a.wav"))
    assert rate == 16000 and np.array_equal(y, pcm)
    # a file at the right rate needs no launch, with or without the flag
    pcm = _write_wav(tmp_path / "b.wav", 0.5 * R.signal(800, 4), 22050)
    assert np.array_equal(a.load_wav(str(tmp_path / "b.wav")), pcm)
    assert np.array_equal(a.load_wav(str(tmp_path / "b.wav"), resample=True), pcm)


def test_cli_parser_takes_resample(monkeypatch, tmp_path):
    """--resample for both corpora, off by default: main() builds the corpus with it."""
    from sat_amd import preprocess as P
    seen = []

    class Corpus:
        def __init__(self, in_dir, out_dir, hp, **kw):
            seen.append(kw)

        def run(self, **kw):
            return []
    monkeypatch.setattr(P, "LJSpeech", Corpus)
    monkeypatch.setattr(P, "VCTK", Corpus)
    for dataset in ("ljspeech", "vctk"):
        assert P.main([dataset, str(tmp_path), str(tmp_path / "o")]) == 0
        assert seen.pop()["resample"] is False
        assert P.main([dataset, str(tmp_path), str(tmp_path / "o"), "--resample"]) == 0
        assert seen.pop()["resample"] is True
    monkeypatch.undo()
    import inspect
    for cls in (P._Corpus, P.VCTK):
        assert inspect.signature(cls.__init__).parameters["resample"].default is False
