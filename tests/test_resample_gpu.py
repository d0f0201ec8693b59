"""sat_resample on the GPU against the float64 oracle (tests/resample_ref.py), and the opt-in
path above it: ``resample_batch``, ``load_wav(path, resample=True)`` and preprocessing with
``--resample`` for both corpora.

Tolerance (not hard-coded): e32 is the largest absolute difference between the float32 CPU
pipeline -- the product's arithmetic in its tap order -- and the oracle on the case's own inputs;
the kernel must stay within 8 x e32.  The mels written by preprocessing are held to the existing
rule for mels (tests/test_audio_gpu.py): 8 x the float32 CPU mel pipeline's error on that audio.

Measured on an MI355X (one run): see DESIGN.md "Resampling"."""
import contextlib
import ctypes
import io
import wave

import numpy as np
import pytest
import torch

import audio_ref as AR
import resample_ref as R
import trim_ref as T

pytestmark = pytest.mark.gpu


def _audio(cuda, **over):
    from sat_amd import audio as A, hparams as H
    hp = H.ljspeech_hparams()
    if over:
        hp.override_from_dict(over)
    return A.Audio(hp, device=cuda)


def _launch(cuda, xs, orig, target, extra=5, fill=float("nan")):
    """One sat_resample launch over the utterances ``xs``: the whole ``out`` [B, need + extra],
    pre-filled with ``fill``."""
    from sat_amd import audio as A, kernels as K
    f = A.resample_filter(orig, target)
    lengths = [len(x) for x in xs]
    host = np.zeros((len(xs), max(lengths)), np.float32)
    for b, x in enumerate(xs):
        host[b, :lengths[b]] = x
    need = max(R.out_length(n, f.L, f.M) for n in lengths)
    out = torch.full((len(xs), need + extra), fill, device=cuda)
    K.resample(torch.from_numpy(host).to(cuda),
               torch.tensor(lengths, dtype=torch.int32, device=cuda), lengths,
               table=torch.from_numpy(np.array(f.table)).to(cuda), L=f.L, M=f.M, offset=f.offset,
               scale=min(1.0, f.L / f.M), out=out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check(got, refs, what):
    e32 = R.e32(refs)
    worst = 0.0
    for b, r in enumerate(refs):
        n = len(r["y64"])
        worst = max(worst, float(np.abs(got[b, :n] - r["y64"]).max()))
        assert not got[b, n:].any() and np.isfinite(got[b]).all()   # exact zeros past the end
    print(f"{what}: |err| {worst:.3e}, e32 {e32:.3e}, ratio {worst / e32:.2f}")
    assert worst <= 8 * e32


@pytest.mark.parametrize("orig,target", R.RATES)
def test_kernel_against_the_oracle(orig, target, cuda):
    """B = 3, lengths (1, 700, 2049): an utterance shorter than the filter, halos crossing both
    edges of the others, downsampling (282 taps), upsampling (L > M) and a single phase."""
    refs = R.reference(orig, target)
    L, M = R.ratio(orig, target)
    assert [len(r["y64"]) for r in refs] == [R.out_length(n, L, M) for n in R.LENGTHS]
    got = _launch(cuda, [r["x"] for r in refs], orig, target)
    assert got.shape[1] == len(refs[2]["y64"]) + 5
    _check(got, refs, f"{orig} -> {target}")
    again = _launch(cuda, [r["x"] for r in refs], orig, target, fill=7.0)
    assert np.array_equal(got, again)                               # bit-identical runs


@pytest.mark.parametrize("orig,target,n", [(48000, 22050, 3001), (16000, 22050, 5000)])
def test_one_utterance_over_several_tiles(orig, target, n, cuda):
    """A workgroup owns 256 outputs: 1379 and 6891 outputs are 5.4 and 26.9 tiles, so interior
    tiles take their halo from inside the utterance and the last tile is partial."""
    refs = R.reference(orig, target, lengths=(n,), seed=1)
    assert len(refs[0]["y64"]) > 4 * 256 and len(refs[0]["y64"]) % 256
    _check(_launch(cuda, [refs[0]["x"]], orig, target, extra=3), refs, f"{orig} -> {target}, {n}")


def test_resample_batch_mixed_rates(cuda):
    a = _audio(cuda)
    rates = [48000, 22050, 16000, 48000]
    xs = [R.signal(n, 40 + i) for i, n in enumerate((900, 500, 333, 1201))]
    out, lengths = a.resample_batch(xs, rates)
    want_len = [R.out_length(len(x), *R.ratio(r, 22050)) for x, r in zip(xs, rates)]
    assert lengths == want_len and [int(o.shape[0]) for o in out] == want_len
    assert all(isinstance(o, torch.Tensor) and o.is_cuda and o.ndim == 1 for o in out)
    assert np.array_equal(out[1].cpu().numpy(), xs[1])              # already at the target
    for i in (0, 2, 3):                                             # the single-rate calls
        one, _ = a.resample_batch([xs[i]], rates[i])
        assert np.array_equal(out[i].cpu().numpy(), one[0].cpu().numpy())
        y64 = R.oracle(xs[i], rates[i], 22050)
        e32 = float(np.abs(R.pipeline32(xs[i], rates[i], 22050) - y64).max())
        assert np.abs(out[i].cpu().numpy() - y64).max() <= 8 * e32
    # device tensors in, another target rate, one rate for all
    dev = [torch.from_numpy(x).to(cuda) for x in xs[:2]]
    out16, len16 = a.resample_batch(dev, 48000, target_rate=16000)
    assert len16 == [300, 167]
    y64 = R.oracle(xs[0], 48000, 16000)
    e32 = float(np.abs(R.pipeline32(xs[0], 48000, 16000) - y64).max())
    assert np.abs(out16[0].cpu().numpy() - y64).max() <= 8 * e32
    with pytest.raises(ValueError):
        a.resample_batch(xs, rates[:3])


def _write_wav(path, y, rate):
    q = np.clip(np.rint(np.asarray(y, np.float64) * 32768.0), -32768, 32767).astype("<i2")
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(rate)
        f.writeframes(q.tobytes())
    return q.astype(np.float32) / np.float32(32768.0)


def test_load_wav_resample(tmp_path, cuda):
    a = _audio(cuda)
    pcm = _write_wav(tmp_path / "a.wav", 0.9 * R.signal(1234, 5), 16000)
    with pytest.raises(ValueError) as e:
        a.load_wav(str(tmp_path / "a.wav"))
    assert "16000" in str(e.value) and "22050" in str(e.value)
    y = a.load_wav(str(tmp_path / "a.wav"), resample=True)
    assert isinstance(y, np.ndarray) and y.dtype == np.float32
    assert y.shape == (-(-1234 * 441 // 320),)
    y64 = R.oracle(pcm, 16000, 22050)
    e32 = float(np.abs(R.pipeline32(pcm, 16000, 22050) - y64).max())
    err = float(np.abs(y - y64).max())
    print(f"load_wav 16000 -> 22050: |err| {err:.3e}, e32 {e32:.3e}, ratio {err / e32:.2f}")
    assert err <= 8 * e32


# ---- preprocessing: 48 kHz wavs, hparams.sample_rate 22050, the smallest n_fft sat_melspec takes
N_FFT, HOP, WIN, MELS = 64, 22, 44, 8
HP = dict(sample_rate=22050, num_freq=N_FFT // 2 + 1, num_mels=MELS, frame_length_ms=2.0,
          frame_shift_ms=1.0)
HP_ARG = ",".join(f"{k}={v}" for k, v in HP.items())


def _mel_check(a, key, mel, y):
    """A target record's mel against melspectrogram_batch of the oracle-resampled audio ``y``,
    within 8 x the float32 CPU mel pipeline's error on that audio (tests/test_audio_gpu.py's
    rule)."""
    assert y.dtype == np.float32
    want, frames = a.melspectrogram_batch([y])
    want = want[0].cpu().numpy()
    assert mel.shape == want.shape == (1 + len(y) // HOP, MELS) and int(frames[0]) == len(want)
    basis = AR.cached_basis(22050, N_FFT, MELS)
    db64, _ = AR.melspectrogram(y, N_FFT, HOP, WIN, basis)
    db32, _ = AR.pipeline32(y, N_FFT, HOP, WIN, basis)
    e32 = float(np.abs(db32 - db64).max())
    err = float(np.abs(mel - want).max())
    print(f"{key}: mel |err| {err:.3e} dB, e32 {e32:.3e} dB, ratio {err / e32:.2f}")
    assert err <= 8 * e32


def _target(out_dir, key):
    from sat_amd import tfrecord as TF
    rec, = list(TF.read_tfrecords(str(out_dir / f"{key}.target.tfrecord")))
    return TF.parse_preprocessed_mel_data(rec)


def test_preprocess_ljspeech_resample(tmp_path, cuda):
    from sat_amd import preprocess as P
    in_dir, out_dir = tmp_path / "in", tmp_path / "out"
    (in_dir / "wavs").mkdir(parents=True)
    keys, pcm = ["LJ001-0001", "LJ001-0002", "LJ001-0003"], {}
    for i, (key, n) in enumerate(zip(keys, (24000, 14401, 19000))):
        pcm[key] = _write_wav(in_dir / "wavs" / f"{key}.wav", AR.make_signal(n, 48000, 20 + i),
                              48000)
    (in_dir / "metadata.csv").write_text("".join(f"{k}|raw|some text\n" for k in keys))
    # without --resample: the existing error, on the first file
    with pytest.raises(ValueError) as e, contextlib.redirect_stdout(io.StringIO()):
        P.main(["ljspeech", str(in_dir), str(out_dir), "--hparams", HP_ARG])
    assert "48000" in str(e.value) and "no resampler" in str(e.value)
    with contextlib.redirect_stdout(io.StringIO()):
        assert P.main(["ljspeech", str(in_dir), str(out_dir), "--resample", "--hparams",
                       HP_ARG]) == 0
    assert (out_dir / "list.csv").read_text().split() == keys
    a = _audio(cuda, **HP)
    for i, key in enumerate(keys):
        t = _target(out_dir, key)
        n22 = -(-len(pcm[key]) * 147 // 320)
        assert (t.id, t.key, t.target_length, t.mel_width) == (i, key.encode(),
                                                               1 + n22 // HOP, MELS)
        _mel_check(a, key, t.mel, R.oracle(pcm[key], 48000, 22050).astype(np.float32))


def test_preprocess_vctk_resample(tmp_path, cuda):
    """One speaker: resampling, then the trim and the mel of the trimmed segment in place."""
    from sat_amd import hparams as H, preprocess as P
    in_dir, out_dir = tmp_path / "in", tmp_path / "out"
    in_dir.mkdir()
    (in_dir / "speaker-info.txt").write_text("ID  AGE  GENDER  ACCENTS\n225  23  F    English\n")
    for sub in ("wav48", "txt"):
        (in_dir / sub / "p225").mkdir(parents=True)
    cases = {"p225_001": (24000, 6000, 18000, 5), "p225_002": (30000, 9000, 24000, 7)}
    pcm = {}
    for key, case in cases.items():
        y = T.signal(case).astype(np.float64)
        y = y + 4e-3 * np.random.default_rng(case[3]).standard_normal(case[0])
        pcm[key] = _write_wav(in_dir / "wav48" / "p225" / f"{key}.wav", y, 48000)
        (in_dir / "txt" / "p225" / f"{key}.txt").write_text("Please call Stella.\n")
    hp = H.vctk_hparams()
    hp.override_from_dict(HP)
    with pytest.raises(ValueError) as e:
        P.VCTK(str(in_dir), str(out_dir), hp, device=cuda).run()
    assert "48000" in str(e.value) and "no resampler" in str(e.value)
    keys = P.VCTK(str(in_dir), str(out_dir), hp, device=cuda, resample=True).run()
    assert keys == list(cases)
    setting = (int(hp.trim_frame_length), int(hp.trim_hop_length), float(hp.trim_top_db))
    pad = int(hp.num_silent_frames * hp.frame_shift_ms * hp.sample_rate / 1000)
    a = _audio(cuda, **HP)
    for i, key in enumerate(keys):
        y = R.oracle(pcm[key], 48000, 22050).astype(np.float32)
        assert T.margin_db(y, *setting) >= T.GUARD_DB               # the exact trim is a fair demand
        s, e_ = T.trim_bounds(y, *setting, pad_samples=pad)
        assert 0 < s < e_ < len(y) and e_ - s > N_FFT // 2
        t = _target(out_dir, key)
        assert (t.id, t.target_length) == (i, 1 + (e_ - s) // HOP)
        _mel_check(a, key, t.mel, np.ascontiguousarray(y[s:e_]))


def test_refusals(cuda):
    from sat_amd import _lib, audio as A, kernels as K
    f = A.resample_filter(48000, 22050)
    wav = torch.zeros(2, 640, device=cuda)
    lengths = torch.tensor([640, 100], dtype=torch.int32, device=cuda)
    table = torch.from_numpy(np.array(f.table)).to(cuda)
    kw = dict(table=table, L=f.L, M=f.M, offset=f.offset, scale=f.L / f.M)
    out = torch.full((2, 293), 7.0, device=cuda)                    # 640 samples give 294
    with pytest.raises(_lib.SatLibraryError) as e:
        K.resample(wav, lengths, [640, 100], out=out, **kw)
    assert e.value.rc == _lib.SAT_ERR_ARGUMENT and "stride_out" in str(e.value)
    ok = torch.full((2, 294), 7.0, device=cuda)
    host = (ctypes.c_int32 * 2)(640, 100)
    args = lambda taps: (wav.data_ptr(), lengths.data_ptr(), ctypes.cast(host, ctypes.c_void_p),
                         2, 640, table.data_ptr(), f.L, f.M, taps, f.offset, f.L / f.M,
                         ok.data_ptr(), 294, K._stream())
    lib = _lib.load()
    assert lib.sat_resample(*args(0)) == _lib.SAT_ERR_ARGUMENT
    assert b"taps" in lib.sat_last_error_string()
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (ok == 7.0).all()                 # nothing was written
    # the same call with its taps is accepted: each refusal is caused by its one change
    assert lib.sat_resample(*args(f.taps)) == 0
    torch.cuda.synchronize()
    assert not ok.cpu().numpy().any()                               # zeros in, zeros out
