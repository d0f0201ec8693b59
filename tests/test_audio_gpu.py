"""sat_melspec / sat_mel_stats on the GPU against the float64 restatement (tests/audio_ref.py).

Tolerance (not hard-coded): e32 is the largest absolute dB difference between the float32 CPU
pipeline (torch.stft float32, float32 matmul, float32 log10) and the float64 restatement on the
case's own inputs; the kernel must stay within 8 x e32.  The same rule holds for the magnitudes,
relative to each frame's largest magnitude.  tests/test_audio_cpu.py checks that no band value
of these inputs is within 100 x of the amplitude floor, so the clamp decides nothing here.

Measured on an MI355X (one run): see DESIGN.md "Audio front end"."""
import numpy as np
import pytest
import torch

import audio_ref as R

pytestmark = pytest.mark.gpu


def _audio(name, cuda):
    from sat_amd import audio as A
    return A.Audio(R.case_hparams(name), device=cuda)


def _run_case(name, cuda):
    a = _audio(name, cuda)
    refs = R.case_reference(name)
    mel, frames, mag = a.melspectrogram_batch([r["y"] for r in refs], return_magnitudes=True)
    torch.cuda.synchronize()
    return a, refs, mel.cpu().numpy(), frames.cpu().numpy(), mag.cpu().numpy()


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_melspec_against_float64(name, cuda):
    c = R.CASES[name]
    a, refs, mel, frames, mag = _run_case(name, cuda)
    e32, e32_mag = R.case_e32(name)
    want_frames = [1 + L // c["hop"] for L in c["lengths"]]
    assert list(frames) == want_frames
    assert mel.shape == (len(refs), max(want_frames), c["num_mels"])
    assert mag.shape == (len(refs), max(want_frames), c["n_fft"] // 2 + 1)
    err = err_mag = 0.0
    for b, r in enumerate(refs):
        n = want_frames[b]
        err_mag = max(err_mag, R.mag_error(mag[b, :n], r["mag64"]))
        err = max(err, float(np.abs(mel[b, :n] - r["db64"]).max()))
        # rows past the utterance's frame count are exactly zero
        assert not mel[b, n:].any() and not mag[b, n:].any()
    print(f"case {name}: mel |err| {err:.3e} dB, e32 {e32:.3e} dB, ratio {err / e32:.2f}; "
          f"magnitudes {err_mag:.3e}, e32 {e32_mag:.3e}, ratio {err_mag / e32_mag:.2f}")
    assert err_mag <= 8 * e32_mag        # an FFT error shows here, a band-sum error only below
    assert err <= 8 * e32


def test_single_utterance_surface(cuda):
    """melspectrogram: [num_mels, frames]; numpy in -> numpy out, device tensor in -> device
    tensor out, both the batch path's values."""
    a = _audio("b", cuda)
    r, = R.case_reference("b")
    got = a.melspectrogram(r["y"])
    assert isinstance(got, np.ndarray) and got.dtype == np.float32
    assert got.shape == r["db64"].T.shape
    dev = a.melspectrogram(torch.from_numpy(r["y"]).to(cuda))
    assert isinstance(dev, torch.Tensor) and dev.is_cuda
    assert np.array_equal(dev.cpu().numpy(), got)
    e32, _ = R.case_e32("b")
    assert np.abs(got - r["db64"].T).max() <= 8 * e32


def test_zero_waveform_is_exactly_the_floor(cuda):
    a = _audio("a", cuda)
    mel, frames, mag = a.melspectrogram_batch([np.zeros(3000, np.float32)],
                                              return_magnitudes=True)
    want = np.float32(20.0 * np.log10(R.AMP_FLOOR) - R.REF_LEVEL_DB)
    assert int(frames[0]) == 11 and not mag.cpu().numpy().any()
    assert (mel.cpu().numpy() == want).all()


def test_mel_stats_ragged(cuda):
    """Case (e): statistics over the valid frames only, against numpy in float64."""
    a, refs, mel, frames, _ = _run_case("e", cuda)
    dmel = torch.from_numpy(mel).to(cuda)
    # poison the padding rows: they must not be read into the statistics
    for b, n in enumerate(frames):
        dmel[b, int(n):] = 1e30
    st = a.mel_statistics(dmel, torch.from_numpy(frames).to(cuda)).cpu().numpy()
    assert st.dtype == np.float64 and st.shape == (3, 4, 80)
    for b, n in enumerate(frames):
        v = mel[b, :int(n)].astype(np.float64)
        assert np.array_equal(st[b, 0], v.min(0)) and np.array_equal(st[b, 1], v.max(0))
        # float64 sums of <= 15 float32 values: only the summation order differs
        assert np.allclose(st[b, 2], v.sum(0), rtol=1e-14, atol=0)
        assert np.allclose(st[b, 3], np.square(v).sum(0), rtol=1e-14, atol=0)


def test_mel_stats_no_frames(cuda):
    from sat_amd import kernels as K
    mel = torch.ones(2, 3, 5, device=cuda)
    out = torch.empty(2, 4, 5, dtype=torch.float64, device=cuda)
    K.mel_stats(mel, torch.tensor([0, 2], dtype=torch.int32, device=cuda), out)
    o = out.cpu().numpy()
    assert (o[0, 0] == np.inf).all() and (o[0, 1] == -np.inf).all() and not o[0, 2:].any()
    assert (o[1] == np.array([1.0, 1.0, 2.0, 2.0])[:, None]).all()


def _refusal_args(cuda, **over):
    """A well-formed small call (n_fft 64) with buffers large enough for every variation."""
    from sat_amd import audio as A
    cfg = dict(n_fft=64, hop=16, win=48, num_mels=4, num_freq=33, stride=400, lengths=[400, 100],
               F_max=26)
    cfg.update(over)
    B = len(cfg["lengths"])
    t = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=cuda)
    basis = t(cfg["num_mels"], cfg["num_freq"])
    out = torch.full((B, cfg["F_max"], cfg["num_mels"]), 7.0, device=cuda)
    kw = dict(n_fft=cfg["n_fft"], hop=cfg["hop"], win=cfg["win"], window=t(8192),
              twiddle=t(8192), basis=basis, band_lo=t(cfg["num_mels"], dt=torch.int32),
              band_hi=t(cfg["num_mels"], dt=torch.int32), ref_level_db=20.0, amp_floor=1e-5,
              out=out)
    wav = t(B, cfg["stride"])
    lengths = torch.tensor(cfg["lengths"], dtype=torch.int32, device=cuda)
    return (wav, lengths, cfg["lengths"]), kw, out


REFUSALS = [
    (dict(n_fft=96, num_freq=49), "UNSUPPORTED"),                 # not a power of two
    (dict(n_fft=32, num_freq=17, win=32), "UNSUPPORTED"),         # below 64
    (dict(n_fft=8192, num_freq=4097, lengths=[400, 100], stride=400), "UNSUPPORTED"),
    (dict(win=65), "ARGUMENT"),                                   # win > n_fft
    (dict(hop=0), "ARGUMENT"),
    (dict(num_freq=32), "ARGUMENT"),                              # != n_fft/2 + 1
    (dict(lengths=[400, 32]), "ARGUMENT"),                        # <= n_fft/2
    (dict(lengths=[401, 100]), "ARGUMENT"),                       # > wav_stride
    (dict(F_max=25), "ARGUMENT"),                                 # largest frame count is 26
]


@pytest.mark.parametrize("over,code", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_refusals_launch_nothing(over, code, cuda):
    from sat_amd import _lib, kernels as K
    args, kw, out = _refusal_args(cuda, **over)
    with pytest.raises(_lib.SatLibraryError) as e:
        K.melspec(*args, **kw)
    assert e.value.rc == getattr(_lib, "SAT_ERR_" + code)
    assert "sat_melspec" in str(e.value)
    torch.cuda.synchronize()
    assert (out == 7.0).all()                                     # nothing was written


def test_well_formed_small_call_is_accepted(cuda):
    """The refusal tests' base call itself runs (so each refusal is caused by its one change):
    zero waveform and zero basis give the floor on valid rows, zeros on the padding rows."""
    from sat_amd import kernels as K
    args, kw, out = _refusal_args(cuda)
    K.melspec(*args, **kw)
    o = out.cpu().numpy()
    assert (o[0] == np.float32(-120.0)).all()
    assert (o[1, :7] == np.float32(-120.0)).all() and not o[1, 7:].any()
