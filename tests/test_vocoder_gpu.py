"""csrc/vocoder.hip on the GPU against the float64 restatement (tests/vocoder_ref.py).

Tolerance (the rule of test_audio_gpu.py, nothing hard-coded): e32 is the largest absolute
difference between the float32 CPU pipeline and the float64 restatement on the case's own input,
relative to the largest absolute value of the float64 result; the kernel must stay within 8 x e32
by the same measure.  tests/test_vocoder_cpu.py checks that e32 itself stays below 1e-3 on every
loop case and that the floor of mel_to_linear decides next to nothing on its case.

Measured on an MI355X (one run): see DESIGN.md section 8d."""
import wave

import numpy as np
import pytest
import torch

import audio_ref as R
import vocoder_ref as V

pytestmark = pytest.mark.gpu


def _audio(name, cuda):
    from sat_amd import audio as A
    return A.Audio(R.case_hparams(V.CASES[name][0]), device=cuda)


def _frames(name):
    return [u["S"].shape[0] for u in V.case_inputs(name)]


def _padded(arrays, dtype, cuda):
    """[B, F_max, ...] device tensor of per-utterance [F_b, ...] arrays, padding rows poisoned
    with a large value: the kernels must not read them."""
    F_max = max(a.shape[0] for a in arrays)
    out = np.full((len(arrays), F_max) + arrays[0].shape[1:], 1e30, dtype)
    for b, a in enumerate(arrays):
        out[b, :a.shape[0]] = a
    return torch.from_numpy(out).to(cuda)


def _check(label, got, pairs, lengths):
    """got [B, stride] against the per-utterance (float64, float32) references."""
    e32 = V.e32_of(pairs)
    err = max(V.rel_error(got[b, :lengths[b]], w64) for b, (w64, _) in enumerate(pairs))
    print(f"{label}: error {err:.3e}, e32 {e32:.3e}, ratio {err / e32:.2f}")
    for b, L in enumerate(lengths):
        assert not got[b, L:].any()                  # exactly zero past the utterance
    assert err <= 8 * e32


# ---------------------------------------------------------------- istft
@pytest.mark.parametrize("name", V.SINGLE + ["ragged"])
def test_istft_against_float64(name, cuda):
    n_fft, hop, win = V.config(name)
    a = _audio(name, cuda)
    frames = _frames(name)
    spec = _padded([u["X"].astype(np.complex64) for u in V.case_inputs(name)], np.complex64, cuda)
    wav = a.istft_batch(spec, frames)
    torch.cuda.synchronize()
    lengths = [hop * (F - 1) for F in frames]
    assert wav.shape == (len(frames), max(lengths))
    _check(f"istft {name}", wav.cpu().numpy(), V.istft_reference(name), lengths)


@pytest.mark.parametrize("name", V.SINGLE + ["ragged"])
def test_round_trip_returns_the_magnitudes(name, cuda):
    """Analysis of the synthesis: the front end's magnitudes of istft(X) are those of the signal
    (float64 |stft| of the float64 istft; on the frames clear of the right-hand reflection also
    the |X| that went in), within the front end's own 8 x e32 of the magnitudes."""
    n_fft, hop, win = V.config(name)
    a = _audio(name, cuda)
    ins = V.case_inputs(name)
    frames = _frames(name)
    spec = _padded([u["X"].astype(np.complex64) for u in ins], np.complex64, cuda)
    wav = a.istft_batch(spec, frames)
    _, got_frames, mag = a.melspectrogram_batch([wav[b, :hop * (F - 1)]
                                                 for b, F in enumerate(frames)],
                                                return_magnitudes=True)
    torch.cuda.synchronize()
    assert list(got_frames.cpu().numpy()) == frames
    mag = mag.cpu().numpy()
    basis = R.cached_basis(R.CASES[V.CASES[name][0]]["sr"], n_fft,
                           R.CASES[V.CASES[name][0]]["num_mels"])
    for b, (u, (x64, _)) in enumerate(zip(ins, V.istft_reference(name))):
        F = frames[b]
        want = np.abs(V.stft(x64, n_fft, hop, win))
        _, mag32 = R.pipeline32(x64.astype(np.float32), n_fft, hop, win, basis)
        e32_mag = R.mag_error(mag32, want)
        err = R.mag_error(mag[b, :F], want)
        clear = [f for f in range(F) if f * hop + n_fft // 2 <= hop * (F - 1) - 1]
        err_in = R.mag_error(mag[b, clear], u["S"][clear])
        print(f"round trip {name}[{b}]: magnitudes {err:.3e} ({err_in:.3e} against the input on "
              f"{len(clear)} frames), e32 {e32_mag:.3e}, ratio {err / e32_mag:.2f}")
        assert err <= 8 * e32_mag and err_in <= 8 * e32_mag
        assert not mag[b, F:].any()


# ---------------------------------------------------------------- mel -> linear
@pytest.mark.parametrize("power", [1.0, 1.5])
def test_mel_to_linear_against_float64(power, cuda):
    from sat_amd import audio as A
    m = V.mel_case()
    a = A.Audio(V.mel_hparams(), device=cuda)
    frames = [x.shape[0] for x in m["mels"]]
    mel = _padded(m["mels"], np.float32, cuda)
    lin = a.mel_to_linear_batch(mel, frames, power=power).cpu().numpy()
    assert lin.shape == (3, 15, 1025)
    # the table is the host's: the reference takes the very one the kernel was given (the case's
    # own differs from it by the rounding of the two mel bases)
    inv = a._build_inv_mel_basis()
    assert np.abs(inv - m["inv_basis"]).max() <= 1e-5 * np.abs(m["inv_basis"]).max()
    args = (m["average"], m["stddev"], m["ref_level_db"], inv, power)
    want = [V.mel_to_linear(x, *args) for x in m["mels"]]
    e32 = max(V.rel_error(V.mel_to_linear32(x, *args), w) for x, w in zip(m["mels"], want))
    err = max(V.rel_error(lin[b, :frames[b]], w) for b, w in enumerate(want))
    print(f"mel_to_linear power {power}: error {err:.3e}, e32 {e32:.3e}, ratio {err / e32:.2f}")
    for b, F in enumerate(frames):
        assert not lin[b, F:].any()                  # padding rows are zero
    assert err <= 8 * e32


# ---------------------------------------------------------------- Griffin-Lim
def _gl(a, name, n_iter, momentum, cuda, rows=None):
    ins = V.case_inputs(name)
    rows = range(len(ins)) if rows is None else rows
    mag = _padded([ins[b]["S"].astype(np.float32) for b in rows], np.float32, cuda)
    ph = _padded([ins[b]["phase0"] for b in rows], np.float32, cuda)
    frames = [ins[b]["S"].shape[0] for b in rows]
    wav = a.griffin_lim_batch(mag, frames, n_iter=n_iter, momentum=momentum, init_phase=ph)
    torch.cuda.synchronize()
    return wav, frames


@pytest.mark.parametrize("n_iter,momentum", V.LOOP_SETTINGS, ids=lambda v: str(v))
@pytest.mark.parametrize("name", V.LOOP_CASES)
def test_griffin_lim_against_float64(name, n_iter, momentum, cuda):
    hop = V.config(name)[1]
    wav, frames = _gl(_audio(name, cuda), name, n_iter, momentum, cuda)
    lengths = [hop * (F - 1) for F in frames]
    assert wav.shape == (len(frames), max(lengths))
    _check(f"griffin_lim {name} n_iter {n_iter} momentum {momentum}", wav.cpu().numpy(),
           V.loop_reference(name, n_iter, momentum), lengths)


@pytest.mark.parametrize("momentum", [0.0, 0.99])
def test_ragged_utterance_equals_itself_alone(momentum, cuda):
    """No cross-talk through padding or pairing: bit for bit."""
    a = _audio("ragged", cuda)
    hop = V.config("ragged")[1]
    batch, frames = _gl(a, "ragged", 3, momentum, cuda)
    for b, F in enumerate(frames):
        alone, _ = _gl(a, "ragged", 3, momentum, cuda, rows=[b])
        assert torch.equal(batch[b, :hop * (F - 1)], alone[0])


def test_two_runs_are_bit_identical(cuda):
    a = _audio("ragged", cuda)
    first, _ = _gl(a, "ragged", 8, 0.99, cuda)
    second, _ = _gl(a, "ragged", 8, 0.99, cuda)
    assert torch.equal(first, second)
    assert bool(torch.isfinite(first).all()) and float(first.abs().max()) > 0


@pytest.mark.parametrize("momentum", [0.0, 0.99])
def test_convergence_follows_the_oracle(momentum, cuda):
    n_fft, hop, win = V.config("a15")
    a = _audio("a15", cuda)
    u, = V.case_inputs("a15")
    S = u["S"].astype(np.float32)
    sc = {}
    for n in (1, 32):
        wav, _ = _gl(a, "a15", n, momentum, cuda)
        sc[n] = V.spectral_convergence(wav[0].cpu().numpy(), S, n_fft, hop, win)
    w64, _ = V.loop_reference("a15", 32, momentum)[0]
    ref = V.spectral_convergence(w64, S, n_fft, hop, win)
    print(f"momentum {momentum}: spectral convergence {sc[1]:.4f} after 1, {sc[32]:.4f} after 32 "
          f"iterations; float64 oracle {ref:.4f} after 32")
    assert sc[32] < sc[1]
    assert abs(sc[32] - ref) <= 0.05 * ref


# ---------------------------------------------------------------- surface
def test_inv_melspectrogram_surface(cuda):
    from sat_amd import audio as A
    m = V.mel_case()
    a = A.Audio(V.mel_hparams(), device=cuda)
    hop = V.config("ragged")[1]
    mel = np.ascontiguousarray(m["mels"][2].T)               # [num_mels, 9 frames]
    got = a.inv_melspectrogram(mel)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32
    assert got.shape == (hop * 8,) and np.isfinite(got).all() and np.abs(got).max() > 0
    dev = a.inv_melspectrogram(torch.from_numpy(mel).to(cuda))
    assert isinstance(dev, torch.Tensor) and dev.is_cuda
    assert np.array_equal(dev.cpu().numpy(), got)            # the default seed reproduces
    wav, lengths = a.inv_melspectrogram_batch(m["mels"], n_iter=4)
    assert wav.shape == (3, hop * 14)
    assert list(lengths.cpu().numpy()) == [hop * 14, hop * 5, hop * 8]
    again, _ = a.inv_melspectrogram_batch(m["mels"], n_iter=4, seed=0)
    other, _ = a.inv_melspectrogram_batch(m["mels"], n_iter=4, seed=1)
    assert torch.equal(wav, again) and not torch.equal(wav, other)
    # the padded tensor with frames is the list's batch
    padded, _ = a.inv_melspectrogram_batch(_padded(m["mels"], np.float32, cuda),
                                           frames=[15, 6, 9], n_iter=4)
    assert torch.equal(padded, wav)


def test_write_predictions_wav_files(tmp_path, cuda):
    from sat_amd import hparams, models as M, params, synthesize as S
    hp = hparams.ljspeech_hparams()
    hp.set_hparam("max_iters", 8)                            # 8 steps of 2 frames
    hp.set_hparam("average_mel_level_db", [-40.0])
    hp.set_hparam("stddev_mel_level_db", [12.0])
    model = M.tacotron_model_factory(hp, None, None, device=cuda,
                                     init_values=params.init_params(hp, seed=5))
    it = iter(M.synthetic_input_fn(hp, 2, N=11, T=16, shape="ljs", seed=4)())
    feats, _ = next(it)
    pred = model.model_fn(feats, None, M.ModeKeys.PREDICT, hp).predictions
    assert pred["mel"].shape[1] == 16
    keys = S.write_predictions([pred], str(tmp_path), hp, wav=True, n_iter=4)
    assert len(keys) == 2
    hop = int(hp.frame_shift_ms / 1000 * hp.sample_rate)
    for key in keys:
        assert (tmp_path / f"{key}.{hp.predicted_mel_extension}").stat().st_size == \
            16 * hp.num_mels * 4
        with wave.open(str(tmp_path / f"{key}.wav"), "rb") as f:
            assert f.getframerate() == hp.sample_rate
            assert f.getsampwidth() == 2 and f.getnchannels() == 1
            assert f.getnframes() == hop * 15
