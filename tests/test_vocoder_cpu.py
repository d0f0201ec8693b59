"""The vocoder without a GPU: the float64 restatement (tests/vocoder_ref.py) checks itself, the
shared inputs meet the conditions that keep the GPU tests honest, the host maths of Audio is the
inverse of the front end's, the ABI carries the new entries, the entries refuse bad arguments on
the host and write_predictions writes the reference's mel files."""
import ctypes
import os

import numpy as np
import pytest

import _sat_path

_sat_path.load()
from sat_amd import _lib  # noqa: E402

import audio_ref as R  # noqa: E402
import vocoder_ref as V  # noqa: E402
from test_abi_cpu import _c_offsets, _c_sizeof, _lib_built  # noqa: E402

needs_lib = pytest.mark.skipif(not _lib_built(), reason="libsat_hip.so not built")

CONFIGS = {"d": (256, 37, 101), "ljspeech": (2048, 275, 1102), "vctk": (4096, 600, 2400)}


# ---------------------------------------------------------------- oracle self-checks
@pytest.mark.parametrize("name", sorted(V.CASES))
def test_istft_inverts_stft(name):
    n_fft, hop, win = V.config(name)
    for u in V.case_inputs(name):
        F = u["X"].shape[0]
        x = V.istft(u["X"], n_fft, hop, win)
        assert x.shape == (hop * (F - 1),)
        assert np.abs(x - u["y"].astype(np.float64)[:hop * (F - 1)]).max() <= 1e-12
        # and its analysis has F frames again
        assert V.stft(x, n_fft, hop, win).shape == u["X"].shape


@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_window_sum_of_squares_is_never_small(cfg):
    n_fft, hop, win = CONFIGS[cfg]
    lows = []
    for F in range(n_fft // (2 * hop) + 2, n_fft // (2 * hop) + 40):
        wss = V.window_sumsquare(F, n_fft, hop, win)
        lows.append(wss[n_fft // 2:n_fft // 2 + hop * (F - 1)].min())
    print(f"{cfg}: smallest window sum of squares over the kept region {min(lows):.4f}")
    assert min(lows) >= 0.99


@pytest.mark.parametrize("momentum", [0.0, 0.99])
def test_griffin_lim_converges(momentum):
    n_fft, hop, win = V.config("a15")
    u, = V.case_inputs("a15")
    S = u["S"].astype(np.float32)
    sc = [V.spectral_convergence(V.griffin_lim(S, u["phase0"], n, momentum, n_fft, hop, win), S,
                                 n_fft, hop, win) for n in (1, 32)]
    print(f"momentum {momentum}: spectral convergence {sc[0]:.4f} after 1, {sc[1]:.4f} after 32")
    assert sc[1] < sc[0]


# ---------------------------------------------------------------- conditions of the GPU tests
@pytest.mark.parametrize("n_iter,momentum", V.LOOP_SETTINGS, ids=lambda v: str(v))
@pytest.mark.parametrize("name", V.LOOP_CASES)
def test_loop_cases_are_well_conditioned(name, n_iter, momentum):
    """8 x e32 is a meaningful bound only while the float32 pipeline itself stays near the
    float64 result: relative e32 below 1e-3, or the case says nothing."""
    e32 = V.e32_of(V.loop_reference(name, n_iter, momentum))
    print(f"{name} n_iter {n_iter} momentum {momentum}: e32 {e32:.3e}")
    assert e32 < 1e-3


def test_convergence_case_is_well_conditioned():
    for momentum in (0.0, 0.99):
        e32 = V.e32_of(V.loop_reference("a15", 32, momentum))
        print(f"a15 n_iter 32 momentum {momentum}: e32 {e32:.3e}")
        assert e32 < 1e-3


def test_mel_to_linear_case_is_clear_of_the_floor():
    m = V.mel_case()
    sums = np.concatenate([V.mel_sums(mel, m["average"], m["stddev"], m["ref_level_db"],
                                      m["inv_basis"]) for mel in m["mels"]], axis=0)
    near = float((sums < 100 * V.LIN_FLOOR).mean())
    print(f"{100 * near:.3f} % of {sums.size} bins within 100 x of the floor")
    assert near <= 0.01


# ---------------------------------------------------------------- host maths
def test_denormalize_inverts_normalize():
    from sat_amd import audio as A
    a = A.Audio(V.mel_hparams())
    S = (20.0 * np.random.default_rng(0).standard_normal((7, 80)) - 40.0).astype(np.float32)
    back = a.denormalize_mel(a.normalize_mel(S))
    assert back.dtype == np.float32
    assert np.abs(back - S).max() <= 4 * np.finfo(np.float32).eps * np.abs(S).max()
    x = np.array([-100.0, -20.0, 0.0, 6.0])
    assert np.allclose(a._amp_to_db(a._db_to_amp(x)), x, rtol=0, atol=1e-12)


def test_inverse_basis_is_a_projector():
    from sat_amd import audio as A
    a = A.Audio(R.case_hparams("a"))
    inv = a._build_inv_mel_basis()
    assert inv.dtype == np.float32 and inv.shape == (1025, 80)
    P = inv.astype(np.float64) @ a._mel_basis.astype(np.float64)
    assert np.abs(P - P.T).max() <= 1e-5
    assert np.abs(P @ P - P).max() <= 1e-5


# ---------------------------------------------------------------- ABI
ENTRIES = ["sat_mel_to_linear", "sat_istft", "sat_griffin_lim", "sat_griffin_lim_scratch_bytes",
           "sat_istft_scratch_bytes"]


def test_abi_binds_the_vocoder_entries():
    assert _lib.ABI_VERSION == 13
    assert set(ENTRIES) <= _lib.header_symbols()
    assert set(ENTRIES) <= _lib.bound_symbols()


def test_griffin_lim_struct_matches_c_layout():
    st = _lib.SatGriffinLim
    fields = [f for f, _ in st._fields_]
    assert ctypes.sizeof(st) == _c_sizeof("SatGriffinLim")
    assert [getattr(st, f).offset for f in fields] == _c_offsets("SatGriffinLim", fields)


@needs_lib
def test_scratch_queries():
    lib = _lib.load()
    al = lambda n: (n + 255) // 256 * 256   # noqa: E731
    B, F, n, hop = 3, 15, 2048, 275
    fb = al(4 * B * F * n)
    assert lib.sat_istft_scratch_bytes(B, F, n) == fb
    ph = al(8 * B * F * (n // 2 + 1))
    x = al(4 * B * hop * (F - 1))
    assert lib.sat_griffin_lim_scratch_bytes(B, F, n, hop, 0) == fb + ph + x
    assert lib.sat_griffin_lim_scratch_bytes(B, F, n, hop, 1) == fb + 2 * ph + x
    assert lib.sat_griffin_lim_scratch_bytes(-1, F, n, hop, 1) < 0


# ---------------------------------------------------------------- host-side refusals
FAKE = 64       # a non-null, aligned pointer: every refusal comes before a launch
_ids = lambda o: ",".join(f"{k}={v}" for k, v in o.items())   # noqa: E731


def _host(v):
    return None if v is None else (ctypes.c_int32 * max(len(v), 1))(*v)


def _gl_call(**over):
    """sat_griffin_lim on a well-formed 2048 descriptor (15 and 6 frames) with fake pointers."""
    frames_host = over.pop("frames_host", [15, 6])
    keep = _host(frames_host)
    d = _lib.SatGriffinLim(B=2, F_max=15, n_fft=2048, hop=275, win=1102, num_freq=1025,
                           wav_stride=275 * 14, n_iter=3, momentum=0.99, mag=FAKE,
                           init_phase=FAKE, frames=FAKE, window=FAKE, twiddle=FAKE, wav=FAKE,
                           scratch=FAKE, scratch_bytes=1 << 40)
    d.frames_host = ctypes.cast(keep, ctypes.c_void_p) if keep is not None else None
    for k, v in over.items():
        setattr(d, k, v)
    lib = _lib.load()
    return lib.sat_griffin_lim(ctypes.byref(d), None), lib.sat_last_error_string().decode()


GL_REFUSALS = [dict(mag=None), dict(init_phase=None), dict(frames=None), dict(frames_host=None),
               dict(window=None), dict(twiddle=None), dict(wav=None), dict(scratch=None),
               dict(frames_host=[15, 4]),             # 275 * 3 = 825 <= 1024
               dict(frames_host=[16, 6]),             # > F_max
               dict(wav_stride=275 * 14 - 1),
               dict(scratch_bytes=1000),
               dict(n_iter=-1),
               dict(momentum=1.0), dict(momentum=-0.1), dict(momentum=float("nan")),
               dict(momentum=float("inf")),
               dict(num_freq=1024), dict(n_fft=3000, num_freq=1501), dict(hop=0),
               dict(win=2049)]


@needs_lib
@pytest.mark.parametrize("over", GL_REFUSALS, ids=_ids)
def test_griffin_lim_entry_refuses(over):
    rc, msg = _gl_call(**over)
    assert rc != 0
    assert "sat_griffin_lim" in msg


@needs_lib
def test_five_frames_are_the_fewest_at_the_shipped_configs():
    """hop * (F - 1) > n_fft / 2: 275 * 4 = 1100 > 1024 and 600 * 4 = 2400 > 2048, while three
    hops fall short in both.  The scratch check follows, so a tiny scratch tells the two apart."""
    for n_fft, hop, win in (CONFIGS["ljspeech"], CONFIGS["vctk"]):
        base = dict(n_fft=n_fft, hop=hop, win=win, num_freq=n_fft // 2 + 1, F_max=5,
                    wav_stride=hop * 4, scratch_bytes=0)
        rc, msg = _gl_call(frames_host=[5, 5], **base)
        assert rc != 0 and "scratch" in msg
        rc, msg = _gl_call(frames_host=[5, 4], **base)
        assert rc != 0 and "reflection" in msg


def _istft_call(**over):
    a = dict(spec=FAKE, frames=FAKE, frames_host=[15, 6], B=2, F_max=15, n_fft=2048, hop=275,
             win=1102, num_freq=1025, window=FAKE, twiddle=FAKE, wav=FAKE, wav_stride=275 * 14,
             scratch=FAKE, scratch_bytes=1 << 40)
    a.update(over)
    lib = _lib.load()
    rc = lib.sat_istft(a["spec"], a["frames"], _host(a["frames_host"]), a["B"], a["F_max"],
                       a["n_fft"], a["hop"], a["win"], a["num_freq"], a["window"], a["twiddle"],
                       a["wav"], a["wav_stride"], a["scratch"], a["scratch_bytes"], None)
    return rc, lib.sat_last_error_string().decode()


ISTFT_REFUSALS = [dict(spec=None), dict(frames=None), dict(frames_host=None), dict(window=None),
                  dict(twiddle=None), dict(wav=None), dict(scratch=None),
                  dict(frames_host=[15, 4]), dict(frames_host=[16, 6]),
                  dict(wav_stride=275 * 14 - 1), dict(scratch_bytes=1000)]


@needs_lib
@pytest.mark.parametrize("over", ISTFT_REFUSALS, ids=_ids)
def test_istft_entry_refuses(over):
    rc, msg = _istft_call(**over)
    assert rc != 0
    assert "sat_istft" in msg


def _mel_call(**over):
    a = dict(mel=FAKE, frames=FAKE, frames_host=[15, 6], B=2, F_max=15, M=80, num_freq=1025,
             inv_basis=FAKE, average=FAKE, stddev=FAKE, ref_level_db=20.0, power=1.5, out=FAKE)
    a.update(over)
    lib = _lib.load()
    rc = lib.sat_mel_to_linear(a["mel"], a["frames"], _host(a["frames_host"]), a["B"], a["F_max"],
                               a["M"], a["num_freq"], a["inv_basis"], a["average"], a["stddev"],
                               a["ref_level_db"], a["power"], a["out"], None)
    return rc, lib.sat_last_error_string().decode()


MEL_REFUSALS = [dict(mel=None), dict(frames=None), dict(frames_host=None), dict(inv_basis=None),
                dict(average=None), dict(stddev=None), dict(out=None),
                dict(frames_host=[16, 6]), dict(frames_host=[15, -1]),
                dict(power=0.0), dict(power=-1.5), dict(power=float("nan"))]


@needs_lib
@pytest.mark.parametrize("over", MEL_REFUSALS, ids=_ids)
def test_mel_to_linear_entry_refuses(over):
    rc, msg = _mel_call(**over)
    assert rc != 0
    assert "sat_mel_to_linear" in msg


@needs_lib
def test_entries_accept_an_empty_batch():
    assert _gl_call(B=0, frames_host=None, frames=None, mag=None, wav=None)[0] == 0
    assert _istft_call(B=0, frames_host=None, frames=None, spec=None, wav=None)[0] == 0
    assert _mel_call(B=0, frames_host=None, frames=None, mel=None, out=None)[0] == 0


# ---------------------------------------------------------------- write_predictions, mel files
def test_write_predictions_mel_files(tmp_path):
    from sat_amd import synthesize as S
    hp = R.case_hparams("a", outputs_per_step=2)
    rng = np.random.default_rng(3)
    mel = rng.standard_normal((3, 40, 80)).astype(np.float32)
    stop = np.full((3, 20), -3.0, np.float32)
    stop[0, 4] = 5.0            # before min_iters: ignored
    stop[0, 10] = 5.0           # t == min_iters: not yet (t > min_iters)
    stop[0, 13] = 5.0           # the stop step: 14 steps, 28 frames
    stop[0, 16] = 5.0
    stop[1, 11] = 0.5           # the first step that may stop: 12 steps, 24 frames
    preds = [dict(key=np.array([b"utt-a", b"utt-b", "utt-c"], dtype=object), mel=mel,
                  stop_token=stop)]
    keys = S.write_predictions(preds, str(tmp_path), hp, wav=False)
    assert keys == ["utt-a", "utt-b", "utt-c"]
    assert S.stop_frames(stop, 2, 40) == [28, 24, 40]
    for b, (key, frames) in enumerate(zip(keys, (28, 24, 40))):
        path = tmp_path / f"{key}.{hp.predicted_mel_extension}"
        assert path.read_bytes() == mel[b, :frames].astype("<f4").tobytes()
        assert not os.path.exists(tmp_path / f"{key}.wav")
