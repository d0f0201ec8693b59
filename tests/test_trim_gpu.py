"""sat_trim_bounds and the segment-reading sat_melspec on the GPU against the float64 restatement
(tests/trim_ref.py).

Bounds are compared exactly.  That is fair because tests/test_trim_cpu.py asserts that no frame
of these cases is within 0.01 dB of the threshold in float64, ten times the worst fp32 error of a
sum of 4096 squares (4096 * 2^-24 relative, about 1e-3 dB).  The frame mean squares themselves are
held to that same worst-case bound, 4096 * 2^-24 relative."""
import ctypes

import numpy as np
import pytest
import torch

import audio_ref as R
import trim_ref as T

pytestmark = pytest.mark.gpu

MS_RTOL = 4096 * 2.0 ** -24


def _run(cuda, ys, setting, pad_samples=0, stride=None, poison=None):
    """(bounds [B, 2], frame_ms [B, F_max]) of a list of waveforms in ONE entry call; samples past
    an utterance's length are set to ``poison``."""
    from sat_amd import kernels as K
    frame_length, hop, top_db = setting
    lengths = [len(y) for y in ys]
    stride = stride or max(lengths)
    host = np.zeros((len(ys), stride), np.float32)
    if poison is not None:
        host[:] = poison
    for b, y in enumerate(ys):
        host[b, :len(y)] = y
    wav = torch.from_numpy(host).to(cuda)
    dlen = torch.tensor(lengths, dtype=torch.int32, device=cuda)
    F_max = 1 + (max(lengths) + 2 * (frame_length // 2) - frame_length) // hop
    bounds = torch.full((len(ys), 2), -7, dtype=torch.int32, device=cuda)
    ms = torch.full((len(ys), F_max), -1.0, device=cuda)
    K.trim_bounds(wav, dlen, lengths, frame_length=frame_length, hop=hop, top_db=top_db,
                  pad_samples=pad_samples, bounds=bounds, frame_ms=ms)
    torch.cuda.synchronize()
    return bounds.cpu().numpy(), ms.cpu().numpy()


def _check_ms(ms_row, y, frame_length, hop):
    _, want = T.frame_db(y, frame_length, hop)
    got = ms_row[:len(want)].astype(np.float64)
    assert np.all(np.abs(got - want) <= MS_RTOL * want + 1e-30)
    assert (ms_row[len(want):] == -1.0).all()           # columns past the frame count: untouched


@pytest.mark.parametrize("setting", T.SETTINGS, ids=str)
@pytest.mark.parametrize("case", T.SIGNALS, ids=str)
def test_bounds_equal_the_restatement(case, setting, cuda):
    y = T.signal(case)
    bounds, ms = _run(cuda, [y], setting)
    print(f"{case} {setting}: bounds {tuple(bounds[0])}, want {T.reference(case, setting)}")
    _check_ms(ms[0], y, setting[0], setting[1])
    assert tuple(bounds[0]) == T.reference(case, setting)
    if (case, setting) in T.EXPECTED:
        assert tuple(bounds[0]) == T.EXPECTED[(case, setting)]


def test_zero_utterance(cuda):
    bounds, ms = _run(cuda, [np.zeros(4000, np.float32)], (1024, 256, 10))
    assert tuple(bounds[0]) == (0, 4000) and not ms.any()
    bounds, _ = _run(cuda, [np.zeros(4000, np.float32)], (1024, 256, 10), pad_samples=300)
    assert tuple(bounds[0]) == (0, 4000)
    # top_db = 0: no frame is above the loudest one -- index (0, 0), widened by the margin only
    bounds, _ = _run(cuda, [T.signal(T.SIGNALS[0])], (1024, 256, 0), pad_samples=300)
    assert tuple(bounds[0]) == (0, 300)


@pytest.mark.parametrize("pad_samples", [0, 300])
@pytest.mark.parametrize("setting", T.SETTINGS, ids=str)
def test_ragged_batch_in_one_call(setting, pad_samples, cuda):
    """All five signals in one call, in rows longer than every utterance and loud past each
    utterance's end (a read past the length would move the loudest frame).  pad_samples = 300
    clamps at 0 for the signal that starts with speech and at L for the one that ends with it."""
    ys = [T.signal(c) for c in T.SIGNALS]
    bounds, ms = _run(cuda, ys, setting, pad_samples=pad_samples, stride=12800, poison=30.0)
    want = [T.reference(c, setting, pad_samples) for c in T.SIGNALS]
    assert [tuple(b) for b in bounds] == want
    for b, y in enumerate(ys):
        _check_ms(ms[b], y, setting[0], setting[1])
    if pad_samples:
        assert want[1][0] == 0 and want[2][1] == len(ys[2])
    again, ms2 = _run(cuda, ys, setting, pad_samples=pad_samples, stride=12800, poison=30.0)
    assert np.array_equal(again, bounds) and np.array_equal(ms2, ms)     # same bits every run


# every path of the frame-energy pass: per-hop partial sums with the smallest and the largest
# ratio that takes them (1 and 1024), the per-frame pass just above (1025), the smallest frame,
# a hop longer than the frame, and more than one tile of 64 frames
PATHS = [(256, 256), (2048, 2), (2050, 2), (2, 1), (64, 100), (1024, 32)]


@pytest.mark.parametrize("frame_length,hop", PATHS)
def test_frame_energies_on_every_path(frame_length, hop, cuda):
    ys = [T.signal(T.SIGNALS[0])[:3000], T.signal(T.SIGNALS[4])[:2049]]
    _, ms = _run(cuda, ys, (frame_length, hop, 10))
    for b, y in enumerate(ys):
        _check_ms(ms[b], y, frame_length, hop)


def test_empty_batch_is_accepted(cuda):
    from sat_amd import kernels as K
    K.trim_bounds(torch.empty(0, 16, device=cuda), torch.empty(0, dtype=torch.int32, device=cuda),
                  [], frame_length=1024, hop=256, top_db=10, pad_samples=0,
                  bounds=torch.empty(0, 2, dtype=torch.int32, device=cuda),
                  frame_ms=torch.empty(0, 4, device=cuda))
    torch.cuda.synchronize()


# ---------------------------------------------------------------- refusals
def _trim_args(cuda, **over):
    """A well-formed small call; ``over`` replaces single arguments (None: a null pointer)."""
    a = dict(lengths_host=[3000, 900], B=2, wav_stride=3000, frame_length=1024, hop=256,
             top_db=10.0, pad_samples=0, ms_stride=12)
    t = dict(wav=torch.zeros(2, 3000, device=cuda),
             lengths=torch.tensor([3000, 900], dtype=torch.int32, device=cuda),
             bounds=torch.full((2, 2), -7, dtype=torch.int32, device=cuda),
             frame_ms=torch.full((2, 12), -1.0, device=cuda))
    ptr = {k: v.data_ptr() for k, v in t.items()}
    for k, v in over.items():
        (ptr if k in ptr else a)[k] = v
    return a, t, ptr


def _trim_call(a, ptr):
    from sat_amd import _lib
    host = a["lengths_host"]
    if host is not None:
        host = (ctypes.c_int32 * max(len(host), 1))(*host)
    lib = _lib.load()
    rc = lib.sat_trim_bounds(ptr["wav"], ptr["lengths"], host, a["B"], a["wav_stride"],
                             a["frame_length"], a["hop"], a["top_db"], a["pad_samples"],
                             ptr["bounds"], ptr["frame_ms"], a["ms_stride"],
                             torch.cuda.current_stream().cuda_stream)
    return rc, lib.sat_last_error_string().decode()


TRIM_REFUSALS = [dict(wav=None), dict(lengths=None), dict(lengths_host=None), dict(bounds=None),
                 dict(frame_ms=None), dict(B=-1), dict(B=65536, lengths_host=[3000] * 65536),
                 dict(hop=0), dict(frame_length=1), dict(top_db=-1.0), dict(top_db=float("nan")),
                 dict(top_db=float("inf")), dict(pad_samples=-1),
                 dict(lengths_host=[3000, 512]), dict(lengths_host=[3001, 900]),
                 dict(ms_stride=11)]


@pytest.mark.parametrize("over", TRIM_REFUSALS, ids=[str(i) for i in range(len(TRIM_REFUSALS))])
def test_trim_refusals_launch_nothing(over, cuda):
    from sat_amd import _lib
    a, t, ptr = _trim_args(cuda, **over)
    rc, msg = _trim_call(a, ptr)
    assert rc == _lib.SAT_ERR_ARGUMENT and "sat_trim_bounds" in msg
    torch.cuda.synchronize()
    assert (t["bounds"] == -7).all() and (t["frame_ms"] == -1.0).all()   # nothing was written


def test_well_formed_small_trim_call_is_accepted(cuda):
    """The refusal tests' base call itself runs: each refusal is caused by its one change."""
    a, t, ptr = _trim_args(cuda)
    rc, msg = _trim_call(a, ptr)
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert t["bounds"].cpu().tolist() == [[0, 3000], [0, 900]]           # zeros: all non-silent
    fm = t["frame_ms"].cpu().numpy()
    assert not fm[0].any() and not fm[1, :4].any() and (fm[1, 4:] == -1.0).all()


def _melspec_args(cuda, lengths, offsets=None):
    """The small well-formed sat_melspec call of tests/test_audio_gpu.py (n_fft 64)."""
    t = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=cuda)
    out = torch.full((2, 26, 4), 7.0, device=cuda)
    kw = dict(n_fft=64, hop=16, win=48, window=t(8192), twiddle=t(8192), basis=t(4, 33),
              band_lo=t(4, dt=torch.int32), band_hi=t(4, dt=torch.int32), ref_level_db=20.0,
              amp_floor=1e-5, out=out)
    if offsets is not None:
        kw.update(offsets=torch.tensor(offsets, dtype=torch.int32, device=cuda),
                  offsets_host=offsets)
    return (t(2, 400), torch.tensor(lengths, dtype=torch.int32, device=cuda), lengths), kw, out


@pytest.mark.parametrize("lengths,offsets", [([300, 100], [-1, 0]), ([400, 100], [0, 301]),
                                             ([400, 100], [1, 0])])
def test_melspec_segment_refusals_launch_nothing(lengths, offsets, cuda):
    from sat_amd import _lib, kernels as K
    args, kw, out = _melspec_args(cuda, lengths, offsets)
    with pytest.raises(_lib.SatLibraryError) as e:
        K.melspec(*args, **kw)
    assert e.value.rc == _lib.SAT_ERR_ARGUMENT and "sat_melspec" in str(e.value)
    torch.cuda.synchronize()
    assert (out == 7.0).all()


def test_melspec_offsets_need_both_copies(cuda):
    from sat_amd import _lib, kernels as K
    args, kw, out = _melspec_args(cuda, [300, 100], [50, 0])
    for drop in ("offsets", "offsets_host"):
        with pytest.raises(_lib.SatLibraryError) as e:
            K.melspec(*args, **{k: v for k, v in kw.items() if k != drop})
        assert e.value.rc == _lib.SAT_ERR_ARGUMENT
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    K.melspec(*args, **kw)                               # the pair together is accepted
    o = out.cpu().numpy()
    assert (o[0, :19] == np.float32(-120.0)).all() and not o[0, 19:].any()


# ---------------------------------------------------------------- Audio: trim, segments
TRIM_HP = dict(trim_top_db=30, trim_frame_length=1024, trim_hop_length=256)


def _audio(cuda, **extra):
    from sat_amd import audio as A
    return A.Audio(R.case_hparams("a", **dict(TRIM_HP, **extra)), device=cuda)


@pytest.mark.parametrize("num_silent_frames", [0, 1])
def test_segment_mel_equals_sliced_mel(num_silent_frames, cuda):
    """melspectrogram_batch(wav, bounds=...) reads the trimmed segments in place: the same bits
    as the mel of the sliced waveforms (reflection inside the segment, not into its
    surroundings), through trim_batch's device tensors and through a list with host bounds."""
    a = _audio(cuda, num_silent_frames=num_silent_frames)
    ys = [T.signal(c) for c in T.SIGNALS]
    pad = int(num_silent_frames * 12.5 * 22050 / 1000)
    wav, bounds = a.trim_batch(ys)
    assert wav.shape == (5, 12345) and bounds.dtype == torch.int32 and bounds.is_cuda
    bh = bounds.cpu().numpy()
    assert [tuple(b) for b in bh] == [T.reference(c, (1024, 256, 30), pad) for c in T.SIGNALS]
    mel, frames, mag = a.melspectrogram_batch(wav, bounds=bounds, return_magnitudes=True)
    sliced = [y[s:e] for y, (s, e) in zip(ys, bh)]
    mel2, frames2, mag2 = a.melspectrogram_batch(sliced, return_magnitudes=True)
    assert torch.equal(frames, frames2) and torch.equal(mel, mel2) and torch.equal(mag, mag2)
    assert frames.cpu().tolist() == [1 + len(s) // 275 for s in sliced]
    mel3, frames3 = a.melspectrogram_batch(ys, bounds=bh)
    assert torch.equal(mel3, mel) and torch.equal(frames3, frames)


def test_null_offsets_are_the_unchanged_call(cuda):
    """offsets = NULL, whether left out (the keyword set of before) or passed as None, and
    all-zero offsets give the same bits."""
    from sat_amd import kernels as K
    a = _audio(cuda)
    ys = [T.signal(c) for c in T.SIGNALS[:3]]
    lengths = [len(y) for y in ys]
    wav, _ = a._upload(ys, "test")
    n_fft, hop, win = a._stft_parameters()
    plan = a._plan(cuda)
    F_max = 1 + max(lengths) // hop
    dlen = torch.tensor(lengths, dtype=torch.int32, device=cuda)
    kw = dict(n_fft=n_fft, hop=hop, win=win, window=plan["window"], twiddle=plan["twiddle"],
              basis=plan["basis"], band_lo=plan["band_lo"], band_hi=plan["band_hi"],
              ref_level_db=20, amp_floor=1e-5)
    outs = []
    for extra in ({}, dict(offsets=None, offsets_host=None),
                  dict(offsets=torch.zeros(3, dtype=torch.int32, device=cuda),
                       offsets_host=[0, 0, 0])):
        out = torch.empty(3, F_max, 80, device=cuda)
        K.melspec(wav, dlen, lengths, out=out, **kw, **extra)
        outs.append(out)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    mel, _ = a.melspectrogram_batch(ys)
    assert torch.equal(mel, outs[0])


def test_audio_trim_surface(cuda):
    """Audio.trim(y) = y[start:stop]: numpy in, numpy out; device tensor in, a view of it out."""
    a = _audio(cuda)
    case = T.SIGNALS[3]
    y = T.signal(case)
    s, e = T.reference(case, (1024, 256, 30))
    got = a.trim(y)
    assert isinstance(got, np.ndarray) and np.array_equal(got, y[s:e])
    d = torch.from_numpy(np.array(y)).to(cuda)
    dv = a.trim(d)
    assert isinstance(dv, torch.Tensor) and dv.is_cuda
    assert dv.data_ptr() == d.data_ptr() + 4 * s and dv.shape == (e - s,)
    assert np.array_equal(dv.cpu().numpy(), y[s:e])
