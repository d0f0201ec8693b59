"""The silence trim without a GPU: the float64 restatement (tests/trim_ref.py) is pinned to the
bounds worked out by hand from librosa 0.6's effects.trim, no frame of the shared cases lies
within the guard band of the threshold (so the GPU test may demand exact bounds), the ABI carries
the new entry and the longer SatMelSpec, and both entries refuse bad arguments on the host."""
import ctypes

import numpy as np
import pytest

import _sat_path

_sat_path.load()
from sat_amd import _lib  # noqa: E402

import trim_ref as T  # noqa: E402
from test_abi_cpu import _c_offsets, _c_sizeof, _lib_built  # noqa: E402

needs_lib = pytest.mark.skipif(not _lib_built(), reason="libsat_hip.so not built")


@pytest.mark.parametrize("key", sorted(T.EXPECTED), ids=str)
def test_restatement_gives_the_pinned_bounds(key):
    case, setting = key
    assert T.reference(case, setting) == T.EXPECTED[key]


def test_zero_utterance_is_non_silent_throughout():
    """max(1e-10, 0) against itself: 0 dB > -top_db in every frame, as in librosa."""
    assert T.trim_bounds(np.zeros(4000, np.float32), 1024, 256, 10) == (0, 4000)
    assert T.trim_bounds(np.zeros(4000, np.float32), 1024, 256, 10, pad_samples=300) == (0, 4000)
    # top_db = 0: nothing is louder than the loudest frame -- no non-silent frame, index (0, 0)
    assert T.trim_bounds(T.signal(T.SIGNALS[0]), 1024, 256, 0) == (0, 0)
    assert T.trim_bounds(T.signal(T.SIGNALS[0]), 1024, 256, 0, pad_samples=300) == (0, 300)


@pytest.mark.parametrize("setting", T.SETTINGS, ids=str)
@pytest.mark.parametrize("case", T.SIGNALS, ids=str)
def test_no_frame_within_the_guard_band(case, setting):
    """An fp32 sum of at most 4096 squares is off by at most about 4096 * 2^-24 relative, 1e-3
    dB; a frame 0.01 dB from the threshold is ten times clear of that.  A case inside the band
    fails here: it may not be dropped."""
    m = T.margin_db(T.signal(case), *setting)
    print(f"{case} {setting}: nearest frame {m:.3f} dB from the threshold")
    assert setting[0] <= 4096
    assert m >= T.GUARD_DB


def test_padding_and_frame_count_of_the_restatement():
    """Odd frame lengths pad by frame_length // 2 on both sides: F = 1 + (L + 2p - n) // hop."""
    y = T.signal(T.SIGNALS[2])
    for n, hop in ((1023, 100), (1024, 256), (400, 160), (2, 1)):
        db, ms = T.frame_db(y, n, hop)
        assert len(ms) == 1 + (len(y) + 2 * (n // 2) - n) // hop
    # the first frame of an even length is centred on sample 0: y[p..1] mirrored, then y[0..p-1]
    _, ms = T.frame_db(y, 8, 4)
    want = np.mean(np.square(np.concatenate([y[4:0:-1], y[:4]]).astype(np.float64)))
    assert ms[0] == pytest.approx(want, rel=1e-15)


def test_pad_samples_follow_the_reference_formula():
    """num_sil_samples = int(num_silent_frames * frame_shift_ms * sample_rate / 1000)."""
    assert int(2 * 12.5 * 48000 / 1000) == 1200
    assert T.trim_bounds(T.signal(T.SIGNALS[0]), 1024, 256, 10, pad_samples=1200) == (592, 8112)
    assert T.trim_bounds(T.signal(T.SIGNALS[0]), 1024, 256, 10, pad_samples=3000) == (0, 9000)


# ---------------------------------------------------------------- ABI
def test_abi_13_binds_the_trim_entry():
    assert _lib.ABI_VERSION == 13
    assert "sat_trim_bounds" in _lib.header_symbols()
    assert len(_lib.SIGNATURES["sat_trim_bounds"]) == 13


def test_melspec_struct_matches_c_layout():
    st = _lib.SatMelSpec
    fields = [f for f, _ in st._fields_]
    assert fields[-2:] == ["offsets", "offsets_host"]
    assert ctypes.sizeof(st) == _c_sizeof("SatMelSpec")
    assert [getattr(st, f).offset for f in fields] == _c_offsets("SatMelSpec", fields)


# ---------------------------------------------------------------- host-side refusals
def _trim_call(**over):
    """sat_trim_bounds with fake non-null pointers: every refusal comes before a launch, so a
    refused call touches no device."""
    fake = ctypes.c_void_p(64)
    a = dict(wav=fake, lengths=fake, lengths_host=[3000, 900], B=2, wav_stride=3000,
             frame_length=1024, hop=256, top_db=10.0, pad_samples=0, bounds=fake, frame_ms=fake,
             ms_stride=12)
    a.update(over)
    host = a["lengths_host"]
    if host is not None:
        host = (ctypes.c_int32 * max(len(host), 1))(*host)
    lib = _lib.load()
    rc = lib.sat_trim_bounds(a["wav"], a["lengths"], host, a["B"], a["wav_stride"],
                             a["frame_length"], a["hop"], a["top_db"], a["pad_samples"],
                             a["bounds"], a["frame_ms"], a["ms_stride"], None)
    return rc, lib.sat_last_error_string().decode()


TRIM_REFUSALS = [dict(wav=None), dict(lengths=None), dict(lengths_host=None), dict(bounds=None),
                 dict(frame_ms=None), dict(B=-1), dict(B=65536, lengths_host=[3000] * 65536),
                 dict(hop=0), dict(frame_length=1), dict(top_db=-1.0), dict(top_db=float("nan")),
                 dict(top_db=float("inf")), dict(pad_samples=-1),
                 dict(lengths_host=[3000, 512]),            # <= frame_length / 2
                 dict(lengths_host=[3001, 900]),            # > wav_stride
                 dict(ms_stride=11)]                        # the longest utterance has 12 frames


@needs_lib
@pytest.mark.parametrize("over", TRIM_REFUSALS, ids=lambda o: ",".join(o))
def test_trim_entry_refuses(over):
    rc, msg = _trim_call(**over)
    assert rc == _lib.SAT_ERR_ARGUMENT
    assert "sat_trim_bounds" in msg


@needs_lib
def test_trim_entry_accepts_an_empty_batch():
    rc, _ = _trim_call(B=0, wav=None, lengths=None, lengths_host=None, bounds=None, frame_ms=None)
    assert rc == 0


def _melspec_desc(**over):
    fake = 64
    lengths = over.pop("lengths_host", [400, 100])
    offsets = over.pop("offsets_host", None)
    d = _lib.SatMelSpec(B=2, wav_stride=400, n_fft=64, hop=16, win=48, num_mels=4, num_freq=33,
                        F_max=26, ref_level_db=20.0, amp_floor=1e-5, wav=fake, lengths=fake,
                        window=fake, twiddle=fake, basis=fake, band_lo=fake, band_hi=fake,
                        out=fake)
    keep = [(ctypes.c_int32 * 2)(*lengths)]
    d.lengths_host = ctypes.cast(keep[0], ctypes.c_void_p)
    if offsets is not None:
        keep.append((ctypes.c_int32 * 2)(*offsets))
        d.offsets_host = ctypes.cast(keep[1], ctypes.c_void_p)
    for k, v in over.items():
        setattr(d, k, v)
    return d, keep


MELSPEC_SEGMENT_REFUSALS = [
    dict(offsets=64, offsets_host=[-1, 0], lengths_host=[300, 100]),      # a negative offset
    dict(offsets=64, offsets_host=[0, 301], lengths_host=[400, 100]),     # 301 + 100 > 400
    dict(offsets=64, offsets_host=[1, 0], lengths_host=[400, 100]),       # 1 + 400 > 400
    dict(offsets=64),                                                     # no host copy
    dict(offsets_host=[0, 0]),                                            # no device copy
]


@needs_lib
@pytest.mark.parametrize("over", MELSPEC_SEGMENT_REFUSALS,
                         ids=[str(i) for i in range(len(MELSPEC_SEGMENT_REFUSALS))])
def test_melspec_entry_refuses_bad_segments(over):
    d, keep = _melspec_desc(**over)
    lib = _lib.load()
    assert lib.sat_melspec(ctypes.byref(d), None) == _lib.SAT_ERR_ARGUMENT
    assert b"sat_melspec" in lib.sat_last_error_string()
