"""Float64 numpy statement of the silence trim (utils/audio.py:40-49 with librosa 0.6
effects.trim semantics), written from the description in include/sat_abi.h, and the shared test
inputs.  Nothing here touches the package under test.

trim: p = frame_length // 2; np.pad(y, p, mode='reflect'); F = 1 + (L + 2p - frame_length) // hop
frames; ms[f] = mean of the frame's squares; db[f] = 10 log10(max(1e-10, ms[f])) - 10 log10(
max(1e-10, max ms)); non-silent iff db[f] > -top_db; index = (first * hop, min(L, (last + 1) *
hop)) or (0, 0); bounds = (max(index0 - pad, 0), min(index1 + pad, L)).
"""
import numpy as np

AMIN = 1e-10
SR = 48000

# (n, a, b, seed): speech on [a, b) of n samples -- in the middle, at the very start, at the very
# end of an odd length, a long odd length, a burst shorter than one frame
SIGNALS = [(9000, 2100, 6300, 0), (6000, 0, 3000, 1), (7001, 3500, 7001, 2),
           (12345, 4000, 9000, 3), (5000, 1000, 1300, 4)]
# (frame_length, hop, top_db): the VCTK setting, the default, a 10 ms / 25 ms framing whose frame
# is no multiple of the hop, an odd frame length
SETTINGS = [(1024, 256, 10), (1024, 256, 30), (400, 160, 10), (1023, 100, 20)]
# the issue's table (pad_samples = 0)
EXPECTED = {((9000, 2100, 6300, 0), (1024, 256, 10)): (1792, 6912),
            ((9000, 2100, 6300, 0), (1023, 100, 20)): (1600, 6900),
            ((7001, 3500, 7001, 2), (1024, 256, 10)): (3072, 7001),
            ((5000, 1000, 1300, 4), (400, 160, 10)): (960, 1600)}
GUARD_DB = 0.01


def sig(n, a, b, seed):
    """A 1e-3 N(0, 1) floor plus 0.5 sin(2 pi 220 t) (0.6 + 0.4 sin(2 pi 3 t)) on [a, b) at
    48 kHz, rounded to 16-bit steps; float32."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64) / SR
    y = 1e-3 * rng.standard_normal(n)
    tone = 0.5 * np.sin(2.0 * np.pi * 220.0 * t) * (0.6 + 0.4 * np.sin(2.0 * np.pi * 3.0 * t))
    y[a:b] += tone[a:b]
    return (np.rint(y * 32768.0) / 32768.0).astype(np.float32)


def frame_db(y, frame_length, hop):
    """(db [F] relative to the loudest frame, ms [F]) in float64."""
    y = np.asarray(y, np.float64)
    p = frame_length // 2
    ypad = np.pad(y, p, mode="reflect")
    F = 1 + (len(ypad) - frame_length) // hop
    idx = np.arange(F)[:, None] * hop + np.arange(frame_length)[None, :]
    ms = np.mean(np.square(ypad[idx]), axis=1)
    db = 10.0 * np.log10(np.maximum(AMIN, ms)) - 10.0 * np.log10(max(AMIN, ms.max()))
    return db, ms


def trim_bounds(y, frame_length, hop, top_db, pad_samples=0):
    db, _ = frame_db(y, frame_length, hop)
    nz = np.flatnonzero(db > -top_db)
    L = len(y)
    i0, i1 = (int(nz[0]) * hop, min(L, (int(nz[-1]) + 1) * hop)) if len(nz) else (0, 0)
    return max(i0 - pad_samples, 0), min(i1 + pad_samples, L)


def margin_db(y, frame_length, hop, top_db):
    """Distance in dB of the frame nearest the threshold."""
    db, _ = frame_db(y, frame_length, hop)
    return float(np.abs(db + top_db).min())


_SIG = {}


def signal(case):
    if case not in _SIG:
        y = sig(*case)
        y.setflags(write=False)
        _SIG[case] = y
    return _SIG[case]


_REF = {}


def reference(case, setting, pad_samples=0):
    """Bounds of a (signal, setting) pair; computed once and shared."""
    key = (case, setting, pad_samples)
    if key not in _REF:
        _REF[key] = trim_bounds(signal(case), *setting, pad_samples=pad_samples)
    return _REF[key]
