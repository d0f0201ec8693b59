"""Float64 statement of the resampler (band-limited interpolation with a Kaiser-windowed sinc),
the float32 CPU pipeline the GPU tolerance is derived from, and the shared test inputs.  Nothing
here touches the package under test.

For rates orig -> target, L / M = target / orig reduced, scale = min(1, L / M):
  h(t) = rolloff sinc(rolloff t) kaiser(t / Z) for |t| <= Z, else 0
  y[n] = scale * sum_k x[k] h((n M / L - k) scale),   n < ceil(len L / M),   x zero outside [0, len)
The oracle evaluates this sum directly from h, with no table.  The argument of h is formed
exactly: (n M / L - k) scale = (n M - k L) / max(L, M), one integer over another.

The constants are the ones resampy's kaiser_best filter (librosa 0.6's default) is known by,
written from memory: neither package is available, so their own output is not what is pinned.
"""
import math

import numpy as np

Z = 64
BETA = 14.769656459379492
ROLLOFF = 0.9475937167399596


def ratio(orig, target):
    g = math.gcd(orig, target)
    return target // g, orig // g


def out_length(n, L, M):
    return (n * L + M - 1) // M


def h(t):
    t = np.asarray(t, np.float64)
    inside = np.abs(t) <= Z
    x = np.where(inside, t / Z, 0.0)
    w = np.i0(BETA * np.sqrt(1.0 - x * x)) / np.i0(BETA)
    return np.where(inside, ROLLOFF * np.sinc(ROLLOFF * t) * w, 0.0)


def half_width(L, M):
    """ceil(Z / scale): input samples on each side of an output that h can reach."""
    return (Z * max(L, M) + L - 1) // L


def oracle(x, orig, target):
    """float64 y of the sum above, no table; a block of outputs at a time."""
    x = np.asarray(x, np.float64)
    L, M = ratio(orig, target)
    n_out, D, reach = out_length(len(x), L, M), max(L, M), half_width(L, M) + 1
    y = np.zeros(n_out, np.float64)
    dk = np.arange(-reach, reach + 2, dtype=np.int64)[None, :]
    for s in range(0, n_out, 4096):
        n = np.arange(s, min(s + 4096, n_out), dtype=np.int64)[:, None]
        k = n * M // L + dk                                 # every input h can reach, and more
        w = h((n * M - k * L).astype(np.float64) / D)
        ok = (k >= 0) & (k < len(x))
        y[s:s + n.shape[0]] = (np.where(ok, x[np.clip(k, 0, len(x) - 1)], 0.0) * w).sum(axis=1)
    return y * min(1.0, L / M)


def table32(orig, target):
    """(table float32 [L, taps], offset): row p holds h, rounded once, at the taps an output of
    phase p = (n M) mod L reads, input floor(n M / L) + offset first."""
    L, M = ratio(orig, target)
    half = half_width(L, M)
    p = np.arange(L, dtype=np.int64)[:, None]
    j = np.arange(2 * half + 2, dtype=np.int64)[None, :]
    return h((p + (half - j) * L).astype(np.float64) / max(L, M)).astype(np.float32), -half


def pipeline32(x, orig, target):
    """The product's arithmetic on the CPU: float32 table; per output 64 interleaved float32
    partial sums (partial l takes taps l, l + 64, .. in order, each step one fused multiply-add),
    a butterfly over the 64 (distances 32, 16, .. 1), times scale in float32."""
    x = np.asarray(x, np.float32)
    L, M = ratio(orig, target)
    table, offset = table32(orig, target)
    taps = table.shape[1]
    n_out = out_length(len(x), L, M)
    rounds = (taps + 63) // 64
    n = np.arange(n_out, dtype=np.int64)
    i0, ph = n * M // L, n * M % L
    k = i0[:, None] + offset + np.arange(rounds * 64, dtype=np.int64)[None, :]
    ok = (k >= 0) & (k < len(x)) & (np.arange(rounds * 64)[None, :] < taps)
    xs = np.where(ok, x[np.clip(k, 0, len(x) - 1)], np.float32(0.0)).astype(np.float64)
    tp = np.zeros((L, rounds * 64), np.float64)
    tp[:, :taps] = table
    acc = np.zeros((n_out, 64), np.float32)
    for r in range(rounds):
        sl = slice(64 * r, 64 * r + 64)
        # a product of two float32 is exact in float64; one rounding of the sum: the fma
        acc = (tp[ph, sl] * xs[:, sl] + acc.astype(np.float64)).astype(np.float32)
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lanes ^ o]
    return acc[:, 0] * np.float32(min(1.0, L / M))


def sine(n, rate, freq):
    return np.sin(2.0 * np.pi * freq * np.arange(n, dtype=np.float64) / rate)


def interior(n_in, orig, target):
    """Slice of the output clear of the zero padding at the utterance's edges:
    ceil(Z / scale) * L / M + 5 samples off each end."""
    L, M = ratio(orig, target)
    m = int(math.ceil(half_width(L, M) * L / M)) + 5
    return slice(m, out_length(n_in, L, M) - m)


# ---- shared GPU-test inputs: random signals in [-1, 1], each with its oracle and e32 once
RATES = [(48000, 22050), (16000, 22050), (44100, 22050)]
LENGTHS = (1, 700, 2049)
_CASE = {}


def signal(n, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, n).astype(np.float32)


def reference(orig, target, lengths=LENGTHS, seed=0):
    """Per utterance dict(x, y64, y32); computed once, shared and read-only."""
    key = (orig, target, tuple(lengths), seed)
    if key not in _CASE:
        out = []
        for i, n in enumerate(lengths):
            x = signal(n, 1000 * seed + 17 * i + orig % 97)
            y64, y32 = oracle(x, orig, target), pipeline32(x, orig, target)
            for a in (x, y64, y32):
                a.setflags(write=False)
            out.append(dict(x=x, y64=y64, y32=y32))
        _CASE[key] = out
    return _CASE[key]


def e32(refs):
    """Largest |float32 pipeline - oracle| over the utterances."""
    return max(float(np.abs(r["y32"] - r["y64"]).max()) for r in refs)
