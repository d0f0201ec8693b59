"""Float64 numpy statement of the vocoder (csrc/vocoder.hip): mel -> linear magnitudes, librosa
0.6 istft, Griffin-Lim with momentum; the float32 CPU pipeline the GPU tolerances are derived from
(the same steps with torch.fft and float32 arithmetic); and the shared test inputs.

Conventions are audio_ref's: frames of n_fft every hop over the signal reflect-padded by n_fft/2, a
periodic Hann of win zero-padded to n_fft.  A spectrum of F frames comes back as hop * (F - 1)
samples, whose analysis has F frames again.
"""
import numpy as np

import audio_ref as R

TINY32 = float(np.finfo(np.float32).tiny)
LIN_FLOOR = 1e-10

# name -> (audio_ref case that carries the stft configuration, signal lengths)
CASES = {
    "d": ("d", [700]),                       # 19 frames of 256
    "b6": ("b", [1400]),                     # 6 frames of 2048
    "a15": ("a", [4000]),                    # 15: an odd count, the half-empty pair
    "c": ("c", [5000]),                      # 9 frames of 4096
    "ragged": ("a", [4000, 1400, 2300]),     # 15, 6, 9 frames
}
SINGLE = ["d", "b6", "a15", "c"]
LOOP_CASES = ["d", "a15", "c", "ragged"]
LOOP_SETTINGS = [(n_iter, momentum) for n_iter in (0, 1, 3) for momentum in (0.0, 0.99)]


def config(name):
    c = R.CASES[CASES[name][0]]
    return c["n_fft"], c["hop"], c["win"]


def signals(name):
    sr = R.CASES[CASES[name][0]]["sr"]
    return [R.make_signal(L, sr, seed=i) for i, L in enumerate(CASES[name][1])]


# ---------------------------------------------------------------- float64
def stft(y, n_fft, hop, win):
    """Complex [frames, n_fft/2 + 1], frames = 1 + len(y) // hop."""
    y = np.asarray(y, np.float64)
    ypad = np.pad(y, n_fft // 2, mode="reflect")
    frames = 1 + (len(ypad) - n_fft) // hop
    idx = np.arange(frames)[:, None] * hop + np.arange(n_fft)[None, :]
    return np.fft.rfft(ypad[idx] * R.window(win, n_fft)[None, :], axis=1)


def window_sumsquare(frames, n_fft, hop, win):
    w2 = R.window(win, n_fft) ** 2
    out = np.zeros(n_fft + hop * (frames - 1))
    for f in range(frames):
        out[f * hop:f * hop + n_fft] += w2
    return out


def istft(X, n_fft, hop, win):
    """librosa 0.6 istft: hop * (frames - 1) samples."""
    X = np.asarray(X, np.complex128)
    F = X.shape[0]
    fr = np.fft.irfft(X, n=n_fft, axis=1) * R.window(win, n_fft)[None, :]
    y = np.zeros(n_fft + hop * (F - 1))
    for f in range(F):
        y[f * hop:f * hop + n_fft] += fr[f]
    wss = window_sumsquare(F, n_fft, hop, win)
    nz = wss > TINY32
    y[nz] /= wss[nz]
    return y[n_fft // 2:n_fft // 2 + hop * (F - 1)]


def griffin_lim(S, phase0, n_iter, momentum, n_fft, hop, win):
    S = np.asarray(S, np.float64)
    angles = np.exp(1j * np.asarray(phase0, np.float64))
    prev = np.zeros_like(angles)
    c = momentum / (1.0 + momentum)
    for _ in range(n_iter):
        reb = stft(istft(S * angles, n_fft, hop, win), n_fft, hop, win)
        t = reb - c * prev
        prev = reb
        angles = t / (np.abs(t) + 1e-16)
    return istft(S * angles, n_fft, hop, win)


def spectral_convergence(x, S, n_fft, hop, win):
    """|| |stft(x)| - S || / || S ||."""
    S = np.asarray(S, np.float64)
    return float(np.linalg.norm(np.abs(stft(x, n_fft, hop, win)) - S) / np.linalg.norm(S))


def mel_sums(mel, average, stddev, ref_level_db, inv_basis32):
    """inv_basis . 10^(dB / 20) before the floor: [frames, num_freq]."""
    db = np.asarray(mel, np.float64) * np.asarray(stddev, np.float64) \
        + np.asarray(average, np.float64) + float(ref_level_db)
    return np.power(10.0, db / 20.0) @ inv_basis32.astype(np.float64).T


def mel_to_linear(mel, average, stddev, ref_level_db, inv_basis32, power):
    return np.maximum(LIN_FLOOR, mel_sums(mel, average, stddev, ref_level_db, inv_basis32)) ** power


# ---------------------------------------------------------------- float32 on the CPU
def _window32(win, n_fft):
    import torch
    return torch.from_numpy(R.window(win, n_fft).astype(np.float32))


def stft32(y, n_fft, hop, win):
    import torch
    y = torch.as_tensor(y, dtype=torch.float32)
    ypad = torch.nn.functional.pad(y[None, None, :], (n_fft // 2, n_fft // 2), mode="reflect")[0, 0]
    fr = ypad.unfold(0, n_fft, hop) * _window32(win, n_fft)[None, :]
    return torch.fft.rfft(fr, dim=1)


def istft32(X, n_fft, hop, win):
    import torch
    F = X.shape[0]
    w = _window32(win, n_fft)
    fr = torch.fft.irfft(X, n=n_fft, dim=1) * w[None, :]
    y = torch.zeros(n_fft + hop * (F - 1), dtype=torch.float32)
    wss = torch.zeros_like(y)
    for f in range(F):
        y[f * hop:f * hop + n_fft] += fr[f]
        wss[f * hop:f * hop + n_fft] += w * w
    nz = wss > TINY32
    y[nz] = y[nz] / wss[nz]
    return y[n_fft // 2:n_fft // 2 + hop * (F - 1)]


def griffin_lim32(S, phase0, n_iter, momentum, n_fft, hop, win):
    import torch
    S = torch.from_numpy(np.array(S, np.float32))
    ph = torch.from_numpy(np.array(phase0, np.float32))
    angles = torch.complex(torch.cos(ph), torch.sin(ph))
    prev = torch.zeros_like(angles)
    c = np.float32(momentum / (1.0 + momentum))
    for _ in range(n_iter):
        reb = stft32(istft32(S * angles, n_fft, hop, win), n_fft, hop, win)
        t = reb - c * prev
        prev = reb
        angles = t / (t.abs() + np.float32(1e-16))
    return istft32(S * angles, n_fft, hop, win).numpy()


def mel_to_linear32(mel, average, stddev, ref_level_db, inv_basis32, power):
    import torch
    t = lambda a: torch.from_numpy(np.array(a, np.float32))
    db = t(mel) * t(stddev) + t(average) + np.float32(ref_level_db)
    amp = torch.pow(torch.tensor(10.0, dtype=torch.float32), db * np.float32(0.05))
    acc = amp @ t(inv_basis32).t()
    return torch.pow(torch.clamp(acc, min=np.float32(LIN_FLOOR)), np.float32(power)).numpy()


def rel_error(got, want64):
    """Largest |got - want| relative to the largest |want|."""
    want64 = np.asarray(want64, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want64).max() / np.abs(want64).max())


# ---------------------------------------------------------------- shared inputs and references
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        v = make()
        for a in (v if isinstance(v, (list, tuple)) else [v]):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[key] = v
    return _CACHE[key]


def case_inputs(name):
    """Per utterance: dict(y, X = its float64 stft, S = |X|, phase0 from default_rng(1))."""
    def make():
        n_fft, hop, win = config(name)
        rng = np.random.default_rng(1)
        out = []
        for y in signals(name):
            X = stft(y, n_fft, hop, win)
            S = np.abs(X)
            ph = rng.uniform(-np.pi, np.pi, S.shape).astype(np.float32)
            for a in (X, S, ph):
                a.setflags(write=False)
            out.append(dict(y=y, X=X, S=S, phase0=ph))
        return out
    return _cached(("in", name), make)


def istft_reference(name):
    """Per utterance (float64 istft of X, float32 CPU istft of X rounded to complex64)."""
    def make():
        import torch
        n_fft, hop, win = config(name)
        return [(istft(u["X"], n_fft, hop, win),
                 istft32(torch.from_numpy(u["X"].astype(np.complex64)), n_fft, hop, win).numpy())
                for u in case_inputs(name)]
    return _cached(("istft", name), make)


def loop_reference(name, n_iter, momentum):
    """Per utterance (float64 waveform, float32 CPU waveform); magnitudes rounded to float32
    first, as the kernel receives them."""
    def make():
        n_fft, hop, win = config(name)
        out = []
        for u in case_inputs(name):
            S32 = u["S"].astype(np.float32)
            out.append((griffin_lim(S32, u["phase0"], n_iter, momentum, n_fft, hop, win),
                        griffin_lim32(S32, u["phase0"], n_iter, momentum, n_fft, hop, win)))
        return out
    return _cached(("gl", name, n_iter, momentum), make)


def e32_of(pairs):
    """e32 of a list of (float64, float32) results: the worst utterance."""
    return max(rel_error(w32, w64) for w64, w32 in pairs)


def mel_case():
    """The mel_to_linear case: the ragged batch's mels in dB, normalised by their own per-bin mean
    and standard deviation (rounded to float32, as hparams carry them).
    dict(mels = list of float32 [F_b, M], average, stddev, basis, inv_basis, ref_level_db)."""
    def make():
        c = R.CASES["a"]
        n_fft, hop, win = config("ragged")
        basis = R.cached_basis(c["sr"], n_fft, c["num_mels"])
        db = [R.melspectrogram(y, n_fft, hop, win, basis)[0] for y in signals("ragged")]
        every = np.concatenate(db, axis=0)
        average = every.mean(axis=0).astype(np.float32)
        stddev = every.std(axis=0).astype(np.float32)
        mels = [((d - average.astype(np.float64)) / stddev.astype(np.float64)).astype(np.float32)
                for d in db]
        inv = np.linalg.pinv(basis.astype(np.float64)).astype(np.float32)
        return dict(mels=mels, average=average, stddev=stddev, basis=basis, inv_basis=inv,
                    ref_level_db=R.REF_LEVEL_DB)
    return _cached(("mel",), make)


def mel_hparams():
    """hparams of the 2048 configuration with the mel case's statistics."""
    m = mel_case()
    return R.case_hparams("a", average_mel_level_db=[float(v) for v in m["average"]],
                          stddev_mel_level_db=[float(v) for v in m["stddev"]])
