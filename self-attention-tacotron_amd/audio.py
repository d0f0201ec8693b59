"""Audio front end: ``utils/audio.py`` without librosa / scipy.

``Audio(hparams)`` keeps the reference's surface (``utils/audio.py:23-73``): ``_stft_parameters``,
``_build_mel_basis``, ``load_wav``, ``save_wav``, ``trim``, ``melspectrogram``, ``normalize_mel``,
``_amp_to_db``, ``_linear_to_mel``.  The feature extraction itself -- reflect padding, framing,
window, FFT, magnitude, mel projection, dB -- is one libsat_hip launch (``csrc/audio.hip``) for a
whole batch of utterances (``melspectrogram_batch``); torch only allocates and copies.  There is
no host fallback: without the library or a GPU ``melspectrogram`` and ``trim`` raise.

``trim`` is librosa 0.6's ``effects.trim`` plus ``num_silent_frames`` of margin
(``utils/audio.py:40-49``), decided on the GPU for a whole batch (``trim_batch``,
``csrc/trim.hip``): frame mean squares of the reflect-padded utterance, the dB test against the
loudest frame, first and last non-silent frame.  ``trim_batch`` returns the uploaded waveforms and
their ``(start, stop)`` bounds; ``melspectrogram_batch(wav, bounds=...)`` then reads each
utterance's segment in place, so the VCTK path is one upload, the trim launch, one read-back of
the bounds (the host needs the lengths and the largest frame count) and one mel launch.

The way back (``csrc/vocoder.hip``) is what a synthesis needs and the reference leaves to an
external vocoder: ``inv_melspectrogram(_batch)`` = ``denormalize_mel`` and ``_db_to_amp``, the
pseudo-inverse of the mel basis (``mel_to_linear_batch``) and Griffin-Lim (``griffin_lim_batch``,
one entry call for the whole loop, built on ``istft_batch``'s kernels).  An utterance of F frames
comes back as ``hop * (F - 1)`` samples, whose analysis has F frames again.

Resampling (``csrc/resample.hip``) is opt-in.  The reference's ``load_wav`` is
``librosa.core.load(path, sr=hparams.sample_rate)``, which resamples whatever it reads; here
``load_wav(path)`` still raises ``ValueError`` on a file at another rate, ``load_wav(path,
resample=True)`` brings it to ``hparams.sample_rate``, and ``resample_batch`` does so for a list of
utterances with one upload and one launch per distinct source rate, returning device tensors that
``trim_batch`` and ``melspectrogram_batch`` take as they are.  The filter is band-limited
interpolation with a Kaiser-windowed sinc (``resample_filter``): for the ratio reduced to L / M the
output times have only L distinct fractional parts, so the table holds the exact filter values
of each phase and nothing is interpolated between its entries.  Its three constants are the ones
librosa 0.6's default resampler (resampy's ``kaiser_best``) is known by, written from memory:
neither librosa nor resampy was available when this was built, so equality with their output is
not pinned.  What is pinned is a float64 evaluation of the same sum straight from the filter
function and its tone and alias properties (tests/resample_ref.py).
"""

from __future__ import annotations

import math
import wave
from collections import namedtuple

import numpy as np

AMP_FLOOR = 1e-5            # utils/audio.py:73

# Kaiser-windowed sinc of the resampler: zero crossings per side, the window's beta, the cut-off
# as a fraction of the lower Nyquist frequency.  The values resampy's kaiser_best filter (librosa
# 0.6's default res_type) is known by -- from memory, neither package was at hand to check.
RESAMPLE_ZEROS = 64
RESAMPLE_BETA = 14.769656459379492
RESAMPLE_ROLLOFF = 0.9475937167399596
RESAMPLE_MAX_PHASES = 1024

ResampleFilter = namedtuple("ResampleFilter", ["table", "L", "M", "taps", "offset"])


def resample_ratio(orig: int, target: int):
    """``target / orig`` reduced to ``(L, M)``: 48000 -> 22050 is (147, 320)."""
    orig, target = int(orig), int(target)
    if orig < 1 or target < 1:
        raise ValueError(f"resample: rates {orig} Hz -> {target} Hz must be positive")
    g = math.gcd(orig, target)
    return target // g, orig // g


def resampled_length(n: int, L: int, M: int) -> int:
    """``ceil(n L / M)``: librosa.resample's output length."""
    return -((-int(n) * int(L)) // int(M))


def resample_kernel_function(t):
    """``h(t) = rolloff sinc(rolloff t) kaiser(t / Z)`` for ``|t| <= Z``, else 0 (float64; t in
    periods of the lower of the two rates)."""
    t = np.asarray(t, np.float64)
    inside = np.abs(t) <= RESAMPLE_ZEROS
    x = np.where(inside, t / RESAMPLE_ZEROS, 0.0)
    window = np.i0(RESAMPLE_BETA * np.sqrt(1.0 - x * x)) / np.i0(RESAMPLE_BETA)
    return np.where(inside, RESAMPLE_ROLLOFF * np.sinc(RESAMPLE_ROLLOFF * t) * window, 0.0)


_FILTERS = {}


def resample_filter(orig: int, target: int) -> ResampleFilter:
    """The polyphase table of ``orig`` Hz -> ``target`` Hz: ``(table, L, M, taps, offset)``.

    With ``L / M`` the reduced ratio and ``scale = min(1, L / M)``, output n lies at input time
    ``n M / L = i0 + p / L`` (``i0 = floor(n M / L)``, phase ``p = (n M) mod L``) and is
    ``scale * sum_j table[p, j] * x[i0 + offset + j]``: ``table[p, j] = h((p / L - offset - j) *
    scale)``, ``offset = -ceil(Z / scale)`` and ``taps = 2 ceil(Z / scale) + 2`` cover the support
    of h for every phase.  The position is formed as one exact integer over ``max(L, M)``, so row
    p is row L - p reversed bit for bit.  float64 throughout, rounded once to float32 [L, taps]."""
    key = (int(orig), int(target))
    f = _FILTERS.get(key)
    if f is None:
        L, M = resample_ratio(orig, target)
        if L > RESAMPLE_MAX_PHASES:
            raise ValueError(f"resample: {orig} Hz -> {target} Hz reduces to {L}/{M}, a table of "
                             f"{L} phases (at most {RESAMPLE_MAX_PHASES}): the two rates are not "
                             "sensibly related")
        half = -((-RESAMPLE_ZEROS * max(L, M)) // L)        # ceil(Z / scale)
        taps = 2 * half + 2
        p = np.arange(L, dtype=np.int64)[:, None]
        j = np.arange(taps, dtype=np.int64)[None, :]
        t = (p + (half - j) * L).astype(np.float64) / float(max(L, M))
        table = resample_kernel_function(t).astype(np.float32)
        table.setflags(write=False)
        f = _FILTERS[key] = ResampleFilter(table, L, M, taps, -half)
    return f


def hz_to_mel(f):
    """Slaney scale: linear at 200/3 Hz per mel below 1000 Hz, logarithmic above (step ln 6.4 / 27)."""
    f = np.asarray(f, np.float64)
    f_sp, min_log_hz = 200.0 / 3.0, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0
    return np.where(f >= min_log_hz,
                    min_log_mel + np.log(np.maximum(f, min_log_hz) / min_log_hz) / logstep,
                    f / f_sp)


def mel_to_hz(m):
    m = np.asarray(m, np.float64)
    f_sp, min_log_hz = 200.0 / 3.0, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def mel_filterbank(sr: int, n_fft: int, n_mels: int) -> np.ndarray:
    """``librosa.filters.mel(sr, n_fft, n_mels)`` at its defaults (fmin 0, fmax sr/2, Slaney scale
    and area normalisation): triangles between consecutive mel points, row i scaled by
    2 / (f[i+2] - f[i]).  Computed in float64, returned as float32 [n_mels, n_fft/2 + 1]."""
    fftfreqs = np.linspace(0.0, sr / 2.0, 1 + n_fft // 2)
    mel_f = mel_to_hz(np.linspace(hz_to_mel(0.0), hz_to_mel(sr / 2.0), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fftfreqs[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    weights = np.maximum(0.0, np.minimum(lower, upper))
    weights *= (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]
    return weights.astype(np.float32)


def band_limits(basis: np.ndarray):
    """First bin with a nonzero weight and one past the last, per row (lo == hi: an empty row)."""
    nz = basis != 0
    any_ = nz.any(axis=1)
    lo = np.where(any_, nz.argmax(axis=1), 0)
    hi = np.where(any_, basis.shape[1] - nz[:, ::-1].argmax(axis=1), 0)
    return lo.astype(np.int32), hi.astype(np.int32)


def hann_window(win_length: int, n_fft: int) -> np.ndarray:
    """Periodic Hann of ``win_length`` centred in ``n_fft`` ((n_fft - win) // 2 zeros in front),
    as librosa's stft pads its window."""
    n = np.arange(win_length, dtype=np.float64)
    w = np.zeros(n_fft, np.float64)
    off = (n_fft - win_length) // 2
    w[off:off + win_length] = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / win_length)
    return w.astype(np.float32)


def twiddle_table(n_fft: int) -> np.ndarray:
    """exp(-2 pi i k / n_fft), k < n_fft/2, as float32 [n_fft/2, 2] rounded from float64; the
    quarter-turn entry is exactly (0, -1)."""
    k = np.arange(n_fft // 2, dtype=np.float64)
    t = np.stack([np.cos(2.0 * np.pi * k / n_fft), -np.sin(2.0 * np.pi * k / n_fft)], axis=1)
    t[0] = (1.0, 0.0)
    t[n_fft // 4] = (0.0, -1.0)
    return t.astype(np.float32)


class Audio:
    def __init__(self, hparams, device=None):
        self.hparams = hparams
        self._mel_basis = self._build_mel_basis()
        self.average_mel_level_db = np.array(hparams.average_mel_level_db, dtype=np.float32)
        self.stddev_mel_level_db = np.array(hparams.stddev_mel_level_db, dtype=np.float32)
        self._device = device
        self._plans = {}            # (n_fft, win, device) -> device-side tables

    # ------------------------------------------------------------------ reference surface
    def _build_mel_basis(self):
        n_fft = (self.hparams.num_freq - 1) * 2
        return mel_filterbank(self.hparams.sample_rate, n_fft, self.hparams.num_mels)

    def _stft_parameters(self):
        n_fft = (self.hparams.num_freq - 1) * 2
        hop_length = int(self.hparams.frame_shift_ms / 1000 * self.hparams.sample_rate)
        win_length = int(self.hparams.frame_length_ms / 1000 * self.hparams.sample_rate)
        return n_fft, hop_length, win_length

    def _read_wav(self, path, any_rate):
        with wave.open(path, "rb") as f:
            rate, width, channels = f.getframerate(), f.getsampwidth(), f.getnchannels()
            raw = f.readframes(f.getnframes())
        if not any_rate and rate != self.hparams.sample_rate:
            raise ValueError(f"{path}: sample rate {rate} Hz, hparams.sample_rate is "
                             f"{self.hparams.sample_rate} Hz (no resampler: convert the file)")
        if width != 2:
            raise ValueError(f"{path}: {8 * width}-bit samples, only 16-bit PCM is read")
        y = np.frombuffer(raw, "<i2").astype(np.float32) / np.float32(32768.0)
        if channels > 1:
            y = y.reshape(-1, channels).mean(axis=1, dtype=np.float32)
        return y, rate

    def read_wav(self, path):
        """``(y, rate)``: ``load_wav``'s reader at whatever rate the file has."""
        return self._read_wav(path, any_rate=True)

    def load_wav(self, path, resample: bool = False):
        """16-bit PCM through the standard ``wave`` module: float32 in [-1, 1) (``/ 32768``),
        channels averaged.  Another rate than hparams.sample_rate is an error, unless
        ``resample`` asks for the conversion (one utterance through ``resample_batch``: on the
        GPU; a file already at the rate is returned as read)."""
        y, rate = self._read_wav(path, any_rate=resample)
        if rate != self.hparams.sample_rate:
            out, _ = self.resample_batch([y], rate)
            return out[0].cpu().numpy()
        return y

    def save_wav(self, wav, path):
        """16-bit PCM mono at hparams.sample_rate; floats are scaled by 32768 and clipped."""
        wav = np.asarray(wav)
        if wav.dtype != np.int16:
            wav = np.clip(np.rint(wav.astype(np.float64) * 32768.0), -32768, 32767).astype("<i2")
        with wave.open(path, "wb") as f:
            f.setnchannels(1)
            f.setsampwidth(2)
            f.setframerate(int(self.hparams.sample_rate))
            f.writeframes(wav.astype("<i2").tobytes())

    def melspectrogram(self, y):
        """[num_mels, frames] like the reference; numpy in, numpy out -- device tensor in, device
        tensor out."""
        import torch
        mel, frames = self.melspectrogram_batch([y])
        if isinstance(y, torch.Tensor):
            from . import kernels as K
            return K.transpose(mel[0])
        return np.ascontiguousarray(mel[0].cpu().numpy().T)

    def trim(self, wav):
        """``wav[start:stop]`` of ``trim_batch``'s bounds: numpy in, numpy out -- device tensor
        in, a view of it out."""
        _, bounds = self.trim_batch([wav])
        start, stop = (int(v) for v in bounds.cpu().numpy()[0])
        return wav[start:stop]

    def normalize_mel(self, S):
        return (S - self.average_mel_level_db) / self.stddev_mel_level_db

    def _linear_to_mel(self, spectrogram):
        return np.dot(self._mel_basis, spectrogram)

    def _amp_to_db(self, x):
        return 20 * np.log10(np.maximum(AMP_FLOOR, x))

    def denormalize_mel(self, S):
        return S * self.stddev_mel_level_db + self.average_mel_level_db

    def _db_to_amp(self, x):
        return np.power(10.0, x * 0.05)

    def _build_inv_mel_basis(self):
        """Pseudo-inverse of the float32 mel basis, computed in float64: float32
        [num_freq, num_mels]."""
        return np.linalg.pinv(self._mel_basis.astype(np.float64)).astype(np.float32)

    def inv_melspectrogram(self, mel):
        """Normalised mel [num_mels, frames] (the reference's orientation) -> waveform of
        ``hop * (frames - 1)`` samples by Griffin-Lim at the defaults of
        ``inv_melspectrogram_batch``; numpy in, numpy out -- device tensor in, device tensor
        out."""
        import torch
        from . import kernels as K
        if isinstance(mel, torch.Tensor):
            rows = K.transpose(mel.contiguous())
            wav, lengths = self.inv_melspectrogram_batch([rows])
            return wav[0]
        rows = np.ascontiguousarray(np.asarray(mel, np.float32).T)
        wav, lengths = self.inv_melspectrogram_batch([rows])
        return wav[0].cpu().numpy()

    # ------------------------------------------------------------------ the GPU path
    def _dev(self):
        import torch
        if self._device is None:
            if not torch.cuda.is_available():
                raise RuntimeError("Audio.melspectrogram runs on the GPU (libsat_hip); none found")
            self._device = torch.device("cuda", torch.cuda.current_device())
        return self._device

    def _plan(self, device):
        """Device-side tables of this (n_fft, win) configuration, built once per device."""
        import torch
        n_fft, hop, win = self._stft_parameters()
        key = (n_fft, win, str(device))
        plan = self._plans.get(key)
        if plan is None:
            lo, hi = band_limits(self._mel_basis)
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
            if win > n_fft:
                raise ValueError(f"frame_length_ms gives a window of {win} samples, longer than "
                                 f"n_fft = {n_fft}")
            plan = {"window": up(hann_window(win, n_fft)),
                    "twiddle": up(twiddle_table(n_fft)), "basis": up(self._mel_basis),
                    "band_lo": up(lo), "band_hi": up(hi)}
            self._plans[key] = plan
        return plan

    def _upload(self, rows, what, noun="waveform", ndim=1):
        """``(padded [B, stride(, C)] on the device, lengths)`` of a list of ``noun`` rows of shape
        [n] (``ndim`` 1) or [n, C] (2), numpy arrays or tensors: one padded upload."""
        import torch
        from . import kernels as K
        if len(rows) == 0:
            raise ValueError(f"{what}: no {noun}")
        on_dev = [isinstance(r, torch.Tensor) for r in rows]
        device = rows[0].device if on_dev[0] and rows[0].is_cuda else self._dev()
        lengths = [int(r.shape[0]) for r in rows]
        if any(r.ndim != ndim for r in rows):
            raise ValueError(f"{what}: {noun}s must be {ndim}-D")
        shape = (len(rows), max(lengths)) + tuple(rows[0].shape[1:])
        if all(on_dev):
            out = K.zeros(*shape, device=device)
            for b, r in enumerate(rows):
                out[b, :lengths[b]].copy_(r)
        else:
            host = np.zeros(shape, np.float32)
            for b, r in enumerate(rows):
                host[b, :lengths[b]] = r.cpu().numpy() if on_dev[b] else r
            out = torch.from_numpy(host).to(device)
        return out, lengths

    def _resample_plan(self, orig, target, device):
        """``resample_filter``'s table on the device, uploaded once per (orig, target, device)."""
        import torch
        key = ("resample", int(orig), int(target), str(device))
        plan = self._plans.get(key)
        if plan is None:
            f = resample_filter(orig, target)
            plan = self._plans[key] = (f, torch.from_numpy(np.array(f.table)).to(device))
        return plan

    def resample_batch(self, wavs, rates, target_rate=None):
        """A list of 1-D waveforms (numpy arrays or tensors) at ``rates`` (one int, or one per
        utterance) brought to ``target_rate`` (default ``hparams.sample_rate``):
        ``(list of 1-D device tensors in input order, their lengths)``.  Utterances are grouped by
        source rate: one padded upload and one launch (csrc/resample.hip) per distinct rate; each
        result is a view of its group's output rows, ``ceil(len * L / M)`` samples for the ratio
        reduced to L / M.  An utterance already at the target passes through (uploaded if it is
        not on the device yet).  Nothing is read back."""
        import torch
        from . import kernels as K
        target = int(self.hparams.sample_rate if target_rate is None else target_rate)
        if len(wavs) == 0:
            raise ValueError("resample_batch: no waveform")
        if isinstance(rates, (int, np.integer)):
            rates = [int(rates)] * len(wavs)
        rates = [int(r) for r in rates]
        if len(rates) != len(wavs):
            raise ValueError(f"resample_batch: {len(rates)} rates for {len(wavs)} waveforms")
        out = [None] * len(wavs)
        for rate in sorted(set(rates)):
            idx = [i for i, r in enumerate(rates) if r == rate]
            if rate == target:
                for i in idx:
                    w = wavs[i]
                    if w.ndim != 1:
                        raise ValueError("resample_batch: waveforms must be 1-D")
                    if not isinstance(w, torch.Tensor):
                        w = torch.from_numpy(np.ascontiguousarray(w, np.float32))
                    out[i] = w if w.is_cuda else w.to(self._dev())
                continue
            wav, lengths = self._upload([wavs[i] for i in idx], "resample_batch")
            f, table = self._resample_plan(rate, target, wav.device)
            new = [resampled_length(n, f.L, f.M) for n in lengths]
            dlen = torch.from_numpy(np.array(lengths, np.int32)).to(wav.device)
            res = torch.empty(len(idx), max(max(new), 1), device=wav.device)
            K.resample(wav, dlen, lengths, table=table, L=f.L, M=f.M, offset=f.offset,
                       scale=min(1.0, f.L / f.M), out=res)
            for b, i in enumerate(idx):
                out[i] = res[b, :new[b]]
        return out, [int(w.shape[0]) for w in out]

    def trim_batch(self, wavs):
        """A list of 1-D waveforms through one padded upload and the trim launch:
        ``(wav [B, stride], bounds [B, 2] int32)`` on the device, ``bounds[b] = (start, stop)`` of
        utterance b under ``hparams.trim_top_db`` / ``trim_frame_length`` / ``trim_hop_length``
        and ``num_silent_frames`` (``utils/audio.py:40-49``).  Nothing is read back."""
        import torch
        from . import kernels as K
        hp = self.hparams
        frame_length, hop = int(hp.trim_frame_length), int(hp.trim_hop_length)
        if frame_length < 2 or hop < 1:
            raise ValueError(f"trim_frame_length {frame_length} / trim_hop_length {hop}: need a "
                             "frame of at least 2 samples and a hop of at least 1")
        pad_samples = int(hp.num_silent_frames * hp.frame_shift_ms * hp.sample_rate / 1000)
        wav, lengths = self._upload(wavs, "trim_batch")
        B = len(lengths)
        F_max = 1 + (max(lengths) + 2 * (frame_length // 2) - frame_length) // hop
        dlen = torch.from_numpy(np.array(lengths, np.int32)).to(wav.device)
        bounds = torch.empty(B, 2, dtype=torch.int32, device=wav.device)
        frame_ms = torch.empty(B, max(F_max, 1), device=wav.device)
        K.trim_bounds(wav, dlen, lengths, frame_length=frame_length, hop=hop,
                      top_db=hp.trim_top_db, pad_samples=pad_samples, bounds=bounds,
                      frame_ms=frame_ms)
        return wav, bounds

    def melspectrogram_batch(self, wavs, bounds=None, return_magnitudes: bool = False):
        """A list of 1-D waveforms (numpy arrays or tensors) through one padded upload and one
        launch: ``(mel [B, F_max, num_mels], frames [B] int32)`` on the device, rows past an
        utterance's frame count zero; with ``return_magnitudes`` also ``[B, F_max, num_freq]``.

        With ``bounds`` ([B, 2] int32, ``trim_batch``'s device tensor or a host array) utterance b
        is ``wavs[b][start:stop]``, read in place; ``wavs`` may then also be ``trim_batch``'s
        ``[B, stride]`` device tensor, which is used as it is."""
        import torch
        from . import kernels as K
        n_fft, hop, win = self._stft_parameters()
        if hop < 1:
            raise ValueError(f"frame_shift_ms gives a hop of {hop} samples")
        if bounds is not None and isinstance(wavs, torch.Tensor) and wavs.ndim == 2:
            wav, row_lengths = wavs, [int(wavs.shape[1])] * int(wavs.shape[0])
        else:
            wav, row_lengths = self._upload(wavs, "melspectrogram_batch")
        device, B = wav.device, len(row_lengths)
        offsets = None
        if bounds is None:
            lengths = row_lengths
        else:
            bh = bounds.cpu().numpy() if isinstance(bounds, torch.Tensor) else np.asarray(bounds)
            if bh.shape != (B, 2):
                raise ValueError(f"melspectrogram_batch: bounds {bh.shape}, expected ({B}, 2)")
            offsets = [int(v) for v in bh[:, 0]]
            lengths = [int(e) - int(s) for s, e in bh]
        frames = [1 + L // hop for L in lengths]
        F_max = max(frames)
        rows = [lengths, frames] if offsets is None else [lengths, frames, offsets]
        meta = torch.from_numpy(np.array(rows, np.int32)).to(device)
        plan = self._plan(device)
        out = torch.empty(B, F_max, self.hparams.num_mels, device=device)
        mag = torch.empty(B, F_max, self.hparams.num_freq, device=device) \
            if return_magnitudes else None
        K.melspec(wav, meta[0], lengths, n_fft=n_fft, hop=hop, win=win, window=plan["window"],
                  twiddle=plan["twiddle"], basis=plan["basis"], band_lo=plan["band_lo"],
                  band_hi=plan["band_hi"], ref_level_db=self.hparams.ref_level_db,
                  amp_floor=AMP_FLOOR, out=out, mag_out=mag,
                  **({} if offsets is None else dict(offsets=meta[2], offsets_host=offsets)))
        return (out, meta[1], mag) if return_magnitudes else (out, meta[1])

    def mel_statistics(self, mel, frames):
        """Per-utterance min, max, sum and sum of squares per mel bin over the valid frames:
        float64 [B, 4, num_mels] on the device (preprocess/ljspeech.py:125-131)."""
        import torch
        from . import kernels as K
        out = torch.empty(mel.shape[0], 4, mel.shape[2], dtype=torch.float64, device=mel.device)
        K.mel_stats(mel, frames, out)
        return out

    # ------------------------------------------------------------------ the vocoder (GPU)
    def _vocoder_plan(self, device):
        """``_plan`` plus the tables of the way back: the inverse mel basis and the mel
        statistics, one value per mel bin."""
        import torch
        plan = self._plan(device)
        if "inv_basis" not in plan:
            M = self.hparams.num_mels
            up = lambda a: torch.from_numpy(np.array(a, np.float32)).to(device)
            plan["inv_basis"] = up(self._build_inv_mel_basis())
            plan["average"] = up(np.broadcast_to(self.average_mel_level_db, (M,)))
            plan["stddev"] = up(np.broadcast_to(self.stddev_mel_level_db, (M,)))
        return plan

    @staticmethod
    def _frames(frames, B, device):
        """``(device int32 [B], host list)`` of frame counts given as a list, array or tensor."""
        import torch
        host = [int(v) for v in (frames.cpu().numpy() if isinstance(frames, torch.Tensor)
                                 else np.asarray(frames))]
        if len(host) != B:
            raise ValueError(f"frames: {len(host)} entries for {B} utterances")
        if isinstance(frames, torch.Tensor) and frames.is_cuda and frames.dtype == torch.int32 \
                and frames.is_contiguous():
            return frames, host
        return torch.from_numpy(np.array(host, np.int32)).to(device), host

    def mel_to_linear_batch(self, mel, frames, power: float = 1.5):
        """Normalised mel [B, F_max, num_mels] on the device -> linear magnitudes
        [B, F_max, num_freq]: denormalise, dB to amplitude, the inverse mel basis, a floor of
        1e-10 and ``** power`` (csrc/vocoder.hip).  Rows past ``frames`` are zero."""
        import torch
        from . import kernels as K
        plan = self._vocoder_plan(mel.device)
        B, F_max, _ = mel.shape
        dframes, host = self._frames(frames, B, mel.device)
        out = torch.empty(B, F_max, self.hparams.num_freq, device=mel.device)
        K.mel_to_linear(mel, dframes, host, inv_basis=plan["inv_basis"], average=plan["average"],
                        stddev=plan["stddev"], ref_level_db=self.hparams.ref_level_db,
                        power=power, out=out)
        return out

    def istft_batch(self, spec, frames):
        """Complex spectra [B, F_max, num_freq] (complex64, or float32 [.., 2]) on the device ->
        ``wav [B, hop * (max frames - 1)]``: librosa 0.6 istft, the inverse of the analysis in
        ``melspectrogram_batch``; samples past ``hop * (frames[b] - 1)`` are zero."""
        import torch
        from . import kernels as K
        n_fft, hop, win = self._stft_parameters()
        if spec.is_complex():
            spec = torch.view_as_real(spec.contiguous())
        plan = self._plan(spec.device)
        B = spec.shape[0]
        dframes, host = self._frames(frames, B, spec.device)
        wav = torch.empty(B, max(hop * (max(host) - 1), 1), device=spec.device)
        K.istft(spec, dframes, host, n_fft=n_fft, hop=hop, win=win, window=plan["window"],
                twiddle=plan["twiddle"], wav=wav)
        return wav

    def griffin_lim_batch(self, mag, frames, n_iter: int = 60, momentum: float = 0.99,
                          init_phase=None, seed: int = 0):
        """Linear magnitudes [B, F_max, num_freq] on the device -> ``wav [B, stride]`` by
        ``n_iter`` Griffin-Lim iterations (``momentum`` 0: the classic algorithm; 0.99: librosa's
        fast variant), one entry call, nothing read back.  Without ``init_phase`` (radians, the
        shape of ``mag``) the start phases are uniform in [-pi, pi) from a device generator
        seeded with ``seed``."""
        import torch
        from . import kernels as K
        n_fft, hop, win = self._stft_parameters()
        plan = self._plan(mag.device)
        B = mag.shape[0]
        dframes, host = self._frames(frames, B, mag.device)
        if init_phase is None:
            gen = torch.Generator(device=mag.device)
            gen.manual_seed(int(seed))
            init_phase = torch.empty_like(mag).uniform_(-np.pi, np.pi, generator=gen)
        wav = torch.empty(B, max(hop * (max(host) - 1), 1), device=mag.device)
        K.griffin_lim(mag, init_phase, dframes, host, n_fft=n_fft, hop=hop, win=win,
                      window=plan["window"], twiddle=plan["twiddle"], n_iter=n_iter,
                      momentum=momentum, wav=wav)
        return wav

    def inv_melspectrogram_batch(self, mels, frames=None, power: float = 1.5, **gl):
        """Normalised mels as ``predict`` returns them -- a list of [F_b, num_mels] arrays or
        tensors, or one padded [B, F_max, num_mels] device tensor with ``frames`` -- to
        ``(wav [B, stride], lengths [B] int32)`` on the device: ``mel_to_linear_batch`` then
        ``griffin_lim_batch`` (whose options ``gl`` are)."""
        import torch
        if isinstance(mels, torch.Tensor) and mels.ndim == 3:
            if frames is None:
                raise ValueError("inv_melspectrogram_batch: a padded tensor needs frames")
            mel = mels.contiguous()
        else:
            mel, frames = self._upload(mels, "inv_melspectrogram_batch", "mel", 2)
        # the host list goes on: a device tensor would be read back once per stage
        dframes, host_frames = self._frames(frames, mel.shape[0], mel.device)
        hop = self._stft_parameters()[1]
        mag = self.mel_to_linear_batch(mel, host_frames, power=power)
        wav = self.griffin_lim_batch(mag, host_frames, **gl)
        lengths = torch.from_numpy(np.array([hop * (f - 1) for f in host_frames],
                                            np.int32)).to(mel.device)
        return wav, lengths
