"""Per-utterance plot files of a synthesis: ``plot_predictions`` (modules/metrics.py:13-53) without
matplotlib.

One colour PNG per utterance, ``<key>.png``: panels stacked top to bottom -- the two attention
alignments, the decoder self-attention heads, the ground-truth mel where the batch has one, the
predicted mel -- each resampled (nearest neighbour, ``imshow(aspect='auto', interpolation='none',
origin='lower')``) into a box of ``Hp x Wp`` pixels with a colour bar strip at its right.  The
alignments use ``jet_table()``, the mels ``magma_table()``.

* ``render_figures``: device tensors go through ``sat_image_minmax`` (once per source tensor) and
  ONE ``sat_figure_render`` launch for the whole batch (csrc/figure.hip); the canvases stay on the
  device.  Host arrays (a CPU model) take ``render_figures_host``, the NumPy statement of the same
  integer and fp32 arithmetic, which gives the same bytes.
* ``encode_png_rgb``: 8-bit RGB PNG (colour type 2) with ``zlib`` + ``struct`` only.
* ``write_plots``: the files of one predicted batch.  Each alignment is cropped to the utterance's
  own source length and its own stop step (``synthesize.stop_frames``), so the mel file, the wav
  and the plot agree.

Not drawn: text.  The reference's title ("record ID", "input text") goes into the PNG's ``tEXt``
chunks ``key`` and ``text``; panel titles, axis labels, tick labels and the colour bars' scales are
not written anywhere.
"""

from __future__ import annotations

import os
import struct
import zlib
from collections import namedtuple
from typing import Dict, List, Optional, Sequence

import numpy as np

from .summary import _chunk

JET, MAGMA = 0, 1
GEOMETRY = dict(Hp=160, Wp=1000, margin=16, cbar=24, background=0xFFFFFF)


class Panel(namedtuple("Panel", ["src", "base", "rows", "cols", "col_stride", "table"])):
    """One crop: element (r, c) at ``src.flatten()[base + c * col_stride + r]``, ``rows x cols``,
    coloured by ``table`` (an index into the tables given to ``render_figures``)."""


# ---------------------------------------------------------------- colour tables
def _piecewise(x: np.ndarray, knots) -> np.ndarray:
    xs, ys = zip(*knots)
    return np.interp(x, xs, ys)


def _to_u8(v: np.ndarray) -> np.ndarray:
    return np.clip(np.floor(255.0 * v + 0.5), 0, 255).astype(np.uint8)


def jet_table() -> np.ndarray:
    """uint8 [256, 3]: the jet map from its piecewise-linear definition, entry i at x = i / 255,
    each channel ``floor(255 v + 0.5)``."""
    x = np.arange(256) / 255.0
    r = _piecewise(x, [(0, 0), (0.35, 0), (0.66, 1), (0.89, 1), (1, 0.5)])
    g = _piecewise(x, [(0, 0), (0.125, 0), (0.375, 1), (0.64, 1), (0.91, 0), (1, 0)])
    b = _piecewise(x, [(0, 0.5), (0.11, 1), (0.34, 1), (0.65, 0), (1, 0)])
    return _to_u8(np.stack([r, g, b], axis=1))


# anchors of the approximation below, 1/8 apart
_MAGMA_ANCHORS = [(0, 0, 4), (28, 16, 68), (79, 18, 123), (129, 37, 129), (181, 54, 122),
                  (229, 80, 100), (251, 135, 97), (254, 194, 135), (252, 253, 191)]


def magma_table() -> np.ndarray:
    """uint8 [256, 3]: an APPROXIMATION of the magma map -- linear interpolation between nine
    anchor colours 1/8 apart -- not matplotlib's 256-entry table.  Dark to light, luminance rising
    along the table."""
    x = np.arange(256) / 255.0
    a = np.asarray(_MAGMA_ANCHORS, np.float64) / 255.0
    xs = np.linspace(0.0, 1.0, len(a))
    return _to_u8(np.stack([np.interp(x, xs, a[:, ch]) for ch in range(3)], axis=1))


def default_tables() -> np.ndarray:
    """uint8 [2, 256, 3]: ``JET``, ``MAGMA``."""
    return np.stack([jet_table(), magma_table()])


# ---------------------------------------------------------------- PNG
def encode_png_rgb(image: np.ndarray, text: Optional[Dict[str, str]] = None,
                   level: int = 6) -> bytes:
    """uint8 [height, width, 3] -> an 8-bit RGB PNG (colour type 2, filter 0 on every line), with
    one ``tEXt`` chunk per item of ``text`` (keyword 1..79 Latin-1 bytes; a character of the value
    outside Latin-1 is written as a backslash escape, tEXt having no other encoding)."""
    a = np.ascontiguousarray(image)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"encode_png_rgb: a non-empty uint8 [H, W, 3] array, got {a.dtype} "
                         f"{a.shape}")
    h, w = a.shape[:2]
    raw = np.zeros((h, 3 * w + 1), np.uint8)
    raw[:, 1:] = a.reshape(h, 3 * w)
    out = b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))
    for k, v in (text or {}).items():
        kw = str(k).encode("latin-1")
        if not 1 <= len(kw) <= 79 or b"\0" in kw:
            raise ValueError(f"encode_png_rgb: tEXt keyword {k!r} must be 1..79 Latin-1 bytes")
        body = str(v).encode("latin-1", errors="backslashreplace").replace(b"\0", b" ")
        out += _chunk(b"tEXt", kw + b"\0" + body)
    return out + _chunk(b"IDAT", zlib.compress(raw.tobytes(), level)) + _chunk(b"IEND", b"")


# ---------------------------------------------------------------- the host statement
def figure_shape(n_panel: int, Hp: int, Wp: int, margin: int, cbar: int):
    """(Hfig, Wfig) of include/sat_abi.h."""
    return n_panel * Hp + (n_panel + 1) * margin, Wp + cbar + 3 * margin


def _crop_host(flat: np.ndarray, base: int, rows: int, cols: int, col_stride: int) -> np.ndarray:
    off = (np.int64(base) + np.arange(cols, dtype=np.int64)[None, :] * np.int64(col_stride)
           + np.arange(rows, dtype=np.int64)[:, None])
    ok = (off >= 0) & (off < flat.size)
    if flat.size == 0:
        return np.zeros(off.shape, np.float32)
    return np.where(ok, flat[np.clip(off, 0, flat.size - 1)], np.float32(0)).astype(np.float32)


def _minmax_host(crop: np.ndarray):
    """sat_image_minmax: min / max over the finite pixels, (0, 0) when there is none."""
    fin = crop[np.isfinite(crop)]
    if fin.size == 0:
        return np.float32(0), np.float32(0)
    return np.float32(fin.min()), np.float32(fin.max())


def _quantise_host(x: np.ndarray, lo, hi) -> np.ndarray:
    """sat_image_render's q: fp32, every operation rounded on its own."""
    x = x.astype(np.float32)
    lo, hi = np.float32(lo), np.float32(hi)
    if not hi > lo:
        return np.zeros(x.shape, np.uint8)
    with np.errstate(all="ignore"):
        t = (np.float32(255) * (x - lo)) / np.float32(hi - lo) + np.float32(0.5)
        ok = np.isfinite(x) & (t > 0)
        q = np.where(t >= 255, np.float32(255), np.floor(t))
    return np.where(ok, q, 0).astype(np.uint8)


def render_figures_host(figures: Sequence[Sequence[Panel]], tables: np.ndarray, Hp: int, Wp: int,
                        margin: int, cbar: int, background: int = 0xFFFFFF) -> np.ndarray:
    """uint8 [n_fig, Hfig, Wfig, 3] of host panels, byte for byte what ``sat_figure_render``
    writes (include/sat_abi.h)."""
    n_panel = len(figures[0]) if len(figures) else 0
    Hfig, Wfig = figure_shape(n_panel, Hp, Wp, margin, cbar)
    bg = np.array([background & 255, background >> 8 & 255, background >> 16 & 255], np.uint8)
    canvas = np.empty((len(figures), Hfig, Wfig, 3), np.uint8)
    canvas[:] = bg
    y = np.arange(Hp, dtype=np.int64)
    x = np.arange(Wp, dtype=np.int64)
    bar = np.zeros(Hp, np.int64) if Hp == 1 else 255 - (255 * y) // (Hp - 1)
    for f, fig in enumerate(figures):
        if len(fig) != n_panel:
            raise ValueError("render_figures: every figure needs the same number of panels")
        for k, p in enumerate(fig):
            lut = tables[min(max(int(p.table), 0), len(tables) - 1)]
            rows, cols = int(p.rows), int(p.cols)
            if rows <= 0 or cols <= 0:
                box = np.broadcast_to(lut[0], (Hp, Wp, 3))
            else:
                flat = np.asarray(p.src, np.float32).reshape(-1)
                crop = _crop_host(flat, int(p.base), rows, cols, int(p.col_stride))
                q = _quantise_host(crop, *_minmax_host(crop))
                rr = ((2 * (Hp - 1 - y) + 1) * rows) // (2 * Hp)
                cc = ((2 * x + 1) * cols) // (2 * Wp)
                box = lut[q[rr][:, cc]]
            y0 = margin + k * (Hp + margin)
            canvas[f, y0:y0 + Hp, margin:margin + Wp] = box
            x0 = 2 * margin + Wp
            canvas[f, y0:y0 + Hp, x0:x0 + cbar] = lut[bar][:, None, :]
    return canvas


# ---------------------------------------------------------------- the device path
_TABLES_DEV: dict = {}


def _device_tables(tables: np.ndarray, device):
    import torch
    key = (str(device), tables.tobytes())
    t = _TABLES_DEV.get(key)
    if t is None:
        t = torch.from_numpy(np.ascontiguousarray(tables)).to(device)
        _TABLES_DEV.clear()                      # one set of tables is all a run uses
        _TABLES_DEV[key] = t
    return t


def render_figures(figures: Sequence[Sequence[Panel]], tables: Optional[np.ndarray] = None,
                   Hp: int = GEOMETRY["Hp"], Wp: int = GEOMETRY["Wp"],
                   margin: int = GEOMETRY["margin"], cbar: int = GEOMETRY["cbar"],
                   background: int = GEOMETRY["background"]):
    """``figures[f][k]``: panel k of figure f (every figure the same number of panels).  With
    device sources: the canvases as a uint8 device tensor [n_fig, Hfig, Wfig, 3] -- one
    ``sat_image_minmax`` per (source tensor, column stride) and one ``sat_figure_render``.  With
    host sources (NumPy arrays or CPU tensors): ``render_figures_host``'s array."""
    tables = default_tables() if tables is None else np.ascontiguousarray(tables, np.uint8)
    flat = [p for fig in figures for p in fig]
    on_device = [bool(getattr(p.src, "is_cuda", False)) for p in flat]
    if not any(on_device):
        host = [[p._replace(src=p.src.detach().numpy() if hasattr(p.src, "detach") else p.src)
                 for p in fig] for fig in figures]
        return render_figures_host(host, tables, Hp, Wp, margin, cbar, background)
    if not all(on_device):
        raise ValueError("render_figures: device and host sources in one call")
    import torch
    from . import kernels as K
    n_fig, n_panel = len(figures), len(figures[0])
    if any(len(fig) != n_panel for fig in figures):
        raise ValueError("render_figures: every figure needs the same number of panels")
    dev = flat[0].src.device
    # one min / max launch per source tensor (and column stride): its panels, in table order
    groups: Dict[tuple, List[int]] = {}
    for i, p in enumerate(flat):
        groups.setdefault((p.src.data_ptr(), int(p.col_stride)), []).append(i)
    mm = torch.empty(len(flat), 2, dtype=torch.float32, device=dev)
    bad = torch.empty(len(flat), dtype=torch.int32, device=dev)
    slot = [0] * len(flat)
    crops = np.array([[int(p.base), max(int(p.rows), 0), max(int(p.cols), 0)] for p in flat],
                     np.int64).reshape(len(flat), 3)
    order = [i for idx in groups.values() for i in idx]
    crops_dev = torch.from_numpy(crops[order]).to(dev)
    base_dev = crops_dev[:, 0].contiguous()
    rows_dev = crops_dev[:, 1].to(torch.int32)
    cols_dev = crops_dev[:, 2].to(torch.int32)
    o = 0
    for (_, stride), idx in groups.items():
        n = len(idx)
        rows_h, cols_h = crops[idx, 1].tolist(), crops[idx, 2].tolist()
        K.image_minmax(flat[idx[0]].src, base_dev[o:o + n], rows_dev[o:o + n], cols_dev[o:o + n],
                       stride, max(rows_h), max(cols_h), mm[o:o + n], bad[o:o + n], rows_h, cols_h)
        for j, i in enumerate(idx):
            slot[i] = o + j
        o += n
    table = K.figure_panels([(p.src, p.base, max(int(p.rows), 0), max(int(p.cols), 0),
                              p.col_stride, p.table, mm[slot[i]]) for i, p in enumerate(flat)])
    table_dev = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(dev)
    Hfig, Wfig = figure_shape(n_panel, Hp, Wp, margin, cbar)
    canvas = torch.empty(n_fig, Hfig, Wfig, 3, dtype=torch.uint8, device=dev)
    K.figure_render(table, table_dev, _device_tables(tables, dev), canvas, Hp, Wp, margin, cbar,
                    background)
    return canvas


# ---------------------------------------------------------------- predictions -> files
def _np(x) -> np.ndarray:
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def _rows_contiguous(a):
    """[B, R, C] (image rows R) -> a dense [B, C, R] array of the same kind: the layout a panel
    addresses (rows contiguous)."""
    if hasattr(a, "detach"):
        return a.transpose(1, 2).contiguous()
    return np.ascontiguousarray(np.swapaxes(np.asarray(a, np.float32), 1, 2))


def _like(x, ref):
    """A host array as float32 on ``ref``'s side (the device of a device tensor)."""
    if hasattr(x, "detach"):
        return x
    x = np.ascontiguousarray(x, np.float32)
    if getattr(ref, "is_cuda", False):
        import torch
        return torch.from_numpy(x).to(ref.device)
    return x


def prediction_panels(p: dict, hparams, frames: Sequence[int], mel=None) -> List[List[Panel]]:
    """The panels of one predictions dict (``model.predict``), one list per utterance:
    ``alignment`` and ``alignment2`` [B, N, T'] cropped to ``source_length[b] x steps_b``, the
    decoder self-attention heads ``alignment3`` / ``alignment4`` [B, T', T'] to ``steps_b x
    steps_b``, ``ground_truth_mel`` [B, T, M] (if any) to ``M x ground_truth_mel_length[b]`` and
    the predicted mel to ``M x frames[b]``; ``steps_b = frames[b] / outputs_per_step``.  ``mel``
    replaces ``p["mel"]`` (``mel_postnet`` under ``use_postnet_v2``) as the last panel."""
    r = int(hparams.outputs_per_step)
    if mel is None:
        mel = p.get("mel_postnet") if getattr(hparams, "use_postnet_v2", False) else p["mel"]
    B, M = int(mel.shape[0]), int(mel.shape[2])
    steps = [int(f) // r for f in frames]
    stacks = []                                  # (dense [B, C, R] source, rows per b, cols per b)
    for name in ("alignment", "alignment2"):
        a = p[name]
        N = int(a.shape[1])
        n_src = (np.minimum(_np(p["source_length"]).reshape(-1), N).tolist()
                 if p.get("source_length") is not None else [N] * B)
        stacks.append((_rows_contiguous(_like(a, mel)), n_src, steps, JET))
    for name in ("alignment3", "alignment4"):
        if p.get(name) is not None:
            stacks.append((_rows_contiguous(_like(p[name], mel)), steps, steps, JET))
    truth = p.get("ground_truth_mel")
    if truth is not None:
        t_len = (np.minimum(_np(p["ground_truth_mel_length"]).reshape(-1),
                            truth.shape[1]).tolist()
                 if p.get("ground_truth_mel_length") is not None else [int(truth.shape[1])] * B)
        truth = _like(truth, mel)
        truth = truth.contiguous() if hasattr(truth, "detach") else truth
        stacks.append((truth, [int(truth.shape[2])] * B, t_len, MAGMA))
    dense = mel.contiguous() if hasattr(mel, "detach") else np.ascontiguousarray(mel, np.float32)
    stacks.append((dense, [M] * B, [int(f) for f in frames], MAGMA))
    return [[Panel(src, b * int(src.shape[1]) * int(src.shape[2]), int(rows[b]), int(cols[b]),
                   int(src.shape[2]), table) for src, rows, cols, table in stacks]
            for b in range(B)]


def write_plots(p: dict, output_dir: str, hparams, frames: Optional[Sequence[int]] = None,
                min_iters: Optional[int] = None, mel=None, **geometry) -> List[str]:
    """Writes ``<key>.png`` for every utterance of the predictions dict ``p`` and returns the
    paths.  ``frames``: the frames each utterance keeps (default: ``synthesize.stop_frames`` of
    ``p["stop_token"]``); ``geometry``: ``Hp, Wp, margin, cbar, background`` (``GEOMETRY``)."""
    from .synthesize import MIN_ITERS, _key, stop_frames
    os.makedirs(output_dir, exist_ok=True)
    ref = mel if mel is not None else p["mel"]
    if frames is None:
        frames = stop_frames(p["stop_token"], int(hparams.outputs_per_step), int(ref.shape[1]),
                             MIN_ITERS if min_iters is None else min_iters)
    keys = [_key(k) for k in np.asarray(p["key"]).reshape(-1)]
    texts = (np.asarray(p["text"], dtype=object).reshape(-1) if p.get("text") is not None
             else [None] * len(keys))
    g = dict(GEOMETRY, **geometry)
    canvas = _np(render_figures(prediction_panels(p, hparams, frames, mel=mel), None, **g))
    paths = []
    for b, key in enumerate(keys):
        text = {"key": key}
        if texts[b] is not None:
            text["text"] = _key(texts[b])
        path = os.path.join(output_dir, f"{key}.png")
        with open(path, "wb") as f:
            f.write(encode_png_rgb(canvas[b], text))
        paths.append(path)
    return paths
