"""NumPy restatement of ``sat_figure_render`` (include/sat_abi.h): the canvas the kernel must
write, byte for byte.  Integer resampling, ``q`` in ``np.float32`` with every operation on its own,
the table lookup, the colour bar strip and the margins.

A panel is any 6-tuple ``(src, base, rows, cols, col_stride, table)`` with ``src`` an array whose
flattened float32 elements are the source (``sat_amd.plots.Panel`` is one)."""

import numpy as np

F = np.float32


def figure_shape(n_panel, Hp, Wp, m, cb):
    return n_panel * Hp + (n_panel + 1) * m, Wp + cb + 3 * m


def read(flat, off):
    """src[off] with reads outside src[0, src_n) giving 0."""
    off = np.asarray(off, np.int64)
    inside = (off >= 0) & (off < flat.size)
    out = np.zeros(off.shape, F)
    out[inside] = flat[off[inside]]
    return out


def minmax(crop):
    """``sat_image_minmax``: over the finite pixels; (0, 0) when there is none."""
    finite = np.isfinite(crop)
    if not finite.any():
        return F(0), F(0)
    return F(crop[finite].min()), F(crop[finite].max())


def q(x, lo, hi):
    """clamp(floor(255 * (x - lo) / (hi - lo) + 0.5), 0, 255); 0 where hi == lo or x not finite."""
    x = np.asarray(x, F)
    out = np.zeros(x.shape, np.uint8)
    if not F(hi) > F(lo):
        return out
    with np.errstate(all="ignore"):
        d = x - F(lo)                 # each line one fp32 operation
        n = F(255) * d
        w = F(hi) - F(lo)
        t = n / w
        t = t + F(0.5)
        assert t.dtype == F
        use = np.isfinite(x) & (t > 0)
        out[use] = np.minimum(np.floor(t[use]), F(255)).astype(np.uint8)
    return out


def box(panel, tables, Hp, Wp):
    src, base, rows, cols, col_stride, table = panel
    lut = tables[int(table)]
    rows, cols = int(rows), int(cols)
    if rows <= 0 or cols <= 0:
        return np.tile(lut[0], (Hp, Wp, 1))
    flat = np.ascontiguousarray(np.asarray(src, F)).reshape(-1)
    r_all = np.arange(rows, dtype=np.int64)[:, None]
    c_all = np.arange(cols, dtype=np.int64)[None, :]
    crop = read(flat, int(base) + c_all * int(col_stride) + r_all)
    lo, hi = minmax(crop)
    y = np.arange(Hp, dtype=np.int64)
    x = np.arange(Wp, dtype=np.int64)
    r = ((2 * (Hp - 1 - y) + 1) * rows) // (2 * Hp)
    c = ((2 * x + 1) * cols) // (2 * Wp)
    off = int(base) + c[None, :] * int(col_stride) + r[:, None]
    return lut[q(read(flat, off), lo, hi)]


def render(figures, tables, Hp, Wp, m, cb, background=0xFFFFFF):
    """uint8 [n_fig, Hfig, Wfig, 3]."""
    tables = np.asarray(tables, np.uint8)
    n_panel = len(figures[0]) if len(figures) else 0
    Hfig, Wfig = figure_shape(n_panel, Hp, Wp, m, cb)
    canvas = np.empty((len(figures), Hfig, Wfig, 3), np.uint8)
    canvas[..., 0] = background & 255
    canvas[..., 1] = (background >> 8) & 255
    canvas[..., 2] = (background >> 16) & 255
    for f, fig in enumerate(figures):
        assert len(fig) == n_panel
        for k, panel in enumerate(fig):
            top = m + k * (Hp + m)
            canvas[f, top:top + Hp, m:m + Wp] = box(panel, tables, Hp, Wp)
            lut = tables[int(panel[5])]
            for y in range(Hp):
                entry = 0 if Hp == 1 else 255 - (255 * y) // (Hp - 1)
                canvas[f, top + y, 2 * m + Wp:2 * m + Wp + cb] = lut[entry]
    return canvas


def decode_png(data):
    """A PNG of colour type 2 / bit depth 8 / filter 0 -> (uint8 [h, w, 3], {keyword: text});
    checks the signature and every chunk's CRC."""
    import struct
    import zlib
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    i, chunks = 8, []
    while i < len(data):
        n, = struct.unpack(">I", data[i:i + 4])
        kind, body = data[i + 4:i + 8], data[i + 8:i + 8 + n]
        crc, = struct.unpack(">I", data[i + 8 + n:i + 12 + n])
        assert crc == zlib.crc32(kind + body) & 0xFFFFFFFF, kind
        chunks.append((kind, body))
        i += 12 + n
    assert chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    w, h, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, filt, lace) == (8, 2, 0, 0, 0)
    raw = zlib.decompress(b"".join(b for k, b in chunks if k == b"IDAT"))
    lines = np.frombuffer(raw, np.uint8).reshape(h, 3 * w + 1)
    assert not lines[:, 0].any()                      # filter type 0 on every line
    text = dict(b.split(b"\0", 1) for k, b in chunks if k == b"tEXt")
    return lines[:, 1:].reshape(h, w, 3), {k.decode("latin-1"): v.decode("latin-1")
                                           for k, v in text.items()}
