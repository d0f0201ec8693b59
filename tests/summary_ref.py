"""Numpy statement of the summary image kernels (csrc/summary.hip) and a stdlib PNG decoder.

``minmax`` / ``render`` restate sat_image_minmax / sat_image_render in float32, one operation at
a time: element (r, c) of image i is ``src[base[i] + c * col_stride + r]``, the crop is
``rows[i] x cols[i]``, q = floor(255 * (x - lo) / (hi - lo) + 0.5) clamped to 0..255 (0 where
hi == lo or x is not finite), source row 0 is the crop's bottom line, everything outside the
crop is 0.  ``decode_png`` inflates an 8-bit grayscale PNG (filters 0..4) without any imaging
library.  ``read_events`` reads a TensorBoard event file back through the package's TFRecord
and protobuf field readers."""
import struct
import zlib

import numpy as np


def crop(src, base, rows, cols, col_stride):
    """The [rows, cols] float32 pixels of one image."""
    flat = np.ascontiguousarray(src, dtype=np.float32).reshape(-1)
    idx = (int(base) + np.arange(cols, dtype=np.int64)[None, :] * int(col_stride)
           + np.arange(rows, dtype=np.int64)[:, None])
    return flat[idx]


def minmax(src, base, rows, cols, col_stride):
    """([I, 2] float32 {lo, hi} over the finite pixels, [I] int32 non-finite counts)."""
    n = len(base)
    mm = np.zeros((n, 2), np.float32)
    bad = np.zeros(n, np.int32)
    for i in range(n):
        x = crop(src, base[i], rows[i], cols[i], col_stride)
        fin = np.isfinite(x)
        bad[i] = x.size - int(fin.sum())
        if fin.any():
            mm[i] = x[fin].min(), x[fin].max()
    return mm, bad


def quantise(x, lo, hi):
    x = np.asarray(x, np.float32)
    lo, hi = np.float32(lo), np.float32(hi)
    out = np.zeros(x.shape, np.uint8)
    if not hi > lo:
        return out
    fin = np.isfinite(x)
    with np.errstate(all="ignore"):
        t = (np.float32(255.0) * (x - lo)) / (hi - lo) + np.float32(0.5)
    assert t.dtype == np.float32
    q = np.clip(np.floor(np.nan_to_num(t, nan=0.0, posinf=255.0, neginf=0.0)), 0, 255)
    out[fin] = q[fin].astype(np.uint8)
    return out


def render(src, base, rows, cols, col_stride, Rmax, Cmax, mm=None):
    """uint8 canvas [I, Rmax, Cmax]."""
    if mm is None:
        mm, _ = minmax(src, base, rows, cols, col_stride)
    n = len(base)
    canvas = np.zeros((n, Rmax, Cmax), np.uint8)
    for i in range(n):
        x = crop(src, base[i], rows[i], cols[i], col_stride)
        canvas[i, :rows[i], :cols[i]] = quantise(x, mm[i, 0], mm[i, 1])[::-1]
    return canvas


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


def decode_png(data: bytes) -> np.ndarray:
    """An 8-bit grayscale, non-interlaced PNG -> uint8 [height, width]; chunk CRCs verified."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n", "not a PNG"
    i, idat, head = 8, b"", None
    while i < len(data):
        n, kind = struct.unpack(">I4s", data[i:i + 8])
        body = data[i + 8:i + 8 + n]
        (crc,) = struct.unpack(">I", data[i + 8 + n:i + 12 + n])
        assert zlib.crc32(kind + body) & 0xFFFFFFFF == crc, f"bad CRC in {kind!r}"
        if kind == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat += body
        elif kind == b"IEND":
            break
        i += 12 + n
    w, h, depth, colour, comp, filt, lace = head
    assert (depth, colour, comp, filt, lace) == (8, 0, 0, 0, 0), head
    raw = zlib.decompress(idat)
    assert len(raw) == h * (w + 1)
    out = np.zeros((h, w), np.uint8)
    prev = [0] * w
    for y in range(h):
        ft = raw[y * (w + 1)]
        line = list(raw[y * (w + 1) + 1:(y + 1) * (w + 1)])
        for x in range(w):
            a = line[x - 1] if x else 0
            b = prev[x]
            c = prev[x - 1] if x else 0
            pred = (0, a, b, (a + b) // 2, _paeth(a, b, c))[ft]
            line[x] = (line[x] + pred) & 0xFF
        out[y] = line
        prev = line
    return out


def read_events(path):
    """An event file back as [{wall_time, step, file_version, scalars: {tag: float32},
    images: {tag: (height, width, png bytes)}}] (checksums verified; tests and tools)."""
    from sat_amd import tfrecord
    out = []
    for rec in tfrecord.read_tfrecords(path, verify=True):
        ev = {"wall_time": None, "step": 0, "file_version": None, "scalars": {}, "images": {}}
        for f, _, v in tfrecord._fields(rec):
            if f == 1:
                ev["wall_time"] = struct.unpack("<d", v)[0]
            elif f == 2:
                ev["step"] = v
            elif f == 3:
                ev["file_version"] = v.decode("utf-8")
            elif f == 5:
                for f2, _, val in tfrecord._fields(v):
                    if f2 != 1:
                        continue
                    d = {f3: x for f3, _, x in tfrecord._fields(val)}
                    tag = d[1].decode("utf-8")
                    if 2 in d:
                        ev["scalars"][tag] = np.frombuffer(d[2], "<f4")[0]
                    if 4 in d:
                        im = {f4: x for f4, _, x in tfrecord._fields(d[4])}
                        ev["images"][tag] = (im[1], im[2], im[4])
        out.append(ev)
    return out
