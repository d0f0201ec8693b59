"""Synthesis plots and prediction records, host side: the RGB PNG encoder, the colour tables, the
NumPy path of ``render_figures`` against tests/figure_ref.py, the prediction record's round trip,
and ``write_predictions`` writing exactly today's files with the new switches off."""
import os
import struct
import zlib

import numpy as np
import pytest

import figure_ref as R


# ---------------------------------------------------------------- PNG
def _decode(data):
    """~20 lines of PNG: signature, chunks with their CRCs, IHDR, inflate, strip filter bytes."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    i, chunks = 8, []
    while i < len(data):
        n, = struct.unpack(">I", data[i:i + 4])
        kind, body = data[i + 4:i + 8], data[i + 8:i + 8 + n]
        assert struct.unpack(">I", data[i + 8 + n:i + 12 + n])[0] == zlib.crc32(kind + body)
        chunks.append((kind, body))
        i += 12 + n
    assert i == len(data) and chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    ihdr = struct.unpack(">IIBBBBB", chunks[0][1])
    w, h = ihdr[:2]
    raw = zlib.decompress(b"".join(b for k, b in chunks if k == b"IDAT"))
    lines = np.frombuffer(raw, np.uint8).reshape(h, 3 * w + 1)
    assert not lines[:, 0].any()
    text = dict(b.split(b"\0", 1) for k, b in chunks if k == b"tEXt")
    return ihdr, lines[:, 1:].reshape(h, w, 3), text


@pytest.mark.parametrize("h,w", [(1, 1), (5, 7), (33, 18)])
def test_encode_png_rgb_round_trip(h, w):
    from sat_amd import plots
    img = np.random.default_rng(h * 100 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    data = plots.encode_png_rgb(img, {"key": "LJ001-0001", "text": "printing, in the only sense"})
    ihdr, pixels, text = _decode(data)
    assert ihdr == (w, h, 8, 2, 0, 0, 0)
    assert (pixels == img).all()
    assert text == {b"key": b"LJ001-0001", b"text": b"printing, in the only sense"}
    assert list(text) == [b"key", b"text"]
    # a non-contiguous view encodes as its values; no text, no tEXt chunk
    ihdr2, pixels2, text2 = _decode(plots.encode_png_rgb(img[::-1, ::-1]))
    assert (pixels2 == img[::-1, ::-1]).all() and text2 == {}
    # figure_ref's decoder (used by the GPU tests) reads the same file the same way
    p3, t3 = R.decode_png(data)
    assert (p3 == img).all() and t3["key"] == "LJ001-0001"


def test_encode_png_rgb_refuses_other_arrays_and_escapes_text():
    from sat_amd import plots
    for bad in (np.zeros((4, 4), np.uint8), np.zeros((4, 4, 4), np.uint8),
                np.zeros((4, 4, 3), np.float32), np.zeros((0, 4, 3), np.uint8)):
        with pytest.raises(ValueError):
            plots.encode_png_rgb(bad)
    with pytest.raises(ValueError):
        plots.encode_png_rgb(np.zeros((1, 1, 3), np.uint8), {"": "x"})
    _, _, text = _decode(plots.encode_png_rgb(np.zeros((1, 1, 3), np.uint8),
                                              {"text": "café あ"}))
    assert text[b"text"] == b"caf\xe9 \\u3042"


# ---------------------------------------------------------------- tables
def test_colour_tables():
    from sat_amd import plots
    jet, magma = plots.jet_table(), plots.magma_table()
    for t in (jet, magma):
        assert t.shape == (256, 3) and t.dtype == np.uint8
    # the piecewise-linear definition at x = 0, 1 and 127 / 255 (r rises 0.35 -> 0.66, g = 1 on
    # 0.375 .. 0.64, b falls 0.34 -> 0.65), channels floor(255 v + 0.5)
    assert jet[0].tolist() == [0, 0, 128] and jet[255].tolist() == [128, 0, 0]
    x = 127 / 255
    mid = [int(np.floor(255 * v + 0.5)) for v in ((x - 0.35) / 0.31, 1.0, 1 - (x - 0.34) / 0.31)]
    assert jet[127].tolist() == mid == [122, 255, 125]
    # magma: dark to light.  Each channel is rounded to the nearest integer (error <= 0.5) and the
    # luminance weights sum to 1, so a rising ramp may dip by less than 1 between neighbours and
    # by nothing between entries an anchor interval (32) apart
    lum = magma.astype(np.float64) @ np.array([0.299, 0.587, 0.114])
    assert np.diff(lum).min() > -1.0
    assert (np.diff(lum[::32]) > 0).all() and lum[255] > lum[224]
    assert lum[0] < 8 and lum[255] > 230
    assert plots.default_tables().shape == (2, 256, 3)


# ---------------------------------------------------------------- the host path
def _figures(rng, n_fig, n_panel):
    from sat_amd.plots import Panel
    a = rng.standard_normal((n_fig, 13, 7)).astype(np.float32)       # [fig, cols, rows]
    b = rng.standard_normal((9, n_fig, 5)).astype(np.float32)        # [cols, fig, rows]
    a[0, 2, 3], a[0, 4, 1], a[0, 5, 5] = np.nan, np.inf, -np.inf
    figs = []
    for f in range(n_fig):
        fig = []
        for k in range(n_panel):
            if k % 2 == 0:
                fig.append(Panel(a, f * 13 * 7, 7 - f, 13 - 2 * f, 7, k % 2))
            else:
                fig.append(Panel(b, f * 5, 5 - f, 9 - f, n_fig * 5, k % 2))
        figs.append(fig)
    return figs


@pytest.mark.parametrize("n_fig,n_panel,Hp,Wp,m,cb", [(1, 2, 5, 32, 2, 3), (3, 5, 4, 6, 1, 2),
                                                      (2, 2, 1, 1, 0, 0), (2, 3, 16, 9, 3, 0)])
def test_host_render_equals_the_reference(n_fig, n_panel, Hp, Wp, m, cb):
    from sat_amd import plots
    figs = _figures(np.random.default_rng(5), n_fig, n_panel)
    tables = plots.default_tables()
    got = plots.render_figures(figs, tables, Hp=Hp, Wp=Wp, margin=m, cbar=cb, background=0x0A141E)
    want = R.render(figs, tables, Hp, Wp, m, cb, 0x0A141E)
    assert got.dtype == np.uint8 and got.shape == want.shape == (
        n_fig, n_panel * Hp + (n_panel + 1) * m, Wp + cb + 3 * m, 3)
    assert (got == want).all()
    if m:
        assert got[0, 0, 0].tolist() == [0x1E, 0x14, 0x0A]             # R, G, B of the background


def test_host_render_edge_crops():
    """An empty crop (table entry 0), a constant source (hi == lo), reads past the source."""
    from sat_amd import plots
    from sat_amd.plots import Panel
    tables = plots.default_tables()
    src = np.full(12, 3.0, np.float32)
    ramp = np.arange(12, dtype=np.float32)
    figs = [[Panel(src, 0, 0, 4, 3, 0), Panel(src, 0, 3, 4, 3, 1), Panel(ramp, 6, 3, 4, 3, 0)]]
    got = plots.render_figures(figs, tables, Hp=3, Wp=4, margin=1, cbar=1)
    assert (got == R.render(figs, tables, 3, 4, 1, 1)).all()
    assert (got[0, 1:4, 1:5] == tables[0][0]).all()
    assert (got[0, 5:8, 1:5] == tables[1][0]).all()
    # the third crop's last two columns lie past the ramp: zeros, the minimum -> entry 0
    assert (got[0, 9:12, 3:5] == tables[0][0]).all() and (got[0, 9, 2] == tables[0][255]).all()


# ---------------------------------------------------------------- the binding's structs
@pytest.mark.parametrize("name", ["SatFigurePanel", "SatFigure"])
def test_figure_structs_match_c_layout(name, tmp_path):
    """Size and field offsets of the ctypes structs against gcc's layout of include/sat_abi.h."""
    import ctypes
    import subprocess
    from sat_amd import _lib
    st = getattr(_lib, name)
    fields = [f for f, _ in st._fields_]
    body = "".join(f'printf("%zu\\n", offsetof({name}, {f}));' for f in fields)
    src = tmp_path / "s.c"
    src.write_text('#include "sat_abi.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                   f'int main(){{printf("%zu\\n", sizeof({name}));{body}}}\n')
    exe = str(tmp_path / "s")
    subprocess.run(["gcc", "-I", os.path.dirname(_lib.HEADER_PATH), str(src), "-o", exe],
                   check=True)
    out = [int(x) for x in subprocess.run([exe], capture_output=True, text=True,
                                          check=True).stdout.split()]
    assert out == [ctypes.sizeof(st)] + [getattr(st, f).offset for f in fields]


# ---------------------------------------------------------------- the prediction record
def test_prediction_record_round_trip(tmp_path):
    from sat_amd import tfrecord as T
    rng = np.random.default_rng(2)
    frames, M = 11, 80
    mel = rng.standard_normal((frames, M)).astype(np.float32)
    truth = rng.standard_normal((17, M)).astype(np.float32)
    source = rng.integers(0, 60, 9)
    path = str(tmp_path / "utt.tfrecord")
    T.write_prediction_result(7, "utt", mel, truth, "some text", source, path)
    rec, = list(T.read_tfrecords(path))
    ex = T.decode_example(rec)
    assert sorted(ex) == sorted(["id", "key", "codes", "codes_length", "codes_width",
                                 "ground_truth_codes", "ground_truth_codes_length", "text",
                                 "source", "source_length"])
    assert len(ex["codes"][1][0]) == frames * M * 4
    got = T.parse_prediction_result(rec)
    assert (got.id, got.key, got.text) == (7, b"utt", b"some text")
    assert (got.codes_length, got.codes_width, got.ground_truth_codes_length) == (frames, M, 17)
    assert got.codes.tobytes() == mel.tobytes() and got.ground_truth_codes.tobytes() == truth.tobytes()
    assert got.source.tolist() == source.tolist() and got.source_length == 9


def _preds(rng):
    mel = rng.standard_normal((3, 24, 80)).astype(np.float32)
    stop = np.full((3, 12), -3.0, np.float32)
    stop[1, 11] = 2.0
    return dict(id=np.array([4, 5, 6]), key=np.array([b"a", b"b", "c"], dtype=object), mel=mel,
                stop_token=stop, text=np.array([b"ta", b"tb", b"tc"], dtype=object),
                source=rng.integers(0, 50, (3, 9)), source_length=np.array([9, 7, 5]),
                alignment=rng.random((3, 9, 12)).astype(np.float32),
                alignment2=rng.random((3, 9, 12)).astype(np.float32),
                alignment3=rng.random((3, 12, 12)).astype(np.float32),
                ground_truth_mel=rng.standard_normal((3, 30, 80)).astype(np.float32),
                ground_truth_mel_length=np.array([30, 22, 26]))


def test_write_predictions_switches_off_writes_todays_files(tmp_path):
    """Both switches off (the default): the mel files alone, byte for byte; on: one .png and one
    .tfrecord per key beside them, the record's codes being the mel file's bytes."""
    from sat_amd import hparams, plots, synthesize as S, tfrecord as T
    hp = hparams.ljspeech_hparams()
    hp.set_hparam("outputs_per_step", 2)
    p = _preds(np.random.default_rng(9))
    off, on = tmp_path / "off", tmp_path / "on"
    assert S.write_predictions([p], str(off), hp, wav=False) == ["a", "b", "c"]
    names = sorted(os.listdir(off))
    assert names == [f"{k}.{hp.predicted_mel_extension}" for k in "abc"]
    geo = dict(Hp=6, Wp=20, margin=2, cbar=3)
    S.write_predictions([p], str(on), hp, wav=False, plots=True, records=True, plot_options=geo)
    ext = hp.predicted_mel_extension
    assert sorted(os.listdir(on)) == sorted(f"{k}.{e}" for k in "abc"
                                            for e in (ext, "png", "tfrecord"))
    frames = S.stop_frames(p["stop_token"], 2, 24)
    assert frames == [24, 24, 24]
    panels = plots.prediction_panels(p, hp, frames)
    assert [(q.rows, q.cols) for q in panels[1]] == [(7, 12), (7, 12), (12, 12), (80, 22), (80, 24)]
    want = R.render(panels, plots.default_tables(), 6, 20, 2, 3)
    for b, k in enumerate("abc"):
        assert (on / f"{k}.{ext}").read_bytes() == (off / f"{k}.{ext}").read_bytes()
        pixels, text = R.decode_png((on / f"{k}.png").read_bytes())
        assert (pixels == want[b]).all() and text == {"key": k, "text": "t" + k}
        rec = T.parse_prediction_result(next(T.read_tfrecords(str(on / f"{k}.tfrecord"))))
        assert rec.codes.tobytes() == (on / f"{k}.{ext}").read_bytes()
        assert rec.ground_truth_codes.shape == (int(p["ground_truth_mel_length"][b]), 80)
        assert rec.source.tolist() == p["source"][b, :p["source_length"][b]].tolist()
        assert (rec.id, rec.key, rec.text) == (4 + b, k.encode(), b"t" + k.encode())
