"""``sat_figure_render`` (csrc/figure.hip) against its NumPy statement (tests/figure_ref.py).

Acceptance is EQUALITY of the uint8 canvases: the resampling is integer arithmetic and ``q`` is
evaluated with every fp32 operation rounded on its own on both sides, so there is nothing to
tolerate.  Every canvas is composed into a window of a larger buffer pre-filled with 0xAA: the
bytes around the window must keep that value (no store outside the canvas), and a run whose
tables and background hold no 0xAA must leave none inside it (every byte written).  Shapes are
the smallest at which the kernel takes another path: a chunk is 12 bytes / 4 pixels, a block 256
chunks, the canvas base 0..3 bytes past a word."""
import ctypes

import numpy as np
import pytest
import torch

import figure_ref as R

pytestmark = pytest.mark.gpu

FILL, GUARD = 0xAA, 64


def _tables():
    """jet and magma, with every 0xAA channel value moved to 0xAB (the 'every byte written' check
    needs canvases that cannot hold the fill value)."""
    from sat_amd import plots
    t = plots.default_tables().copy()
    t[t == FILL] = FILL + 1
    return t


def _compose(cuda, figs, Hp, Wp, m, cb, offset=0, background=0x101418, tables=None, runs=1):
    """Upload the sources, run min / max per panel and ONE figure launch into a window ``offset``
    bytes past a word inside a guarded buffer -> (canvas, guard bytes before, after) as numpy."""
    from sat_amd import kernels as K
    tables = _tables() if tables is None else tables
    dev_src = {}
    rows = []
    keep = []
    for fig in figs:
        for src, base, r, c, stride, table in fig:
            if id(src) not in dev_src:
                flat = np.ascontiguousarray(src, np.float32).reshape(-1)
                dev_src[id(src)] = torch.from_numpy(flat).to(cuda) if flat.size else \
                    torch.zeros(1, device=cuda)[:0]
            d = dev_src[id(src)]
            mm = torch.full((1, 2), 7.0, device=cuda)
            bad = torch.zeros(1, dtype=torch.int32, device=cuda)
            r0, c0 = max(int(r), 0), max(int(c), 0)
            K.image_minmax(d, torch.tensor([base], dtype=torch.int64, device=cuda),
                           torch.tensor([r0], dtype=torch.int32, device=cuda),
                           torch.tensor([c0], dtype=torch.int32, device=cuda), stride, r0, c0, mm,
                           bad, [r0], [c0])
            keep.append(mm)
            rows.append((d, base, r, c, stride, table, mm))
    n_fig, n_panel = len(figs), len(figs[0])
    Hfig, Wfig = R.figure_shape(n_panel, Hp, Wp, m, cb)
    total = n_fig * Hfig * Wfig * 3
    buf = torch.full((total + 2 * GUARD + 8,), FILL, dtype=torch.uint8, device=cuda)
    o = GUARD + (-buf.data_ptr() % 4) + offset
    canvas = buf[o:o + total].view(n_fig, Hfig, Wfig, 3)
    assert canvas.data_ptr() % 4 == offset
    host = K.figure_panels(rows)
    table_dev = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(cuda)
    lut = torch.from_numpy(tables).to(cuda)
    outs = []
    for _ in range(runs):
        canvas.fill_(FILL)
        K.figure_render(host, table_dev, lut, canvas, Hp, Wp, m, cb, background)
        torch.cuda.synchronize()
        outs.append(buf.cpu().numpy().copy())
    for other in outs[1:]:
        assert other.tobytes() == outs[0].tobytes()                     # two runs, the same bytes
    got = outs[0]
    return got[o:o + total].reshape(n_fig, Hfig, Wfig, 3), got[:o], got[o + total:]


def _check(cuda, figs, Hp, Wp, m, cb, offset=0, background=0x101418, runs=1):
    tables = _tables()
    canvas, before, after = _compose(cuda, figs, Hp, Wp, m, cb, offset, background, tables, runs)
    want = R.render(figs, tables, Hp, Wp, m, cb, background)
    differ = int((canvas != want).sum())
    print(f"bytes that differ: {differ} of {want.size}")
    assert differ == 0
    assert (before == FILL).all() and (after == FILL).all()            # guards untouched
    assert not (canvas == FILL).any()                                   # every byte written
    return canvas


def _sources(seed=0):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((3, 40, 23)).astype(np.float32)     # [fig][cols][rows], stride 23
    b = rng.random((37, 3, 11)).astype(np.float32)              # [cols][fig][rows], stride 33
    return a, b


def _ragged(n_fig, n_panel, seed=0):
    """Panels alternating between two source tensors with different column strides; crops shrink
    with the figure index."""
    a, b = _sources(seed)
    figs = []
    for f in range(n_fig):
        fig = []
        for k in range(n_panel):
            if k % 2 == 0:
                fig.append((a, f * 40 * 23, 23 - 5 * f - k, 40 - 9 * f, 23, k % 2))
            else:
                fig.append((b, f * 11, 11 - 3 * f, 37 - 4 * f - k, 33, k % 2))
        figs.append(fig)
    return figs


@pytest.mark.parametrize("n_fig,n_panel", [(1, 2), (3, 2), (1, 5), (3, 5)])
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_ragged_figures_from_two_sources_at_every_base_offset(cuda, n_fig, n_panel, offset):
    """Crops larger and smaller than the box in both directions (23 / 11 rows into Hp 16, 40 / 37
    columns into Wp 29), Wfig * 3 = 3 * (29 + 3 + 6) = 114: not a multiple of 4."""
    _check(cuda, _ragged(n_fig, n_panel), 16, 29, 2, 3, offset=offset)


@pytest.mark.parametrize("rows,cols,Hp,Wp,m,cb", [
    (1, 1, 4, 6, 1, 1),          # one source pixel repeated over the box
    (40, 60, 5, 7, 1, 2),        # rows > Hp, cols > Wp: skipping
    (3, 5, 16, 32, 2, 2),        # rows < Hp, cols < Wp: repeating
    (7, 13, 5, 32, 1, 3),        # non-dividing ratios
    (7, 13, 1, 32, 1, 3),        # Hp == 1: colour bar entry 0
    (7, 13, 5, 1, 0, 0),         # Wp == 1, no margin, no colour bar
    (9, 9, 8, 9, 1, 0),          # Wfig = 12: Wfig * 3 a multiple of 4
    (9, 9, 8, 9, 1, 1),          # Wfig = 13: not one
    (9, 9, 8, 10, 2, 0),         # Wfig = 16
    (50, 70, 64, 500, 3, 5),     # several blocks (Wfig * Hfig * 3 / 12 > 256 chunks)
])
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_resampling_cases(cuda, rows, cols, Hp, Wp, m, cb, offset):
    rng = np.random.default_rng(rows * 1000 + cols)
    src = rng.standard_normal((cols, rows + 2)).astype(np.float32)
    src2 = rng.random((cols, rows)).astype(np.float32)
    figs = [[(src, 1, rows, cols, rows + 2, 0), (src2, 0, rows, cols, rows, 1)]]
    canvas = _check(cuda, figs, Hp, Wp, m, cb, offset=offset)
    if Hp == 1:
        assert (canvas[0, m, 2 * m + Wp:2 * m + Wp + cb] == _tables()[0][0]).all()


def test_empty_crops_nonfinite_constant_and_out_of_range(cuda):
    """rows == 0 / cols == 0 / negative (table entry 0); NaN, +inf, -inf pixels (entry 0, and left
    out of min / max); a constant source (hi == lo: entry 0); a crop whose columns run past src_n
    and one that starts before the source (reads give 0)."""
    tables = _tables()
    a, _ = _sources(3)
    bad = a[0].copy()
    bad[2, 3], bad[5, 1], bad[7, 7], bad[0, 0] = np.nan, np.inf, -np.inf, np.nan
    const = np.full((6, 4), 2.5, np.float32)
    ramp = np.arange(40, dtype=np.float32) + 1
    figs = [[(a, 0, 0, 10, 23, 0), (a, 0, 10, 0, 23, 1), (bad, 0, 23, 40, 23, 0),
             (const, 0, 4, 6, 4, 1), (ramp, 20, 5, 8, 5, 0)],
            [(a, 0, -3, 10, 23, 1), (bad, 23, 9, 9, 23, 1), (const, 0, 4, 6, 4, 0),
             (ramp, -7, 5, 6, 5, 1), (ramp, 35, 5, 8, 5, 0)]]
    canvas = _check(cuda, figs, 8, 19, 1, 2, offset=1)
    box = lambda f, k: canvas[f, 1 + k * 9:1 + k * 9 + 8, 1:20]                      # noqa: E731
    assert (box(0, 0) == tables[0][0]).all() and (box(0, 1) == tables[1][0]).all()
    assert (box(1, 0) == tables[1][0]).all()
    assert (box(0, 3) == tables[1][0]).all() and (box(1, 2) == tables[0][0]).all()


def test_two_runs_give_the_same_bytes(cuda):
    _check(cuda, _ragged(3, 5, seed=4), 16, 29, 2, 3, offset=3, runs=2)


def test_render_figures_device_path(cuda):
    """plots.render_figures on device tensors (one min / max launch per source tensor, one figure
    launch) equals its host path and the reference."""
    from sat_amd import plots
    from sat_amd.plots import Panel
    figs = _ragged(3, 5, seed=2)
    dev = {}
    on_dev = [[Panel(dev.setdefault(id(p[0]), torch.from_numpy(p[0]).to(cuda)), *p[1:])
               for p in fig] for fig in figs]
    got = plots.render_figures(on_dev, None, Hp=12, Wp=21, margin=2, cbar=4)
    assert got.is_cuda and got.dtype == torch.uint8
    want = R.render(figs, plots.default_tables(), 12, 21, 2, 4)
    assert (got.cpu().numpy() == want).all()
    host = plots.render_figures([[Panel(*p) for p in fig] for fig in figs], None, Hp=12, Wp=21,
                                margin=2, cbar=4)
    assert (host == want).all()


# ---------------------------------------------------------------- refusals
def _valid(cuda):
    """A valid one-figure, one-panel call as raw structs -> (SatFigure, host table, tensors)."""
    from sat_amd import _lib
    src = torch.arange(24, dtype=torch.float32, device=cuda)
    mm = torch.tensor([0.0, 23.0], device=cuda)
    lut = torch.from_numpy(_tables()).to(cuda)
    host = (_lib.SatFigurePanel * 1)()
    host[0].src, host[0].src_n, host[0].base, host[0].col_stride = src.data_ptr(), 24, 0, 4
    host[0].minmax, host[0].rows, host[0].cols, host[0].table = mm.data_ptr(), 4, 6, 0
    table_dev = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(cuda)
    Hfig, Wfig = R.figure_shape(1, 4, 6, 1, 1)
    canvas = torch.full((1, Hfig, Wfig, 3), FILL, dtype=torch.uint8, device=cuda)
    d = _lib.SatFigure(n_fig=1, n_panel=1, Hp=4, Wp=6, margin=1, cbar=1, n_tables=2,
                       background=0, panels=table_dev.data_ptr(),
                       panels_host=ctypes.addressof(host), lut=lut.data_ptr(),
                       canvas=canvas.data_ptr())
    return d, host, (src, mm, lut, table_dev, canvas)


def _set(**kw):
    def change(d, host):
        for k, v in kw.items():
            setattr(d, k, v)
    return change


def _panel(**kw):
    def change(d, host):
        for k, v in kw.items():
            setattr(host[0], k, v)
    return change


REFUSALS = {
    "null panels": _set(panels=None), "null lut": _set(lut=None), "null canvas": _set(canvas=None),
    "negative n_fig": _set(n_fig=-1), "negative n_panel": _set(n_panel=-1),
    "negative margin": _set(margin=-1), "negative cbar": _set(cbar=-1),
    "Hp 0": _set(Hp=0), "Wp 0": _set(Wp=0),
    "too many panels": _set(n_fig=256, n_panel=256, panels_host=None),
    "no table": _set(n_tables=0), "too many tables": _set(n_tables=9),
    "table index": _panel(table=2), "negative table index": _panel(table=-1),
    "null src": _panel(src=None), "null minmax": _panel(minmax=None),
    "negative src_n": _panel(src_n=-1), "negative col_stride": _panel(col_stride=-1),
}


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_refusals_launch_nothing(cuda, what):
    from sat_amd import _lib
    lib = _lib.load()
    d, host, keep = _valid(cuda)
    canvas = keep[-1]
    REFUSALS[what](d, host)
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.sat_figure_render(ctypes.byref(d), stream) == _lib.SAT_ERR_ARGUMENT
    assert b"sat_figure_render" in lib.sat_last_error_string()
    torch.cuda.synchronize()
    assert (canvas == FILL).all()


def test_misaligned_pointers_and_null_descriptor_are_refused(cuda):
    from sat_amd import _lib
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.sat_figure_render(None, stream) == _lib.SAT_ERR_ARGUMENT
    for field in ("lut", "src", "minmax"):
        d, host, keep = _valid(cuda)
        if field == "lut":
            d.lut = d.lut + 1
        else:
            setattr(host[0], field, getattr(host[0], field) + 2)
        assert lib.sat_figure_render(ctypes.byref(d), stream) == _lib.SAT_ERR_ARGUMENT
        torch.cuda.synchronize()
        assert (keep[-1] == FILL).all()
    # the untouched descriptor is accepted and fills the canvas
    d, host, keep = _valid(cuda)
    assert lib.sat_figure_render(ctypes.byref(d), stream) == 0
    torch.cuda.synchronize()
    assert not (keep[-1] == FILL).any()
    # nothing to draw: accepted, nothing launched
    d, host, keep = _valid(cuda)
    d.n_fig = 0
    assert lib.sat_figure_render(ctypes.byref(d), stream) == 0
    torch.cuda.synchronize()
    assert (keep[-1] == FILL).all()
