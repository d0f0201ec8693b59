"""Training summaries on the GPU: the image kernels (csrc/summary.hip) against their numpy
statement (tests/summary_ref.py), their entry refusals, and the model surface -- event files of
a six-step run over the graph cache, training unperturbed by summaries, evaluate()'s means.

Kernel acceptance: the kernel evaluates floor(255 * (x - lo) / (hi - lo) + 0.5) with every fp32
operation rounded on its own (no contraction, IEEE division), as numpy does, so the canvases are
asserted EQUAL to the reference, pixel for pixel (the issue's one-grey-level allowance is not
used); pixels at lo are 0, pixels at hi 255, everything outside the crop 0.  min / max and the
non-finite counts are exact (no arithmetic in them).  Shapes sit around the 32-wide tile."""
import os

import numpy as np
import pytest
import torch

import summary_ref as R

pytestmark = pytest.mark.gpu


def _launch(cuda, src, base, rows, cols, col_stride, Rmax, Cmax, shift=0, host=True):
    """Run minmax + render on ``src`` (numpy, flat or not) placed ``shift`` floats past a
    16-byte boundary.  Returns (canvas, minmax, nonfinite) as numpy."""
    from sat_amd import kernels as K
    flat = np.ascontiguousarray(src, np.float32).reshape(-1)
    buf = torch.zeros(flat.size + 8, device=cuda)
    o = (-(buf.data_ptr() // 4) % 4) + shift
    d = buf[o:o + flat.size]
    assert d.data_ptr() % 16 == 4 * shift
    d.copy_(torch.from_numpy(flat))
    n = len(base)
    tb = torch.tensor(base, dtype=torch.int64, device=cuda)
    tr = torch.tensor(rows, dtype=torch.int32, device=cuda)
    tc = torch.tensor(cols, dtype=torch.int32, device=cuda)
    mm = torch.full((n, 2), 7.0, device=cuda)
    bad = torch.full((n,), -1, dtype=torch.int32, device=cuda)
    canvas = torch.full((n, Rmax, Cmax), 99, dtype=torch.uint8, device=cuda)
    hr, hc = (rows, cols) if host else (None, None)
    K.image_minmax(d, tb, tr, tc, col_stride, Rmax, Cmax, mm, bad, hr, hc)
    K.image_render(d, tb, tr, tc, col_stride, mm, canvas, hr, hc)
    torch.cuda.synchronize()
    return canvas.cpu().numpy(), mm.cpu().numpy(), bad.cpu().numpy()


def _check(src, base, rows, cols, col_stride, Rmax, Cmax, got):
    canvas, mm, bad = got
    want_mm, want_bad = R.minmax(src, base, rows, cols, col_stride)
    assert mm.tobytes() == want_mm.tobytes() and (bad == want_bad).all()
    want = R.render(src, base, rows, cols, col_stride, Rmax, Cmax, want_mm)
    diff = np.abs(canvas.astype(np.int32) - want.astype(np.int32))
    print(f"max grey-level difference {int(diff.max()) if diff.size else 0}, "
          f"pixels that differ {int((diff > 0).sum())} of {diff.size}")
    assert diff.max(initial=0) == 0
    for i in range(len(base)):
        r, c = rows[i], cols[i]
        assert not canvas[i, r:, :].any() and not canvas[i, :, c:].any()    # outside the crop
        x = R.crop(src, base[i], r, c, col_stride)[::-1]
        if want_mm[i, 1] > want_mm[i, 0]:
            assert (canvas[i, :r, :c][x == want_mm[i, 0]] == 0).all()
            assert (canvas[i, :r, :c][x == want_mm[i, 1]] == 255).all()
        else:
            assert not canvas[i].any()
    return canvas


@pytest.mark.parametrize("rows,cols", [(1, 1), (31, 64), (33, 37), (64, 33)])
@pytest.mark.parametrize("shift", [0, 1])
def test_full_canvas_sizes_around_the_tile(cuda, rows, cols, shift):
    """One image that fills its canvas; contiguous columns (col_stride == rows), at a 16-byte
    aligned base and one float past it (the scalar path)."""
    rng = np.random.default_rng(rows * 100 + cols)
    src = rng.standard_normal(rows * cols).astype(np.float32) * 3 - 4       # negative values too
    args = ([0], [rows], [cols], rows, rows, cols)
    _check(src, *args, _launch(cuda, src, *args, shift=shift))


def test_alignment_history_layout_five_crops_one_launch(cuda):
    """A[t][b][n] with B = 3 (col_stride = B * N != rows): five images of different crops, all
    smaller than the 40 x 70 canvas, rendered by one launch; bases b * N are not all multiples
    of four floats, so aligned and unaligned images share the launch."""
    T, B, N = 70, 3, 37
    rng = np.random.default_rng(3)
    src = rng.random((T, B, N)).astype(np.float32)
    base = [0, N, 2 * N, 0, N]
    rows = [37, 33, 1, 32, 5]
    cols = [70, 37, 64, 1, 33]
    args = (base, rows, cols, B * N, 40, 70)
    canvas = _check(src, *args, _launch(cuda, src, *args))
    # the picture itself: image 1, bottom line = source row n = 0 of utterance 1 over time
    x = src[:37, 1, :33].T
    lo, hi = x.min(), x.max()
    assert (canvas[1, 32, :37] == R.quantise(x[0], lo, hi)).all()
    # without the host copies of the crop lengths the launch is the same
    again = _launch(cuda, src, *args, host=False)[0]
    assert (again == canvas).all()


def test_mel_layout_negative_values_and_aligned_stride(cuda):
    """X[b][t][m] (rows m = 80, columns t, col_stride 80 -- every column 16-byte aligned, so
    the 16-byte lanes run with a scalar tail at rows 76..78), mel-range negative values."""
    Bn, T, M = 2, 45, 80
    rng = np.random.default_rng(5)
    src = (rng.random((Bn, T, M)).astype(np.float32) * 7 - 8)
    args = ([0, T * M], [79, 80], [45, 31], M, 80, 48)
    _check(src, *args, _launch(cuda, src, *args))


def test_constant_image_is_black(cuda):
    src = np.full(33 * 37, -2.5, np.float32)
    args = ([0], [33], [37], 33, 33, 37)
    canvas, mm, bad = _launch(cuda, src, *args)
    assert not canvas.any() and mm.tolist() == [[-2.5, -2.5]] and bad.tolist() == [0]


def test_nonfinite_pixels_are_counted_and_black(cuda):
    rng = np.random.default_rng(9)
    src = rng.standard_normal((2, 33 * 37)).astype(np.float32)
    src[0, [0, 40, 700, 1220]] = [np.nan, np.inf, -np.inf, np.nan]
    src[1] = np.nan                                         # no finite pixel at all
    args = ([0, 33 * 37], [33, 33], [37, 37], 33, 33, 37)
    got = _launch(cuda, src, *args)
    canvas = _check(src, *args, got)
    assert got[2].tolist() == [4, 33 * 37] and got[1][1].tolist() == [0.0, 0.0]
    x = R.crop(src, 0, 33, 37, 33)[::-1]
    assert (canvas[0][~np.isfinite(x)] == 0).all() and not canvas[1].any()
    assert canvas[0].max() == 255                           # the finite range still spans 0..255


def _refusal_kw(cuda):
    return dict(src=torch.zeros(64 * 64, device=cuda),
                base=torch.zeros(2, dtype=torch.int64, device=cuda),
                rows=torch.full((2,), 8, dtype=torch.int32, device=cuda),
                cols=torch.full((2,), 8, dtype=torch.int32, device=cuda), col_stride=64,
                minmax=torch.zeros(2, 2, device=cuda),
                nonfinite=torch.zeros(2, dtype=torch.int32, device=cuda),
                canvas=torch.full((2, 16, 24), 5, dtype=torch.uint8, device=cuda))


def _raw(entry, kw, **over):
    """The C entry itself through ``_lib.call`` (which raises SatLibraryError on a refusal),
    so that a null pointer or a negative size reaches it."""
    from sat_amd import _lib
    a = dict(src=kw["src"].data_ptr(), src_n=kw["src"].numel(), base=kw["base"].data_ptr(),
             rows=kw["rows"].data_ptr(), cols=kw["cols"].data_ptr(), col_stride=64, n=2, Rmax=16,
             Cmax=24, rows_host=None, cols_host=None, minmax=kw["minmax"].data_ptr(),
             out=(kw["nonfinite"] if entry == "sat_image_minmax" else kw["canvas"]).data_ptr())
    a.update(over)
    stream = torch.cuda.current_stream().cuda_stream
    _lib.call(entry, a["src"], a["src_n"], a["base"], a["rows"], a["cols"], a["col_stride"],
              a["n"], a["Rmax"], a["Cmax"], a["rows_host"], a["cols_host"], a["minmax"], a["out"],
              stream)


@pytest.mark.parametrize("entry", ["sat_image_minmax", "sat_image_render"])
def test_entries_refuse_before_launching(cuda, entry):
    """A null pointer, a negative size and a crop larger than the canvas come back as
    SAT_ERR_ARGUMENT; the outputs keep what they held, so nothing was launched."""
    from sat_amd import _lib, kernels as K
    kw = _refusal_kw(cuda)
    for over in (dict(src=None), dict(base=None), dict(rows=None), dict(cols=None),
                 dict(minmax=None), dict(out=None), dict(src_n=-1), dict(col_stride=-64),
                 dict(n=-2), dict(Rmax=-16), dict(Cmax=-24)):
        with pytest.raises(_lib.SatLibraryError) as e:
            _raw(entry, kw, **over)
        assert e.value.rc == _lib.SAT_ERR_ARGUMENT, over
    for hr, hc, msg in (([8, 17], [8, 8], "rows[1] = 17"), ([8, 8], [25, 8], "cols[0] = 25"),
                        ([-1, 8], [8, 8], "rows[0] = -1")):
        with pytest.raises(_lib.SatLibraryError) as e:
            if entry == "sat_image_minmax":
                K.image_minmax(kw["src"], kw["base"], kw["rows"], kw["cols"], 64, 16, 24,
                               kw["minmax"], kw["nonfinite"], hr, hc)
            else:
                K.image_render(kw["src"], kw["base"], kw["rows"], kw["cols"], 64, kw["minmax"],
                               kw["canvas"], hr, hc)
        assert e.value.rc == _lib.SAT_ERR_ARGUMENT and msg in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert (kw["canvas"] == 5).all() and not kw["minmax"].any()
    _raw(entry, kw)                                          # the unchanged request is accepted
    torch.cuda.synchronize()
    if entry == "sat_image_render":
        assert not kw["canvas"].any()                        # a zero source renders black


# ------------------------------------------------------------------ the model surface
def _hp(**kw):
    from sat_amd import hparams
    return hparams.ljspeech_hparams(max_iters=24, **kw)


SUMMARY_HP = dict(save_summary_steps=2, alignment_save_steps=3, save_training_time_metrics=True)


@pytest.fixture(scope="module")
def batches():
    """Six batches of one padded shape (the small model of tests/test_checkpoint_gpu.py)."""
    from sat_amd import models
    it = models.synthetic_input_fn(_hp(), 2, N=13, T=16, shape="ljs", seed=20)()
    out = [next(it) for _ in range(6)]
    assert len({b[0].source.shape for b in out}) == 1
    return out


def _events(d):
    files = [f for f in os.listdir(d) if f.startswith("events.out.tfevents.")]
    assert len(files) == 1, files
    return R.read_events(os.path.join(d, files[0]))


@pytest.fixture(scope="module")
def run(cuda, batches, tmp_path_factory):
    """Six TRAIN steps with summaries over the graph cache (step 1 eager + capture, steps 2..6
    replays), stepped through model_fn so that every step's returned loss is kept."""
    from sat_amd import models
    d = str(tmp_path_factory.mktemp("summaries"))
    m = models.DualSourceSelfAttentionTacotronModel(_hp(**SUMMARY_HP), model_dir=d, device=cuda,
                                                    graph_cache=2, summaries=True)
    losses = []
    for f, l in batches:
        losses.append(m.model_fn(f, l, models.ModeKeys.TRAIN).loss)
    assert m._graphs.misses == 1 and m._graphs.hits == 5
    m.flush_summaries()
    torch.cuda.synchronize()
    out, sv = m._graphs.last_record
    rec = dict(model=m, dir=d, losses=[x.cpu().numpy() for x in losses],
               AL1=sv["dec"].AL1.cpu().numpy(), events=_events(d),
               params=m.engine.params.cpu())
    return rec


def test_scalar_events_at_the_summary_steps(run):
    evs = run["events"]
    assert evs[0]["file_version"] == "brain.Event:2"
    scal = {e["step"]: e["scalars"] for e in evs if e["scalars"]}
    assert sorted(scal) == [2, 4, 6]
    for step, s in scal.items():
        want = run["losses"][step - 1]
        assert s["loss_with_teacher"].tobytes() == want.astype("<f4").tobytes(), step
        assert s["code_loss"] == s["code_loss_with_teacher"]
        assert s["done_loss"] == s["done_loss_with_teacher"]
        assert np.float32(s["code_loss"] + s["done_loss"]) == pytest.approx(want[0], rel=1e-6)
        assert s["l2_regularization_loss"] == 0.0 and s["global_norm"] > 0
        assert 0 < s["learning_rate"] < 1e-3 and s["global_step/sec"] > 0


def test_image_events_at_the_alignment_steps(run, batches):
    evs = run["events"]
    imgs = {e["step"]: e["images"] for e in evs if e["images"]}
    assert sorted(imgs) == [3, 6]
    tags = set(imgs[6])
    for name in ("alignment1", "alignment2", "mel_predicted", "mel_target"):
        assert {f"{name}/0", f"{name}/1"} <= tags and f"{name}/2" not in tags     # min(B, 3) = 2
    # step 6's alignment1/0: source_length_0 lines of T'_0 steps, equal to the reference's
    # rendering of the trainer's alignment buffer after step 6 (the arithmetic is pinned)
    f, l = batches[5]
    r = _hp().outputs_per_step
    n0, t0 = int(f.source_length[0]), -(-int(l.target_length[0]) // r)
    h, w, png = imgs[6]["alignment1/0"]
    got = R.decode_png(png)
    assert (h, w) == (n0, t0) == got.shape
    AL1 = run["AL1"]                                        # [T' + 1, B, N]
    _, B, N = AL1.shape
    want = R.render(AL1, [B * N], [n0], [t0], B * N, n0, t0)[0]
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    print("alignment1/0 max grey-level difference", int(diff.max()))
    assert diff.max() == 0 and got.max() == 255
    hm, wm, _ = imgs[6]["mel_target/1"]
    assert (hm, wm) == (80, int(l.target_length[1]))


def test_replayed_plots_are_the_steps_own(cuda, run, batches):
    """Ties the image source to the step: an EAGER run (no graph cache, no summaries) of the same
    seed and batches holds step 6's and step 3's tensors in ordinary memory; replays are
    bit-identical to eager steps, so the plots written from the replayed graph's static buffers
    must equal the reference's rendering of the eager tensors."""
    from sat_amd import models
    imgs = {e["step"]: e["images"] for e in run["events"] if e["images"]}
    m = models.DualSourceSelfAttentionTacotronModel(_hp(**SUMMARY_HP), device=cuda, graph_cache=0)
    r = _hp().outputs_per_step
    for step, (f, l) in enumerate(batches, 1):
        m.model_fn(f, l, models.ModeKeys.TRAIN)
        if step not in (3, 6):
            continue
        torch.cuda.synchronize()
        sv = m._trainer.last_saved
        AL1, S2, mel = (x.cpu().numpy() for x in (sv["dec"].AL1, sv["dec"].S2, sv["mel"]))
        _, B, N = AL1.shape
        _, T, M = mel.shape
        for i in range(B):
            n, t = int(f.source_length[i]), int(l.target_length[i])
            tp = -(-t // r)
            for tag, want in (
                    (f"alignment1/{i}", R.render(AL1, [B * N + i * N], [n], [tp], B * N, n, tp)),
                    (f"alignment2/{i}", R.render(S2, [i * N], [n], [tp], B * N, n, tp)),
                    (f"mel_predicted/{i}", R.render(mel, [i * T * M], [M], [t], M, M, t)),
                    (f"mel_target/{i}", R.render(np.asarray(l.codes), [i * T * M], [M], [t], M,
                                                 M, t))):
                got = R.decode_png(imgs[step][tag][2])
                assert got.shape == want[0].shape and (got == want[0]).all(), (step, tag)
    assert torch.equal(m.engine.params.cpu(), run["params"])


def test_plots_under_a_padded_step_count(cuda, batches, tmp_path):
    """graph_t_quantum pads T' inside the graph cache (8 -> 9 steps here, 16 -> 18 frames), so
    the step's own tensors are larger than the caller's batch: strides and canvases must come
    from them, the crops from target_length.  mel_target is checked against the caller's
    unpadded batch (utterance 1 sits at another base in the padded tensor), the predicted
    frames and the alignments against the step's recorded tensors."""
    from sat_amd import models
    d = str(tmp_path / "quantum")
    m = models.DualSourceSelfAttentionTacotronModel(_hp(**SUMMARY_HP), model_dir=d, device=cuda,
                                                    graph_cache=2, graph_t_quantum=3,
                                                    summaries=True)
    for f, l in batches[:3]:                               # step 3 draws, from a replay
        m.model_fn(f, l, models.ModeKeys.TRAIN)
    assert m._graphs.misses == 1 and m._graphs.hits == 2
    m.flush_summaries()
    torch.cuda.synchronize()
    _, sv = m._graphs.last_record
    AL1, mel = sv["dec"].AL1.cpu().numpy(), sv["mel"].cpu().numpy()
    f, l = batches[2]
    r = _hp().outputs_per_step
    assert AL1.shape[0] == 9 + 1 and mel.shape[1] == 18 and np.asarray(l.codes).shape[1] == 16
    imgs = {e["step"]: e["images"] for e in _events(d) if e["images"]}
    assert sorted(imgs) == [3]
    _, B, N = AL1.shape
    M = mel.shape[2]
    for i in range(B):
        n, t = int(f.source_length[i]), int(l.target_length[i])
        tp = -(-t // r)
        for tag, want in (
                (f"alignment1/{i}", R.render(AL1, [B * N + i * N], [n], [tp], B * N, n, tp)),
                (f"mel_predicted/{i}", R.render(mel, [i * 18 * M], [M], [t], M, M, t)),
                (f"mel_target/{i}", R.render(np.asarray(l.codes), [i * 16 * M], [M], [t], M, M,
                                             t))):
            got = R.decode_png(imgs[3][tag][2])
            assert got.shape == want[0].shape and (got == want[0]).all(), tag


def test_summaries_do_not_perturb_training(cuda, run, batches, tmp_path):
    from sat_amd import models
    d = str(tmp_path / "plain")
    m = models.DualSourceSelfAttentionTacotronModel(_hp(**SUMMARY_HP), model_dir=d, device=cuda,
                                                    graph_cache=2)
    m.train(lambda: iter(batches), 6)
    torch.cuda.synchronize()
    assert torch.equal(m.engine.params.cpu(), run["params"])
    # the default: model_dir holds checkpoint files only
    names = os.listdir(d)
    assert names and all(n.startswith("model.ckpt-") or n == "checkpoint" for n in names), names
    assert m._recorders == {} and m._graphs.last_record is None


def test_evaluate_returns_the_streaming_means(cuda, run, batches):
    from sat_amd import models
    from sat_amd.summary import EVAL_METRICS
    m = run["model"]
    m.save()                                               # evaluate() restores the newest file
    per = []
    for f, l in batches[:2]:
        spec = m.model_fn(f, l, models.ModeKeys.EVAL)
        per.append({k: float(spec.eval_metric_ops[k].item()) for k in EVAL_METRICS}
                   | {"loss": float(spec.loss.item())})
    got = m.evaluate(lambda: iter(batches[:2]), 2)
    assert set(got) == set(EVAL_METRICS) | {"loss", "global_step"} and got["global_step"] == 6
    for k in (*EVAL_METRICS, "loss"):
        assert got[k] == (per[0][k] + per[1][k]) / 2, k
    assert got["l2_regularization_loss"] == 0.0
    assert got["loss"] == pytest.approx(got["code_loss"] + got["done_loss"], rel=1e-6)
    # the same numbers, and the first batch's plots, in model_dir/eval at the restored step
    evs = _events(os.path.join(run["dir"], "eval"))
    scal = [e for e in evs if e["scalars"]]
    assert len(scal) == 1 and scal[0]["step"] == 6
    for k in (*EVAL_METRICS, "loss"):
        assert scal[0]["scalars"][k] == np.float32(got[k]), k
    imgs = [e for e in evs if e["images"]]
    assert len(imgs) == 1 and imgs[0]["step"] == 6
    assert {"alignment1/0", "alignment2/1", "mel_predicted/0", "mel_target/1"} <= set(imgs[0]["images"])
    assert any(t.startswith("decoder_self_attention0_head0/") for t in imgs[0]["images"])
    assert any(t.startswith("encoder_self_attention0_head0/") for t in imgs[0]["images"])
