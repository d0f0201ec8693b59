"""The VQ-code kernels (csrc/codes.hip) and the code path through the model on the GPU, against
the numpy restatement (codes_ref.py).  Every expected value is a zero, a one or an integer:
comparisons are bit for bit (``np.array_equal`` / ``torch.equal``), no tolerance anywhere."""
import os

import numpy as np
import pytest
import torch

import codes_ref as CR

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "codes")


def _seqs(lengths, C, seed=0):
    """Indices whose first and last positions of every utterance hold 0 and C - 1."""
    rng = np.random.default_rng(seed)
    out = []
    for n in lengths:
        s = rng.integers(0, C, n).astype(np.int32)
        s[-1] = C - 1
        s[0] = 0 if n > 1 else s[0]
        out.append(s)
    return out


def _guarded(dev, shape, dtype=torch.float32):
    """``(buffer, inner view, guard size)``: a NaN-filled (int64: -7-filled) buffer with at least
    two rows of guard elements on each side of the inner view the kernel is handed.  The guard is
    a multiple of 4 elements, so the view keeps the allocation's 16-byte alignment."""
    n = int(np.prod(shape))
    g = max(64, -(-2 * int(shape[-1]) // 4) * 4)
    fill = float("nan") if dtype.is_floating_point else -7
    buf = torch.full((g + n + g,), fill, dtype=dtype, device=dev)
    return buf, buf[g:g + n].view(shape), g


def _run_batch(dev, seqs, C, T_pad, r=1, check=True):
    from sat_amd import kernels as K
    B = len(seqs)
    offsets = np.zeros(B + 1, np.int64)
    np.cumsum([len(s) for s in seqs], out=offsets[1:])
    idx = torch.tensor(np.concatenate(seqs).astype(np.int32), device=dev)
    off = torch.tensor(offsets, device=dev)
    shapes = {"codes": (B, T_pad, C), "done": (B, T_pad // r), "code_loss_mask": (B, T_pad),
              "binary_loss_mask": (B, T_pad)}
    bufs = {k: _guarded(dev, s) for k, s in shapes.items()}
    bufs["target_length"] = _guarded(dev, (B,), torch.int64)
    err = None
    try:
        K.codes_batch(idx, off, offsets, C=C, T_pad=T_pad, r=r, check=check,
                      **{k: v[1] for k, v in bufs.items()})
    except ValueError as e:
        err = e
    torch.cuda.synchronize()
    return bufs, err


def _check_guards(bufs):
    for name, (buf, inner, g) in bufs.items():
        for edge in (buf[:g], buf[g + inner.numel():]):
            ok = torch.isnan(edge).all() if buf.dtype.is_floating_point else (edge == -7).all()
            assert bool(ok), f"{name}: a guard element was written"


CASES = [((7, 1, 4), T_pad, C) for T_pad in (7, 12) for C in (256, 5, 4, 1)] \
    + [((33, 64, 1), 64, 8)]
NAMES = ("codes", "done", "code_loss_mask", "binary_loss_mask", "target_length")


def _compare(cuda, seqs, C, T_pad, r):
    bufs, err = _run_batch(cuda, seqs, C, T_pad, r)
    assert err is None
    want = dict(zip(NAMES, CR.batch(seqs, C, T_pad, r)))
    for name, w in want.items():
        got = bufs[name][1].cpu().numpy()
        assert got.dtype == w.dtype and got.shape == w.shape
        unwritten = np.isnan(got) if got.dtype.kind == "f" else got == -7
        assert not unwritten.any(), f"{name}: an element was left unwritten"
        assert np.array_equal(got, w), name
    _check_guards(bufs)
    again, _ = _run_batch(cuda, seqs, C, T_pad, r)
    for name in NAMES:
        assert torch.equal(bufs[name][1], again[name][1]), f"{name}: two runs differ"


@pytest.mark.parametrize("lengths,T_pad,C", CASES)
def test_codes_batch(cuda, lengths, T_pad, C):
    _compare(cuda, _seqs(lengths, C), C, T_pad, 1)


@pytest.mark.parametrize("C", (4, 5))
def test_codes_batch_outputs_per_step_2(cuda, C):
    """``done`` has one entry per r frames; an utterance shorter than r has no done step."""
    _compare(cuda, _seqs((7, 1, 4), C), C, 12, 2)


@pytest.mark.parametrize("C", (256, 5))
@pytest.mark.parametrize("bad", ("C", -1))
def test_codes_batch_refuses_an_index_out_of_range(cuda, C, bad):
    from sat_amd import kernels as K
    seqs = _seqs((7, 1, 4), C)
    value = C if bad == "C" else -1
    seqs[2][1] = value
    seqs[2][3] = value                        # a later one: the lowest position is reported
    bufs, err = _run_batch(cuda, seqs, C, 12)
    assert isinstance(err, ValueError)
    assert "utterance 2" in str(err) and "position 1" in str(err) and str(value) in str(err)
    _check_guards(bufs)
    # the bad positions are stored nowhere: their rows are zeros, everything else as usual
    clean = [s.copy() for s in seqs]
    want = CR.batch([np.where((s < 0) | (s >= C), 0, s) for s in clean], C, 12)[0]
    want[2, 1] = 0
    want[2, 3] = 0
    assert np.array_equal(bufs["codes"][1].cpu().numpy(), want)
    # the word was cleared after the report: a clean batch passes again
    assert int(K.codes_error_word(cuda).item()) == 0
    _, err = _run_batch(cuda, _seqs((7, 1, 4), C), C, 12)
    assert err is None


def test_codes_batch_refusals_before_launch(cuda):
    from sat_amd import _lib, kernels as K
    dev = cuda
    idx = torch.zeros(12, dtype=torch.int32, device=dev)

    def call(offsets, C=8, T_pad=8, r=1, **kw):
        off = torch.tensor(offsets, dtype=torch.int64, device=dev)
        return K.codes_batch(idx[:offsets[-1]], off, offsets, C=C, T_pad=T_pad, r=r, **kw)

    call([0, 7, 8, 12])                                               # the accepted form
    for kw, text in ((dict(C=0), "C 0 < 1"), (dict(T_pad=6), "T_pad 6 <"),
                     (dict(T_pad=9, r=2), "multiple of r"), (dict(offsets=[0, 7, 7, 12]), "< 1"),
                     (dict(offsets=[0, 7, 6, 12]), "< 1")):
        offsets = kw.pop("offsets", [0, 7, 8, 12])
        with pytest.raises(_lib.SatLibraryError, match=text) as e:
            call(offsets, **kw)
        assert e.value.rc == _lib.SAT_ERR_ARGUMENT
    # misaligned outputs: codes 4 bytes off a 16-byte boundary (C % 4 == 0)
    raw = torch.empty(3 * 8 * 8 + 4, device=dev)
    with pytest.raises(_lib.SatLibraryError, match="16-byte aligned") as e:
        call([0, 7, 8, 12], codes=raw[1:1 + 3 * 8 * 8].view(3, 8, 8))
    assert e.value.rc == _lib.SAT_ERR_ARGUMENT
    call([0, 7, 8, 12], C=5, codes=raw[1:1 + 3 * 8 * 5].view(3, 8, 5))   # 4-byte rows: accepted
    torch.cuda.synchronize()


def _argmax_rows(R, C, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((R, C)).astype(np.float32)
    x[0, 0] = 9.0                                    # the maximum at index 0
    if R > 1:
        x[1, C - 1] = 9.0                            # ... and at C - 1
    if R > 2:
        x[2] = -np.abs(x[2]) - 1.0                   # an all-negative row
    if R > 3 and C >= 3:
        x[3, [C // 3, C // 2, C - 1]] = 7.5          # an exact tie of three: the lowest wins
    if R > 4:
        x[4] = 0.25                                  # every entry ties
    return x


@pytest.mark.parametrize("C", (5, 64, 256, 1025))
@pytest.mark.parametrize("R", (1, 37))
def test_codes_argmax(cuda, R, C):
    from sat_amd import kernels as K
    x = _argmax_rows(R, C, seed=C + R)
    want = CR.argmax(x)
    if R > 3 and C >= 3:
        assert want[3] == min(C // 3, C // 2) and want[4] == 0
    ld = C + 3                                       # a row stride larger than C
    wide = torch.full((R, ld), float("inf"), device=cuda)
    wide[:, :C] = torch.tensor(x, device=cuda)
    for xin in (torch.tensor(x, device=cuda), wide[:, :C]):
        idx, onehot = K.codes_argmax(xin, onehot=True)
        assert idx.dtype == torch.int32 and tuple(idx.shape) == (R,)
        assert np.array_equal(idx.cpu().numpy(), want)
        assert np.array_equal(onehot.cpu().numpy(), CR.one_hot(want, C))
        idx2 = K.codes_argmax(xin)
        assert torch.equal(idx, idx2)
    # 3-d input, as the decoder's [B, T, C] outputs
    if R == 37:
        x3 = torch.tensor(x[:36].reshape(4, 9, C), device=cuda)
        assert np.array_equal(K.codes_argmax(x3).cpu().numpy(), want[:36].reshape(4, 9))


def test_codes_argmax_refusals(cuda):
    from sat_amd import _lib
    x = torch.zeros(4, 8, device=cuda)
    out = torch.zeros(4, dtype=torch.int32, device=cuda)
    L = _lib.load()
    assert L.sat_codes_argmax(x.data_ptr(), 8, 4, 0, out.data_ptr(), None, 0, None) \
        == _lib.SAT_ERR_ARGUMENT
    assert L.sat_codes_argmax(x.data_ptr(), 7, 4, 8, out.data_ptr(), None, 0, None) \
        == _lib.SAT_ERR_ARGUMENT
    assert b"row stride" in L.sat_last_error_string()


# ---------------------------------------------------------------- model level
C_MODEL = 16


def _hp(**kw):
    from sat_amd import hparams
    return hparams.codes_hparams(C_MODEL, **dict(dict(source="char", phoneme="none",
                                                      max_iters=24), **kw))


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    from sat_amd import preprocess
    out = tmp_path_factory.mktemp("codes_records")
    keys = preprocess.Codes(GOLDEN, str(out), _hp(), C_MODEL, compact=True).run()
    return out, keys


def _batches(corpus, hp, batch_size, keys=None):
    from sat_amd import datasets as D
    out, all_keys = corpus
    keys = keys or all_keys
    ds = D.create_from_tfrecord_files(
        [str(out / f"{k}.source.tfrecord") for k in keys],
        [str(out / f"{k}.target.tfrecord") for k in keys], hp, cycle_length=1)
    return ds.prepare_and_zip().group_by_batch(batch_size)


def test_train_step_equals_the_host_one_hot_route(cuda, corpus):
    """preprocess -> dataset -> sat_codes_batch against the same batch built as a host one-hot
    and uploaded: one TRAIN step, bitwise-equal loss and gradients."""
    from sat_amd import models as MD, params
    hp = _hp()
    feats, labels = next(iter(_batches(corpus, hp, 3)))
    seqs = [labels.code_index[labels.offsets[b]:labels.offsets[b + 1]] for b in range(3)]
    codes, done, cmask, bmask, tl = CR.batch(seqs, C_MODEL, int(labels.target_length.max()))
    host = MD.PreprocessedTargetData(labels.id, labels.key, codes, tl, done, cmask, bmask)
    vals = params.init_params(hp, seed=5)
    got = {}
    for name, lab in (("device", labels), ("host", host)):
        model = MD.DualSourceSelfAttentionTacotronModel(hp, device=cuda, init_values=vals,
                                                        seed=11)
        spec = model.model_fn(feats, lab, MD.ModeKeys.TRAIN, hp)
        torch.cuda.synchronize()
        got[name] = (spec.loss.clone(), model.engine.grads.clone(), model.engine.params.clone())
    assert bool(torch.isfinite(got["device"][0]).all())
    assert float(got["device"][1].abs().max()) > 0
    for a, b in zip(got["device"], got["host"]):
        assert torch.equal(a, b)


def test_predict_code_files_parse_back(cuda, corpus, tmp_path):
    from sat_amd import kernels as K, models as MD, params, predict_code as PC, tfrecord as R
    from sat_amd.synthesize import stop_frames
    hp = _hp()
    keys = ["p225_001", "p225_test"]
    model = MD.DualSourceSelfAttentionTacotronModel(hp, device=cuda,
                                                    init_values=params.init_params(hp, seed=5))

    def input_fn():
        return iter(_batches(corpus, hp, 1, keys).merge_target_to_source().dataset)

    written = PC.predict_codes(model, input_fn, str(tmp_path), hp)
    assert written == keys
    want = {w[0]: w for w in CR.read_corpus(GOLDEN)}
    for p, (features, _) in zip(model.predict(input_fn), input_fn()):
        key = features.key[0].decode()
        n = stop_frames(p["stop_token"], 1, p["mel"].shape[1])[0]
        idx = K.codes_argmax(p["mel"].contiguous())[0, :n].cpu().numpy()
        assert np.array_equal(idx, CR.argmax(p["mel"][0, :n].cpu().numpy()))
        dense = np.fromfile(tmp_path / f"{key}.mfbsp", "<f4").reshape(-1, C_MODEL)
        assert np.array_equal(dense, CR.one_hot(idx, C_MODEL))
        assert np.array_equal(dense, p["codes"][0, :n].cpu().numpy())   # predict()'s own one-hot
        (rec,) = R.read_tfrecords(str(tmp_path / f"{key}.tfrecord"))
        r = R.parse_prediction_result(rec)
        _, _, text, truth = want[key]
        assert np.array_equal(r.codes, dense) and r.codes_width == C_MODEL
        assert np.array_equal(r.ground_truth_codes, CR.one_hot(truth, C_MODEL))
        assert r.key.decode() == key and r.text.decode() == text.lower()
        assert r.source_length == len(text) == len(r.source)
        assert (tmp_path / f"{key}.txt").read_text() == text.lower()
        assert (tmp_path / f"{key}.preds.txt").read_text() == " ".join(map(str, idx)) + "\n"
        assert (tmp_path / f"{key}.truth.txt").read_text() == " ".join(map(str, truth)) + "\n"
    # --limit
    assert PC.predict_codes(model, input_fn, str(tmp_path / "one"), hp, limit=1) == keys[:1]
