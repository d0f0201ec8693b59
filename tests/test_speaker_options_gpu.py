"""The fork's speaker options on the GPU (speaker_embedding_projection_out_dim,
speaker_embedd_to_decoder, speaker_for_synthesis) against the literal fp64 form of
tests/speaker_options_ref.py: the three kernels of csrc/speaker.hip, the teacher-forced forward
and every parameter gradient, PREDICT, checkpoints."""
import functools
import warnings

import numpy as np
import pytest
import torch

import speaker_options_ref as SR
import transition_agent_ref as R

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ 1. kernels against numpy
def _dev(a, cuda):
    return torch.tensor(a).to(cuda)


@pytest.mark.parametrize("C", [8, 72, 224])         # 72, 224: no multiple of 64
def test_rows_bias_fwd_is_exact(cuda, C):
    from sat_amd import kernels as K
    rng = np.random.default_rng(C)
    Bn, N = 4, 40
    y = rng.standard_normal((Bn, N, C)).astype(np.float32)
    bias = rng.standard_normal((Bn, C)).astype(np.float32)
    lens = np.array([40, 33, 0, 7], np.int64)       # a zero-length utterance
    for L in (lens, None):
        got = K.rows_bias_fwd(_dev(y, cuda), _dev(bias, cuda), None if L is None else _dev(L, cuda))
        np.testing.assert_array_equal(got.cpu().numpy(), SR.rows_bias_fwd_np(y, bias, L))
    # strided destination: the middle columns of a wider buffer, the rest untouched
    wide = rng.standard_normal((Bn, N, C + 24)).astype(np.float32)
    g = _dev(wide, cuda)
    K.rows_bias_fwd(g[:, :, 8:8 + C], _dev(bias, cuda), _dev(lens, cuda))
    want = wide.copy()
    want[:, :, 8:8 + C] = SR.rows_bias_fwd_np(wide[:, :, 8:8 + C], bias, lens)
    np.testing.assert_array_equal(g.cpu().numpy(), want)
    # step-major [T, B, C]: the rows of utterance b are y[:, b]
    ys = np.ascontiguousarray(y.transpose(1, 0, 2))
    got = K.rows_bias_fwd(_dev(ys, cuda), _dev(bias, cuda), step_major=True)
    np.testing.assert_array_equal(got.cpu().numpy(), ys + bias[None])


@pytest.mark.parametrize("C", [8, 72, 224])
def test_rows_bias_bwd_matches_an_fp64_sum(cuda, C):
    from sat_amd import kernels as K
    rng = np.random.default_rng(100 + C)
    Bn, N = 4, 40
    dy = rng.standard_normal((Bn, N, C)).astype(np.float32)
    lens = np.array([40, 33, 0, 7], np.int64)

    def check(got, ref):
        got = got.cpu().numpy().astype(np.float64)
        rel = np.abs(got - ref) / np.maximum(np.abs(ref), 1e-30)
        print(f"C={C}: worst relative error {rel[ref != 0].max():.3e}")
        assert np.all(np.abs(got - ref) <= 1e-6 * np.abs(ref))
    for L in (lens, None):
        got = K.rows_bias_bwd(_dev(dy, cuda), None if L is None else _dev(L, cuda))
        check(got, SR.rows_bias_bwd_np(dy, L))
        if L is not None:
            assert not got[2].any()
    a = K.rows_bias_bwd(_dev(dy, cuda), _dev(lens, cuda))
    b = K.rows_bias_bwd(_dev(dy, cuda), _dev(lens, cuda))
    assert torch.equal(a, b)                                        # no atomics
    # strided source (columns of a wider buffer) and the step-major form
    wide = rng.standard_normal((Bn, N, C + 24)).astype(np.float32)
    check(K.rows_bias_bwd(_dev(wide, cuda)[:, :, 8:8 + C], _dev(lens, cuda)),
          SR.rows_bias_bwd_np(wide[:, :, 8:8 + C], lens))
    ys = np.ascontiguousarray(dy.transpose(1, 0, 2))
    check(K.rows_bias_bwd(_dev(ys, cuda), step_major=True), SR.rows_bias_bwd_np(dy))


def test_ctx_tail_fill(cuda):
    from sat_amd import kernels as K
    rng = np.random.default_rng(7)
    T, Bn, W, S = 7, 3, 44, 8
    ctx = rng.standard_normal((T, Bn, W)).astype(np.float32)
    s = rng.standard_normal((Bn, S)).astype(np.float32)
    for col0, t0, t1 in ((36, 1, 7), (28, 0, 7), (36, 3, 3)):
        g = _dev(ctx, cuda)
        K.ctx_tail_fill(g, col0, _dev(s, cuda), t0, t1)
        np.testing.assert_array_equal(g.cpu().numpy(), SR.ctx_tail_fill_np(ctx, col0, s, t0, t1))
    # its backward is the column sum over the steps
    got = K.rows_bias_bwd(_dev(ctx, cuda)[1:, :, 36:], step_major=True).cpu().numpy()
    ref = ctx[1:, :, 36:].astype(np.float64).sum(0)
    assert np.all(np.abs(got - ref) <= 1e-6 * np.abs(ref))


def test_entries_refuse_bad_arguments(cuda):
    from sat_amd import _lib
    from sat_amd import kernels as K
    y = torch.zeros(2, 5, 12, device=cuda)
    b = torch.zeros(2, 12, device=cuda)
    for fn in (lambda: K.rows_bias_fwd(y[:, :, 1:9], b[:, :8].contiguous()),      # not 16-byte aligned
               lambda: K.rows_bias_fwd(y[:, :, :6], b[:, :6]),                    # C % 4
               lambda: K.rows_bias_bwd(y[:, :, 2:10]),
               lambda: K.ctx_tail_fill(y, 2, torch.zeros(5, 8, device=cuda), 0, 2)):  # col0 % 4
        with pytest.raises(_lib.SatLibraryError) as e:
            fn()
        assert e.value.rc == _lib.SAT_ERR_ARGUMENT
    lib = _lib.load()
    assert lib.sat_rows_bias_fwd(None, 0, 0, None, 0, 1, 1, 4, None, None) == _lib.SAT_ERR_ARGUMENT
    assert lib.sat_rows_bias_bwd(None, 0, 0, None, 0, 1, 1, 4, None, None) == _lib.SAT_ERR_ARGUMENT
    assert lib.sat_ctx_tail_fill(None, 0, 0, 0, None, 0, 0, 1, 1, 4, None) == _lib.SAT_ERR_ARGUMENT


# ------------------------------------------------------------------ 2. model against the literal form
@functools.lru_cache(maxsize=None)
def _case(key, agent, train, persistent=False):
    """One teacher-forced step on the GPU and in the fp64 literal form (computed once, shared by
    the forward and the gradient tests)."""
    from sat_amd import data, decoder, engine, params
    from oracle import sat_oracle as O
    cuda = torch.device("cuda:0")
    hp = SR.make_hparams(key, agent=agent)
    vals = SR.make_values(hp)
    m = engine.Tacotron(hp, cuda, init_values=vals, persistent_decoder=persistent)
    batch = SR.make_batch(hp)
    masks = data.synthetic_masks(hp, SR.B, SR.N, SR.T, seed=SR.BATCH_SEED + 9) if train else None
    gb = {k: torch.tensor(v).to(cuda) for k, v in batch.items()}
    gm = None if masks is None else {k: torch.tensor(v).to(cuda) for k, v in masks.items()}
    with warnings.catch_warnings():
        # a requested persistent path must not fall back
        warnings.simplefilter("error", decoder.PersistentFallbackWarning)
        out, sv = m.forward(gb, gm, training=train)
    m.backward(sv)
    torch.cuda.synchronize()
    assert int(sv["spk_err"].item()) == 0
    grads = m.grads_dict()
    got = {k: out[k].detach().double().cpu() for k in ("mel", "stop", "alignment1", "alignment2")}
    got["loss"] = float(out["loss"].item())
    mp = pytest.MonkeyPatch()
    try:
        if agent:
            R.patch_oracle(mp, O, True, False)
        p64 = {k: v.requires_grad_(True) for k, v in O.to_torch(vals).items()}
        ref = SR.model_forward(O, p64, O.to_torch(params.init_bn_buffers(hp)), hp,
                               O.to_torch(batch), None if masks is None else O.to_torch(masks),
                               train)
        ref["loss"].backward()
    finally:
        mp.undo()
    ref = {k: (v.detach() if isinstance(v, torch.Tensor) else v) for k, v in ref.items()}
    return hp, grads, {k: v.grad for k, v in p64.items()}, got, ref


CASES = ([(None, False, False), (None, False, True)] +
         [(k, a, False) for k in sorted(SR.OPTIONS) for a in (False, True)] +
         [("all", False, True), ("all", True, True)])
IDS = [f"{k or 'stock'}-{'agent' if a else 'plain'}-{'train' if t else 'eval'}" for k, a, t in CASES]


@pytest.mark.parametrize("key,agent,train", CASES, ids=IDS)
def test_forward_matches_the_literal_reference(cuda, key, agent, train):
    """mel / stop / loss at the tolerances of tests/test_model_fwd_gpu.py, both alignment
    histories at the 2e-5 of the decode and transition-agent tests; and the algebra's premise,
    sum_n alpha = 1 within 1e-6 at every step, on the reference's own alignments."""
    hp, _, _, got, ref = _case(key, agent, train)
    err = (got["mel"] - ref["mel"]).abs()
    d_stop = float((got["stop"].reshape(-1) - ref["stop"].reshape(-1)).abs().max())
    d_loss = abs(got["loss"] - float(ref["loss"]))
    d_al = [float((got[k] - ref[k].transpose(0, 1)).abs().max())
            for k in ("alignment1", "alignment2")]
    print(f"mel mean {float(err.mean()):.3e} max {float(err.max()):.3e} stop {d_stop:.3e} "
          f"loss {d_loss:.3e} alignments {d_al[0]:.3e} {d_al[1]:.3e}")
    for k in ("alignment1", "alignment2"):
        assert float((ref[k].sum(-1) - 1).abs().max()) <= 1e-6
    if ref["pre"] is not None:
        assert float(ref["pre"].abs().min()) >= 1e-4                 # clear of the ReLU kink
    assert float(err.mean()) < 1e-5 and float(err.max()) < 2e-4
    assert d_stop < 2e-4
    assert d_loss < 1e-5
    assert max(d_al) <= 2e-5


def _compare(grads, g64, tol=2e-4):
    """tests/test_model_bwd_gpu.py::_compare (same bar, same zero-gradient floor)."""
    bad, worst = [], ("", 0.0)
    gmax = max(float(g.abs().max()) for g in g64.values())
    for name, gr in g64.items():
        g_ref = gr.numpy()
        g = grads[name].astype(np.float64)
        scale = max(np.abs(g_ref).max(), 1e-4 * gmax)
        err = np.abs(g - g_ref).max() / scale
        if err > worst[1]:
            worst = (name, float(err))
        if not np.isfinite(err) or err > tol:
            bad.append((name, float(err), float(scale)))
    return bad, worst


def _widened(hp):
    names = []
    if hp.speaker_embedding_projection_out_dim > -1:
        names += ["speaker_embedding_projection/kernel", "speaker_embedding_projection/bias"]
    if hp.speaker_embedd_to_decoder:
        names += ["decoder/attention1/memory_layer/kernel", "decoder/attention2/memory_layer/kernel",
                  "decoder/attention_lstm/kernel", "decoder/lstm1/kernel"]
    return names


@pytest.mark.parametrize("key,agent,train", CASES, ids=IDS)
def test_all_parameter_gradients_match_autograd(cuda, key, agent, train):
    hp, grads, g64, _, _ = _case(key, agent, train)
    assert set(grads) == set(g64)
    bad, worst = _compare(grads, g64)
    print(f"worst gradient {worst}")
    assert not bad, bad
    if key is not None:
        for n in ["speaker_embedding"] + _widened(hp):
            assert float(g64[n].abs().max()) > 0 and np.abs(grads[n]).max() > 0, n
    if key is not None and hp.speaker_embedd_to_decoder:
        # the speaker rows themselves (TF row order [c1 | s | ..]) carry gradient
        S = hp.speaker_embedding_projection_out_dim if key == "all" else SR.SPK_DIM
        g = grads["decoder/attention1/memory_layer/kernel"][256:256 + S]
        assert np.abs(g).max() > 0
        if agent:
            g = grads["decoder/attention1/transition_factor_projection/kernel"][256:256 + S]
            assert np.abs(g).max() > 0


def test_persistent_path_stays_eligible_and_matches(cuda):
    """speaker_embedd_to_decoder reaches the persistent kernels only through hoisted terms, so
    the one-launch decoder keeps taking it (no fall-back warning) and meets the same bars."""
    from sat_amd import decoder, params
    hp, grads, g64, got, ref = _case("all", False, True, True)
    assert decoder.persistent_ineligible_reason(params.resolve_dims(hp), SR.B, SR.N) is None
    err = (got["mel"] - ref["mel"]).abs()
    assert float(err.mean()) < 1e-5 and float(err.max()) < 2e-4
    assert abs(got["loss"] - float(ref["loss"])) < 1e-5
    bad, worst = _compare(grads, g64)
    print(f"worst gradient {worst}")
    assert not bad, bad


# ------------------------------------------------------------------ 3. PREDICT
def test_predict_with_a_fixed_speaker_equals_predict_with_those_ids(cuda):
    from sat_amd import models as M
    x = SR.FIXED_SPEAKER
    over = dict(max_iters=12, speaker_embedd_to_decoder=True,
                speaker_embedding_projection_out_dim=SR.PROJ)
    hp_ids = SR.make_hparams(None, **over)
    hp_fix = SR.make_hparams(None, speaker_for_synthesis=x, **over)
    feats, _ = next(iter(M.synthetic_input_fn(hp_ids, 3, N=14, T=20, shape="ljs", seed=2)()))
    assert not np.all(np.asarray(feats.speaker_id) == x)
    same = feats._replace(speaker_id=np.full_like(np.asarray(feats.speaker_id), x))
    preds = []
    for hp, f in ((hp_ids, same), (hp_fix, feats)):
        model = M.tacotron_model_factory(hp, None, None, device=cuda, seed=3)
        preds.append(model.model_fn(f, None, M.ModeKeys.PREDICT, hp).predictions)
    torch.cuda.synchronize()
    for k in ("mel", "stop_token", "alignment", "alignment2"):
        assert torch.equal(preds[0][k], preds[1][k]), k
    assert bool(torch.isfinite(preds[0]["mel"]).all())
    # and the ids matter: the batch's own speakers give another output
    model = M.tacotron_model_factory(hp_ids, None, None, device=cuda, seed=3)
    other = model.model_fn(feats, None, M.ModeKeys.PREDICT, hp_ids).predictions
    assert other["mel"].shape != preds[0]["mel"].shape or not torch.equal(other["mel"], preds[0]["mel"])
    with pytest.raises(ValueError, match="225..376"):
        M.tacotron_model_factory(SR.make_hparams(None, speaker_for_synthesis=3), None, None,
                                 device=cuda)


def test_teacher_forced_incremental_equals_training(cuda):
    """The per-step decoder (wide attention-RNN rows filled by sat_ctx_tail_fill, per-utterance
    LSTM1 / agent rows) fed the teacher frames reproduces the training forward, at the tolerances
    of tests/test_inference_gpu.py::test_teacher_forced_incremental_equals_training."""
    from sat_amd import engine
    from sat_amd.inference import FreeRunningDecoder
    hp = SR.make_hparams("all", agent=True)
    m = engine.Tacotron(hp, cuda, init_values=SR.make_values(hp), persistent_decoder=False)
    gb = {k: torch.tensor(v).to(cuda) for k, v in SR.make_batch(hp).items()}
    with torch.no_grad():
        tr, _ = m.forward(gb, None, training=False, need_grad=False)
    dec = FreeRunningDecoder(m, helper="validation", feed="target")
    inc = dec.run(gb)
    assert dec.last_path != "persistent"
    d_mel = (tr["mel"] - inc["mel"]).abs()
    d_stop = (tr["stop"].view_as(inc["stop"]) - inc["stop"]).abs()
    print(f"mel max {float(d_mel.max()):.3e} mean {float(d_mel.mean()):.3e} "
          f"stop max {float(d_stop.max()):.3e}")
    assert float(d_mel.max()) <= 5e-5 and float(d_mel.mean()) <= 2e-6
    assert float(d_stop.max()) <= 5e-5
    for k in ("alignment1", "alignment2"):
        assert float((tr[k].permute(1, 2, 0) - inc[k]).abs().max()) <= 2e-5, k
    # the one-launch decode declares these configurations ineligible
    hp2 = SR.make_hparams("to_decoder_only", outputs_per_step=2)
    d2 = FreeRunningDecoder(engine.Tacotron(hp2, cuda, persistent_decoder=False))
    assert "speaker_embedd_to_decoder" in d2._why_not(1, 20, 50)


# ------------------------------------------------------------------ 4. checkpoints
def test_checkpoint_resumes_bitwise_and_refuses_a_narrow_warm_start(cuda, tmp_path):
    from sat_amd import checkpoint as C
    from sat_amd import hparams, models
    wide = hparams.vctk_hparams(max_iters=12, speaker_embedd_to_decoder=True)
    narrow = hparams.vctk_hparams(max_iters=12)
    it = models.synthetic_input_fn(wide, 2, N=13, T=16, shape="ljs", seed=20)()
    bs = [next(it) for _ in range(2)]
    assert bs[0][0].source.shape == bs[1][0].source.shape

    def state(m):
        t = m._trainer
        torch.cuda.synchronize()
        return {"params": m.engine.params.cpu(), "exp_avg": t.exp_avg.cpu(),
                "exp_avg_sq": t.exp_avg_sq.cpu(), "bn": m.engine.bn.buf.cpu(),
                "global_step": t.global_step.cpu(), "seed": t.seed.cpu()}
    a = models.DualSourceSelfAttentionTacotronModel(wide, device=cuda)
    a.train(lambda: iter(bs), 2)
    b = models.DualSourceSelfAttentionTacotronModel(wide, device=cuda)
    b.train(lambda: iter(bs[:1]), 1)
    path = b._trainer.save(str(tmp_path / "model.ckpt-1.npz"))
    c = models.DualSourceSelfAttentionTacotronModel(wide, device=cuda, seed=77)
    c.restore(path)
    c.train(lambda: iter(bs[1:]), 1)
    sa, sc = state(a), state(c)
    assert [k for k in sa if not torch.equal(sa[k], sc[k])] == []
    assert int(sa["global_step"]) == 2
    # the file holds the TF shapes; a checkpoint with the narrower kernels is refused whole
    n = models.DualSourceSelfAttentionTacotronModel(narrow, device=cuda)
    n.train(lambda: iter(bs[:1]), 1)
    (tmp_path / "narrow").mkdir()
    npath = n._trainer.save(str(tmp_path / "narrow" / "model.ckpt-1.npz"))
    with pytest.raises(C.CheckpointError, match="has shape"):
        models.DualSourceSelfAttentionTacotronModel(wide, device=cuda, warm_start_from=npath)
    w = models.DualSourceSelfAttentionTacotronModel(wide, device=cuda, seed=5)
    before = w.engine.params.clone()
    with pytest.raises(C.CheckpointError):
        w.restore(npath)
    assert torch.equal(before, w.engine.params)
