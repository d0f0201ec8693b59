"""ForwardAttention's transition agent and cumulative weights on the GPU (per-step launch path)
against the fp64 restatement of tests/transition_agent_ref.py: the plugin-level step, the
teacher-forced model and every parameter gradient, the incremental decoder, model_fn."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import transition_agent_ref as R

pytestmark = pytest.mark.gpu

A1 = "decoder/attention1"


# ------------------------------------------------------------------ 1. step level, plugin surface
@pytest.mark.parametrize("key", sorted(R.FLAGS))
def test_mechanism_steps_match_restatement(cuda, key):
    """B=3, N=45 (two position tiles, the second partial), one utterance inside the first tile;
    alpha_t, the state and u_t of 6 chained steps within 2e-5 of the fp64 restatement."""
    from sat_amd import attentions as A
    from oracle import sat_oracle as O
    agent, cum = key in ("agent", "both"), key in ("cumulative", "both")
    B, N, M, Q, units = 3, 45, 64, 48, 224
    g = torch.Generator().manual_seed(3)
    memory = torch.randn(B, N, M, generator=g)
    lengths = torch.tensor([45, 33, 7])
    fn = A.attention_mechanism_factory(A.AttentionOptions("forward", units, 10, 5, False, cum,
                                                          agent))
    mech = fn(memory.to(cuda), lengths.to(cuda), query_depth=Q, seed=9)
    assert (f"{R.TF}/kernel" in mech.variables) == agent
    if agent:
        assert tuple(mech.variables[f"{R.TF}/kernel"].shape) == (M + units, 1)
        mech.variables[f"{R.TF}/kernel"].mul_(R.AGENT_SCALE)
    p = {f"m/{k}": v.detach().cpu().double() for k, v in mech.variables.items()}
    ref = R.agent_oracle_class(O, agent, cum)(p, "m", memory.double(), lengths)
    state = mech.initial_state(B)
    rstate = ref.initial_state(B, N, torch.float64)
    us = []
    for step in range(6):
        query = torch.randn(B, Q, generator=g)
        a, state = mech(query.to(cuda), state)
        ra, rstate = ref(query.double(), rstate)
        torch.cuda.synchronize()
        for name, x, y in (("alpha", a, ra), ("state", state[0], rstate[0]),
                           ("u", state[2], rstate[2])):
            err = float((x.cpu().double() - y).abs().max())
            print(f"{key} step {step} {name}: max abs err {err:.3e}")
            assert tuple(x.shape) == tuple(y.shape)
            assert err <= 2e-5, (key, step, name, err)
        assert torch.all(a[1, 33:] == 0) and torch.all(a[2, 7:] == 0)   # masked memory
        us.append(state[2].cpu())
    if agent:
        assert float(torch.stack(us).max() - torch.stack(us).min()) > 0.05
    else:
        assert all(torch.all(u == 0.5) for u in us)


# ------------------------------------------------------------------ 2. agent at rest == stock path
def test_agent_at_rest_equals_stock_per_step_forward(cuda):
    """w = 0, b_u = 0 give u_t = sigmoid(0) = 0.5 exactly, so the teacher-forced forward with the
    agent on must equal the stock per-step forward bit for bit."""
    from sat_amd import data, engine, hparams, params
    hp0 = hparams.ljspeech_hparams()
    hp1 = hparams.ljspeech_hparams(**R.FLAGS["agent"])
    vals0 = params.init_params(hp0, seed=5)
    vals1 = dict(vals0)
    d = params.resolve_dims(hp1)
    vals1[f"{A1}/{R.TF}/kernel"] = np.zeros((d.m1 + d.d1, 1), np.float32)
    vals1[f"{A1}/{R.TF}/bias"] = np.zeros((1,), np.float32)
    batch = data.synthetic_batch(hp0, 3, N=45, T=24, shape="ljs", seed=0)
    gb = {k: torch.tensor(v).to(cuda) for k, v in batch.items()}
    outs = []
    for hp, vals in ((hp0, vals0), (hp1, vals1)):
        m = engine.Tacotron(hp, cuda, init_values=vals, persistent_decoder=False)
        with torch.no_grad():
            out, _ = m.forward(gb, None, training=False, need_grad=False)
        torch.cuda.synchronize()
        outs.append({k: out[k].clone() for k in ("mel", "stop", "alignment1", "alignment2")})
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k


# ------------------------------------------------------------------ 3. all parameter gradients
def _run(cuda, monkeypatch, key, train, B=3, N=45, T=24, seed=R.FIXTURE_SEED):
    from sat_amd import data, engine, hparams, params
    from oracle import sat_oracle as O
    hp = hparams.ljspeech_hparams(**R.FLAGS[key])
    vals = R.fixture_values(hp)
    m = engine.Tacotron(hp, cuda, init_values=vals, persistent_decoder=False)
    batch = data.synthetic_batch(hp, B, N=N, T=T, shape="ljs", seed=seed)
    Np, Tp = batch["source"].shape[1], batch["mel"].shape[1] // hp.outputs_per_step
    masks = data.synthetic_masks(hp, B, Np, Tp, seed=seed + 9) if train else None
    gb = {k: torch.tensor(v).to(cuda) for k, v in batch.items()}
    gm = None if masks is None else {k: torch.tensor(v).to(cuda) for k, v in masks.items()}
    out, sv = m.forward(gb, gm, training=train)
    m.backward(sv)
    torch.cuda.synchronize()
    grads = m.grads_dict()
    R.patch_oracle(monkeypatch, O, key in ("agent", "both"), key in ("cumulative", "both"))
    p64 = {k: v.requires_grad_(True) for k, v in O.to_torch(vals).items()}
    bufs = O.to_torch(params.init_bn_buffers(hp))
    ref = O.model_forward(p64, bufs, hp, O.to_torch(batch),
                          None if masks is None else O.to_torch(masks), training=train)
    ref["loss"].backward()
    return grads, p64, out, ref


def _compare(grads, p64, tol=2e-4):
    """tests/test_model_bwd_gpu.py::_compare (same bar, same zero-gradient floor)."""
    bad, worst = [], ("", 0.0)
    gmax = max(float(p.grad.abs().max()) for p in p64.values())
    for name, p in p64.items():
        g_ref = p.grad.numpy()
        g = grads[name].astype(np.float64)
        scale = max(np.abs(g_ref).max(), 1e-4 * gmax)
        err = np.abs(g - g_ref).max() / scale
        if err > worst[1]:
            worst = (name, float(err))
        if not np.isfinite(err) or err > tol:
            bad.append((name, float(err), float(scale)))
    return bad, worst


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("key", sorted(R.FLAGS))
def test_all_parameter_gradients_match_restatement(cuda, monkeypatch, key, train):
    grads, p64, out, ref = _run(cuda, monkeypatch, key, train)
    dl = abs(float(out["loss"].item()) - float(ref["loss"].detach()))
    bad, worst = _compare(grads, p64)
    print(f"{key} train={train}: loss diff {dl:.3e}, worst gradient {worst}")
    assert dl < 1e-5
    assert not bad, bad
    if key != "cumulative":
        for n in (f"{A1}/{R.TF}/kernel", f"{A1}/{R.TF}/bias"):
            assert np.abs(grads[n]).max() > 0 and float(p64[n].grad.abs().max()) > 0, n


# ------------------------------------------------------------------ 4. training == incremental
def test_teacher_forced_incremental_equals_training(cuda):
    """tests/test_inference_gpu.py::test_teacher_forced_incremental_equals_training with both
    flags on: the per-step free-running decoder fed the teacher frames reproduces the training
    forward (same tolerances; the alignments at the 2e-5 of the decode tests)."""
    from sat_amd import data, engine, hparams
    from sat_amd.inference import FreeRunningDecoder
    hp = hparams.ljspeech_hparams(**R.FLAGS["both"])
    B, N, T = 3, 15, 40
    m = engine.Tacotron(hp, cuda, init_values=R.fixture_values(hp), persistent_decoder=False)
    b = data.synthetic_batch(hp, B, N=N, T=T, shape="ljs", seed=9)
    gb = {k: torch.tensor(v).to(cuda) for k, v in b.items()}
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
    for k, h in (("alignment1", tr["alignment1"]), ("alignment2", tr["alignment2"])):
        got = inc[k]                                         # [B, N, T'] beside [T', B, N]
        assert float((h.permute(1, 2, 0) - got).abs().max()) <= 2e-5, k


# ------------------------------------------------------------------ 5. surface
def test_model_fn_train_and_predict_with_both_flags(cuda):
    from sat_amd import decoder, hparams, models as M
    hp = hparams.ljspeech_hparams(**R.FLAGS["both"])
    hp.set_hparam("max_iters", 12)
    model = M.tacotron_model_factory(hp, None, None, device=cuda, seed=3)
    feats, labels = next(iter(M.synthetic_input_fn(hp, 3, N=14, T=20, shape="ljs", seed=2)()))
    decoder._FALLBACK_WARNED.clear()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        losses = [float(model.model_fn(feats, labels, M.ModeKeys.TRAIN, hp).loss.item())
                  for _ in range(2)]
        spec = model.model_fn(feats, None, M.ModeKeys.PREDICT, hp)
    assert all(np.isfinite(x) for x in losses)
    assert bool(torch.isfinite(spec.predictions["mel"]).all())
    fb = [w for w in rec if issubclass(w.category, decoder.PersistentFallbackWarning)]
    assert len(fb) == 1, [str(w.message) for w in fb]
    assert "use_forward_attention_transition_agent" in str(fb[0].message)
    names = [p.name for p in model.engine.layout.specs]
    assert f"{A1}/{R.TF}/kernel" in names and f"{A1}/{R.TF}/bias" in names


def test_step_entry_refuses_an_agent_request_without_the_projection(cuda):
    from sat_amd import _lib
    from sat_amd import kernels as K
    B, N, D1, M1, D2, M2 = 2, 9, 32, 8, 32, 4
    f32 = dict(device=cuda, dtype=torch.float32)
    z = lambda *s: torch.zeros(*s, **f32)   # noqa: E731
    pst = K.part_stride(M1, M2)
    kw = dict(B=B, N=N, D1=D1, M1=M1, D2=D2, M2=M2, F=5, KW=10, NT=32, ntiles=1, att1_forward=1,
              u=0.5, q=z(B, D1 + D2), q_sb=D1 + D2, K1=z(B, N, D1), V1=z(B, N, M1),
              K2=z(B, N, D2), V2=z(B, N, M2),
              lengths=torch.full((B,), N, dtype=torch.int64, device=cuda), s_prev=z(B, N),
              a_prev=z(B, N), v1=z(D1), b1=z(D1), convW=z(10, 1, 5), convb=z(5), locW=z(5, D1),
              v2=z(D2), e1=z(B, N), e2=z(B, N), part=z(B, 1, pst), part_stride=pst,
              s_out=z(B, N), a_out=z(B, N), s2_out=z(B, N), ctx=z(B, M1 + M2), ctx_sb=M1 + M2,
              u_prev=torch.full((B,), 0.5, **f32), u_out=z(B))
    with pytest.raises(_lib.SatLibraryError) as e:
        K.attn_step_fwd(**kw, agent_w=None, agent_b=z(1))
    assert e.value.rc == _lib.SAT_ERR_ARGUMENT and "agent_w" in str(e.value)
    K.attn_step_fwd(**kw, agent_w=z(M1 + D1), agent_b=z(1))      # complete request: accepted
    torch.cuda.synchronize()
    assert torch.all(kw["u_out"] == 0.5)
    a = _lib.SatAttnAgentBwd()                                    # all-zero sizes: refused
    assert _lib.load().sat_attn_agent_bwd(ctypes.byref(a), None) == _lib.SAT_ERR_ARGUMENT
