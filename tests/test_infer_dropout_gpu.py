"""apply_dropout_on_inference on the GPU: the per-step launch path and the one-launch decode
(sat_decode_persistent with its dropout option) against the float64 restatement of the oracle's
free-running loop with explicit prenet masks (infer_dropout_ref.py), against each other, and
through model_fn.

Bounds.  The comparisons keep the bars they carry today with the switch off: 2e-4 (mel, stop) and
2e-5 (alignments) against the float64 oracle (test_inference_gpu.py), 2e-5 and 2e-6 between the
two paths (test_decode_persistent_gpu.py).  They hold under the switch, so none is replaced.  To
show how much room they leave, the reference is also evaluated in float32 on the CPU; its
distance to the float64 result, ``e32``, is the scale of one float32 evaluation of that decode,
and every test prints its distance as a multiple of e32 before it asserts (the figures are in
DESIGN.md section 5a-2; 8 x e32, the multiple the resample tests use, would be the replacement
had a bar not held).  Every comparison also asserts, from the reference alone, that taking the
masks away moves the mel frames and stop logits by more than their bar: a wrong mask element
cannot hide under it.  (The alignments barely see the masks with fresh weights; they are bounded
all the same.)
The masks are re-drawn here with K.rng_fill from the documented seed and stream ids
(inference.DROP_STREAM0 + layer), never taken from the decoder.  Measured ratios: DESIGN.md
section 5a-2."""
import functools

import numpy as np
import pytest
import torch

import infer_dropout_ref as R

pytestmark = pytest.mark.gpu

SEED = 7
KEYS = ("mel", "stop", "alignment1", "alignment2")
BARS_ORACLE = {"mel": 2e-4, "stop": 2e-4, "alignment1": 2e-5, "alignment2": 2e-5}
BARS_PATHS = {"mel": 2e-5, "stop": 2e-5, "alignment1": 2e-6, "alignment2": 2e-6}


def _hp(preset, drop=True):
    from sat_amd import hparams
    hp = getattr(hparams, f"{preset}_hparams")()
    if drop:
        hp.set_hparam("apply_dropout_on_inference", True)
    return hp


@functools.lru_cache(maxsize=None)
def _case(preset, B, N, T=20, stop_bias=None, bseed=2):
    """Host side of a case: hparams (switch on), fresh weights, a synthetic batch."""
    from sat_amd import data, params
    hp = _hp(preset)
    vals = params.init_params(hp, seed=5)
    if stop_bias is not None:
        vals["decoder/stop_token_projection/bias"] = np.full((1,), stop_bias, np.float32)
    b = data.synthetic_batch(hp, B, N=N, T=T, shape="ljs", seed=bseed)
    return hp, vals, b


def _model(cuda, case, drop=True, hp=None):
    from sat_amd import engine
    hp0, vals, b = case
    if hp is None:
        hp = hp0 if drop else hp0.copy()
        if not drop:
            hp.set_hparam("apply_dropout_on_inference", False)
    m = engine.Tacotron(hp, cuda, init_values=vals)
    gb = {k: torch.tensor(v).to(cuda) for k, v in b.items()}
    return m, gb


def _redraw(cuda, d, Tm, B, seed, keep=0.5):
    """The masks of a (T', B) decode re-drawn with K.rng_fill: seed, DROP_STREAM0 + layer."""
    from sat_amd import kernels as K
    from sat_amd.inference import DROP_STREAM0, drop_on_value, prenet_drops
    sd = torch.tensor([seed], dtype=torch.int64, device=cuda)
    out = []
    for i, drops in enumerate(prenet_drops(d)):
        if not drops:
            out.append(None)
            continue
        t = torch.empty(Tm, B, d.dec_prenet[i], device=cuda)
        K.rng_fill(t, sd, DROP_STREAM0 + i, keep, drop_on_value(keep))
        out.append(t.cpu())
    return out


_REFS = {}


def _refs(key, case, masks, **kw):
    """(float64 reference, e32 per output, float64 reference without masks), computed once."""
    if key not in _REFS:
        from oracle import sat_oracle as O
        from sat_amd import params
        hp, vals, b = case
        p, bufs, tb = O.to_torch(vals), O.to_torch(params.init_bn_buffers(hp)), O.to_torch(b)
        with torch.no_grad():
            r64 = R.infer_free_running_masked(p, bufs, hp, tb, masks, **kw)
            r32 = R.infer_free_running_masked(R.as32(p), R.as32(bufs), hp, R.as32(tb), masks, **kw)
            off = R.infer_free_running_masked(p, bufs, hp, tb, (None, None), **kw)
        assert r64["steps"] == r32["steps"] == off["steps"]
        e32 = {k: float((r32[k].double() - r64[k]).abs().max()) for k in KEYS}
        _REFS[key] = (r64, e32, off)
    return _REFS[key]


def _gpu(out, k):
    x = out[k].double().cpu()
    return x.permute(0, 2, 1) if k.startswith("alignment") else x      # [B, N, T'] -> [B, T', N]


def _check_vs_ref(name, out, r64, e32, off, bars=BARS_ORACLE):
    bad = []
    for k in KEYS:
        dist = float((_gpu(out, k) - r64[k]).abs().max())
        bound = bars[k]
        moved = float((off[k] - r64[k]).abs().max())
        print(f"{name} {k}: gpu-ref {dist:.3e} e32 {e32[k]:.3e} ratio {dist / e32[k]:.2f} "
              f"bound {bound:.3e} masks move the reference by {moved:.3e}")
        if k in ("mel", "stop"):
            assert moved > bound, (k, moved, bound)    # the bar can tell the masks are there
        if not dist <= bound:
            bad.append((k, dist, bound))
    assert not bad, bad


@pytest.mark.parametrize("preset,mode", [("ljspeech", "mel"), ("ljspeech", "softmax"),
                                         ("vctk", "mel")])
def test_launch_path_matches_reference(cuda, preset, mode):
    """Per-step launches, (B, N) = (3, 15), 40 steps: mel feedback under the stop-token helper
    (min_iters = max_iters) and softmax feedback under the validation helper; the VCTK preset
    (speaker_embedd_to_prenet) decodes with layer 0 clean."""
    from sat_amd.inference import FreeRunningDecoder
    T = 40
    case = _case(preset, 3, 15, T=80 if mode == "softmax" else 20)
    m, gb = _model(cuda, case)
    if mode == "softmax":
        kw, rkw = dict(helper="validation", feed="softmax"), dict(helper="validation",
                                                                  feed="softmax")
    else:
        kw, rkw = dict(max_iters=T, min_iters=T), dict(max_iters=T, min_iters=T)
    out = FreeRunningDecoder(m, persistent=False, seed=SEED, **kw).run(gb)
    assert out["steps"] == T
    masks = _redraw(cuda, m.d, T, 3, SEED)
    assert (masks[0] is None) == (preset == "vctk") and masks[1] is not None
    r64, e32, off = _refs((preset, mode), case, masks, **rkw)
    _check_vs_ref(f"launch[{preset},{mode}]", out, r64, e32, off)
    if preset == "vctk":
        # a mask on layer 0 as well would sit outside the bound: layer 0 ran clean
        from oracle import sat_oracle as O
        from sat_amd import params
        from sat_amd.inference import DROP_STREAM0
        hp, vals, b = case
        m0 = torch.tensor(R.host_masks(_model_dims(_hp("ljspeech")), T, 3, SEED, 0.5,
                                       DROP_STREAM0)[0])
        with torch.no_grad():
            both = R.infer_free_running_masked(
                O.to_torch(vals), O.to_torch(params.init_bn_buffers(hp)), hp, O.to_torch(b),
                (m0, masks[1]), **rkw)
        far = float((both["mel"] - r64["mel"]).abs().max())
        assert far > BARS_ORACLE["mel"], far


def _model_dims(hp):
    from sat_amd import params
    return params.resolve_dims(hp)


@pytest.mark.parametrize("B,N,T", [(1, 7, 40), (3, 15, 40), (8, 200, 40), (3, 15, 130)])
def test_one_launch_matches_launch_path(cuda, B, N, T):
    """The in-kernel draw equals sat_rng_fill's: same seed, the one-launch decode against the
    per-step launches.  T' = 130 takes the step parity slots and t B P past small values."""
    from sat_amd.inference import FreeRunningDecoder
    case = _case("ljspeech", B, N)
    m, gb = _model(cuda, case)
    one = FreeRunningDecoder(m, persistent=True, max_iters=T, min_iters=T, seed=SEED)
    ref = FreeRunningDecoder(m, persistent=False, max_iters=T, min_iters=T, seed=SEED)
    a, r = one.run(gb), ref.run(gb)
    assert one.last_path == "persistent" and ref.last_path == "launches"
    assert a["steps"] == r["steps"] == T
    masks = _redraw(cuda, m.d, T, B, SEED)
    key = ("ljspeech", "mel") if (B, N, T) == (3, 15, 40) else ("ljspeech", "mel", B, N, T)
    r64, e32, off = _refs(key, case, masks, max_iters=T, min_iters=T)
    bad = []
    for k in KEYS:
        dist = float((a[k] - r[k]).abs().max())
        bound = BARS_PATHS[k]
        moved = float((off[k] - r64[k]).abs().max())
        print(f"paths[{B},{N},{T}] {k}: one-launch vs launches {dist:.3e} e32 {e32[k]:.3e} "
              f"ratio {dist / e32[k]:.2f} bound {bound:.3e} masks move the reference {moved:.3e}")
        if k in ("mel", "stop"):
            assert moved > bound, (k, moved, bound)
        if not dist <= bound:
            bad.append((k, dist, bound))
    sa, sr = a["decoder_self_alignments"][0], r["decoder_self_alignments"][0]
    assert float((sa - sr).abs().max()) <= 2e-6
    assert not bad, bad


def test_one_launch_matches_reference(cuda):
    """The one-launch decode against the float64 reference directly, (3, 15), 40 steps."""
    from sat_amd.inference import FreeRunningDecoder
    T = 40
    case = _case("ljspeech", 3, 15)
    m, gb = _model(cuda, case)
    dec = FreeRunningDecoder(m, persistent=True, max_iters=T, min_iters=T, seed=SEED)
    out = dec.run(gb)
    assert dec.last_path == "persistent" and out["steps"] == T
    masks = _redraw(cuda, m.d, T, 3, SEED)
    r64, e32, off = _refs(("ljspeech", "mel"), case, masks, max_iters=T, min_iters=T)
    _check_vs_ref("one-launch[3,15]", out, r64, e32, off)


@pytest.mark.parametrize("persistent", [True, False], ids=["one_launch", "launches"])
def test_determinism_and_seed(cuda, persistent):
    """Same seed on a fresh decoder: bitwise equal.  A second run() on one decoder draws other
    masks (the seed advanced by one on the device) -- those of a fresh decoder seeded one
    higher.  Another seed differs."""
    from sat_amd.inference import FreeRunningDecoder
    case = _case("ljspeech", 3, 15)
    m, gb = _model(cuda, case)
    kw = dict(persistent=persistent, max_iters=24, min_iters=24)
    d1 = FreeRunningDecoder(m, seed=SEED, **kw)
    a = d1.run(gb)
    a2 = d1.run(gb)
    b = FreeRunningDecoder(m, seed=SEED, **kw).run(gb)
    c = FreeRunningDecoder(m, seed=SEED + 1, **kw).run(gb)
    assert int(d1.seed.item()) == SEED + 2
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k
        assert torch.equal(a2[k], c[k]), k
    assert not torch.equal(a["mel"], a2["mel"])
    assert not torch.equal(a["mel"], c["mel"])
    # a shared device word: two decoders draw from one sequence
    word = torch.tensor([SEED], dtype=torch.int64, device=cuda)
    e = FreeRunningDecoder(m, seed=word, **kw).run(gb)
    f = FreeRunningDecoder(m, seed=word, **kw).run(gb)
    assert torch.equal(e["mel"], a["mel"]) and torch.equal(f["mel"], a2["mel"])
    with pytest.raises(ValueError, match="seed tensor"):
        FreeRunningDecoder(m, seed=torch.zeros(1, device=cuda), **kw)


@pytest.mark.parametrize("bias", [8.0, -8.0])
def test_stop_token_same_step_on_both_paths(cuda, bias):
    from sat_amd.inference import FreeRunningDecoder
    case = _case("ljspeech", 3, 9, stop_bias=bias)
    m, gb = _model(cuda, case)
    one = FreeRunningDecoder(m, persistent=True, max_iters=30, min_iters=10, seed=SEED)
    ref = FreeRunningDecoder(m, persistent=False, max_iters=30, min_iters=10, seed=SEED)
    a, r = one.run(gb), ref.run(gb)
    assert one.last_path == "persistent" and ref.last_path == "launches"
    assert a["steps"] == r["steps"] == (12 if bias > 0 else 30)
    assert float((a["mel"] - r["mel"]).abs().max()) <= 2e-5


@pytest.mark.parametrize("persistent", [True, False], ids=["one_launch", "launches"])
def test_switch_off_is_the_parent_decode(cuda, persistent):
    """apply_dropout_on_inference=False, and hparams that never mention the switch, decode
    bitwise alike on both paths (and take no seed)."""
    from sat_amd import hparams
    from sat_amd.inference import FreeRunningDecoder
    case = _case("ljspeech", 3, 15)
    off = hparams.ljspeech_hparams()
    bare = hparams.HParams(**{k: v for k, v in off.values().items()
                              if k != "apply_dropout_on_inference"})
    assert "apply_dropout_on_inference" not in bare
    outs = []
    for hp in (off, bare):
        m, gb = _model(cuda, case, hp=hp)
        dec = FreeRunningDecoder(m, persistent=persistent, max_iters=24, min_iters=24, seed=SEED)
        assert not dec.drop and dec.seed is None
        outs.append(dec.run(gb))
        assert dec.last_path == ("persistent" if persistent else "launches")
    for k in KEYS:
        assert torch.equal(outs[0][k], outs[1][k]), k
    m, gb = _model(cuda, case)
    on = FreeRunningDecoder(m, persistent=persistent, max_iters=24, min_iters=24,
                            seed=SEED).run(gb)
    assert not torch.equal(on["mel"], outs[0]["mel"])


def test_graph_decode_equals_eager_under_the_switch(cuda):
    """graphs=True: the fill launch stays outside the captured chunks, so a replayed decode
    draws what the eager one draws, run after run."""
    from sat_amd.inference import FreeRunningDecoder
    case = _case("ljspeech", 3, 15, T=40)
    m, gb = _model(cuda, case)
    kw = dict(helper="validation", feed="softmax", persistent=False, seed=SEED)
    eager = FreeRunningDecoder(m, **kw)
    graph = FreeRunningDecoder(m, graphs=True, check_every=5, **kw)
    for _ in range(2):
        a, b = eager.run(gb), graph.run(gb)
        for k in KEYS:
            assert torch.equal(a[k], b[k]), k


class _Missing(dict):
    def __missing__(self, k):
        return None


def _records(b):
    from sat_amd.models import (MelData, PreprocessedSourceData, PreprocessedTargetData,
                                SourceData)
    ids = np.arange(b["source"].shape[0])
    if "speaker_id" in b:
        return (SourceData(ids, ids, b["source"], b["source_length"], b["speaker_id"], None, None,
                           None),
                MelData(ids, ids, b["mel"], b["mel"].shape[2], b["target_length"], b["done"],
                        b["mel_mask"], b["done_mask"]))
    return (PreprocessedSourceData(ids, ids, b["source"], b["source_length"], None),
            PreprocessedTargetData(ids, ids, b["mel"], b["target_length"], b["done"],
                                   b["mel_mask"], b["done_mask"]))


@pytest.mark.parametrize("preset", ["ljspeech", "vctk"])
def test_eval_teacher_forced_pass_takes_the_masks(cuda, preset):
    """model_fn EVAL under the switch: the validation decode draws with the model's seed, the
    teacher-forced pass with the seed after it (each draw advances the word once);
    loss_with_teacher equals the float64 teacher-forced forward with those prenet masks
    (everything else eval: zoneout blend, no other dropout, BN moving statistics) within the
    1e-5 bar of test_model_fn_eval_losses_match_oracle, and differs from the switch-off value
    by more than that bar.  (The oracle's MultiSpeakerPreNet wants a layer-0 mask: ones.)"""
    from oracle import sat_oracle as O
    from sat_amd import models as MD, params
    B, N, T = 2, 12, 24
    case = _case(preset, B, N, T=T, bseed=8)
    hp, vals, b = case
    model = MD.DualSourceSelfAttentionTacotronModel(hp, device=cuda, init_values=vals, seed=SEED)
    feats, labels = _records(b)
    spec = model.model_fn(feats, labels, MD.ModeKeys.EVAL, hp)
    mt = spec.eval_metric_ops
    Tp = T // hp.outputs_per_step
    masks = _redraw(cuda, model.engine.d, Tp, B, SEED + 1)
    assert int(model._infer_seed().item()) == SEED + 2
    md = _Missing({f"dec/prenet{i}": m for i, m in enumerate(masks) if m is not None})
    assert (preset == "vctk") == ("dec/prenet0" not in md)
    if preset == "vctk":
        md["dec/prenet0"] = torch.ones(Tp, B, model.engine.d.dec_prenet[0])
    p, bufs, tb = O.to_torch(vals), O.to_torch(params.init_bn_buffers(hp)), O.to_torch(b)
    with torch.no_grad():
        r64 = O.model_forward(p, bufs, hp, tb, _Missing({k: v.double() for k, v in md.items()}),
                              training=False)
        r32 = O.model_forward(R.as32(p), R.as32(bufs), hp, R.as32(tb), md, training=False)
        off = O.model_forward(p, bufs, hp, tb, None, training=False)
    got = {"loss": mt["loss_with_teacher"], "l1": mt["code_loss_with_teacher"] * 10.0,
           "bce": mt["done_loss_with_teacher"]}
    bad = []
    for k in ("loss", "l1", "bce"):
        e32 = abs(float(r32[k]) - float(r64[k]))
        dist = abs(float(got[k].item()) - float(r64[k]))
        moved = abs(float(off[k]) - float(r64[k]))
        # one float32 rounding of the value itself is the floor of e32 (a scalar can land on
        # the float64 value by luck)
        e32 = max(e32, abs(float(r64[k])) * 2.0 ** -24)
        bound = 1e-5 * max(1.0, abs(float(r64[k])))
        print(f"eval[{preset}] {k}: gpu-ref {dist:.3e} e32 {e32:.3e} ratio {dist / e32:.2f} "
              f"bound {bound:.3e} masks move the reference by {moved:.3e}")
        assert moved > bound, (k, moved, bound)
        if not dist <= bound:
            bad.append((k, dist, bound))
    assert not bad, bad
    # the switch-off model's value is the unmasked forward's
    hp_off = hp.copy()
    hp_off.set_hparam("apply_dropout_on_inference", False)
    m_off = MD.DualSourceSelfAttentionTacotronModel(hp_off, device=cuda, init_values=vals,
                                                    seed=SEED)
    v_off = m_off.model_fn(feats, labels, MD.ModeKeys.EVAL, hp_off).eval_metric_ops
    assert m_off._infer_seed_dev is None
    assert float(v_off["code_loss_with_teacher"].item()) != \
        float(mt["code_loss_with_teacher"].item())


def test_evaluate_and_predict_through_model_fn(cuda):
    """evaluate() and predict() run under the switch; the model's seed word is shared: two
    predictions of one batch differ, a model built with the same seed repeats the sequence;
    forced-alignment EVAL runs its masked first pass too."""
    from sat_amd import models as MD
    hp, vals, b = _case("ljspeech", 2, 11, T=16, bseed=4)
    hp = hp.copy()
    hp.set_hparam("max_iters", 12)

    def mk():
        return MD.DualSourceSelfAttentionTacotronModel(hp, device=cuda, init_values=vals,
                                                       seed=SEED)
    fn = MD.synthetic_input_fn(hp, 2, N=11, T=16, shape="ljs", seed=4)

    def two(model):
        it = iter(fn())
        feats, _ = next(it)
        return [model.model_fn(feats, None, MD.ModeKeys.PREDICT, hp).predictions["mel"].clone()
                for _ in range(2)]
    a, b2 = two(mk()), two(mk())
    assert not torch.equal(a[0], a[1])
    assert torch.equal(a[0], b2[0]) and torch.equal(a[1], b2[1])
    first = next(iter(mk().predict(fn)))
    assert torch.equal(first["mel"], a[0])
    ev = mk().evaluate(fn, steps=2)
    assert all(np.isfinite(v) for v in ev.values())
    ev2 = mk().evaluate(fn, steps=2)
    assert ev == ev2
    hp_f = hp.copy()
    hp_f.set_hparam("use_forced_alignment_mode", True)
    mf = MD.DualSourceSelfAttentionTacotronModel(hp_f, device=cuda, init_values=vals, seed=SEED)
    evf = mf.evaluate(fn, steps=1)
    assert np.isfinite(evf["loss"])
    assert int(mf._infer_seed().item()) == SEED + 3      # first pass, forced decode, teacher pass


def test_synthesize_same_seed_same_files(cuda, tmp_path):
    """``synthesize --hparams apply_dropout_on_inference=True --seed 7 --no-wav`` twice: the
    .mfbsp files are identical (an empty checkpoint directory: the weights are the seed's too)."""
    import json
    import os
    from sat_amd import hparams, preprocess, synthesize as S
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "codes")
    C = 16
    hp = hparams.codes_hparams(C, source="char", phoneme="none", max_iters=24)
    rec = tmp_path / "records"
    keys = preprocess.Codes(golden, str(rec), hp, C, compact=True).run()[:2]
    (tmp_path / "list").mkdir()
    (tmp_path / "list" / "test.csv").write_text("\n".join(keys) + "\n")
    (tmp_path / "ckpt").mkdir()
    (tmp_path / "hp.json").write_text(json.dumps(hp.values()))

    def run(out, seed):
        rc = S.main(["--source-data-root", str(rec), "--target-data-root", str(rec),
                     "--checkpoint-dir", str(tmp_path / "ckpt"), "--selected-list-dir",
                     str(tmp_path / "list"), "--output-dir", str(tmp_path / out),
                     "--hparam-json-file", str(tmp_path / "hp.json"), "--hparams",
                     "apply_dropout_on_inference=True", "--seed", str(seed), "--no-wav"])
        assert rc == 0
        return [(tmp_path / out / f"{k}.mfbsp").read_bytes() for k in keys]
    a, b = run("a", 7), run("b", 7)
    assert a == b and all(len(x) > 0 for x in a)
