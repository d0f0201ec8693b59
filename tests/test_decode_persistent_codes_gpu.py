"""The one-launch free-running decode of the VQ-code models (num_mels = num_codes, r = 1; any
output width): sat_decode_persistent with its history option, with and without the speaker and
dropout options (decode_persistent_kernel<kDrop, kSpk, true>), and the projection of the z
history after the launch, against the per-step launch path of the same FreeRunningDecoder,
against the float64 oracle, and through model_fn.

Bars: the ones the mel files carry, not new ones -- between the two paths mel / stop 2e-5 and
alignments / decoder self-alignment rows 2e-6 (test_decode_persistent_gpu.py,
test_decode_persistent_spk_gpu.py), against the float64 oracle 2e-4 and 2e-5.  Weights: the codes
preset from params.init_params(hp, seed=5); the speaker ids of a multi-speaker batch differ."""
import functools

import numpy as np
import pytest
import torch

import infer_dropout_ref as R

pytestmark = pytest.mark.gpu

SEED = 7
KEYS = ("mel", "stop", "alignment1", "alignment2")
BARS_PATHS = {"mel": 2e-5, "stop": 2e-5, "alignment1": 2e-6, "alignment2": 2e-6}
BARS_ORACLE = {"mel": 2e-4, "stop": 2e-4, "alignment1": 2e-5, "alignment2": 2e-5}


def _hp(C, multi=False, drop=False, **over):
    from sat_amd import hparams
    hp = hparams.codes_hparams(C, **dict(dict(source="char", phoneme="none",
                                              use_speaker_embedding=multi), **over))
    if drop:
        hp.set_hparam("apply_dropout_on_inference", True)
    return hp


@functools.lru_cache(maxsize=None)
def _case(B, N, C, multi=False, drop=False, stop_bias=None):
    """Host side of a case: hparams, fresh weights, a synthetic batch (multi-speaker: B distinct
    speakers of the preset's num_speakers / speaker_embedding_offset)."""
    from sat_amd import data, params
    hp = _hp(C, multi, drop)
    vals = params.init_params(hp, seed=5)
    if stop_bias is not None:
        vals["decoder/stop_token_projection/bias"] = np.full((1,), stop_bias, np.float32)
    b = data.synthetic_batch(hp, B, N=N, T=20, shape="ljs", seed=2)
    if multi:
        off = hp.speaker_embedding_offset
        assert (hp.num_speakers, off) == (152, 225)
        b["speaker_id"] = np.asarray([off + (37 * g) % hp.num_speakers for g in range(B)],
                                     b["speaker_id"].dtype)
        assert len(set(b["speaker_id"].tolist())) == B
    return hp, vals, b


def _model(cuda, case):
    from sat_amd import engine
    hp, vals, b = case
    m = engine.Tacotron(hp, cuda, init_values=vals)
    gb = {k: torch.tensor(v).to(cuda) for k, v in b.items()}
    return m, gb


def _both(m, gb, **kw):
    from sat_amd.inference import FreeRunningDecoder
    one = FreeRunningDecoder(m, persistent=True, **kw)
    ref = FreeRunningDecoder(m, persistent=False, **kw)
    a = one.run(gb)
    assert one.last_path == "persistent"
    r = ref.run(gb)
    assert ref.last_path == "launches"
    return a, r


def _check_paths(name, a, r, T):
    assert a["steps"] == r["steps"] == T
    assert a["mel"].shape == r["mel"].shape
    bad = []
    for k in KEYS:
        dist = float((a[k] - r[k]).abs().max())
        print(f"{name} {k}: one-launch vs launches {dist:.3e} bound {BARS_PATHS[k]:.1e}")
        if not dist <= BARS_PATHS[k]:
            bad.append((k, dist))
    sa, sr = a["decoder_self_alignments"][0], r["decoder_self_alignments"][0]
    dist = float((sa - sr).abs().max())
    print(f"{name} decoder self-alignments: {dist:.3e} bound 2.0e-06")
    if not dist <= 2e-6:
        bad.append(("decoder_self_alignments", dist))
    assert not bad, bad


def _gpu(out, k):
    x = out[k].double().cpu()
    return x.permute(0, 2, 1) if k.startswith("alignment") else x      # [B, N, T'] -> [B, T', N]


def _check_oracle(name, out, ref):
    assert out["steps"] == ref["steps"]
    bad = []
    for k in KEYS:
        dist = float((_gpu(out, k) - ref[k]).abs().max())
        print(f"{name} {k}: gpu-oracle {dist:.3e} bound {BARS_ORACLE[k]:.1e}")
        if not dist <= BARS_ORACLE[k]:
            bad.append((k, dist))
    dist = float((out["decoder_self_alignments"][0].double().cpu()
                  - ref["decoder_self_alignments"][0]).abs().max())
    print(f"{name} decoder self-alignments: gpu-oracle {dist:.3e} bound 2.0e-05")
    if not dist <= 2e-5:
        bad.append(("decoder_self_alignments", dist))
    assert not bad, bad


def _oracle(case, masks=(None, None), **kw):
    from oracle import sat_oracle as O
    from sat_amd import params
    hp, vals, b = case
    with torch.no_grad():
        return R.infer_free_running_masked(O.to_torch(vals),
                                           O.to_torch(params.init_bn_buffers(hp)), hp,
                                           O.to_torch(b), masks, **kw)


# ------------------------------------------------------------------ 1. against the launch path
@pytest.mark.parametrize("B,N,C", [(1, 7, 13), (3, 15, 256), (8, 200, 1025)])
def test_one_launch_matches_launch_path(cuda, B, N, C):
    """One group, one attention workgroup and an odd width; ragged lengths in a partly filled
    grid; all eight groups, N not a multiple of 32 and the reference's own 1025 columns.  40
    steps: the cache rows and the z-history writers wrap over the 32 workgroups."""
    m, gb = _model(cuda, _case(B, N, C))
    assert (m.d.num_mels, m.d.r, m.d.multi_speaker) == (C, 1, False)
    T = 40
    a, r = _both(m, gb, max_iters=T, min_iters=T)
    assert tuple(a["mel"].shape) == (B, T, C)
    _check_paths(f"paths[{B},{N},{C}]", a, r, T)


# ------------------------------------------------------------------ 2. the multi-speaker model
def test_multi_speaker_matches_launch_path_and_oracle(cuda):
    case = _case(3, 15, 256, multi=True)
    m, gb = _model(cuda, case)
    assert m.d.multi_speaker and m.d.num_mels == 256
    T = 40
    a, r = _both(m, gb, max_iters=T, min_iters=T)
    _check_paths("spk paths[3,15,256]", a, r, T)
    _check_oracle("spk oracle[3,15,256]", a, _oracle(case, max_iters=T, min_iters=T))


def test_single_speaker_matches_oracle(cuda):
    case = _case(3, 15, 256)
    m, gb = _model(cuda, case)
    from sat_amd.inference import FreeRunningDecoder
    T = 40
    dec = FreeRunningDecoder(m, persistent=True, max_iters=T, min_iters=T)
    out = dec.run(gb)
    assert dec.last_path == "persistent"
    _check_oracle("oracle[3,15,256]", out, _oracle(case, max_iters=T, min_iters=T))


# ------------------------------------------------------------------ 3. dropout kept on
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


@pytest.mark.parametrize("multi", [False, True], ids=["single", "multi"])
def test_dropout_same_seed_same_masks_on_both_paths(cuda, multi):
    """apply_dropout_on_inference: the same seed on both paths gives the same masks (the paths
    agree within the bars, and lie outside them from the switch-off decode); two one-launch runs
    from one seed are bit-identical; the float64 loop fed the re-drawn masks is met."""
    from sat_amd.inference import FreeRunningDecoder
    case = _case(3, 15, 256, multi=multi, drop=True)
    m, gb = _model(cuda, case)
    assert m.d.multi_speaker == multi
    T = 40
    a, r = _both(m, gb, max_iters=T, min_iters=T, seed=SEED)
    _check_paths(f"dropout paths[multi={multi}]", a, r, T)
    again = FreeRunningDecoder(m, persistent=True, max_iters=T, min_iters=T, seed=SEED).run(gb)
    for k in KEYS:
        assert torch.equal(a[k], again[k]), k
    m_off, _ = _model(cuda, _case(3, 15, 256, multi=multi))
    off = FreeRunningDecoder(m_off, persistent=True, max_iters=T, min_iters=T).run(gb)
    for k in ("mel", "stop"):
        moved = float((off[k] - a[k]).abs().max())
        print(f"dropout[multi={multi}] {k}: switch off vs on {moved:.3e}")
        assert moved > BARS_PATHS[k], (k, moved)
    masks = _redraw(cuda, m.d, T, 3, SEED)
    assert (masks[0] is None) == multi and masks[1] is not None
    _check_oracle(f"dropout oracle[multi={multi}]", a,
                  _oracle(case, tuple(masks), max_iters=T, min_iters=T))


# ------------------------------------------------------------------ 4. stop token
@pytest.mark.parametrize("bias", [8.0, -8.0])
def test_stop_token_same_step_on_both_paths(cuda, bias):
    """The decode ends by itself after min_iters (bias 8) or runs to max_iters (bias -8): both
    paths report the same steps and the rows before it agree."""
    m, gb = _model(cuda, _case(3, 9, 256, multi=True, stop_bias=bias))
    a, r = _both(m, gb, max_iters=30, min_iters=10)
    T = 12 if bias > 0 else 30
    _check_paths(f"stop[{bias}]", a, r, T)
    assert tuple(a["mel"].shape) == (3, T, 256) and tuple(a["stop"].shape) == (3, T)


# ------------------------------------------------------------------ 5. the default path
def _count(monkeypatch, K, calls):
    """Record which options every K.decode_persistent call is given: "hist+spk", "plain", ..."""
    real = K.decode_persistent

    def counted(**kw):
        calls.append("+".join(o for o in ("hist", "spk", "drop") if kw.get(o) is not None)
                     or "plain")
        return real(**kw)

    monkeypatch.setattr(K, "decode_persistent", counted)


def test_default_takes_one_launch(cuda, monkeypatch):
    """persistent=None on a codes model reaches the history entry; rerunning the plan is
    bit-identical (static buffers re-cleared and rewritten)."""
    from sat_amd import kernels as K
    from sat_amd.inference import FreeRunningDecoder
    calls = []
    _count(monkeypatch, K, calls)
    m, gb = _model(cuda, _case(3, 15, 256))
    dec = FreeRunningDecoder(m, max_iters=40, min_iters=40)
    a = dec.run(gb)
    assert dec.last_path == "persistent" and calls == ["hist"]
    c = dec.run(gb)
    for k in KEYS:
        assert torch.equal(a[k], c[k]), k


def test_ljspeech_preset_keeps_the_mel_row_entry(cuda, monkeypatch):
    from sat_amd import data, engine, hparams, kernels as K, params
    from sat_amd.inference import FreeRunningDecoder
    calls = []
    _count(monkeypatch, K, calls)
    hp = hparams.ljspeech_hparams()
    m = engine.Tacotron(hp, cuda, init_values=params.init_params(hp, seed=5))
    b = data.synthetic_batch(hp, 2, N=9, T=20, shape="ljs", seed=2)
    dec = FreeRunningDecoder(m, max_iters=12, min_iters=12)
    out = dec.run({k: torch.tensor(v).to(cuda) for k, v in b.items()})
    assert dec.last_path == "persistent" and calls == ["plain"]
    assert tuple(out["mel"].shape) == (2, 24, 80)


def test_model_fn_predict_codes_equal_launch_path_argmax(cuda, monkeypatch):
    """model_fn PREDICT on a multi-speaker codes model takes the history entry through
    persistent=None; its ``codes`` are the one-hot of the argmax of the launch path's ``mel``.
    A row may be left out only where the float64 oracle's two top logits are closer than the
    mel bar between the paths (2e-5: within it the argmax is not determined); at most 1 % of
    the rows, asserted on the oracle alone.  Untrained logits are small (|mel| < 0.04), so
    near-ties are common at large widths; C = 16 (the fixture corpus' width), 40 steps and batch
    seed 3 give 120 rows whose smallest oracle gap is 4.5e-5: none is left out."""
    from oracle import sat_oracle as O
    from sat_amd import inference as I
    from sat_amd import kernels as K
    from sat_amd import models as M
    from sat_amd import params
    C, T = 16, 40
    hp = _hp(C, multi=True, max_iters=T)
    feats, _ = next(iter(M.synthetic_input_fn(hp, 3, N=14, T=20, shape="ljs", seed=3)()))
    assert len(set(np.asarray(feats.speaker_id).tolist())) > 1
    vals = params.init_params(hp, seed=5)
    calls = []
    _count(monkeypatch, K, calls)
    model = M.DualSourceSelfAttentionTacotronModel(hp, device=cuda, init_values=vals)
    one = model.model_fn(feats, None, M.ModeKeys.PREDICT, hp).predictions
    assert calls == ["hist+spk"]
    monkeypatch.setattr(I.FreeRunningDecoder, "_persistent_ok", lambda self, B, N, Tm: False)
    model = M.DualSourceSelfAttentionTacotronModel(hp, device=cuda, init_values=vals)
    ref = model.model_fn(feats, None, M.ModeKeys.PREDICT, hp).predictions
    assert len(calls) == 1
    assert one["mel"].shape == ref["mel"].shape == one["codes"].shape
    for k, bar in (("mel", 2e-5), ("stop_token", 2e-5), ("alignment", 2e-6), ("alignment2", 2e-6),
                   ("alignment3", 2e-6), ("alignment4", 2e-6)):
        assert float((one[k] - ref[k]).abs().max()) <= bar, k
    batch = {"source": feats.source, "source_length": feats.source_length,
             "speaker_id": feats.speaker_id}
    with torch.no_grad():
        orc = O.infer_free_running(O.to_torch(vals), O.to_torch(params.init_bn_buffers(hp)), hp,
                                   O.to_torch(batch), max_iters=T)
    assert orc["steps"] == one["mel"].shape[1]
    top = orc["mel"].topk(2, dim=2).values
    tie = (top[..., 0] - top[..., 1]) < BARS_PATHS["mel"]                  # [B, T]
    print(f"near-tie rows of the oracle: {int(tie.sum())} of {tie.numel()}")
    assert int(tie.sum()) <= tie.numel() // 100
    want = torch.zeros_like(ref["mel"])
    want.scatter_(2, ref["mel"].argmax(dim=2, keepdim=True), 1.0)
    keep = ~tie.to(one["codes"].device)
    assert bool((one["codes"].sum(dim=2) == 1).all())
    assert torch.equal(one["codes"][keep], want[keep])
    assert torch.equal(one["codes"].argmax(2)[keep].cpu(), orc["mel"].argmax(2)[keep.cpu()])


def test_default_falls_back_when_one_launch_refused(cuda, monkeypatch):
    """The fall-back warning path covers the history entries."""
    from sat_amd import _lib
    from sat_amd import kernels as K
    from sat_amd.inference import FreeRunningDecoder
    m, gb = _model(cuda, _case(3, 15, 256))
    T = 20
    ref = FreeRunningDecoder(m, persistent=False, max_iters=T, min_iters=T).run(gb)

    def refused(*a, **kw):
        raise _lib.SatLibraryError("sat_decode_persistent: fewer than 256 co-resident workgroups",
                                   _lib.SAT_ERR_UNSUPPORTED)

    monkeypatch.setattr(K, "decode_persistent", refused)
    dec = FreeRunningDecoder(m, max_iters=T, min_iters=T)
    with pytest.warns(RuntimeWarning, match="falls back to per-step launches"):
        out = dec.run(gb)
    assert dec.last_path == "launches"
    assert out["steps"] == ref["steps"] == T
    for k in KEYS:
        assert torch.equal(out[k], ref[k]), k
    with pytest.raises(_lib.SatLibraryError):
        FreeRunningDecoder(m, persistent=True, max_iters=T, min_iters=T).run(gb)


# ------------------------------------------------------------------ 6. bad arguments
def test_bad_arguments_return_the_error_code_and_launch_nothing(cuda, monkeypatch):
    """B = 9, N = 257, T = 513 and a null ZH on the arguments of a real decode: every history
    entry answers SAT_ERR_ARGUMENT, and neither the history buffers nor the error word are
    touched."""
    from sat_amd import _lib
    from sat_amd import kernels as K
    from sat_amd.inference import DROP_STREAM0, FreeRunningDecoder
    got = {}
    real = K.decode_persistent

    def record(*, hist, spk, drop, **kw):
        got.update(hist=hist, spk=spk, kw=kw)
        return real(hist=hist, spk=spk, drop=drop, **kw)

    monkeypatch.setattr(K, "decode_persistent", record)
    m, gb = _model(cuda, _case(3, 15, 256, multi=True))
    dec = FreeRunningDecoder(m, persistent=True, max_iters=20, min_iters=20)
    dec.run(gb)
    assert dec.last_path == "persistent" and got
    hist, spk, kw = got["hist"], got["spk"], got["kw"]
    ZH, STOP = hist[0], hist[1]
    ZH.fill_(-7.0)
    STOP.fill_(-7.0)
    kw["err"].zero_()
    seed = torch.tensor([SEED], dtype=torch.int64, device=cuda)
    drop = (seed, DROP_STREAM0, DROP_STREAM0 + 1, 0.5)
    entries = {
        "hist": lambda h, k: real(hist=h, **k),
        "hist_dropout": lambda h, k: real(hist=h, drop=drop, **k),
        "hist_spk": lambda h, k: real(hist=h, spk=spk, **k),
        "hist_spk_dropout": lambda h, k: real(hist=h, spk=spk, drop=drop, **k),
    }
    bad = [(hist, dict(kw, B=9)), (hist, dict(kw, N=257)), (hist, dict(kw, T=513)),
           ((None,) + tuple(hist[1:]), kw)]
    for name, call in entries.items():
        for h, k in bad:
            with pytest.raises(_lib.SatLibraryError) as e:
                call(h, k)
            assert e.value.rc == _lib.SAT_ERR_ARGUMENT, (name, str(e.value))
    torch.cuda.synchronize()
    assert bool((ZH == -7.0).all()) and bool((STOP == -7.0).all())
    assert int(kw["err"].item()) == 0
