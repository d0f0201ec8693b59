"""The one-launch free-running decode of the multi-speaker (VCTK) model: sat_decode_persistent with
its speaker option, without and with dropout (decode_persistent_kernel<kDrop, true>) against the
per-step launch path of the same FreeRunningDecoder, against the float64 oracle, and through
model_fn.

Bars: the ones the single-speaker files carry, not new ones -- between the two paths mel / stop
2e-5 and alignments / decoder self-alignment rows 2e-6 (test_decode_persistent_gpu.py), against
the float64 oracle mel / stop 2e-4 and alignments 2e-5 (test_one_launch_matches_oracle,
test_infer_dropout_gpu.py).  Weights: the VCTK preset from params.init_params(hp, seed=5); the
speaker ids differ within every batch."""
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


def _hp(drop=False, **over):
    from sat_amd import hparams
    hp = hparams.vctk_hparams(**over)
    if drop:
        hp.set_hparam("apply_dropout_on_inference", True)
    return hp


@functools.lru_cache(maxsize=None)
def _case(B, N, drop=False, stop_bias=None, same_rows=False, over=()):
    """Host side of a case: hparams, fresh weights, a synthetic batch with B distinct speakers
    (``same_rows``: every utterance carries utterance 0's source row and length)."""
    from sat_amd import data, params
    hp = _hp(drop, **dict(over))
    vals = params.init_params(hp, seed=5)
    if stop_bias is not None:
        vals["decoder/stop_token_projection/bias"] = np.full((1,), stop_bias, np.float32)
    b = data.synthetic_batch(hp, B, N=N, T=20, shape="ljs", seed=2)
    off = hp.speaker_embedding_offset
    b["speaker_id"] = np.asarray([off + (37 * g) % hp.num_speakers for g in range(B)],
                                 b["speaker_id"].dtype)
    assert len(set(b["speaker_id"].tolist())) == B
    if same_rows:
        b["source"][:] = b["source"][0]
        b["source_length"][:] = b["source_length"][0]
    return hp, vals, b


def _model(cuda, case, hp=None):
    from sat_amd import engine
    hp0, vals, b = case
    m = engine.Tacotron(hp0 if hp is None else hp, cuda, init_values=vals)
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
@pytest.mark.parametrize("B,N", [(1, 7), (3, 15), (8, 200)])
def test_one_launch_matches_launch_path(cuda, B, N):
    """One utterance; a partly filled grid with ragged tiles; the full 8 groups with N not a
    multiple of 32."""
    m, gb = _model(cuda, _case(B, N))
    assert m.d.multi_speaker
    T = 40
    a, r = _both(m, gb, max_iters=T, min_iters=T)
    _check_paths(f"paths[{B},{N}]", a, r, T)


# ------------------------------------------------------------------ 2. against the oracle
def test_default_takes_one_launch_and_matches_oracle(cuda):
    """persistent=None picks the one-launch decode for the VCTK preset; (3, 15), 40 steps against
    the float64 oracle's own PREDICT restatement."""
    from oracle import sat_oracle as O
    from sat_amd import params
    from sat_amd.inference import FreeRunningDecoder
    case = _case(3, 15)
    hp, vals, b = case
    m, gb = _model(cuda, case)
    T = 40
    dec = FreeRunningDecoder(m, max_iters=T)
    out = dec.run(gb)
    assert dec.last_path == "persistent"
    with torch.no_grad():
        ref = O.infer_free_running(O.to_torch(vals), O.to_torch(params.init_bn_buffers(hp)), hp,
                                   O.to_torch(b), max_iters=T)
    _check_oracle("oracle[3,15]", out, ref)


# ------------------------------------------------------------------ 3. the row is per utterance
def test_speaker_row_is_indexed_per_utterance(cuda):
    """B = 4, the same source row and length everywhere, four speakers: utterance g > 0 differs
    from utterance 0 by more than the bar (in the oracle and on the GPU), and each utterance
    equals the B = 1 decode of its speaker."""
    from sat_amd.inference import FreeRunningDecoder
    case = _case(4, 15, same_rows=True)
    hp, vals, b = case
    T = 40
    ref = _oracle(case, max_iters=T, min_iters=T)
    for g in range(1, 4):
        moved = float((ref["mel"][g] - ref["mel"][0]).abs().max())
        print(f"oracle: speaker {g} vs 0 moves the mel frames by {moved:.3e}")
        assert moved > 100 * BARS_PATHS["mel"], (g, moved)
    m, gb = _model(cuda, case)
    dec = FreeRunningDecoder(m, persistent=True, max_iters=T, min_iters=T)
    out = dec.run(gb)
    assert dec.last_path == "persistent" and out["steps"] == T
    for g in range(1, 4):
        assert float((out["mel"][g] - out["mel"][0]).abs().max()) > 100 * BARS_PATHS["mel"]
    one = FreeRunningDecoder(m, persistent=True, max_iters=T, min_iters=T)
    for g in range(4):
        sb = {k: v[g:g + 1].contiguous() for k, v in gb.items()}
        solo = one.run(sb)
        assert one.last_path == "persistent" and solo["steps"] == T
        for k in KEYS:
            dist = float((out[k][g:g + 1] - solo[k]).abs().max())
            assert dist <= BARS_PATHS[k], (g, k, dist)


# ------------------------------------------------------------------ 4. options that change the row
def test_projected_speaker_row_matches_launch_path(cuda):
    m, gb = _model(cuda, _case(3, 15, over=(("speaker_embedding_projection_out_dim", 8),)))
    assert m.d.multi_speaker
    T = 40
    a, r = _both(m, gb, max_iters=T, min_iters=T)
    _check_paths("paths[projection]", a, r, T)


def test_fixed_speaker_equals_a_batch_of_that_speaker(cuda):
    from sat_amd.inference import FreeRunningDecoder
    x, T = 300, 40
    case = _case(3, 15)
    hp, vals, b = case
    assert not np.any(b["speaker_id"] == x)
    m_fix, gb = _model(cuda, case, hp=_hp(speaker_for_synthesis=x))
    m_ids, _ = _model(cuda, case)
    same = dict(gb, speaker_id=torch.full_like(gb["speaker_id"], x))
    d_fix = FreeRunningDecoder(m_fix, persistent=True, max_iters=T, min_iters=T)
    d_ids = FreeRunningDecoder(m_ids, persistent=True, max_iters=T, min_iters=T)
    a, c = d_fix.run(gb), d_ids.run(same)
    assert d_fix.last_path == d_ids.last_path == "persistent"
    for k in KEYS:
        assert torch.equal(a[k], c[k]), k
    other = d_ids.run(gb)                     # the batch's own speakers give another output
    assert float((other["mel"] - a["mel"]).abs().max()) > 100 * BARS_PATHS["mel"]


# ------------------------------------------------------------------ 5. stop token
@pytest.mark.parametrize("bias", [8.0, -8.0])
def test_stop_token_same_step_on_both_paths(cuda, bias):
    m, gb = _model(cuda, _case(3, 9, stop_bias=bias))
    a, r = _both(m, gb, max_iters=30, min_iters=10)
    assert a["steps"] == r["steps"] == (12 if bias > 0 else 30)
    assert float((a["mel"] - r["mel"]).abs().max()) <= 2e-5


# ------------------------------------------------------------------ 6. determinism
def test_rerun_is_deterministic(cuda):
    """Two decodes on one plan (scratch and d0 slots re-cleared, caches rewritten): bitwise."""
    from sat_amd.inference import FreeRunningDecoder
    m, gb = _model(cuda, _case(4, 30))
    dec = FreeRunningDecoder(m, max_iters=64, min_iters=64, persistent=True)
    a = dec.run(gb)
    c = dec.run(gb)
    for k in KEYS:
        assert torch.equal(a[k], c[k]), k


# ------------------------------------------------------------------ 7. the dropout instantiation
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


@pytest.mark.parametrize("T", [40, 130])
def test_dropout_one_launch_matches_launch_path_and_oracle(cuda, T):
    """apply_dropout_on_inference: the same seed on both paths, (3, 15); 130 steps exercises the
    step-parity slots and takes t B P past small values.  The switch-off decode lies outside the
    bar from the switch-on one (a kernel that ignores the mask cannot pass), and the one-launch
    result meets the oracle bars against the float64 loop fed layer 1's re-drawn mask (layer 0
    clean: the MultiSpeakerPreNet drops under is_training only)."""
    from sat_amd.inference import FreeRunningDecoder
    case = _case(3, 15, drop=True)
    m, gb = _model(cuda, case)
    assert m.d.multi_speaker
    a, r = _both(m, gb, max_iters=T, min_iters=T, seed=SEED)
    _check_paths(f"dropout paths[{T}]", a, r, T)
    m_off, _ = _model(cuda, _case(3, 15))
    off = FreeRunningDecoder(m_off, persistent=True, max_iters=T, min_iters=T).run(gb)
    for k in ("mel", "stop"):
        moved = float((off[k] - a[k]).abs().max())
        print(f"dropout[{T}] {k}: switch off vs on {moved:.3e}")
        assert moved > BARS_PATHS[k], (k, moved)
    masks = _redraw(cuda, m.d, T, 3, SEED)
    assert masks[0] is None and masks[1] is not None
    ref = _oracle(case, (None, masks[1]), max_iters=T, min_iters=T)
    _check_oracle(f"dropout oracle[{T}]", a, ref)


# ------------------------------------------------------------------ 8. fallback
def test_default_falls_back_when_one_launch_refused(cuda, monkeypatch):
    from sat_amd import _lib
    from sat_amd import kernels as K
    from sat_amd.inference import FreeRunningDecoder
    m, gb = _model(cuda, _case(3, 15))
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


# ------------------------------------------------------------------ 9. surface
def test_model_fn_predict_takes_one_launch(cuda, monkeypatch):
    """model_fn PREDICT on a VCTK model reaches the new kernel through persistent=None; its
    predictions lie within the bars of those of a model whose decoder is held on the launches."""
    from sat_amd import inference as I
    from sat_amd import kernels as K
    from sat_amd import models as M
    hp = _hp(max_iters=24)
    feats, _ = next(iter(M.synthetic_input_fn(hp, 3, N=14, T=20, shape="ljs", seed=2)()))
    assert len(set(np.asarray(feats.speaker_id).tolist())) > 1
    calls = []
    real = K.decode_persistent

    def counted(**kw):
        calls.append(kw.get("spk") is not None)     # the speaker option given
        return real(**kw)

    monkeypatch.setattr(K, "decode_persistent", counted)
    model = M.tacotron_model_factory(hp, None, None, device=cuda, seed=3)
    one = model.model_fn(feats, None, M.ModeKeys.PREDICT, hp).predictions
    assert calls == [True]
    monkeypatch.setattr(I.FreeRunningDecoder, "_persistent_ok", lambda self, B, N, Tm: False)
    model = M.tacotron_model_factory(hp, None, None, device=cuda, seed=3)
    ref = model.model_fn(feats, None, M.ModeKeys.PREDICT, hp).predictions
    assert len(calls) == 1
    assert one["mel"].shape == ref["mel"].shape
    for k, bar in (("mel", 2e-5), ("stop_token", 2e-5), ("alignment", 2e-6), ("alignment2", 2e-6),
                   ("alignment3", 2e-6), ("alignment4", 2e-6)):
        assert float((one[k] - ref[k]).abs().max()) <= bar, k
