"""apply_dropout_on_inference without a GPU: the mask layout rule, which layers drop, that the
switch leaves the one-launch eligibility alone, and that the masked restatement of the oracle's
free-running loop is the oracle's loop when no layer is masked."""
import types

import numpy as np
import pytest
import torch

import infer_dropout_ref as R
import philox_ref


def _fake(hp):
    from sat_amd import params
    return types.SimpleNamespace(hp=hp, d=params.resolve_dims(hp), device=torch.device("cpu"))


@pytest.mark.parametrize("P", [128, 256])
@pytest.mark.parametrize("B", [1, 3, 8])
def test_mask_element_rule_matches_fill(B, P):
    """Element (t, b, col) of a [T'][B][P] fill is word ((t B + b) P + col) % 4 of the Philox
    block of counter ((t B + b) P + col) // 4 -- every element of T' = 3 steps."""
    from sat_amd.inference import DROP_STREAM0, drop_on_value
    Tm, seed, keep = 3, 0x1234_5678_9ABC, 0.5
    on = drop_on_value(keep)
    assert on == 2.0
    sid = DROP_STREAM0 + (0 if P == 256 else 1)
    fill = philox_ref.mask(Tm * B * P, seed, sid, keep, on).reshape(Tm, B, P)
    got = np.array([[[R.mask_element(t, b, c, B, P, seed, sid, keep, on) for c in range(P)]
                     for b in range(B)] for t in range(Tm)], dtype=np.float32)
    assert np.array_equal(got, fill)
    assert set(np.unique(fill)) == {0.0, 2.0}


def test_segments_follow_the_layout():
    """prenet_mask_segments: one segment per dropping layer, n = T' B P_l, stream DROP_STREAM0 + l,
    on = 1 / keep, every mask 256-byte aligned."""
    from sat_amd import hparams
    from sat_amd import inference as I
    d = _fake(hparams.ljspeech_hparams()).d
    n, views, segs = I.prenet_mask_segments(d, 5, 3, 0.5)
    assert [v[0] for v in views] == [0, 1]
    assert [v[2] for v in views] == [(5, 3, 256), (5, 3, 128)]
    assert [(s[1], s[2], s[3], s[4]) for s in segs] == [
        (5 * 3 * 256, I.DROP_STREAM0, 0.5, 2.0), (5 * 3 * 128, I.DROP_STREAM0 + 1, 0.5, 2.0)]
    assert all(s[0] % 64 == 0 for s in segs) and segs[1][0] >= segs[0][1]
    assert n >= segs[1][0] + segs[1][1]


def test_layer0_clean_rule_follows_multi_speaker():
    """MultiSpeakerPreNet drops under is_training only: with speaker_embedd_to_prenet layer 0 has
    no mask outside training; without a speaker embedding both layers drop."""
    from sat_amd import hparams
    from sat_amd import inference as I
    lj = _fake(hparams.ljspeech_hparams()).d
    vc = _fake(hparams.vctk_hparams()).d
    assert not lj.multi_speaker and vc.multi_speaker
    assert I.prenet_drops(lj) == [True, True]
    assert I.prenet_drops(vc) == [False, True]
    _, views, segs = I.prenet_mask_segments(vc, 4, 2, 0.5)
    assert [v[0] for v in views] == [1] and segs[0][2] == I.DROP_STREAM0 + 1
    hp = hparams.vctk_hparams()
    hp.set_hparam("speaker_embedd_to_prenet", False)
    assert I.prenet_drops(_fake(hp).d) == [True, True]


def _why_not(hp, B, N, Tm, feed="mel", device="cuda"):
    """FreeRunningDecoder._why_not on a stand-in for the decoder (what the method reads: d, hp,
    forced, feed, m.device), so that the GPU-model answers can be asked without a GPU."""
    from sat_amd import params
    from sat_amd.inference import FreeRunningDecoder
    me = types.SimpleNamespace(d=params.resolve_dims(hp), hp=hp, forced=None, feed=feed,
                               m=types.SimpleNamespace(device=torch.device(device)))
    return FreeRunningDecoder._why_not(me, B, N, Tm)


def test_why_not_is_unchanged_by_the_switch():
    """_why_not answers the same with the switch on as with it off: eligible and ineligible
    shapes, feeds, presets and devices."""
    from sat_amd import hparams
    for preset in ("ljspeech", "vctk"):
        off = getattr(hparams, f"{preset}_hparams")()
        on = getattr(hparams, f"{preset}_hparams")()
        on.set_hparam("apply_dropout_on_inference", True)
        for feed in ("mel", "softmax", "target"):
            for device in ("cuda", "cpu"):
                for shape in ((3, 15, 40), (8, 256, 512), (9, 15, 40), (3, 257, 40),
                              (3, 15, 513)):
                    assert (_why_not(on, *shape, feed=feed, device=device)
                            == _why_not(off, *shape, feed=feed, device=device))
    on = hparams.ljspeech_hparams()
    on.set_hparam("apply_dropout_on_inference", True)
    assert _why_not(on, 3, 15, 40) == "" and _why_not(on, 8, 256, 512) == ""
    assert _why_not(on, 9, 15, 40) != "" and _why_not(on, 3, 15, 40, feed="softmax") != ""
    assert _why_not(on, 3, 15, 40, device="cpu") == "not a GPU model"


def test_switch_needs_a_gpu_model():
    """The masks are device draws: with the switch on, a model that is not on a GPU is refused
    at construction instead of decoding with other semantics; with it off nothing changes."""
    from sat_amd import hparams
    from sat_amd.inference import FreeRunningDecoder
    on = hparams.ljspeech_hparams()
    on.set_hparam("apply_dropout_on_inference", True)
    with pytest.raises(NotImplementedError, match="apply_dropout_on_inference"):
        FreeRunningDecoder(_fake(on), seed=7)
    dec = FreeRunningDecoder(_fake(hparams.ljspeech_hparams()), seed=7)
    assert not dec.drop and dec.seed is None


def test_masked_restatement_equals_oracle_without_masks():
    """infer_free_running_masked(None, None) == O.infer_free_running exactly: stop-token helper
    with mel feedback, validation helper with softmax and target feedback, both presets."""
    from oracle import sat_oracle as O
    from sat_amd import data, hparams, params
    for preset in ("ljspeech", "vctk"):
        hp = getattr(hparams, f"{preset}_hparams")()
        p = O.to_torch(params.init_params(hp, seed=5))
        bufs = O.to_torch(params.init_bn_buffers(hp))
        b = O.to_torch(data.synthetic_batch(hp, 2, N=9, T=12, shape="ljs", seed=2))
        for kw in (dict(max_iters=6, min_iters=2), dict(helper="validation", feed="softmax"),
                   dict(helper="validation", feed="target")):
            ref = O.infer_free_running(p, bufs, hp, b, **kw)
            got = R.infer_free_running_masked(p, bufs, hp, b, (None, None), **kw)
            assert got["steps"] == ref["steps"]
            for k in ("mel", "stop", "alignment1", "alignment2"):
                assert torch.equal(got[k], ref[k]), (preset, kw, k)
            assert torch.equal(got["decoder_self_alignments"][0],
                               ref["decoder_self_alignments"][0])


def test_masks_change_the_reference():
    """A mask reaches the reference's output: the restatement is not blind to its argument."""
    from oracle import sat_oracle as O
    from sat_amd import data, hparams, params
    from sat_amd.inference import DROP_STREAM0
    hp = hparams.ljspeech_hparams()
    p = O.to_torch(params.init_params(hp, seed=5))
    bufs = O.to_torch(params.init_bn_buffers(hp))
    b = O.to_torch(data.synthetic_batch(hp, 2, N=9, T=12, shape="ljs", seed=2))
    d = params.resolve_dims(hp)
    ms = [torch.tensor(m) for m in R.host_masks(d, 4, 2, 7, 0.5, DROP_STREAM0)]
    clean = R.infer_free_running_masked(p, bufs, hp, b, (None, None), max_iters=4, min_iters=4)
    drop = R.infer_free_running_masked(p, bufs, hp, b, ms, max_iters=4, min_iters=4)
    # float64 on both sides: equal masks would give exactly 0 (the fresh weights' mel frames are
    # ~1e-4 in size, the masks move them by ~1e-5)
    assert float((clean["mel"] - drop["mel"]).abs().max()) > 1e-6
    assert float((clean["alignment1"] - drop["alignment1"]).abs().max()) > 0.0
