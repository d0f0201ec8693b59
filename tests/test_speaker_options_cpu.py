"""The fork's speaker options on the host: parameter inventory and layout, the TF <-> arena row
order, option checks, the fixture's distance from the projection's ReLU kink, and the numpy
restatements of the speaker kernels (GPU comparison: test_speaker_options_gpu.py)."""
import zlib

import numpy as np
import pytest
import torch

import speaker_options_ref as SR


def _crc(items):
    return zlib.crc32(repr(sorted(items)).encode())


def _layout(hp):
    from sat_amd import params
    return params.Layout(params.param_specs(hp))


def test_defaults_keep_the_layout_of_the_parent_commit():
    """Literal numbers of the parent commit: tensor count, parameter count, arena size and the
    CRC-32 of ``repr(sorted(...items()))`` of its shapes and offsets (LJSpeech, VCTK)."""
    from sat_amd import hparams, params
    for hp, want in ((hparams.ljspeech_hparams(), (143, 6227928, 6228416, 121305031, 113178392)),
                     (hparams.vctk_hparams(), (148, 6300504, 6300992, 91214668, 267904672))):
        L = _layout(hp)
        got = (len(L.specs), L.num_params, L.total, _crc(L.shapes.items()), _crc(L.offsets.items()))
        assert got == want
        assert not L.row_perms
        d = params.resolve_dims(hp)
        assert (d.spk_to_decoder, d.spk_proj, d.spk_fixed) == (False, -1, -1)
        assert d.spk_width == (16 if hp.use_speaker_embedding else 0)
    L = _layout(hparams.ljspeech_hparams())
    assert L.offsets["decoder/attention_lstm/kernel"] == 3697536
    assert L.shapes["decoder/attention_lstm/kernel"] == (672, 1024)
    assert L.shapes["decoder/lstm1/kernel"] == (800, 1024)


def test_each_option_gives_the_reference_shapes():
    from sat_amd import hparams
    base = _layout(hparams.vctk_hparams()).shapes
    a1, a2 = "decoder/attention1", "decoder/attention2"
    # projection: Dense(P) with bias; MultiSpeakerPreNet's fan-in becomes P
    sh = _layout(hparams.vctk_hparams(speaker_embedding_projection_out_dim=8)).shapes
    assert sh["speaker_embedding_projection/kernel"] == (16, 8)
    assert sh["speaker_embedding_projection/bias"] == (8,)
    assert sh["decoder/prenet0/speaker_projection/kernel"] == (8, 256)
    assert sh["decoder/attention_lstm/kernel"] == base["decoder/attention_lstm/kernel"]
    # to-decoder: S rows per source
    for P, S in ((-1, 16), (8, 8)):
        for agent in (False, True):
            hp = hparams.vctk_hparams(speaker_embedd_to_decoder=True,
                                      speaker_embedding_projection_out_dim=P,
                                      use_forward_attention_transition_agent=agent)
            sh = _layout(hp).shapes
            assert sh[f"{a1}/memory_layer/kernel"] == (256 + S, 224)
            assert sh[f"{a2}/memory_layer/kernel"] == (32 + S, 32)
            assert sh["decoder/attention_lstm/kernel"] == (128 + 256 + 32 + 2 * S + 256, 1024)
            assert sh["decoder/lstm1/kernel"] == (256 + 256 + 32 + 2 * S + 256, 1024)
            assert sh["decoder/lstm2/kernel"] == base["decoder/lstm2/kernel"]
            assert sh["speaker_embedding"] == (152, 16)
            assert ("speaker_embedding_projection/kernel" in sh) == (P > -1)
            tf_ = f"{a1}/transition_factor_projection/kernel"
            assert (sh[tf_] == (256 + S + 224, 1)) if agent else (tf_ not in sh)
    # to-decoder without to-prenet: plain prenets, the table is still there
    sh = _layout(hparams.vctk_hparams(speaker_embedd_to_decoder=True,
                                      speaker_embedd_to_prenet=False)).shapes
    assert "speaker_embedding" in sh and "decoder/prenet0/kernel" in sh
    assert "decoder/prenet0/speaker_projection/kernel" not in sh
    assert sh["decoder/attention_lstm/kernel"] == (128 + 256 + 32 + 32 + 256, 1024)
    # neither destination: no table, no projection
    sh = _layout(hparams.vctk_hparams(speaker_embedd_to_prenet=False,
                                      speaker_embedding_projection_out_dim=8)).shapes
    assert "speaker_embedding" not in sh and "speaker_embedding_projection/kernel" not in sh


def test_resolve_dims_combinations():
    from sat_amd import hparams, params
    d = params.resolve_dims(hparams.vctk_hparams(speaker_embedd_to_decoder=True,
                                                 speaker_embedd_to_prenet=False))
    assert (d.multi_speaker, d.spk_to_decoder, d.has_speaker, d.spk_width) == (False, True, True, 16)
    d = params.resolve_dims(SR.make_hparams("all"))
    assert (d.multi_speaker, d.spk_to_decoder, d.spk_proj, d.spk_width, d.spk_fixed) == \
        (True, True, 8, 8, SR.FIXED_SPEAKER)
    # the options need the speaker embedding itself (the reference fails without it too)
    for kw in (dict(speaker_embedd_to_decoder=True), dict(speaker_for_synthesis=0),
               dict(speaker_embedding_projection_out_dim=8)):
        with pytest.raises(ValueError, match="use_speaker_embedding"):
            params.resolve_dims(hparams.ljspeech_hparams(**kw))
    with pytest.raises(ValueError, match="multiple of 4"):
        params.resolve_dims(hparams.vctk_hparams(speaker_embedd_to_decoder=True,
                                                 speaker_embedding_projection_out_dim=6))
    # still refused
    with pytest.raises(NotImplementedError):
        params.resolve_dims(hparams.vctk_hparams(speaker_embedd_to_postnet=True))
    with pytest.raises(NotImplementedError):
        params.resolve_dims(hparams.vctk_hparams(use_speaker_embedding=False,
                                                 use_external_speaker_embedding=True))


def test_speaker_for_synthesis_range():
    from sat_amd import hparams, params
    for x in (225, 376):
        assert params.resolve_dims(hparams.vctk_hparams(speaker_for_synthesis=x)).spk_fixed == x
    for x in (0, 224, 377):
        with pytest.raises(ValueError, match=r"225\.\.376"):
            params.resolve_dims(hparams.vctk_hparams(speaker_for_synthesis=x))


@pytest.mark.parametrize("agent", [False, True])
def test_widened_kernels_round_trip_and_keep_tf_row_order(agent):
    """pack / unpack and to_internal / from_internal are inverse, and the arena holds the TF rows
    [.. | c1 | s | c2 | s | ..] as [.. | c1 | c2 | .. | s | s] (columns gate-interleaved)."""
    from sat_amd import params
    hp = SR.make_hparams("all", agent=agent)
    L = _layout(hp)
    vals = params.init_params(hp, seed=3)
    back = L.unpack(L.pack(vals))
    for k, v in vals.items():
        np.testing.assert_array_equal(back[k], v)
        np.testing.assert_array_equal(L.from_internal(k, L.to_internal(k, v)), v)
    S, p, M1, M2, A, D = 8, 128, 256, 32, 256, 256
    k = "decoder/attention_lstm/kernel"
    ext = vals[k]
    inner = params.from_internal(k, L.to_internal(k, ext))          # rows moved, columns back
    want = np.concatenate([ext[:p + M1], ext[p + M1 + S:p + M1 + S + M2], ext[-A:],
                           ext[p + M1:p + M1 + S], ext[p + M1 + S + M2:p + M1 + 2 * S + M2]])
    np.testing.assert_array_equal(inner, want)
    k = "decoder/lstm1/kernel"
    ext = vals[k]
    inner = params.from_internal(k, L.to_internal(k, ext))
    want = np.concatenate([ext[:A + M1], ext[A + M1 + S:A + M1 + S + M2], ext[-D:],
                           ext[A + M1:A + M1 + S], ext[A + M1 + S + M2:A + M1 + 2 * S + M2]])
    np.testing.assert_array_equal(inner, want)
    k = "decoder/attention1/transition_factor_projection/kernel"
    if agent:
        ext = vals[k]
        want = np.concatenate([ext[:M1], ext[M1 + S:], ext[M1:M1 + S]])
        np.testing.assert_array_equal(L.to_internal(k, ext), want)
    assert set(L.row_perms) == {"decoder/attention_lstm/kernel", "decoder/lstm1/kernel"} | \
        ({k} if agent else set())


def test_fixture_stays_clear_of_the_projection_kink():
    """min |pre-activation| of the projection in fp64, for the batch's speakers and the fixed
    one (the figures quoted in speaker_options_ref.py)."""
    from oracle import sat_oracle as O
    for key in ("projection", "all"):
        hp = SR.make_hparams(key)
        p = O.to_torch(SR.make_values(hp))
        _, pre = SR.speaker_vector(p, hp, O.to_torch(SR.make_batch(hp)))
        lo = float(pre.abs().min())
        print(f"{key}: min |pre-activation| {lo:.3e}")
        assert lo >= 1e-4
        assert bool((pre > 0).any()) and bool((pre < 0).any())      # the ReLU does something


def test_alignments_sum_to_one_in_the_reference():
    """The algebra's premise, on the reference's own alignments."""
    from oracle import sat_oracle as O
    from sat_amd import params
    hp = SR.make_hparams("all")
    p = O.to_torch(SR.make_values(hp))
    with torch.no_grad():
        ref = SR.model_forward(O, p, O.to_torch(params.init_bn_buffers(hp)), hp,
                               O.to_torch(SR.make_batch(hp)), None, False)
    for k in ("alignment1", "alignment2"):
        assert tuple(ref[k].shape) == (SR.B, SR.T, SR.N)
        assert float((ref[k].sum(-1) - 1).abs().max()) <= 1e-6


def test_numpy_restatements_of_the_kernels():
    rng = np.random.default_rng(0)
    y = rng.standard_normal((3, 5, 8)).astype(np.float32)
    bias = rng.standard_normal((3, 8)).astype(np.float32)
    out = SR.rows_bias_fwd_np(y, bias, [5, 2, 0])
    np.testing.assert_array_equal(out[0], y[0] + bias[0])
    np.testing.assert_array_equal(out[1, :2], y[1, :2] + bias[1])
    np.testing.assert_array_equal(out[1, 2:], y[1, 2:])
    np.testing.assert_array_equal(out[2], y[2])
    np.testing.assert_array_equal(SR.rows_bias_fwd_np(y, bias), y + bias[:, None])
    s = SR.rows_bias_bwd_np(y, [5, 2, 0])
    np.testing.assert_allclose(s[1], y[1, :2].astype(np.float64).sum(0))
    assert not s[2].any()
    ctx = np.zeros((4, 3, 12), np.float32)
    f = SR.ctx_tail_fill_np(ctx, 4, bias, 1, 4)
    assert not f[0].any() and not f[:, :, :4].any()
    np.testing.assert_array_equal(f[2, :, 4:], bias)
