"""The L2 regulariser on the host: which tensors it sums (params.is_l2_regularized against
explicit lists), the arena ranges handed to the kernel (params.l2_segments) and the
data-parallel gradient weight.  The training step does not call the kernel yet, so resolve_dims
still refuses use_l2_regularization=True (tests/test_surface_cpu.py); the set does not depend on
the switch."""
import os

import numpy as np
import pytest

import l2_ref

REF = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_examples")

ENCODER = (
    ["encoder/prenet0/kernel", "encoder/prenet1/kernel"]
    + [f"encoder/cbhg/conv_bank/K{k}/kernel" for k in range(1, 17)]
    + ["encoder/cbhg/proj1/kernel", "encoder/cbhg/proj2/kernel"]
    + [f"encoder/cbhg/highway{i}/{g}/kernel" for i in range(4) for g in "HT"]
    + ["encoder/self_attention_projection/kernel"]
    + [f"encoder/self_attention0/mha/{p}_projection/kernel"
       for p in ("query", "key", "value", "output")]
    + ["encoder/self_attention0/transform/kernel"])
ATTENTION = [
    "decoder/attention1/memory_layer/kernel", "decoder/attention1/query_layer/kernel",
    "decoder/attention1/attention_variable", "decoder/attention1/location_conv/kernel",
    "decoder/attention1/location_layer/kernel",
    "decoder/attention2/memory_layer/kernel", "decoder/attention2/query_layer/kernel",
    "decoder/attention2/attention_v"]
HEAD = ([f"decoder/self_attention0/mha/{p}_projection/kernel"
         for p in ("query", "key", "value", "output")]
        + ["decoder/self_attention0/transform/kernel", "decoder/out_projection/kernel"])
SPEAKER_PRENET = ["decoder/prenet0/dense0/kernel", "decoder/prenet0/speaker_projection/kernel",
                  "decoder/prenet0/dense/kernel", "decoder/prenet1/kernel"]
EXPECTED = {
    "ljspeech": ENCODER + ["decoder/prenet0/kernel", "decoder/prenet1/kernel"] + ATTENTION + HEAD,
    "vctk": ENCODER + SPEAKER_PRENET + ATTENTION + HEAD,
    # transition agent + speaker projection + speaker vector appended to both memories
    "vctk_options": (ENCODER + ["speaker_embedding_projection/kernel"] + SPEAKER_PRENET
                     + ATTENTION[:5] + ["decoder/attention1/transition_factor_projection/kernel"]
                     + ATTENTION[5:] + HEAD),
}
LSTM_KERNELS = ["encoder/cbhg/lstm_fw/kernel", "encoder/cbhg/lstm_bw/kernel",
                "decoder/attention_lstm/kernel", "decoder/lstm1/kernel", "decoder/lstm2/kernel"]


def _hp(which):
    from sat_amd import hparams
    base = which.split("_")[0]
    hp = hparams.create_hparams(os.path.join(REF, base, "self-attention-tacotron.json"))
    if which == "vctk_options":
        hp.set_hparam("use_forward_attention_transition_agent", True)
        hp.set_hparam("speaker_embedding_projection_out_dim", 64)
        hp.set_hparam("speaker_embedd_to_decoder", True)
    return hp


@pytest.mark.parametrize("which", list(EXPECTED))
def test_regularised_set_is_the_explicit_list(which):
    from sat_amd import params as PR
    specs = PR.param_specs(_hp(which))
    got = [p.name for p in specs if PR.is_l2_regularized(p.name)]
    assert got == EXPECTED[which]
    names = {p.name for p in specs}
    assert set(EXPECTED[which]) <= names
    out = names - set(got)
    # everything left out is an embedding, a bias, a BN scale / shift, an LSTM kernel or the
    # stop-token kernel
    for n in out:
        leaf = n.rsplit("/", 1)[-1]
        assert (leaf in ("bias", "gamma", "beta", "attention_bias", "embedding",
                         "speaker_embedding")
                or n in LSTM_KERNELS or n == "decoder/stop_token_projection/kernel"), n
    assert "decoder/out_projection/kernel" in got
    assert "decoder/stop_token_projection/kernel" in out
    assert "decoder/attention1/attention_bias" in out
    assert "embedding" in out
    assert set(LSTM_KERNELS) <= out
    assert not any(PR.is_l2_regularized(n) for n in LSTM_KERNELS)


def test_named_speaker_and_agent_tensors():
    from sat_amd import params as PR
    specs = PR.param_specs(_hp("vctk_options"))
    names = {p.name for p in specs}
    for n in ("speaker_embedding_projection/kernel", "speaker_embedding",
              "decoder/attention1/transition_factor_projection/kernel",
              "decoder/prenet0/speaker_projection/kernel"):
        assert n in names
    assert PR.is_l2_regularized("speaker_embedding_projection/kernel")
    assert not PR.is_l2_regularized("speaker_embedding_projection/bias")
    assert not PR.is_l2_regularized("speaker_embedding")
    assert not PR.is_l2_regularized("embedding")
    assert PR.is_l2_regularized("decoder/attention1/transition_factor_projection/kernel")
    assert PR.is_l2_regularized("decoder/prenet0/speaker_projection/kernel")
    assert not PR.is_l2_regularized("decoder/attention1/attention_bias")
    # a forward attention as source 2 has a location_conv of its own: both kernels are in
    hp = _hp("ljspeech")
    hp.set_hparam("attention2", "forward")
    got = {p.name for p in PR.param_specs(hp) if PR.is_l2_regularized(p.name)}
    assert {"decoder/attention1/location_conv/kernel", "decoder/attention2/location_conv/kernel",
            "decoder/attention2/attention_variable"} <= got
    assert "decoder/attention2/attention_bias" not in got


@pytest.mark.parametrize("which", list(EXPECTED))
def test_segments(which):
    """Ranges lie inside selected tensors, are sorted and disjoint, cover every selected element
    once and no padding, and two tensors share a range only when nothing -- no padding, no other
    tensor -- lies between them."""
    from sat_amd import params as PR
    specs = PR.param_specs(_hp(which))
    lay = PR.Layout(specs)
    segs = PR.l2_segments(specs, lay)
    size = {p.name: int(np.prod(p.shape)) for p in specs}
    sel = np.zeros(lay.total, bool)                     # selected elements of the arena
    for p in specs:
        if PR.is_l2_regularized(p.name):
            sel[lay.offsets[p.name]:lay.offsets[p.name] + size[p.name]] = True
    cover = np.zeros(lay.total, np.int32)
    prev_end = -1
    for off, n in segs:
        assert n > 0 and 0 <= off and off + n <= lay.total
        assert off > prev_end, "sorted, disjoint, and merged where they touch"
        prev_end = off + n
        cover[off:off + n] += 1
    assert np.array_equal(cover, sel.astype(np.int32))
    assert sum(n for _, n in segs) == sum(size[n] for n in EXPECTED[which])
    assert len(segs) < len(EXPECTED[which]), "neighbours without padding are merged"
    # the 16 conv-bank kernels (sizes k * 128 * 128, multiples of 64) form ONE range; their
    # biases and BN vectors follow, so proj1's kernel starts another
    o1 = lay.offsets["encoder/cbhg/conv_bank/K1/kernel"]
    end = lay.offsets["encoder/cbhg/conv_bank/K16/kernel"] + size["encoder/cbhg/conv_bank/K16/kernel"]
    assert (o1, end - o1) in segs
    assert (lay.offsets["encoder/cbhg/proj1/kernel"], size["encoder/cbhg/proj1/kernel"]) in segs
    # attention_variable is followed by attention_bias, which is not regularised: a range ends
    # exactly where that vector ends (the padding rule is test_segments_merge_only_without_padding's)
    o = lay.offsets["decoder/attention1/attention_variable"]
    e = o + size["decoder/attention1/attention_variable"]
    assert any(off + n == e for off, n in segs)


def test_segments_merge_only_without_padding():
    from sat_amd import params as PR
    S = PR.ParamSpec
    specs = [S("a/kernel", (64,)), S("b/kernel", (3, 64)), S("c/kernel", (5,)),
             S("d/kernel", (7,)), S("d/bias", (64,)), S("e/kernel", (128,)),
             S("f/attention_v", (64,))]
    lay = PR.Layout(specs)
    assert PR.l2_segments(specs, lay) == [(0, 64 + 192 + 5), (320, 7), (448, 128 + 64)]


@pytest.mark.parametrize("world", [1, 2, 8])
def test_grad_weight_times_grad_scale_is_the_weight(world):
    """Adam uses grad_scale * g with grad_scale = 1 / world: the regulariser's factor on the
    SUM-reduced arena makes the effective gradient weight * w, in float32 as the kernels carry
    the two factors."""
    from sat_amd import dp
    F32 = np.float32
    for lam in (1e-7, 1e-2, 0.3):
        gs = 1.0 / world
        gw = dp.l2_grad_weight(lam, gs)
        assert gs * gw == lam
        assert F32(F32(gs) * F32(gw)) == F32(lam)


def test_reference_restatement():
    """l2_ref on a hand-computed case: two selected tensors and one left out."""
    w = {"a": np.array([1.0, 2.0], np.float32), "b": np.array([[3.0]], np.float32),
         "bias": np.array([100.0], np.float32)}
    sel = lambda n: n != "bias"                                               # noqa: E731
    assert l2_ref.l2_loss64(w, 0.5, sel) == 0.5 * (5.0 / 2 + 9.0 / 2)
    assert float(l2_ref.l2_loss32(w, 0.5, sel)) == 3.5
    assert l2_ref.e32(w, 0.5, sel) == 0.0
