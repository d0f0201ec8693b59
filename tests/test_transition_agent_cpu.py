"""ForwardAttention's transition agent and cumulative weights, host side (no GPU): the parameter
inventory, the persistent kernels' eligibility, the factories, and the fp64 restatement the GPU
tests are checked against (tests/transition_agent_ref.py)."""
import numpy as np
import pytest
import torch

import transition_agent_ref as R

A1 = "decoder/attention1"


def test_agent_variables_exist_iff_the_flag_is_on():
    from sat_amd import hparams, params
    names = (f"{A1}/{R.TF}/kernel", f"{A1}/{R.TF}/bias")
    for key, over in R.FLAGS.items():
        hp = hparams.ljspeech_hparams(**over)
        vals = params.init_params(hp, seed=5)
        if key == "cumulative":
            assert not any(n in vals for n in names)
            continue
        d = params.resolve_dims(hp)
        assert vals[names[0]].shape == (d.m1 + d.d1, 1) == (480, 1)
        assert vals[names[1]].shape == (1,) and float(vals[names[1]][0]) == 0.0
        assert np.abs(vals[names[0]]).max() > 0                       # glorot like other kernels
        order = [p.name for p in params.param_specs(hp)]
        assert order.index(names[0]) == order.index(f"{A1}/location_layer/kernel") + 1
    d = params.resolve_dims(hparams.ljspeech_hparams(**R.FLAGS["both"]))
    assert d.transition_agent and d.cumulative_weights


def test_flags_off_inventory_is_unchanged():
    """LJSpeech, both flags off: 143 tensors, 6 227 928 parameters, a 6 228 416-float arena (the
    figures of the code before the feature)."""
    from sat_amd import hparams, params
    hp = hparams.ljspeech_hparams()
    specs = params.param_specs(hp)
    assert len(specs) == 143
    assert params.count_params(hp) == 6227928
    assert params.Layout(specs).total == 6228416
    assert not any(R.TF in p.name for p in specs)
    d = params.resolve_dims(hp)
    assert d.transition_agent is False and d.cumulative_weights is False
    on = params.param_specs(hparams.ljspeech_hparams(**R.FLAGS["both"]))
    assert [p.name for p in on if R.TF not in p.name] == [p.name for p in specs]
    assert params.count_params(hparams.ljspeech_hparams(**R.FLAGS["both"])) == 6227928 + 481


def test_persistent_kernels_are_ineligible_and_say_why():
    from sat_amd import decoder, hparams, params
    assert decoder.persistent_ineligible_reason(
        params.resolve_dims(hparams.ljspeech_hparams()), 32, 200) is None
    why = decoder.persistent_ineligible_reason(
        params.resolve_dims(hparams.ljspeech_hparams(**R.FLAGS["agent"])), 32, 200)
    assert "use_forward_attention_transition_agent" in why
    why = decoder.persistent_ineligible_reason(
        params.resolve_dims(hparams.ljspeech_hparams(**R.FLAGS["cumulative"])), 32, 200)
    assert "cumulative_weights" in why
    assert not decoder.persistent_eligible(
        params.resolve_dims(hparams.ljspeech_hparams(**R.FLAGS["both"])), 32, 200)


def test_one_launch_decode_is_ineligible():
    import types
    from sat_amd import hparams, params
    from sat_amd.inference import FreeRunningDecoder
    for over, want in (({}, ""), (R.FLAGS["agent"], "transition_agent"),
                       (R.FLAGS["cumulative"], "cumulative_weights")):
        hp = hparams.ljspeech_hparams(**over)
        fake = types.SimpleNamespace(hp=hp, d=params.resolve_dims(hp),
                                     device=torch.device("cuda"))
        why = FreeRunningDecoder(fake)._why_not(4, 100, 200)
        assert (why == "") if not want else (want in why)


@pytest.mark.parametrize("key", sorted(R.FLAGS))
def test_factories_accept_the_flags(key):
    from sat_amd import attentions as A, hparams
    hp = hparams.ljspeech_hparams(**R.FLAGS[key])
    fns = (A.attention_factory(hp),) + A.dual_source_attention_factory(hp) + \
        (A.force_alignment_attention_factory(hp),) + \
        A.force_alignment_dual_source_attention_factory(hp)
    for fn in fns:
        assert fn.options.cumulative_weights == hp.cumulative_weights
        assert fn.options.use_transition_agent == hp.use_forward_attention_transition_agent
    # a host tensor is refused for being a host tensor, no longer for the option
    with pytest.raises(TypeError):
        fns[0](torch.zeros(2, 5, 8), torch.tensor([5, 3]), query_depth=4)


def test_restatement_at_rest_is_the_stock_oracle():
    """w = 0, b_u = 0: sigmoid(0) = 0.5 exactly, so the restatement with the agent on must be the
    stock ForwardAttentionOracle bit for bit over chained steps (checks the checker)."""
    from oracle import sat_oracle as O
    from sat_amd import params as PR
    B, N, M, Q, units = 3, 45, 64, 48, 224
    specs = []
    PR._attention(specs, "m", "forward", M, Q, units, 10, 5, transition_agent=True)
    p = {k: torch.tensor(v, dtype=torch.float64) for k, v in PR.init_specs(specs, 9).items()}
    p[f"m/{R.TF}/kernel"].zero_()
    g = torch.Generator().manual_seed(3)
    memory = torch.randn(B, N, M, generator=g).double()
    lengths = torch.tensor([45, 33, 7])
    stock = O.ForwardAttentionOracle(p, "m", memory, lengths)
    mine = R.agent_oracle_class(O, True, False)(p, "m", memory, lengths)
    s0 = stock.initial_state(B, N, torch.float64)
    s1 = mine.initial_state(B, N, torch.float64)
    for _ in range(6):
        q = torch.randn(B, Q, generator=g).double()
        a0, s0 = stock(q, s0)
        a1, s1 = mine(q, s1)
        assert torch.equal(a0, a1)
        for x, y in zip(s0, s1):
            assert torch.equal(x, y)


def test_fixture_moves_the_transition_factor(monkeypatch):
    """The gradient test of test_transition_agent_gpu.py would prove little if u_t stayed at 0.5:
    with the projection kernel scaled by AGENT_SCALE the fp64 model's u_t spans more than 0.05
    over the fixture's steps (B=3, N=45, T=24, eval)."""
    from oracle import sat_oracle as O
    from sat_amd import data, hparams, params
    hp = hparams.ljspeech_hparams(**R.FLAGS["both"])
    vals = R.fixture_values(hp)
    built = R.patch_oracle(monkeypatch, O, True, True)
    batch = data.synthetic_batch(hp, 3, N=45, T=24, shape="ljs", seed=R.FIXTURE_SEED)
    with torch.no_grad():
        O.model_forward(O.to_torch(vals), O.to_torch(params.init_bn_buffers(hp)), hp,
                        O.to_torch(batch), None, training=False)
    u = torch.stack(built[0].u_hist)
    assert u.shape[0] == 24 // hp.outputs_per_step
    assert float(u.max() - u.min()) > 0.05, (float(u.min()), float(u.max()))
