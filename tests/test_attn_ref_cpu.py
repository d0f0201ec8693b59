"""Anchors tests/attn_ref.py (the kernels'-layout reference of test_attn_step_gpu.py) to the
float64 oracle's attention mechanisms and to tests/transition_agent_ref.py, and its reverse step
(step_bwd / agent_bwd chained with the kernels' hand-off operands) to autograd of a whole chain.
CPU only."""
import pytest
import torch

import attn_ref as R
import transition_agent_ref as TA

F64 = torch.float64
TF = TA.TF


def _rand(g, *shape, scale=1.0):
    return scale * torch.randn(*shape, generator=g, dtype=F64)


def _oracle_params(g, M, Q, D1, D2, F, KW):
    """Parameters under the oracle's names; the scales make the location term and the agent count
    (asserted below) and keep the alignments spread."""
    p = {"a1/memory_layer/kernel": _rand(g, M, D1, scale=0.3),
         "a1/query_layer/kernel": _rand(g, Q, D1, scale=0.3),
         "a1/location_conv/kernel": _rand(g, KW, 1, F, scale=0.5),
         "a1/location_conv/bias": _rand(g, F, scale=0.2),
         "a1/location_layer/kernel": _rand(g, F, D1, scale=0.5),
         "a1/attention_variable": _rand(g, D1, scale=0.15),
         "a1/attention_bias": _rand(g, D1, scale=0.2),
         "a1/attention_v": _rand(g, D1, scale=0.15),
         f"a1/{TF}/kernel": _rand(g, M + D1, 1, scale=0.4),
         f"a1/{TF}/bias": _rand(g, 1, scale=0.2),
         "a2/memory_layer/kernel": _rand(g, M, D2, scale=0.3),
         "a2/query_layer/kernel": _rand(g, Q, D2, scale=0.3),
         "a2/attention_v": _rand(g, D2, scale=0.3)}
    return p


def _kernel_params(p, forward=True):
    return dict(v1=p["a1/attention_variable"] if forward else p["a1/attention_v"],
                b1=p["a1/attention_bias"] if forward else None,
                convW=p["a1/location_conv/kernel"][:, 0, :], convb=p["a1/location_conv/bias"],
                locW=p["a1/location_layer/kernel"], v2=p["a2/attention_v"],
                agent_w=p[f"a1/{TF}/kernel"], agent_b=p[f"a1/{TF}/bias"])


DIMS = dict(B=3, N=45, M=12, Q=10, D1=32, D2=32, F=5, KW=10)
LENGTHS = torch.tensor([45, 33, 7])


def _setup(seed, **over):
    d = dict(DIMS, **over)
    g = torch.Generator().manual_seed(seed)
    p = _oracle_params(g, d["M"], d["Q"], d["D1"], d["D2"], d["F"], d["KW"])
    memory = _rand(g, d["B"], d["N"], d["M"])
    queries = [_rand(g, d["B"], d["Q"]) for _ in range(4)]
    return d, g, p, memory, queries


@pytest.mark.parametrize("kind", ["forward", "additive"])
def test_steps_match_oracle(kind):
    """step_fwd stepped 4 times from the initial state == ForwardAttentionOracle /
    AdditiveAttentionOracle for mechanism 1 and AdditiveAttentionOracle for mechanism 2 (1e-12):
    alignments, the state the next step convolves, both contexts; exact zeros and -inf past the
    lengths; the statistics row is what the combine kernel's comment says."""
    from oracle import sat_oracle as O
    d, g, p, memory, queries = _setup(3)
    B, N = d["B"], d["N"]
    fwd = kind == "forward"
    o1 = O.make_attention(kind, p, "a1", memory, LENGTHS)
    o2 = O.make_attention("additive", p, "a2", memory, LENGTHS)
    st1, st2 = o1.initial_state(B, N, F64), o2.initial_state(B, N, F64)
    mem = (o1.keys, o1.values, o2.keys, o2.values, LENGTHS)
    kp = _kernel_params(p, fwd)
    pw = {k: kp[k] for k in ("v1", "b1", "convW", "convb", "locW", "v2")}
    s_prev, a_prev = (st1[0], st1[1]) if fwd else (st1, st1)
    for query in queries:
        ra1, st1 = o1(query, st1)
        ra2, st2 = o2(query, st2)
        q = torch.cat([query @ p["a1/query_layer/kernel"], query @ p["a2/query_layer/kernel"]], 1)
        o = R.step_fwd(q, *mem, s_prev, a_prev, 0.5, **pw, att1_forward=fwd)
        rs = st1[0] if fwd else st1
        for got, ref in ((o.a, ra1), (o.s, rs), (o.s2, ra2),
                         (o.c1, (ra1.unsqueeze(1) @ o1.values).squeeze(1)),
                         (o.c2, (ra2.unsqueeze(1) @ o2.values).squeeze(1))):
            assert float((got - ref).abs().max()) <= 1e-12
        for b, L in enumerate(LENGTHS.tolist()):
            for x in (o.s, o.a, o.s2):
                assert torch.equal(x[b, L:], torch.zeros(N - L, dtype=F64))
            assert bool(torch.isinf(o.e1[b, L:]).all()) and bool(torch.isfinite(o.e1[b, :L]).all())
            assert bool(torch.isinf(o.e2[b, L:]).all())
        assert (o.loc is None) == (not fwd)
        e1v = o.e1.masked_fill(torch.isinf(o.e1), -1e30)
        assert torch.equal(o.stats[:, 0], e1v.max(1).values)
        assert float((o.stats[:, 1] - torch.exp(o.e1 - o.stats[:, :1]).sum(1)).abs().max()) <= 1e-12
        if fwd:
            assert float((o.stats[:, 2] - (o.prior * o.s).sum(1)).abs().max()) <= 1e-15
        else:
            assert float((o.stats[:, 2] - 1.0).abs().max()) <= 1e-12
        assert float((o.stats[:, 3] - torch.exp(o.e2 - o.e2.max(1, keepdim=True).values).sum(1))
                     .abs().max()) <= 1e-12
        s_prev, a_prev = o.s, o.a


@pytest.mark.parametrize("key", sorted(TA.FLAGS))
def test_steps_match_agent_restatement(key):
    """step_fwd with u_prev / u_out / state_out stepped 4 times == transition_agent_ref's
    restatement for each of its three flag sets (1e-12): alignments, state and u_t; with the agent
    on, u_t leaves 0.5 by far more than rounding."""
    from oracle import sat_oracle as O
    agent, cum = key in ("agent", "both"), key in ("cumulative", "both")
    d, g, p, memory, queries = _setup(5)
    B, N = d["B"], d["N"]
    ref = TA.agent_oracle_class(O, agent, cum)(p, "a1", memory, LENGTHS)
    o2 = O.make_attention("additive", p, "a2", memory, LENGTHS)
    rstate = ref.initial_state(B, N, F64)
    mem = (ref.keys, ref.values, o2.keys, o2.values, LENGTHS)
    qs = [torch.cat([x @ p["a1/query_layer/kernel"], x @ p["a2/query_layer/kernel"]], 1)
          for x in queries]
    outs, states = R.chain_fwd(qs, mem, (rstate[0], rstate[1], rstate[2].reshape(B)),
                               _kernel_params(p), agent=agent, cumulative=cum)
    us = []
    for query, o in zip(queries, outs):
        ra, rstate = ref(query, rstate)
        assert float((o.a - ra).abs().max()) <= 1e-12
        assert float(((o.state_out if cum else o.s) - rstate[0]).abs().max()) <= 1e-12
        if agent:
            assert float((o.u_out - rstate[2].reshape(B)).abs().max()) <= 1e-12
            us.append(o.u_out)
        else:
            assert o.u_out is None and torch.equal(rstate[2], 0.5 * torch.ones(B, 1, dtype=F64))
        assert (o.state_out is None) == (not cum)
    if agent:
        us = torch.stack(us)
        assert float(us.max() - us.min()) > 0.05
    # the state each step started from is the previous step's hand-off
    assert torch.equal(states[1][1], outs[0].a)
    assert torch.equal(states[2][0], outs[1].state_out if cum else outs[1].s)


def _chain_case(seed, agent, cum, T=3):
    d, g, p, memory, _ = _setup(seed)
    B, N, D1, D2, M = d["B"], d["N"], d["D1"], d["D2"], d["M"]
    mask = (torch.arange(N).unsqueeze(0) < LENGTHS.unsqueeze(1)).to(F64)
    # keys / values with junk past the lengths: the contract is masked energies, not zero keys
    mem = (_rand(g, B, N, D1), _rand(g, B, N, M), _rand(g, B, N, D2), _rand(g, B, N, 8), LENGTHS)
    qs = [_rand(g, B, D1 + D2) for _ in range(T)]
    s0 = torch.softmax(_rand(g, B, N).masked_fill(mask == 0, float("-inf")), dim=1)
    a0 = torch.softmax(_rand(g, B, N).masked_fill(mask == 0, float("-inf")), dim=1)
    u0 = torch.tensor([0.5, 0.3, 0.8], dtype=F64)
    dctxs = [_rand(g, B, M + 8) for _ in range(T)]
    return qs, mem, (s0, a0, u0), _kernel_params(p), dctxs


@pytest.mark.parametrize("agent,cum", [(False, False), (True, False), (False, True), (True, True)])
def test_chained_step_bwd_matches_end_to_end_autograd(agent, cum):
    """A 3-step float64 chain differentiated end to end (random upstream gradients on every step's
    contexts) against step_bwd / agent_bwd chained in reverse with y, df, ds and du handed from
    step to step: every step's dq, de1, de2 and df agree to 1e-10.  Pins the hand-off conventions
    (u_{t-1} in the prior but u_t in dalpha_t; which step's s multiplies Y; the agent's dz enters
    dctx before the step's own backward) without a GPU.  u_0 differs per utterance and from 0.5."""
    qs, mem, state, par, dctxs = _chain_case(11 + 2 * agent + cum, agent, cum)
    ref = R.chain_grads(qs, mem, state, par, dctxs, agent=agent, cumulative=cum)
    got = R.chain_bwd(qs, mem, state, par, dctxs, agent=agent, cumulative=cum)
    for t in range(len(qs)):
        for name in ("dq", "de1", "de2", "df"):
            x, y = getattr(got, name)[t], getattr(ref, name)[t]
            assert float(y.abs().max()) > 1e-3, (t, name)
            assert float((x - y).abs().max()) <= 1e-10, (t, name)
        for b, L in enumerate(LENGTHS.tolist()):
            assert torch.equal(got.de1[t][b, L:], torch.zeros(45 - L, dtype=F64))
            assert torch.equal(got.de2[t][b, L:], torch.zeros(45 - L, dtype=F64))
    # an earlier step's gradient really carries the later steps' signals
    alone = R.step_bwd(qs[0], *mem, *state, **{k: par[k] for k in
                       ("v1", "b1", "convW", "convb", "locW", "v2")}, dctx=dctxs[0])
    assert float((alone.de1 - ref.de1[0]).abs().max()) > 1e-4


def test_location_conv_transposed_is_the_convolutions_gradient():
    """location_conv_transposed == autograd of location_features, odd and even kernel widths and a
    kernel wider than the row (TF SAME: left = (KW - 1) // 2)."""
    g = torch.Generator().manual_seed(2)
    for KW, N in ((1, 5), (4, 9), (5, 9), (10, 45), (32, 7)):
        s = _rand(g, 2, N).requires_grad_(True)
        W, b, df = _rand(g, KW, 3), _rand(g, 3), _rand(g, 2, N, 3)
        f = R.location_features(s, W, b)
        (f * df).sum().backward()
        assert float((R.location_conv_transposed(df, W) - s.grad).abs().max()) <= 1e-12
        # against the oracle's Conv1D
        from oracle import sat_oracle as O
        ref = O.conv1d_same(s.detach().unsqueeze(-1), W.unsqueeze(1), b)
        assert float((f.detach() - ref).abs().max()) <= 1e-12


def test_agent_bwd_matches_autograd():
    """agent_bwd == autograd of u_t = sigmoid([c1 | q[:D1]] . w + b) for an upstream du."""
    g = torch.Generator().manual_seed(8)
    B, M1, D1, D2 = 3, 12, 32, 32
    c1 = _rand(g, B, M1).requires_grad_(True)
    q = _rand(g, B, D1 + D2).requires_grad_(True)
    w, b, du, dctx = _rand(g, M1 + D1, 1, scale=0.3), _rand(g, 1), _rand(g, B), _rand(g, B, M1 + 4)
    u = torch.sigmoid(torch.cat([c1, q[:, :D1]], 1) @ w.reshape(-1) + b)
    (u * du).sum().backward()
    dz, out, dq_extra = R.agent_bwd(du, u.detach(), w, dctx, M1, D1, D2)
    assert float((out[:, :M1] - dctx[:, :M1] - c1.grad).abs().max()) <= 1e-12
    assert torch.equal(out[:, M1:], dctx[:, M1:])
    assert float((dq_extra - q.grad).abs().max()) <= 1e-12
    assert float((dz - du * u.detach() * (1 - u.detach())).abs().max()) == 0.0


def test_fixtures_are_sensitive():
    """From the float64 reference alone: the location term moves e1 by more than 1e-2 somewhere,
    the alignments are not one-hot, and from the initial state (alpha_0 one-hot at 0, s_0 zero)
    some position n >= 2 inside the length has an alpha that exists only through the 1e-7 floor."""
    qs, mem, state, par, _ = _chain_case(11, False, False)
    pw = {k: par[k] for k in ("v1", "b1", "convW", "convb", "locW", "v2")}
    o = R.step_fwd(qs[0], *mem, *state, **pw)
    flat = R.step_fwd(qs[0], *mem, *state, **dict(pw, locW=torch.zeros_like(pw["locW"])))
    valid = torch.isfinite(o.e1)
    assert float((o.e1 - flat.e1)[valid].abs().max()) > 1e-2
    for x in (o.s, o.a, o.s2):
        assert float(x[:2].max()) < 0.9          # the two utterances longer than a few positions
    B, N = state[0].shape
    s0 = torch.zeros(B, N, dtype=F64)
    a0 = torch.cat([torch.ones(B, 1, dtype=F64), torch.zeros(B, N - 1, dtype=F64)], 1)
    i = R.step_fwd(qs[0], *mem, s0, a0, 0.5, **pw)
    assert torch.equal(i.prior[:, 2:], torch.full((B, N - 2), 1e-7, dtype=F64))
    assert float(i.a[0, 2:45].min()) > 0.0 and float(i.a[0, 2:].max()) < 1e-5
    assert float(i.a[2, 2:7].min()) > 0.0 and torch.equal(i.a[2, 7:], torch.zeros(N - 7, dtype=F64))
    nofloor = ((1 - 0.5) * a0 + 0.5 * R.shift_right(a0)) * i.s
    assert torch.equal(nofloor[:, 2:], torch.zeros(B, N - 2, dtype=F64))
