"""Plain-torch restatement of the decoder's whole attention chain over T' steps, in the operand
layout of SatDecAttnFwd / SatDecAttnBwd (include/sat_abi.h), composed from the tree's two step
references: lstm_ref.step (the zoneout attention RNN) and attn_ref.step_fwd (the dual-source
step, scalar u, no transition agent, no cumulative state).  Dtype-agnostic: float64 operands give
the reference, float32 operands the reference's own float32 error.  Shared by
test_attn_chain_ref_cpu.py (which ties it to the oracle's decoder) and test_attn_chain_gpu.py.

Per step t (decoder.py's per-step branch is the authority on the wiring):
    rows   = REC0[t] = [c1_{t-1} | c2_{t-1} | h0_{t-1}]         (row 0: the caller's initial state)
    h0'_t, c0_t, h0_t, gates = zoneout LSTM(X0[t], rows, W0r, C0[t], h0_{t-1})
    q_t    = h0'_t @ [Wq1 | Wq2]                                 (the RAW output, not the state)
    s_t, alpha_t, s2_t, c1_t, c2_t = attention step(q_t, S1[t], AL1[t])
    REC0[t+1] = [c1_t | c2_t | h0_t],  C0[t+1] = c0_t,  S1[t+1] = s_t,  AL1[t+1] = alpha_t
"""
from types import SimpleNamespace

import torch

import attn_ref as A
import lstm_ref as L

PAR = ("v1", "b1", "convW", "convb", "locW", "v2")


def chain(X0, W0r, Wq1, Wq2, mem, s0, a0, rec0, c0, par, masks, zc, zh, u=0.5):
    """All T' steps.

    ``X0`` [T][B][4U] (the hoisted input projection + bias, gate-interleaved [U][4]); ``W0r``
    [M1+M2+U][U][4] (or [.][4U]), rows [c1 | c2 | h0]; ``Wq1`` [U][D1], ``Wq2`` [U][D2]; ``mem`` =
    (K1 [B][N][D1], V1 [B][N][M1], K2 [B][N][D2], V2 [B][N][M2], lengths [B]); ``s0``, ``a0``
    [B][N] (row 0 of S1 / AL1); ``rec0`` [B][M1+M2+U], ``c0`` [B][U] (row 0 of REC0 / C0);
    ``par``: v1, b1 [D1], convW [KW][F], convb [F], locW [F][D1], v2 [D2]; ``masks`` None (eval
    blend) or (mask_c, mask_h) each [T][B][U].

    Returns the histories the forward entry writes -- REC0 [T+1][B][M1+M2+U], C0 [T+1][B][U],
    H0RAW [T][B][U], G0 [T][B][4U], Q [T][B][D1+D2], S1, AL1 [T+1][B][N], S2 [T][B][N],
    ST [T][B][4] = (max e1, sum exp(e1 - max), sum prior s, sum exp(e2 - max e2)), LOC
    [T][B][N][F], ZH [T][B][N][D1+D2] (tanh of both energy pre-activations, every position) --
    with PRE [T][B][4U], the attention RNN's gate pre-activations (not a kernel output) --
    and, for autograd, the per-step graph tensors ``ctx`` ([c1_t | c2_t]), ``q``, ``e1``, ``e2``,
    ``loc`` (lists of T).  Differentiable in every floating operand."""
    T, B, G4 = X0.shape
    U = G4 // 4
    K1, V1, K2, V2, lengths = mem
    D1 = K1.shape[-1]
    C = V1.shape[-1] + V2.shape[-1]
    W = W0r.reshape(C + U, U, 4)
    Wq = torch.cat([Wq1, Wq2], dim=1)
    pw = {k: par[k] for k in PAR}
    rec, cs, s1, al = [rec0], [c0], [s0], [a0]
    raw, g0, qs, s2, st, loc, zh_, ctx, e1, e2, pre = ([] for _ in range(11))
    for t in range(T):
        rows = rec[-1]
        mc = None if masks is None else masks[0][t]
        mh = None if masks is None else masks[1][t]
        hn, c, h, gates, p_ = L.step(X0[t].reshape(B, U, 4), rows, W, cs[-1], rows[:, C:], mc, mh,
                                    zc, zh)
        q = hn @ Wq
        o = A.step_fwd(q, K1, V1, K2, V2, lengths, s1[-1], al[-1], u, **pw)
        pre1 = K1 + q[:, :D1].unsqueeze(1) + par["b1"] + o.loc @ par["locW"]
        pre2 = K2 + q[:, D1:].unsqueeze(1)
        c12 = torch.cat([o.c1, o.c2], dim=-1)
        rec.append(torch.cat([c12, h], dim=-1)), cs.append(c), s1.append(o.s), al.append(o.a)
        raw.append(hn), g0.append(gates.reshape(B, G4)), qs.append(q), s2.append(o.s2)
        st.append(o.stats), loc.append(o.loc)
        zh_.append(torch.tanh(torch.cat([pre1, pre2], dim=-1)))
        ctx.append(c12), e1.append(o.e1), e2.append(o.e2), pre.append(p_.reshape(B, G4))
    sk = torch.stack
    return SimpleNamespace(REC0=sk(rec), C0=sk(cs), H0RAW=sk(raw), G0=sk(g0), Q=sk(qs), S1=sk(s1),
                           AL1=sk(al), S2=sk(s2), ST=sk(st), LOC=sk(loc), ZH=sk(zh_), PRE=sk(pre),
                           ctx=ctx, q=qs, e1=e1, e2=e2, loc=loc)


def chain_grads(X0, W0r, Wq1, Wq2, mem, s0, a0, rec0, c0, par, masks, zc, zh, DH0, RD_in, u=0.5):
    """Autograd of sum(H0RAW . DH0) + sum_t ctx_t . RD_in[t] through ``chain``: what
    sat_decoder_attention_bwd hands the post-loop parameter-gradient pass (backward.py).
    DG0 [T][B][4U] (at X0, i.e. at the gate pre-activations), DCTX [T][B][M1+M2] (the FULL
    dL/dctx_t: RD_in[t] plus what step t+1's attention RNN sends back), DE1, DE2 [T][B][N] (at
    the masked energies: 0 past the length), DFH [T][B][N][F] (at the location features), DQP
    [T][B][D1+D2] (at q_t, fully reduced).  Returns (forward namespace, dict of gradients)."""
    X0 = X0.detach().clone().requires_grad_(True)
    o = chain(X0, W0r, Wq1, Wq2, mem, s0, a0, rec0, c0, par, masks, zc, zh, u)
    T = X0.shape[0]
    loss = (o.H0RAW * DH0).sum() + sum((c * RD_in[t]).sum() for t, c in enumerate(o.ctx))
    g = torch.autograd.grad(loss, [X0] + o.ctx + o.e1 + o.e2 + o.loc + o.q)
    sk = lambda k: torch.stack(g[1 + k * T:1 + (k + 1) * T])          # noqa: E731
    return o, dict(DG0=g[0], DCTX=sk(0), DE1=sk(1), DE2=sk(2), DFH=sk(3), DQP=sk(4))
