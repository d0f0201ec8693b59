"""Plain-torch restatement of the per-step dual-source attention kernels (csrc/attention.hip:
sat_attn_step_fwd, sat_attn_step_bwd, sat_attn_agent_bwd) in the kernels' own operand layout,
shared by test_attn_ref_cpu.py (which ties it to the oracle and to autograd of a whole chain) and
test_attn_step_gpu.py.  Dtype-agnostic: float64 operands give the reference, float32 operands the
reference's own float32 error that the GPU tests' bars are made of.

Operands (SatAttnStep): q [B, D1 + D2]; K1 [B, N, D1], V1 [B, N, M1], K2 [B, N, D2], V2 [B, N, M2];
lengths [B]; s_prev, a_prev [B, N]; u a scalar or [B]; v1, b1 [D1] (b1 may be None); convW [KW, F]
(the Conv1D kernel [KW, 1, F]), convb [F], locW [F, D1]; v2 [D2]; agent_w [M1 + D1], agent_b a
scalar, [1] or [B]; cumulative: state_out = s + s_prev.
"""
from types import SimpleNamespace

import torch


def _u_col(u, like):
    """u as a [B, 1] (or broadcastable scalar) tensor of like's dtype."""
    if torch.is_tensor(u):
        return u.to(like.dtype).reshape(-1, 1)
    return torch.tensor(float(u), dtype=like.dtype)


def location_features(s_prev, convW, convb):
    """f[b, n, :] = convb + sum_j s_prev[b, n + j - left] convW[j, :], TF SAME padding:
    left = (KW - 1) // 2 zeros in front, KW - 1 - left behind."""
    KW = convW.shape[0]
    B, N = s_prev.shape
    left = (KW - 1) // 2
    sp = torch.cat([s_prev.new_zeros(B, left), s_prev, s_prev.new_zeros(B, KW - 1 - left)], dim=1)
    f = convb.expand(B, N, -1)
    for j in range(KW):
        f = f + sp[:, j:j + N].unsqueeze(-1) * convW[j]
    return f


def location_conv_transposed(df, convW):
    """dS[b, n] = sum_{j, f} df[b, n - j + left, f] convW[j, f] over the rows inside [0, N): the
    gradient the convolution's input receives from the gradient df [B, N, F] of its output."""
    KW = convW.shape[0]
    B, N, _ = df.shape
    left = (KW - 1) // 2
    dS = df.new_zeros(B, N)
    for j in range(KW):
        w = df @ convW[j]                          # [B, N], row m contributes to n = m + j - left
        sh = j - left
        lo, hi = max(0, -sh), min(N, N - sh)       # rows m with 0 <= m + sh < N
        if hi > lo:
            dS[:, lo + sh:hi + sh] = dS[:, lo + sh:hi + sh] + w[:, lo:hi]
    return dS


def shift_right(a):
    """a[n - 1] with a zero at n = 0."""
    return torch.cat([torch.zeros_like(a[:, :1]), a[:, :-1]], dim=1)


def step_fwd(q, K1, V1, K2, V2, lengths, s_prev, a_prev, u, v1, b1, convW, convb, locW, v2, *,
             att1_forward=True, agent_w=None, agent_b=None, cumulative=False):
    """One attention step.  Returns a namespace with loc (the location features f, None for the
    additive mechanism 1), e1, e2 (-inf past the length), s, a, s2 (exact 0 past the length),
    c1, c2, stats [B, 4] = (max e1, sum exp(e1 - max), sum prior s, sum exp(e2 - max e2)) as the
    combine kernel defines them, u_out (None without agent_w), state_out (None unless cumulative)
    and prior (None for the additive mechanism 1).  Differentiable in every floating operand."""
    B, N, D1 = K1.shape
    mask = torch.arange(N).unsqueeze(0) < lengths.reshape(-1, 1)
    q1, q2 = q[:, :D1], q[:, D1:]
    pre1 = K1 + q1.unsqueeze(1)
    if b1 is not None:
        pre1 = pre1 + b1
    loc = None
    if att1_forward:
        loc = location_features(s_prev, convW, convb)
        if q.requires_grad and not loc.requires_grad:
            loc = loc.requires_grad_(True)         # a graph node even when s_prev is a constant
        pre1 = pre1 + loc @ locW
    ninf = float("-inf")
    e1 = (v1 * torch.tanh(pre1)).sum(-1).masked_fill(~mask, ninf)
    e2 = (v2 * torch.tanh(K2 + q2.unsqueeze(1))).sum(-1).masked_fill(~mask, ninf)
    m1, m2 = e1.max(dim=1, keepdim=True).values, e2.max(dim=1, keepdim=True).values
    p1, p2 = torch.exp(e1 - m1.detach()), torch.exp(e2 - m2.detach())
    z1, z2 = p1.sum(1, keepdim=True), p2.sum(1, keepdim=True)
    s, s2 = p1 / z1, p2 / z2
    prior = None
    if att1_forward:
        uc = _u_col(u, s)
        prior = (1 - uc) * a_prev + uc * shift_right(a_prev) + 1e-7
        at = prior * s
        sa = at.sum(1, keepdim=True)
        a = at / sa
    else:
        a = s
        sa = s.sum(1, keepdim=True)
    c1 = (a.unsqueeze(1) @ V1).squeeze(1)
    c2 = (s2.unsqueeze(1) @ V2).squeeze(1)
    stats = torch.cat([m1, z1, sa, z2], dim=1)
    u_out = None
    if agent_w is not None:
        z = torch.cat([c1, q1], dim=-1) @ agent_w.reshape(-1) + agent_b.reshape(-1)
        u_out = torch.sigmoid(z)
    state_out = s + s_prev if cumulative else None
    return SimpleNamespace(loc=loc, e1=e1, e2=e2, s=s, a=a, s2=s2, c1=c1, c2=c2, stats=stats,
                           u_out=u_out, state_out=state_out, prior=prior)


def upstream(y_next, df_next, ds_next, u_t, convW, like):
    """The signals step t receives from step t + 1, as the ABI comment of SatAttnStepBwd defines
    them: dalpha_t[n] = (1 - u_t) Y[n] + u_t Y[n + 1] (Y[N] = 0) and dS_t = (transposed location
    convolution of df_next) + ds_next; zeros for the operands that are None (the last step)."""
    dalpha = torch.zeros_like(like)
    if y_next is not None:
        uc = _u_col(u_t, like)
        y1 = torch.cat([y_next[:, 1:], torch.zeros_like(y_next[:, :1])], dim=1)
        dalpha = (1 - uc) * y_next + uc * y1
    dS = torch.zeros_like(like)
    if df_next is not None:
        dS = dS + location_conv_transposed(df_next, convW)
    if ds_next is not None:
        dS = dS + ds_next
    return dalpha, dS


def step_bwd(q, K1, V1, K2, V2, lengths, s_prev, a_prev, u, v1, b1, convW, convb, locW, v2, *,
             dctx, y_next=None, df_next=None, ds_next=None, u_t=None, att1_forward=True):
    """One reverse step: autograd of dctx . [c1 | c2] + dalpha . a + dS . s through step_fwd.
    ``u`` is the factor the forward step used (u_{t-1}), ``u_t`` the one step t + 1 used (None:
    the same).  Returns de1, de2 (gradients at the masked energies), df_out (at the location
    features), y_out (at the prior), dq [B, D1 + D2] (the kernel's dqp summed over its tile rows),
    du [B] (dup summed over tiles) and ds_out = dS.  For the additive mechanism 1 there is no
    recursion: y_next / df_next / ds_next are not read and df_out, y_out, du are None."""
    q = q.detach().clone().requires_grad_(True)
    ut = None
    if att1_forward:
        ut = (u.detach().clone() if torch.is_tensor(u) else
              torch.full((q.shape[0],), float(u), dtype=q.dtype)).requires_grad_(True)
    o = step_fwd(q, K1, V1, K2, V2, lengths, s_prev, a_prev, ut, v1, b1, convW, convb, locW, v2,
                 att1_forward=att1_forward)
    loss = (dctx * torch.cat([o.c1, o.c2], dim=-1)).sum()
    dS = None
    if att1_forward:
        dalpha, dS = upstream(y_next, df_next, ds_next, u if u_t is None else u_t, convW, o.s)
        loss = loss + (dalpha * o.a).sum() + (dS * o.s).sum()
        de1, de2, dq, df, y, du = torch.autograd.grad(loss, [o.e1, o.e2, q, o.loc, o.prior, ut])
    else:
        de1, de2, dq = torch.autograd.grad(loss, [o.e1, o.e2, q])
        df = y = du = None
    return SimpleNamespace(de1=de1, de2=de2, df_out=df, y_out=y, dq=dq, du=du, ds_out=dS)


def agent_bwd(du, u_t, agent_w, dctx, M1, D1, D2):
    """sat_attn_agent_bwd: dz = du u_t (1 - u_t) with du [B] the tile sum of dup; returns dz [B],
    the context gradient with dz agent_w[:M1] added to its first M1 columns, and the extra query
    gradient row [dz agent_w[M1:] | 0 (D2)]."""
    w = agent_w.reshape(-1)
    dz = du * u_t * (1 - u_t)
    out = dctx.clone()
    out[:, :M1] = out[:, :M1] + dz.unsqueeze(1) * w[:M1]
    dq_extra = torch.cat([dz.unsqueeze(1) * w[M1:M1 + D1], dctx.new_zeros(dctx.shape[0], D2)], 1)
    return dz, out, dq_extra


# ------------------------------------------------------------------------------ a T-step chain

def chain_fwd(qs, mem, state, par, *, agent=False, cumulative=False):
    """T chained steps.  qs: list of q_t; mem = (K1, V1, K2, V2, lengths); state = (S_0, alpha_0,
    u_0 [B]); par = dict(v1, b1, convW, convb, locW, v2[, agent_w, agent_b]).  Returns the list of
    step outputs and the list of the states each step started from."""
    outs, states = [], []
    S, al, u = state
    pw = {k: par[k] for k in ("v1", "b1", "convW", "convb", "locW", "v2")}
    for q in qs:
        states.append((S, al, u))
        o = step_fwd(q, *mem, S, al, u, **pw, cumulative=cumulative,
                     agent_w=par["agent_w"] if agent else None,
                     agent_b=par["agent_b"] if agent else None)
        outs.append(o)
        S, al = (o.state_out if cumulative else o.s), o.a
        u = o.u_out if agent else u
    return outs, states


def chain_grads(qs, mem, state, par, dctxs, *, agent=False, cumulative=False):
    """End-to-end autograd of sum_t dctxs[t] . [c1_t | c2_t] through chain_fwd: per step the
    gradients at q_t, e1_t, e2_t and f_t (lists of T tensors each)."""
    qs = [q.detach().clone().requires_grad_(True) for q in qs]
    outs, _ = chain_fwd(qs, mem, state, par, agent=agent, cumulative=cumulative)
    loss = sum((g * torch.cat([o.c1, o.c2], dim=-1)).sum() for g, o in zip(dctxs, outs))
    T = len(qs)
    grads = torch.autograd.grad(loss, qs + [o.e1 for o in outs] + [o.e2 for o in outs] +
                                [o.loc for o in outs])
    return SimpleNamespace(dq=grads[:T], de1=grads[T:2 * T], de2=grads[2 * T:3 * T],
                           df=grads[3 * T:], outs=outs)


def chain_bwd(qs, mem, state, par, dctxs, *, agent=False, cumulative=False):
    """The same gradients from step_bwd / agent_bwd chained in reverse, handing y, df, ds and du
    from step t + 1 to step t exactly as the decoder's reverse loop hands the kernels' outputs."""
    with torch.no_grad():
        outs, states = chain_fwd(qs, mem, state, par, agent=agent, cumulative=cumulative)
    T = len(qs)
    K1, V1, K2, V2, lengths = mem
    M1, D1, D2 = V1.shape[-1], K1.shape[-1], K2.shape[-1]
    pw = {k: par[k] for k in ("v1", "b1", "convW", "convb", "locW", "v2")}
    res = SimpleNamespace(dq=[None] * T, de1=[None] * T, de2=[None] * T, df=[None] * T)
    y = df = ds = None
    du = torch.zeros_like(states[0][2])
    for t in reversed(range(T)):
        S, al, u = states[t]
        u_next = outs[t].u_out if agent else u          # the factor step t + 1 used
        dctx, dq_extra = dctxs[t], 0.0
        if agent:
            _, dctx, dq_extra = agent_bwd(du, u_next, par["agent_w"], dctx, M1, D1, D2)
        r = step_bwd(qs[t], *mem, S, al, u, **pw, dctx=dctx, y_next=y, df_next=df,
                     ds_next=ds if cumulative else None, u_t=u_next)
        res.dq[t], res.de1[t], res.de2[t], res.df[t] = r.dq + dq_extra, r.de1, r.de2, r.df_out
        y, df, ds, du = r.y_out, r.df_out, r.ds_out, r.du
    return res
