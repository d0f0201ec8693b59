"""sat_attn_param_grads (the attention parameter gradients summed over every decoder step,
modules/forward_attention.py:16-23, 68-122 and TF BahdanauAttention's memory / score variables)
against a torch fp64 restatement (energies recomputed from K, q and the location features), for
every compiled variant of the kernel -- <1,5>, <1,0>, <2,0>, <2,8> -- and what its entry accepts
or refuses.

Tolerance: 2e-5 * scale * max(1, sqrt(T / 32)) per output, scale = its largest reference
magnitude.  It was set for the kernel's fast exp2 / rcp form of tanh on the LJSpeech shape and is
used unchanged for the other instantiations of the same body."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _case(T, B, N, D1=224, D2=32, F=5, KW=10, seed=0):
    """F = 0: the additive first mechanism, without b1 / locW / loc / s_prev / df."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    c = dict(K1=r(B, N, D1) * 0.5, K2=r(B, N, D2) * 0.5, q=r(T, B, D1 + D2) * 0.5,
             v1=r(D1), v2=r(D2), de1=r(T, B, N), de2=r(T, B, N))
    if F > 0:
        c.update(b1=r(D1) * 0.1, locW=r(F, D1) * 0.3, loc=r(T, B, N, F),
                 s_prev=torch.rand(T, B, N, generator=g), df=r(T, B, N, F))
    return c


def _reference(c, D1, F, KW):
    d = {k: v.double() for k, v in c.items()}
    x1 = d["K1"][None] + d["q"][:, :, None, :D1]
    if F > 0:
        x1 = x1 + d["b1"] + torch.einsum("tbnf,fd->tbnd", d["loc"], d["locW"])
    z1 = torch.tanh(x1)
    z2 = torch.tanh(d["K2"][None] + d["q"][:, :, None, D1:])
    dp1 = d["de1"][..., None] * d["v1"] * (1 - z1 * z1)
    dp2 = d["de2"][..., None] * d["v2"] * (1 - z2 * z2)
    out = dict(dK1=dp1.sum(0), dK2=dp2.sum(0),
               dv1=(z1 * d["de1"][..., None]).sum((0, 1, 2)),
               dv2=(z2 * d["de2"][..., None]).sum((0, 1, 2)))
    if F == 0:
        return out, z1, z2
    out["dWloc"] = torch.einsum("tbnf,tbnd->fd", d["loc"], dp1)
    # dconvW[j][f] = sum s_{t-1}[n + j - padl] df_t[n][f]; dconvb[f] = sum df_t[n][f]
    T, B, N = d["de1"].shape
    padl = (KW - 1) // 2
    sp = torch.nn.functional.pad(d["s_prev"], (padl, KW - 1 - padl))
    win = torch.stack([sp[..., j:j + N] for j in range(KW)], -1)          # [T, B, N, KW]
    out["dconvW"] = torch.einsum("tbnj,tbnf->jf", win, d["df"])
    out["dconvb"] = d["df"].sum((0, 1, 2))
    return out, z1, z2


def _padded(x, lead, strides, cuda):
    """x on the device as a view whose ``lead`` leading dims have the given element strides
    (the trailing dims dense); the storage between the rows is NaN."""
    inner = x[(0,) * lead].numel()
    size = sum((n - 1) * s for n, s in zip(x.shape[:lead], strides)) + inner
    buf = torch.full((size,), float("nan"), device=cuda)
    tail = list(x.shape[lead:])
    dense, k = [], 1
    for n in reversed(tail):
        dense.insert(0, k)
        k *= n
    view = buf.as_strided(list(x.shape), list(strides) + dense)
    view.copy_(x)
    return buf, view


def _launch(cuda, c, T, B, N, D1, D2, F, KW, ts, nondense=False, pg_extra=0):
    """Run the entry on NaN-prefilled outputs; returns the named gradients in float64 on the
    host, the raw partial rows, the device inputs and their clones from before the call."""
    from sat_amd import kernels as K
    dv = {k: v.to(cuda).contiguous() for k, v in c.items()}
    bufs = dict(dv)
    s_ts = B * N
    if nondense:
        qs1 = D1 + D2 + 8
        bufs["q"], dv["q"] = _padded(c["q"], 2, (B * qs1 + 16, qs1), cuda)
        if F > 0:
            s_ts = B * N + 12
            bufs["s_prev"], dv["s_prev"] = _padded(c["s_prev"], 1, (s_ts,), cuda)
    before = {k: v.clone() for k, v in bufs.items()}
    pgmin = K.pg_stride(D1, D2, F, KW)
    assert pgmin == (D1 + F * D1 + KW * F + F + D2 + 3) // 4 * 4
    pgs = pgmin + pg_extra
    parts = max(ts, 1)
    PG = torch.full((parts * K.attn_param_grad_rows(B, N), pgs), float("nan"), device=cuda)
    dK1s = torch.full((parts, B, N, D1), float("nan"), device=cuda)
    dK2s = torch.full((parts, B, N, D2), float("nan"), device=cuda)
    q = dv["q"]
    K.attn_param_grads(
        T=T, B=B, N=N, D1=D1, D2=D2, F=F, KW=KW, att1_forward=1 if F > 0 else 0, K1=dv["K1"],
        K2=dv["K2"], q=q, q_tstride=q.stride(0), q_bstride=q.stride(1), b1=dv.get("b1"),
        v1=dv["v1"], locW=dv.get("locW"), v2=dv["v2"], loc=dv.get("loc"),
        s_prev=dv.get("s_prev"), s_tstride=s_ts, de1=dv["de1"], de2=dv["de2"], df=dv.get("df"),
        dK1=dK1s, dK2=dK2s, pg=PG, pg_stride=pgs, tsplit=ts)
    torch.cuda.synchronize()
    PG = PG.double().cpu()
    pg = PG.sum(0)
    o = 0
    got = {}
    # pg layout: [dv1 | dWloc | dconvW | dconvb | dv2], F = 0: [dv1 | dv2]
    for name, n in (("dv1", D1), ("dWloc", F * D1), ("dconvW", KW * F), ("dconvb", F),
                    ("dv2", D2)):
        if n:
            got[name] = pg[o:o + n]
        o += n
    if F > 0:
        got["dWloc"] = got["dWloc"].view(F, D1)
        got["dconvW"] = got["dconvW"].view(KW, F)
    got["dK1"], got["dK2"] = dK1s[0].double().cpu(), dK2s[0].double().cpu()
    return got, PG, bufs, before


def _check(got, ref, T):
    assert set(got) == set(ref)
    for k, want in ref.items():
        assert got[k].shape == want.shape, k
        err = float((got[k] - want).abs().max())      # NaN (an unwritten element) fails too
        scale = float(want.abs().max()) + 1e-12
        print(f"{k}: err {err:.3e} scale {scale:.3e} rel {err / scale:.2e}")
        assert err <= 2e-5 * scale * max(1.0, (T / 32) ** 0.5), (k, err, scale)


@pytest.mark.parametrize("T,B,N,ts", [(7, 2, 13, 1), (33, 3, 200, 1), (500, 2, 61, 1),
                                      (7, 2, 13, 3), (33, 3, 200, 2), (500, 2, 61, 4),
                                      (5, 1, 9, 5)])
def test_attn_param_grads(cuda, T, B, N, ts):
    """sat_attn_param_grads against float64 autograd, unsplit and with the T steps split into
    ts ranges (tsplit; T = ts: one step per range)."""
    D1, D2, F, KW = 224, 32, 5, 10
    c = _case(T, B, N, D1, D2, F, KW, seed=T + N)
    ref, _, _ = _reference(c, D1, F, KW)
    got, _, _, _ = _launch(cuda, c, T, B, N, D1, D2, F, KW, ts)
    _check(got, ref, T)


A, C = (7, 2, 13, 1), (33, 2, 70, 2)
VARIANTS = (
    # <1,0>: the additive first mechanism (att1_forward = 0), D1 + D2 <= 256
    [(d, s) for d in ((64, 32, 0, 0), (224, 32, 0, 0)) for s in (A, (9, 3, 5, 8), (1, 1, 1, 0))] +
    # <2,0>: two column slots per lane (D1 + D2 > 256)
    [(d, s) for d in ((256, 64, 0, 0), (448, 64, 0, 0)) for s in (A, C)] +
    # <2,8> with one live slot: F = 8 at D1 + D2 <= 256 (the second slot is all padding)
    [(d, s) for d in ((224, 32, 8, 7), (32, 32, 8, 1)) for s in (A, (5, 1, 9, 5))] +
    # <2,8> with both slots, KW * F + F = 64 conv lanes: all of a wave
    [((256, 64, 8, 7), s) for s in ((7, 2, 13, 3), (33, 2, 70, 1))] +
    # <1,5> edges: KW 1 and 11 (60 conv lanes), N < KW, N = 1, ranges of 1 and 2 steps, T = 1
    [((224, 32, 5, 1), (5, 2, 13, 2)), ((224, 32, 5, 1), (9, 1, 6, 0)),
     ((224, 32, 5, 11), (9, 2, 13, 8)), ((224, 32, 5, 11), (1, 1, 13, 0)),
     ((224, 32, 5, 10), (9, 2, 3, 8)), ((224, 32, 5, 10), (5, 3, 3, 2)),
     ((224, 32, 5, 10), (1, 1, 1, 0)), ((224, 32, 5, 10), (5, 2, 1, 2))])


@pytest.mark.parametrize("dims,shape", VARIANTS,
                         ids=["D{}+{}-F{}-KW{}-T{}-B{}-N{}-ts{}".format(*d, *s)
                              for d, s in VARIANTS])
def test_attn_param_grads_variants(cuda, dims, shape):
    """Every compiled variant against float64.  tsplit 0 and 1 are unsplit; 8 over T = 9 gives
    ranges of 1 and 2 steps, 2 over T = 5 ranges of 2 and 3, so the 4-step unroll's tail runs
    with 1, 2 and 3 live steps; T = 33 / ts 1 runs whole unrolls plus a tail of 1."""
    (D1, D2, F, KW), (T, B, N, ts) = dims, shape
    c = _case(T, B, N, D1, D2, F, KW, seed=D1 + F + T + N)
    ref, _, _ = _reference(c, D1, F, KW)
    got, _, _, _ = _launch(cuda, c, T, B, N, D1, D2, F, KW, ts)
    _check(got, ref, T)


@pytest.mark.parametrize("dims", [(224, 32, 5, 10), (256, 64, 8, 7), (224, 32, 0, 0)],
                         ids=lambda d: "D{}+{}-F{}-KW{}".format(*d))
def test_attn_param_grads_nondense(cuda, dims):
    """q as a view with padded batch and step strides, s_prev with a padded step stride (NaN
    between the rows: a read outside a row shows), pg_stride 8 above the minimum.  Same float64
    reference; the extra pg columns are exactly 0 in every partial row; no input is written."""
    D1, D2, F, KW = dims
    T, B, N, ts = 7, 2, 13, 3
    c = _case(T, B, N, D1, D2, F, KW, seed=3 + D1)
    ref, _, _ = _reference(c, D1, F, KW)
    got, PG, bufs, before = _launch(cuda, c, T, B, N, D1, D2, F, KW, ts, nondense=True,
                                    pg_extra=8)
    _check(got, ref, T)
    assert PG.shape[1] == (D1 + F * D1 + KW * F + F + D2 + 3) // 4 * 4 + 8
    assert bool((PG[:, -8:] == 0).all())
    for k, v in bufs.items():
        assert torch.equal(v.view(torch.int32), before[k].view(torch.int32)), k


def _refusal_args(cuda, T=16, B=2, N=13, D1=224, D2=32, F=5, KW=10, D1a=None, D2a=None):
    """A valid call's kwargs over buffers allocated for (D1a, D2a) >= (D1, D2)."""
    from sat_amd import kernels as K
    D1a, D2a = D1a or D1, D2a or D2
    z = lambda *s: torch.zeros(*s, device=cuda)   # noqa: E731
    nan = lambda *s: torch.full(s, float("nan"), device=cuda)   # noqa: E731
    pgs = K.pg_stride(D1a, D2a, 8, 8)
    return dict(T=T, B=B, N=N, D1=D1, D2=D2, F=F, KW=KW, att1_forward=1, K1=z(B, N, D1a),
                K2=z(B, N, D2a), q=z(T, B, D1a + D2a), q_tstride=B * (D1 + D2),
                q_bstride=D1 + D2, b1=z(D1a), v1=z(D1a), locW=z(8, D1a), v2=z(D2a),
                loc=z(T, B, N, 8), s_prev=z(T, B, N), s_tstride=B * N, de1=z(T, B, N),
                de2=z(T, B, N), df=z(T, B, N, 8), dK1=nan(8, B, N, D1a), dK2=nan(8, B, N, D2a),
                pg=nan(8 * K.attn_param_grad_rows(B, N), pgs), pg_stride=K.pg_stride(D1, D2, F, KW),
                tsplit=1)


@pytest.mark.parametrize("change,match", [
    (dict(D1=256, D2=32, q_tstride=2 * 288, q_bstride=288, pg_stride=2048), "F must be"),
    (dict(F=3), "F must be"),
    (dict(KW=12, pg_stride=2048), "KW\\*F"),
    (dict(tsplit=9), "tsplit"),
    (dict(T=3, tsplit=4), "tsplit"),
    (dict(D1=222), "multiples of 4"),
    (dict(q_bstride=257), "aligned"),
    (dict(pg_stride=1428), "pg stride"),
    (dict(loc=None), "histories"),
    (dict(D1=448, D2=64, F=8, KW=7, q_tstride=2 * 512, q_bstride=512, pg_stride=4160), "LDS"),
])
def test_attn_param_grads_refusals(cuda, change, match):
    """What the entry cannot run it refuses with SAT_ERR_ARGUMENT before any launch (outputs
    keep their NaN prefill).  The last case fits every other rule but would need 4 * 4160 * 4 =
    66,560 bytes of dynamic LDS, above the 64 KB a launch may ask for."""
    from sat_amd import _lib, kernels as K
    kw = _refusal_args(cuda, D1a=448, D2a=64)
    K.attn_param_grads(**kw)                            # the base call itself is accepted
    torch.cuda.synchronize()
    assert bool(torch.isfinite(kw["dK1"].flatten()[:2 * 13 * 224]).all())
    for k in ("dK1", "dK2", "pg"):
        kw[k].fill_(float("nan"))
    assert K.pg_stride(224, 32, 5, 10) == 1432 and K.pg_stride(448, 64, 8, 7) == 4160
    kw.update(change)
    with pytest.raises(_lib.SatLibraryError, match=match) as e:
        K.attn_param_grads(**kw)
    assert e.value.rc == _lib.SAT_ERR_ARGUMENT
    torch.cuda.synchronize()
    for k in ("dK1", "dK2", "pg"):
        assert bool(torch.isnan(kw[k]).all()), k


def test_attn_param_grads_lds_limit_is_the_bound(cuda):
    """pg_stride 4096 (4 * 4096 * 4 bytes = 64 KB exactly) is the largest accepted and runs;
    4100 is refused."""
    from sat_amd import _lib, kernels as K
    D1, D2, F, KW, T, B, N = 224, 32, 5, 10, 5, 1, 5
    c = _case(T, B, N, D1, D2, F, KW, seed=1)
    ref, _, _ = _reference(c, D1, F, KW)
    got, PG, _, _ = _launch(cuda, c, T, B, N, D1, D2, F, KW, 1, pg_extra=4096 - 1432)
    assert PG.shape[1] == 4096 and bool((PG[:, 1432:] == 0).all())
    _check(got, ref, T)
    with pytest.raises(_lib.SatLibraryError, match="LDS"):
        _launch(cuda, c, T, B, N, D1, D2, F, KW, 1, pg_extra=4100 - 1432)
