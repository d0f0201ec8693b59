"""sat_attn_step_fwd / sat_attn_step_bwd / sat_attn_agent_bwd (csrc/attention.hip) against
tests/attn_ref.py in float64, kernel by kernel, away from the presets' single shape.

Buffers.  Every operand the kernels write lives in a NaN-filled buffer with 4 guard floats on each
side whose padding must still be NaN afterwards; q, ctx, dctx and ctx_t are column blocks of wider
NaN rows (q_sb > D1 + D2, ctx_sb / dctx_sb > M1 + M2).  Keys and values past an utterance's
length hold finite non-zero junk: the contract is masked energies, not zero keys.

The bar.  For each output tensor the kernel's largest absolute error against the float64 reference
must be at most 8 x the largest absolute error of the same reference evaluated in float32 (the
factor test_encoder_lstm_gpu.py uses), with a floor of 1e-7 x the tensor's largest magnitude so
that an exactly representable reference does not make the bar zero.  The backward is fed the
float64 reference's forward state rounded to float32, so a backward failure cannot hide behind a
forward one.  The largest err / bar each test function has shown on an MI355X is in its docstring.

Exact: s, a, s2, y_out, de1, de2 are 0 past the lengths; e1, e2 are -inf there; optional outputs
of a mechanism that does not have them (loc_out, y_out, df_out of the additive mechanism 1) are
never written.

Forward kernels (12 tile kernels + 2 combine kernels) -> cases of FWD_CASES that run them:
  attn_energy_wide_kernel<5,16,true>        preset, preset-init, w5x16-full, nostats
  attn_energy_wide_kernel<5,32,true>        w5x32-d96, w5x32-n512
  attn_energy_wide_kernel<8,16,true>        w8-f1, w8-f3, w8-f8-n1, w8-f3-lpp32
  attn_energy_wide_kernel<0,16,false>       add-preset, add-lpp32, add-nob1
  attn_energy_kernel<5,7,1,true>            n5-preset, n5-b8
  attn_energy_kernel<8,8,2,true>            n8-f3, n8-f5-d256, n8-f5-d2x64, n8-f8, n8-f1
  attn_energy_kernel<0,8,2,false>           nadd-d96, nadd-d256
  attn_energy_wide_kernel<5,16,true,true>   ub-preset, ub-b8
  attn_energy_wide_kernel<5,32,true,true>   ub-w5x32
  attn_energy_wide_kernel<8,16,true,true>   ub-w8-f3, ub-w8-f8
  attn_energy_kernel<5,7,1,true,true>       ub-n5
  attn_energy_kernel<8,8,2,true,true>       ub-n8-f1, ub-n8-f5
  attn_combine_kernel<false>                every case without u_prev / u_out / state_out
  attn_combine_kernel<true>                 every ub-* case, agent-scalar-u, cum-scalar-u
Each tile kernel runs at least once with a ragged last tile (N % 32 != 0) and once with D1 < 256.
Backward: test_step_bwd is the product {(8,4), (16,4), (16,8), (16,16), (32,4), (32,8), (32,16)}
(NT, waves; waves = 0 is 16 and is what the (.,16) cases pass for NT = 16 / 32 in half the cases)
x F in {0, 1, 3, 5, 8} x {plain, EXT} x {last, inner step}: attn_bwd_kernel<NT, F, waves> and
attn_bwd_kernel<NT, F, waves, true>, over the rotating dimension sets of BWD_DIMS.
"""
import math

import pytest
import torch

import attn_ref as R

pytestmark = pytest.mark.gpu

NAN = float("nan")
FLOAT_OPS = ("q", "K1", "V1", "K2", "V2", "s_prev", "a_prev", "v1", "b1", "convW", "convb", "locW",
             "v2")
ORDER = ("q", "K1", "V1", "K2", "V2", "lengths", "s_prev", "a_prev", "u", "v1", "b1", "convW",
         "convb", "locW", "v2")


def _note(name, ratio):
    print(f"RATIO {name} {ratio:.4f}")


class Buf:
    """A float32 operand inside a NaN-filled buffer: contiguous with 4 guard floats on each side,
    or (``strided``) a [B, n] column block at column 4 of a [B, roundup(n, 4) + 8] buffer."""

    def __init__(self, dev, shape, data=None, strided=False):
        self.strided, self.shape = strided, tuple(shape)
        if strided:
            B, n = shape
            self.buf = torch.full((B, (n + 3) // 4 * 4 + 8), NAN, device=dev)
            self.sb = self.buf.shape[1]
        else:
            self.n = math.prod(shape)
            self.buf = torch.full(((self.n + 3) // 4 * 4 + 8,), NAN, device=dev)
        self.v = self._view(self.buf)
        if data is not None:
            self.v.copy_(data.to(torch.float32))
        assert self.v.data_ptr() % 16 == 0

    def _view(self, buf):
        if self.strided:
            return buf[:, 4:4 + self.shape[1]]
        return buf[4:4 + self.n].view(self.shape)

    def intact(self):
        c = self.buf.clone()
        self._view(c).fill_(NAN)
        return bool(torch.isnan(c).all())

    def untouched(self):
        return bool(torch.isnan(self.buf).all())

    def cpu(self):
        return self.v.double().cpu()


def _bar(r32, r64):
    return max(8.0 * float((r32.double() - r64).abs().max()), 1e-7 * float(r64.abs().max()))


def _ratio(got, r64, r32):
    """max |got - r64| / bar; an all-zero reference must be met exactly."""
    assert got.shape == r64.shape, (got.shape, r64.shape)
    assert bool(torch.isfinite(got).all())
    err, bar = float((got - r64).abs().max()), _bar(r32, r64)
    return 0.0 if err == 0.0 else (err / bar if bar > 0.0 else float("inf"))


def _lengths(B, N):
    """N itself, a tile boundary, 1 and mid-tile values, as far as B and N allow."""
    cand = [N, min(32, N), min(7, N), 1, max(1, N - 5), min(N, 33), max(1, N // 2), min(N, 17)]
    return torch.tensor(cand[:B], dtype=torch.int64)


def make_inputs(seed, B, N, D1, D2, M1, M2, F, KW, *, fwd=True, lengths=None, init=False,
                per_u=False, agent=None, nob1=False):
    """float32-valued operands of one step on the CPU (the float64 reference sees the same
    values).  agent: None, or agent_b_sb (0: one bias, 1: a bias per utterance)."""
    g = torch.Generator().manual_seed(seed)
    f = lambda *s, scale=1.0: (scale * torch.randn(*s, generator=g)).float()   # noqa: E731
    lengths = _lengths(B, N) if lengths is None else torch.tensor(lengths, dtype=torch.int64)
    mask = torch.arange(N).unsqueeze(0) < lengths.unsqueeze(1)

    def dist():
        return torch.softmax(f(B, N, scale=1.5).masked_fill(~mask, float("-inf")), dim=1)

    d = dict(q=f(B, D1 + D2), K1=f(B, N, D1, scale=0.5), V1=f(B, N, M1), K2=f(B, N, D2, scale=0.5),
             V2=f(B, N, M2), lengths=lengths, s_prev=dist(), a_prev=dist(),
             v1=f(D1, scale=2.5 / math.sqrt(D1)), b1=f(D1, scale=0.2), convW=f(KW, F, scale=0.5),
             convb=f(F, scale=0.2), locW=f(F, D1, scale=0.5), v2=f(D2, scale=2.5 / math.sqrt(D2)))
    d["u"] = (0.1 + 0.8 * torch.rand(B, generator=g)).float() if per_u else 0.3
    if init:
        d["s_prev"] = torch.zeros(B, N)
        d["a_prev"] = torch.cat([torch.ones(B, 1), torch.zeros(B, N - 1)], 1)
    if nob1 or (not fwd and seed % 2):
        d["b1"] = None
    if agent is not None:
        d["agent_w"] = f(M1 + D1, scale=0.1)
        d["agent_b"] = f(B if agent else 1, scale=0.3)
    return d


def cast(d, dtype):
    return {k: v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v
            for k, v in d.items()}


def ref_fwd(d, dtype, fwd, cum):
    c = cast(d, dtype)
    return R.step_fwd(*[c[k] for k in ORDER], att1_forward=fwd, agent_w=c.get("agent_w"),
                      agent_b=c.get("agent_b"), cumulative=cum)


def dev_ops(dev, d):
    """Device operands: q strided, the rest contiguous NaN-guarded."""
    ops = {}
    for k in FLOAT_OPS + ("agent_w", "agent_b"):
        v = d.get(k)
        if v is not None:
            ops[k] = Buf(dev, v.shape, v, strided=(k == "q"))
    if torch.is_tensor(d["u"]):
        ops["u_prev"] = Buf(dev, d["u"].shape, d["u"])
    return ops


# ------------------------------------------------------------------------------ forward

class Fwd:
    def __init__(self, dev, *, B, N, D1, D2, M1, M2, F, KW, lpp=0, fwd=True, seed=1, lengths=None,
                 init=False, per_u=False, agent=None, cum=False, loc_out=True, stats=True,
                 nob1=False, pst_extra=0):
        from sat_amd import kernels
        self.dims = dict(B=B, N=N, D1=D1, D2=D2, M1=M1, M2=M2, F=F, KW=KW)
        self.fwd, self.cum, self.agent = fwd, cum, agent
        self.d = make_inputs(seed, **self.dims, fwd=fwd, lengths=lengths, init=init, per_u=per_u,
                             agent=agent, nob1=nob1)
        self.r64, self.r32 = (ref_fwd(self.d, t, fwd, cum) for t in (torch.float64, torch.float32))
        self.ins = dev_ops(dev, self.d)
        ntiles = (N + 31) // 32
        pst = kernels.part_stride(M1, M2) + pst_extra
        o = dict(e1=Buf(dev, (B, N)), e2=Buf(dev, (B, N)), part=Buf(dev, (B, ntiles, pst)),
                 s_out=Buf(dev, (B, N)), a_out=Buf(dev, (B, N)), s2_out=Buf(dev, (B, N)),
                 ctx=Buf(dev, (B, M1 + M2), strided=True))
        if stats:
            o["stats"] = Buf(dev, (B, 4))
        if loc_out:
            o["loc_out"] = Buf(dev, (B, N, F))
        if agent is not None:
            o["u_out"] = Buf(dev, (B,))
        if cum:
            o["state_out"] = Buf(dev, (B, N))
        self.outs = o
        self.kw = dict(**self.dims, NT=32, ntiles=ntiles, att1_forward=int(fwd), lpp=lpp,
                       u=0.3 if per_u else self.d["u"], lengths=self.d["lengths"].to(dev),
                       q_sb=self.ins["q"].sb, ctx_sb=o["ctx"].sb, part_stride=pst,
                       agent_b_sb=int(agent or 0),
                       **{k: b.v for k, b in self.ins.items()}, **{k: b.v for k, b in o.items()})
        if per_u:
            self.kw["u"] = 0.9       # must not be read when u_prev is given

    def run(self, phases=0):
        from sat_amd import kernels
        kernels.attn_step_fwd(**self.kw, phases=phases)
        torch.cuda.synchronize()

    def check(self):
        """Padding intact, masked positions exact, every output within its bar; returns the
        largest err / bar."""
        for b in list(self.ins.values()) + list(self.outs.values()):
            assert b.intact()
        o, r64, r32 = self.outs, self.r64, self.r32
        L = self.d["lengths"]
        N, M1 = self.dims["N"], self.dims["M1"]
        dead = torch.arange(N).unsqueeze(0) >= L.unsqueeze(1)
        worst = {}
        for name, k in (("s_out", "s"), ("a_out", "a"), ("s2_out", "s2")):
            got = o[name].cpu()
            assert torch.equal(got[dead], torch.zeros(int(dead.sum()), dtype=torch.float64)), name
            worst[k] = _ratio(got, getattr(r64, k), getattr(r32, k))
        for name in ("e1", "e2"):
            got = o[name].cpu()
            assert bool((got[dead] == float("-inf")).all()), name
            z = lambda x: x.double().masked_fill(dead, 0.0)   # noqa: E731
            worst[name] = _ratio(z(got), z(getattr(r64, name)), z(getattr(r32, name)))
        ctx = o["ctx"].cpu()
        worst["c1"] = _ratio(ctx[:, :M1], r64.c1, r32.c1)
        worst["c2"] = _ratio(ctx[:, M1:], r64.c2, r32.c2)
        if "stats" in o:
            worst["stats"] = _ratio(o["stats"].cpu(), r64.stats, r32.stats)
        if "loc_out" in o:
            if self.fwd:
                worst["loc"] = _ratio(o["loc_out"].cpu(), r64.loc, r32.loc)
            else:
                assert o["loc_out"].untouched()      # the additive mechanism has none
        if "u_out" in o:
            worst["u_out"] = _ratio(o["u_out"].cpu(), r64.u_out, r32.u_out)
        if "state_out" in o:
            worst["state"] = _ratio(o["state_out"].cpu(), r64.state_out, r32.state_out)
        self.worst = worst
        return max(worst.values())


PRESET = dict(B=3, N=45, D1=224, D2=32, M1=256, M2=32, F=5, KW=10)
SMALL = dict(B=3, N=7, D1=32, D2=32, M1=4, M2=4)
MID = dict(B=3, N=33, D1=96, D2=64, M1=252, M2=4)
B8 = dict(B=8, N=100, D1=96, D2=64, M1=64, M2=32)

FWD_CASES = {
    # ---- attn_energy_wide_kernel<5,16,true>
    "preset": dict(PRESET),
    "preset-init": dict(PRESET, init=True),
    "w5x16-full": dict(B=8, N=64, D1=256, D2=64, M1=64, M2=4, F=5, KW=10, lpp=16),
    "nostats": dict(PRESET, N=100, lpp=16, stats=False, loc_out=False, pst_extra=4),
    # ---- attn_energy_wide_kernel<5,32,true>
    "w5x32-d96": dict(MID, F=5, KW=5, lpp=32),
    "w5x32-n512": dict(B=1, N=512, D1=256, D2=32, M1=64, M2=32, F=5, KW=10, lpp=32),
    # ---- attn_energy_wide_kernel<8,16,true>
    "w8-f1": dict(SMALL, F=1, KW=1),
    "w8-f3": dict(B8, F=3, KW=32, lpp=16),
    "w8-f8-n1": dict(B=1, N=1, D1=256, D2=32, M1=256, M2=32, F=8, KW=5, lpp=16),
    "w8-f3-lpp32": dict(PRESET, F=3, KW=5, lpp=32),
    # ---- attn_energy_wide_kernel<0,16,false>
    "add-preset": dict(PRESET, fwd=False),
    "add-lpp32": dict(B=8, N=33, D1=256, D2=64, M1=4, M2=4, F=5, KW=10, fwd=False, lpp=32),
    "add-nob1": dict(MID, F=5, KW=10, fwd=False, nob1=True, lpp=16),
    # ---- attn_energy_kernel<5,7,1,true>
    "n5-preset": dict(PRESET, lpp=8),
    "n5-b8": dict(B=8, N=100, D1=224, D2=32, M1=64, M2=4, F=5, KW=10, lpp=8),
    # ---- attn_energy_kernel<8,8,2,true>
    "n8-f3": dict(MID, F=3, KW=5, lpp=8),
    "n8-f5-d256": dict(B=1, N=64, D1=256, D2=32, M1=256, M2=32, F=5, KW=10, lpp=8),
    "n8-f5-d2x64": dict(PRESET, D2=64, lpp=8),
    "n8-f8": dict(SMALL, F=8, KW=32, lpp=8),
    "n8-f1": dict(B8, F=1, KW=10, lpp=8, init=True),
    # ---- attn_energy_kernel<0,8,2,false>
    "nadd-d96": dict(B=3, N=45, D1=96, D2=32, M1=64, M2=32, F=5, KW=10, fwd=False, lpp=8),
    "nadd-d256": dict(B=8, N=32, D1=256, D2=64, M1=252, M2=4, F=5, KW=10, fwd=False, lpp=8),
    # ---- the UB twins (per-utterance u_prev) and attn_combine_kernel<true>
    "ub-preset": dict(PRESET, per_u=True, agent=0, cum=True),
    "ub-b8": dict(B8, F=5, KW=10, lpp=16, per_u=True, agent=1),
    "ub-w5x32": dict(MID, F=5, KW=5, lpp=32, per_u=True, cum=True),
    "ub-w8-f3": dict(PRESET, F=3, KW=5, per_u=True, agent=0),
    "ub-w8-f8": dict(SMALL, B=8, F=8, KW=32, lpp=32, per_u=True, stats=False),
    "ub-n5": dict(PRESET, lpp=8, per_u=True, agent=1, cum=True, loc_out=False),
    "ub-n8-f1": dict(MID, F=1, KW=1, lpp=8, per_u=True, agent=0),
    "ub-n8-f5": dict(B=1, N=512, D1=256, D2=64, M1=4, M2=4, F=5, KW=10, lpp=8, per_u=True, cum=True),
    "agent-scalar-u": dict(PRESET, agent=0),
    "cum-scalar-u": dict(MID, F=5, KW=10, cum=True, init=True),
}


@pytest.mark.parametrize("name", sorted(FWD_CASES))
def test_step_fwd(cuda, name):
    """Every forward tile kernel and both combine kernels (table in the module docstring): loc, e1,
    e2, s, a, s2, c1, c2, stats, u_out and state_out against float64, exact zeros / -inf past the
    lengths, NaN padding intact, absent optional outputs.
    Largest err/bar observed: 0.68 (agent-scalar-u; 0.64 ub-preset, 0.50 n8-f3)."""
    c = Fwd(cuda, seed=sum(map(ord, name)), **FWD_CASES[name])
    c.run()
    worst = c.check()
    _note(f"test_step_fwd[{name}]", worst)
    print({k: round(v, 3) for k, v in c.worst.items()})
    assert worst <= 1.0, c.worst


def test_initial_state_floor(cuda):
    """From the initial state (alpha_0 one-hot at 0, s_0 = 0) every position n >= 2 has a prior of
    exactly the 1e-7 floor: its alpha must be positive and match the reference to the bar of the
    floor's own scale (a dropped floor gives exact zeros).
    Largest err/bar observed: 0.16 (of the bar over positions 2.. alone)."""
    c = Fwd(cuda, seed=5, **dict(PRESET, init=True))
    c.run()
    assert c.check() <= 1.0
    a, ra, ra32 = c.outs["a_out"].cpu(), c.r64.a, c.r32.a.double()
    L = c.d["lengths"].tolist()
    worst = 0.0
    for b in range(3):
        hi = L[b]
        assert hi > 2 and float(a[b, 2:hi].min()) > 0.0
        worst = max(worst, _ratio(a[b, 2:hi], ra[b, 2:hi], ra32[b, 2:hi]))
    _note("test_initial_state_floor", worst)
    assert worst <= 1.0


@pytest.mark.parametrize("name", ["preset", "n5-preset", "ub-preset", "add-preset", "w8-f3"])
def test_phases_split_is_bitwise_the_single_call(cuda, name):
    """phases = 1 (tile kernel) followed by phases = 2 (combine) writes bit for bit what
    phases = 0 writes."""
    one = Fwd(cuda, seed=3, **FWD_CASES[name])
    two = Fwd(cuda, seed=3, **FWD_CASES[name])
    one.run(0)
    two.run(1)
    assert two.outs["s_out"].untouched() and two.outs["ctx"].untouched()   # no combine yet
    two.run(2)
    assert one.check() <= 1.0
    bits = lambda b: b.buf.contiguous().view(torch.int32)   # noqa: E731  (NaN padding included)
    for k in one.outs:
        assert torch.equal(bits(one.outs[k]), bits(two.outs[k])), k


# ------------------------------------------------------------------------------ backward

BWD_DIMS = [dict(PRESET), dict(SMALL, KW=1), dict(B=8, N=33, D1=96, D2=64, M1=64, M2=4, KW=5),
            dict(B=3, N=100, D1=256, D2=64, M1=252, M2=32, KW=32),
            dict(B=2, N=64, D1=224, D2=32, M1=64, M2=32, KW=10),
            dict(B=1, N=32, D1=32, D2=64, M1=256, M2=4, KW=5),
            dict(B=3, N=45, D1=96, D2=32, M1=4, M2=32, KW=10)]
PAIRS = [(8, 4), (16, 4), (16, 8), (16, 16), (32, 4), (32, 8), (32, 16)]


class Bwd:
    """One reverse step.  ext: None (plain), "all" (u_prev, u_t, dup, ds_next, ds_out and a dqp
    row stride with one spare row), "u" (u_prev alone: u_t is then u_prev), "cum" (ds only)."""

    def __init__(self, dev, dims, *, F, NT, waves, ext=None, last=False, seed=1, lengths=None):
        dm = dict(dims)
        dm.pop("F", None)
        fwd = F > 0
        dm["F"] = F if fwd else 5
        B, N, D1, D2, M1, M2 = (dm[k] for k in ("B", "N", "D1", "D2", "M1", "M2"))
        self.dims, self.fwd, self.ext, self.last = dm, fwd, ext, last
        per_u = ext in ("all", "u")
        self.d = d = make_inputs(seed, **dm, fwd=fwd, per_u=per_u, lengths=lengths)
        g = torch.Generator().manual_seed(seed + 1)
        f = lambda *s, scale=1.0: (scale * torch.randn(*s, generator=g)).float()   # noqa: E731
        up = dict(dctx=f(B, M1 + M2))
        if fwd and not last:
            up.update(y_next=f(B, N, scale=0.5), df_next=f(B, N, dm["F"], scale=0.5))
            if ext in ("all", "cum"):
                up["ds_next"] = f(B, N, scale=0.5)
        if ext == "all":
            up["u_t"] = (0.1 + 0.8 * torch.rand(B, generator=g)).float()
        self.up = up
        f64 = ref_fwd(d, torch.float64, fwd, False)
        self.r64, self.r32 = (self._ref(t) for t in (torch.float64, torch.float32))
        self.ins = dev_ops(dev, d)
        ctx64 = torch.cat([f64.c1, f64.c2], 1)
        state = dict(s_t=f64.s, a_t=f64.a, s2_t=f64.s2, stats=f64.stats)   # float64 -> float32
        for k, v in state.items():
            self.ins[k] = Buf(dev, v.shape, v)
        self.ins["ctx_t"] = Buf(dev, ctx64.shape, ctx64, strided=True)
        self.ins["dctx"] = Buf(dev, up["dctx"].shape, up["dctx"], strided=True)
        for k in ("y_next", "df_next", "ds_next", "u_t"):
            if k in up:
                self.ins[k] = Buf(dev, up[k].shape, up[k])
        ntiles = (N + NT - 1) // NT
        self.ntiles, self.spare = ntiles, 1 if ext == "all" else 0
        o = dict(y_out=Buf(dev, (B, N)), df_out=Buf(dev, (B, N, dm["F"])), de1_out=Buf(dev, (B, N)),
                 de2_out=Buf(dev, (B, N)), dqp=Buf(dev, (B, ntiles + self.spare, D1 + D2)))
        if ext == "all":
            o["dup"] = Buf(dev, (B, ntiles))
        if ext in ("all", "cum"):
            o["ds_out"] = Buf(dev, (B, N))
        self.outs = o
        names = {k: b.v for k, b in self.ins.items() if k not in ("agent_w", "agent_b")}
        self.kw = dict(**dm, NT=NT, ntiles=ntiles, att1_forward=int(fwd), waves=waves,
                       u=0.9 if per_u else d["u"], dctx_sb=self.ins["dctx"].sb,
                       ctx_sb=self.ins["ctx_t"].sb, q_sb=self.ins["q"].sb,
                       dqp_sb=(ntiles + 1) * (D1 + D2) if ext == "all" else 0,
                       **names, **{k: b.v for k, b in o.items()})

    def _ref(self, dtype):
        c, u = cast(self.d, dtype), cast(self.up, dtype)
        return R.step_bwd(*[c[k] for k in ORDER], dctx=u["dctx"], y_next=u.get("y_next"),
                          df_next=u.get("df_next"), ds_next=u.get("ds_next"), u_t=u.get("u_t"),
                          att1_forward=self.fwd)

    def run(self):
        from sat_amd import kernels
        kernels.attn_step_bwd(**self.kw)
        torch.cuda.synchronize()

    def check(self):
        for b in list(self.ins.values()) + list(self.outs.values()):
            assert b.intact()
        o, r64, r32 = self.outs, self.r64, self.r32
        N = self.dims["N"]
        dead = torch.arange(N).unsqueeze(0) >= self.d["lengths"].unsqueeze(1)
        zeros = torch.zeros(int(dead.sum()), dtype=torch.float64)
        w = {}
        for name, k in (("de1_out", "de1"), ("de2_out", "de2")):
            got = o[name].cpu()
            assert torch.equal(got[dead], zeros), name
            w[k] = _ratio(got, getattr(r64, k), getattr(r32, k))
        dqp = o["dqp"].cpu() if not self.spare else None
        if self.spare:
            assert bool(torch.isnan(o["dqp"].v[:, self.ntiles]).all())    # the agent's row
            dqp = o["dqp"].v[:, :self.ntiles].double().cpu()
        w["dq"] = _ratio(dqp.sum(1), r64.dq, r32.dq)
        if self.fwd:
            y = o["y_out"].cpu()
            assert torch.equal(y[dead], zeros)
            w["y"] = _ratio(y, r64.y_out, r32.y_out)
            w["df"] = _ratio(o["df_out"].cpu(), r64.df_out, r32.df_out)
        else:
            assert o["y_out"].untouched() and o["df_out"].untouched()
        if "dup" in o:
            w["du"] = _ratio(o["dup"].cpu().sum(1), r64.du, r32.du)
        if "ds_out" in o:
            w["ds"] = _ratio(o["ds_out"].cpu(), r64.ds_out, r32.ds_out)
        self.worst = w
        return max(w.values())


def _bwd_cases():
    out, i = [], 0
    for NT, waves in PAIRS:
        for F in (0, 1, 3, 5, 8):
            for ext in ((None,) if F == 0 else (None, "all")):
                for last in (True, False):
                    # waves = 0 is the default 16; pass it in every other (.,16) case
                    w = 0 if (waves == 16 and NT > 8 and i % 2) else waves
                    out.append(pytest.param(NT, w, F, ext, last, i % len(BWD_DIMS),
                                            id=f"nt{NT}-w{waves}-f{F}-{ext or 'plain'}-"
                                               f"{'last' if last else 'inner'}"))
                    i += 1
    return out


@pytest.mark.parametrize("NT,waves,F,ext,last,dims", _bwd_cases())
def test_step_bwd(cuda, NT, waves, F, ext, last, dims):
    """attn_bwd_kernel<NT, F, waves[, EXT]> for every legal (NT, waves) x F in {0 (additive), 1, 3,
    5, 8} x plain / EXT (u_prev != u_t, dup, ds_next / ds_out, a dqp row stride with a spare row)
    x last (y_next = df_next = NULL) / inner step: de1, de2, y_out, df_out, the tile sums of dqp
    and dup, ds_out against float64 autograd of the reference step.
    Largest err/bar observed: 0.96 (de1 of one case, 0.95 df of another; third largest 0.73, du)."""
    c = Bwd(cuda, BWD_DIMS[dims], F=F, NT=NT, waves=waves, ext=ext, last=last,
            seed=17 * NT + waves + F + dims)
    c.run()
    worst = c.check()
    _note(f"test_step_bwd[{max(c.worst, key=c.worst.get)}]", worst)
    assert worst <= 1.0, c.worst


@pytest.mark.parametrize("ext,last,NT,waves", [("u", False, 32, 0), ("u", True, 16, 8),
                                               ("cum", False, 32, 8), ("cum", True, 8, 4),
                                               (None, False, 8, 16), ("all", False, 8, 8)])
def test_step_bwd_partial_ext(cuda, ext, last, NT, waves):
    """EXT with only some of its operands: u_prev alone (u_t NULL: dalpha_t uses u_prev), ds_next /
    ds_out alone with the scalar u; NT = 8 runs its 4-wave kernel whatever ``waves`` asks for;
    N = 512 (64 tiles of 8) in the plain inner step.
    Largest err/bar observed: 0.32."""
    dims = dict(B=1, N=512, D1=96, D2=32, M1=64, M2=4, KW=5) if ext is None else BWD_DIMS[2]
    c = Bwd(cuda, dims, F=5, NT=NT, waves=waves, ext=ext, last=last, seed=91)
    c.run()
    worst = c.check()
    _note(f"test_step_bwd_partial_ext[{max(c.worst, key=c.worst.get)}]", worst)
    assert worst <= 1.0, c.worst


@pytest.mark.parametrize("ntiles", [1, 4, 16])
def test_agent_bwd(cuda, ntiles):
    """sat_attn_agent_bwd: dz, the first M1 columns of a wider dctx row (dctx_sb > M1; the columns
    behind them untouched) and the extra query-gradient row (dq_sb > D1 + D2, zeros in its D2
    part) against the float64 restatement.
    Largest err/bar observed: 0.13."""
    from sat_amd import kernels
    B, M1, M2, D1, D2 = 3, 252, 4, 96, 32
    g = torch.Generator().manual_seed(ntiles)
    f = lambda *s, scale=1.0: (scale * torch.randn(*s, generator=g)).float()   # noqa: E731
    dup, u_t, w, dctx = f(B, ntiles), torch.rand(B, generator=g).float(), f(M1 + D1, scale=0.3), f(B, M1 + M2)
    r64 = R.agent_bwd(dup.double().sum(1), u_t.double(), w.double(), dctx.double(), M1, D1, D2)
    r32 = R.agent_bwd(dup.sum(1), u_t, w, dctx, M1, D1, D2)
    ins = dict(dup=Buf(cuda, dup.shape, dup), u_t=Buf(cuda, (B,), u_t), agent_w=Buf(cuda, w.shape, w))
    dz, dc = Buf(cuda, (B,)), Buf(cuda, dctx.shape, dctx, strided=True)
    dq = Buf(cuda, (B, D1 + D2), strided=True)
    kernels.attn_agent_bwd(B=B, ntiles=ntiles, M1=M1, D1=D1, D2=D2, dz_out=dz.v, dctx=dc.v,
                           dctx_sb=dc.sb, dq_extra=dq.v, dq_sb=dq.sb, **{k: b.v for k, b in ins.items()})
    torch.cuda.synchronize()
    for b in list(ins.values()) + [dz, dc, dq]:
        assert b.intact()
    assert torch.equal(dc.cpu()[:, M1:], dctx.double()[:, M1:])
    assert torch.equal(dq.cpu()[:, D1:], torch.zeros(B, D2, dtype=torch.float64))
    worst = max(_ratio(x.cpu(), y, z) for x, y, z in zip((dz, dc, dq), r64, r32))
    _note("test_agent_bwd", worst)
    assert worst <= 1.0


@pytest.mark.parametrize("both", [False, True], ids=["stock", "agent+cumulative"])
def test_chain_of_three_steps(cuda, both):
    """T = 3, B = 2, N = 45: kernel forward steps, then kernel reverse steps with the agent launch
    in between, handing y, df, ds, dup and u exactly as the decoder's loops do; every step's dq
    (tile rows and the agent's row summed), de1 and de2 against end-to-end float64 autograd of the
    reference chain, bar from the same chain in float32.
    Largest err/bar observed: 0.31."""
    from sat_amd import kernels
    T, B, N, D1, D2, M1, M2, F, KW = 3, 2, 45, 224, 32, 64, 32, 5, 10
    d = make_inputs(77, B, N, D1, D2, M1, M2, F, KW, lengths=[45, 33], per_u=True, agent=0)
    g = torch.Generator().manual_seed(78)
    qs = [torch.randn(B, D1 + D2, generator=g) for _ in range(T)]
    dctxs = [torch.randn(B, M1 + M2, generator=g) for _ in range(T)]
    if not both:
        d["u"] = torch.full((B,), 0.5)
    refs = []
    for t in (torch.float64, torch.float32):
        c = cast(d, t)
        refs.append(R.chain_grads([q.to(t) for q in qs], tuple(c[k] for k in ORDER[1:6]),
                                  (c["s_prev"], c["a_prev"], c["u"]), c, [x.to(t) for x in dctxs],
                                  agent=both, cumulative=both))
    r64, r32 = refs
    dv = {k: v.to(cuda) for k, v in d.items() if torch.is_tensor(v)}
    z = lambda *s: torch.full(s, NAN, device=cuda)   # noqa: E731
    NT, ntiles, parts = 32, 2, 3 if both else 2
    pst = kernels.part_stride(M1, M2)
    S, AL, U = z(T + 1, B, N), z(T + 1, B, N), z(T + 1, B)
    SM, S2, CTX, ST, LOC = z(T, B, N), z(T, B, N), z(T, B, M1 + M2), z(T, B, 4), z(T, B, N, F)
    S[0], AL[0], U[0] = dv["s_prev"], dv["a_prev"], dv["u"]
    Q = torch.stack(qs).to(cuda)
    par = {k: dv[k] for k in ("v1", "b1", "convW", "convb", "locW", "v2")}
    mem = {k: dv[k] for k in ("K1", "V1", "K2", "V2")}
    dims = dict(B=B, N=N, D1=D1, M1=M1, D2=D2, M2=M2, F=F, KW=KW, NT=NT, ntiles=ntiles,
                att1_forward=1, u=0.5)
    for t in range(T):
        ext = dict(u_prev=U[t], u_out=U[t + 1], agent_w=dv["agent_w"], agent_b=dv["agent_b"],
                   state_out=S[t + 1]) if both else {}
        kernels.attn_step_fwd(**dims, **mem, **par, q=Q[t], q_sb=D1 + D2, lengths=dv["lengths"],
                              s_prev=S[t], a_prev=AL[t], e1=z(B, N), e2=z(B, N),
                              part=z(B, ntiles, pst), part_stride=pst,
                              s_out=SM[t] if both else S[t + 1], a_out=AL[t + 1], s2_out=S2[t],
                              ctx=CTX[t], ctx_sb=M1 + M2, stats=ST[t], loc_out=LOC[t], **ext)
    RD = torch.stack(dctxs).to(cuda)
    DQP, DE1, DE2, DFH = z(T, B, parts, D1 + D2), z(T, B, N), z(T, B, N), z(T, B, N, F)
    YA, DSC = [z(B, N), z(B, N)], [z(B, N), z(B, N)]
    DUP, DZ = torch.zeros(B, ntiles, device=cuda), z(T, B)
    cur = 0
    for t in reversed(range(T)):
        last = t == T - 1
        ext = {}
        if both:
            kernels.attn_agent_bwd(B=B, ntiles=ntiles, M1=M1, D1=D1, D2=D2, dup=DUP, u_t=U[t + 1],
                                   agent_w=dv["agent_w"], dz_out=DZ[t], dctx=RD[t], dctx_sb=M1 + M2,
                                   dq_extra=DQP[t][:, ntiles], dq_sb=parts * (D1 + D2))
            ext = dict(dup=DUP, u_prev=U[t], u_t=U[t + 1], dqp_sb=parts * (D1 + D2),
                       ds_next=None if last else DSC[cur], ds_out=DSC[1 - cur])
        kernels.attn_step_bwd(**dims, V1=mem["V1"], V2=mem["V2"], K1=mem["K1"], K2=mem["K2"], **par,
                              dctx=RD[t], dctx_sb=M1 + M2, ctx_t=CTX[t], ctx_sb=M1 + M2,
                              y_next=None if last else YA[cur], s_t=SM[t] if both else S[t + 1],
                              a_t=AL[t + 1], a_prev=AL[t], s_prev=S[t], s2_t=S2[t], stats=ST[t],
                              df_next=None if last else DFH[t + 1], q=Q[t], q_sb=D1 + D2,
                              y_out=YA[1 - cur], df_out=DFH[t], de1_out=DE1[t], de2_out=DE2[t],
                              dqp=DQP[t], **ext)
        cur = 1 - cur
    torch.cuda.synchronize()
    worst = 0.0
    for t in range(T):
        for got, k in ((DQP[t].double().cpu().sum(1), "dq"), (DE1[t].double().cpu(), "de1"),
                       (DE2[t].double().cpu(), "de2"), (DFH[t].double().cpu(), "df")):
            worst = max(worst, _ratio(got, getattr(r64, k)[t], getattr(r32, k)[t]))
    _note("test_chain_of_three_steps", worst)
    assert worst <= 1.0


# ------------------------------------------------------------------------------ refusals

def _fwd_kw(dev, **over):
    """A complete, valid forward request on zero operands (B = 2, N = 9, one tile)."""
    from sat_amd import kernels as K
    dm = dict(B=2, N=9, D1=32, M1=8, D2=32, M2=4, F=5, KW=10)
    dm.update({k: over.pop(k) for k in list(over) if k in dm})
    B, N, D1, M1, D2, M2, F, KW = (dm[k] for k in ("B", "N", "D1", "M1", "D2", "M2", "F", "KW"))
    z = lambda *s: torch.zeros(*[max(x, 1) for x in s], device=dev)   # noqa: E731
    ntiles = (N + 31) // 32
    pst = K.part_stride(max(M1, 0), max(M2, 0))
    kw = dict(**dm, NT=32, ntiles=ntiles, att1_forward=1, u=0.5, q=z(B, D1 + D2), q_sb=D1 + D2,
              K1=z(B, N, D1), V1=z(B, N, M1), K2=z(B, N, D2), V2=z(B, N, M2),
              lengths=torch.full((B,), N, dtype=torch.int64, device=dev), s_prev=z(B, N),
              a_prev=z(B, N), v1=z(D1), b1=z(D1), convW=z(KW, F), convb=z(F), locW=z(F, D1),
              v2=z(D2), e1=z(B, N), e2=z(B, N), part=z(B, ntiles, pst + 4), part_stride=pst,
              s_out=z(B, N), a_out=z(B, N), s2_out=z(B, N), ctx=z(B, M1 + M2), ctx_sb=M1 + M2)
    kw.update(over)
    return kw


def _off4(t):
    """The same values 4 bytes further on: a pointer that is not 16-byte aligned."""
    flat = torch.zeros(t.numel() + 4, device=t.device)
    v = flat[1:1 + t.numel()].view(t.shape)
    assert v.data_ptr() % 16 == 4
    return v


REFUSED_FWD = {
    "K1 misaligned": (dict(mis="K1"), "16-byte aligned"),
    "V1 misaligned": (dict(mis="V1"), "16-byte aligned"),
    "K2 misaligned": (dict(mis="K2"), "16-byte aligned"),
    "V2 misaligned": (dict(mis="V2"), "16-byte aligned"),
    "part misaligned": (dict(mis="part"), "16-byte aligned"),
    "part_stride % 4": (dict(part_stride_add=2), "part_stride must be a multiple of 4"),
    "D1 = 0": (dict(D1=0), "must be >= 1"),
    "D2 = 0": (dict(D2=0), "must be >= 1"),
    "M1 = 0": (dict(M1=0), "must be >= 1"),
    "M2 = 0": (dict(M2=0), "must be >= 1"),
    "M1 < 0": (dict(M1=-4), "must be >= 1"),
    "forward attention, F = 0": (dict(F=0), "needs F >= 1"),
    "forward attention, F < 0": (dict(F=-1), "needs F >= 1"),
    "forward attention, KW = 0": (dict(KW=0), "KW >= 1"),
}


@pytest.mark.parametrize("name", sorted(REFUSED_FWD))
def test_step_fwd_refuses(cuda, name):
    """sat_attn_step_fwd returns the argument error, with a message that names the cause, for
    operands its float4 loads / stores cannot take (K1, V1, K2, V2, part off 16 bytes, a part
    stride off 4 floats), a dimension below 1 (the clamped loads would index -1) and forward
    attention without location features or with an empty location kernel.  Nothing is launched."""
    from sat_amd import _lib, kernels as K
    over, msg = REFUSED_FWD[name]
    over = dict(over)
    mis, add = over.pop("mis", None), over.pop("part_stride_add", 0)
    kw = _fwd_kw(cuda, **over)
    K.attn_step_fwd(**_fwd_kw(cuda))                      # the unchanged request is accepted
    if mis:
        kw[mis] = _off4(kw[mis])
    kw["part_stride"] += add
    with pytest.raises(_lib.SatLibraryError) as e:
        K.attn_step_fwd(**kw)
    assert e.value.rc == _lib.SAT_ERR_ARGUMENT and msg in str(e.value), str(e.value)
    torch.cuda.synchronize()


def test_step_fwd_n512_runs_n513_is_refused(cuda):
    """N = 512 (16 tiles) is the largest memory the forward step takes and is correct (FWD_CASES
    w5x32-n512 / ub-n8-f5 check it in full); N = 513 is refused with a message that says 512."""
    from sat_amd import _lib, kernels as K
    c = Fwd(cuda, seed=4, **dict(FWD_CASES["w5x32-n512"], lpp=0))
    c.run()
    assert c.check() <= 1.0
    with pytest.raises(_lib.SatLibraryError) as e:
        K.attn_step_fwd(**_fwd_kw(cuda, N=513))
    assert e.value.rc == _lib.SAT_ERR_ARGUMENT and "N <= 512" in str(e.value)


@pytest.mark.parametrize("F,KW,msg", [(0, 10, "needs F >= 1"), (-1, 10, "needs F >= 1"),
                                      (5, 0, "KW >= 1")])
def test_step_bwd_refuses_forward_attention_without_location_features(cuda, F, KW, msg):
    """sat_attn_step_bwd refuses att1_forward with F < 1 (it would back-propagate an additive
    step) or KW < 1, as the forward does; the same request with F = 5, KW = 10 is accepted."""
    from sat_amd import _lib, kernels as K
    c = Bwd(cuda, BWD_DIMS[1], F=5, NT=32, waves=0, last=True, seed=2)
    c.run()
    assert c.check() <= 1.0
    with pytest.raises(_lib.SatLibraryError) as e:
        K.attn_step_bwd(**dict(c.kw, F=F, KW=KW))
    assert e.value.rc == _lib.SAT_ERR_ARGUMENT and msg in str(e.value), str(e.value)
