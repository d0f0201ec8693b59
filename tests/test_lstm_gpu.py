"""sat_lstm_step(s)_fwd / _bwd (csrc/lstm.hip) against tests/lstm_ref.py in float64, kernel by
kernel: the general LDS-staged step, the batch <= 8 register step, the multi-problem launches and
the reverse step, at ragged shapes, with every optional operand present and absent.

Outputs live in NaN-filled buffers; strided operands are column blocks of wider NaN buffers whose
padding must still be NaN afterwards.  Every pointer is 16-byte aligned and every stride a
multiple of 4 except in the refusal tests, which never reach the device.

Bounds (derived, as in test_gemm_gpu.py).  With D = |rows| @ |W| + |xproj or bias| + 1 per gate:
  gate pre-activation error <= 6e-7 D (fp32 accumulation), each activation adds 1e-6 (sat_common.h:
  ~2e-7 for one exp + reciprocal, tanh_lstm doubles it, the rest is margin), so
  |gates - ref| <= 6e-7 D + 1e-6 =: gb; c_out, h_raw, h_out are within 4 (1 + |c_prev|) max_g gb of
  their (row, unit).  Backward, fed the reference's float64 gates rounded to float32:
  |dgates - ref| <= 6e-7 A + 1e-6 (1 + |dy| + |dh_carry| + |dc_carry|), A the absolute-value
  version of the length 4U + DQ dot; the two carries obey the same bound.
The largest err / bound each test function has shown on an MI355X is in its docstring.
"""
import math

import pytest
import torch

import lstm_ref as R

pytestmark = pytest.mark.gpu

NAN = float("nan")
ZC, ZH = 0.1, 0.15


def _note(name, ratio):
    print(f"RATIO {name} {ratio:.4f}")


class Buf:
    """A float32 operand inside a NaN-filled buffer: contiguous with 4 guard floats on each side,
    or (``strided``) a [B, n] column block at column 4 of a [B, roundup(n, 4) + 8] buffer."""

    def __init__(self, dev, shape, data=None, strided=False):
        self.strided = strided
        self.shape = tuple(shape)
        if strided:
            B, n = shape
            self.buf = torch.full((B, (n + 3) // 4 * 4 + 8), NAN, device=dev)
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

    def cpu(self):
        return self.v.double().cpu()


def _view_of(b):
    return None if b is None else b.v


# ------------------------------------------------------------------------------ forward

class Fwd:
    """Inputs (float32 values, reference in float64), device operands and output buffers of one
    forward step.  ``segs`` = (k0, K1, K2) splits the row over rin / rin1 / rin2."""

    def __init__(self, dev, B, U, K, *, masks, xmode, state, seed, segs=None, lengths=None, t=0):
        g = torch.Generator().manual_seed(seed)
        f = lambda *s, scale=1.0: (scale * torch.randn(*s, generator=g)).float()   # noqa: E731
        self.B, self.U, self.K = B, U, K
        rows, W = f(B, K), f(K, U, 4, scale=0.1)
        xb = f(B, U, 4) if xmode == "xproj" else f(U, 4, scale=0.5) if xmode == "bias" else None
        cp, hp = (f(B, U), f(B, U)) if state else (None, None)
        mc = (torch.rand(B, U, generator=g) < 0.8).float() if masks else None
        mh = (torch.rand(B, U, generator=g) < 0.8).float() if masks else None
        dd = lambda x: None if x is None else x.double()   # noqa: E731
        valid = None if lengths is None else t < lengths
        self.ref = R.step(dd(xb), rows.double(), W.double(), dd(cp), dd(hp), dd(mc), dd(mh), ZC, ZH,
                          valid=valid)
        D = rows.double().abs() @ W.double().abs().reshape(K, -1)
        D = D.view(B, U, 4) + (0.0 if xb is None else xb.double().abs()) + 1.0
        self.gb = 6e-7 * D + 1e-6
        self.sb = 4.0 * (1.0 + (0.0 if cp is None else cp.double().abs())) * self.gb.amax(-1)
        self.valid, self.cp, self.hp = valid, cp, hp
        k0, K1, K2 = segs or (K, 0, 0)
        assert k0 + K1 + K2 == K
        seg = lambda a, b: Buf(dev, (B, b - a), rows[:, a:b], strided=True) if b > a else None  # noqa: E731
        self.ins = dict(rin=seg(0, k0), rin1=seg(k0, k0 + K1), rin2=seg(k0 + K1, K),
                        xproj=Buf(dev, (B, 4 * U), xb.reshape(B, -1), strided=True) if xmode == "xproj" else None,
                        bias=Buf(dev, (U, 4), xb) if xmode == "bias" else None,
                        W=Buf(dev, (K, U, 4), W),
                        c_prev=Buf(dev, (B, U), cp) if state else None,
                        h_prev=Buf(dev, (B, U), hp, strided=True) if state else None,
                        mask_c=Buf(dev, (B, U), mc) if masks else None,
                        mask_h=Buf(dev, (B, U), mh) if masks else None)
        self.outs = dict(h_raw=Buf(dev, (B, U), strided=True), c_out=Buf(dev, (B, U)),
                         h_out=Buf(dev, (B, U), strided=True), gates=Buf(dev, (B, U, 4)))
        self.lengths = None if lengths is None else lengths.to(dev)
        self.kw = dict(B=B, U=U, K=K, t=t, zc=ZC, zh=ZH, lengths=self.lengths,
                       **{k: _view_of(v) for k, v in self.ins.items()},
                       **{k: v.v for k, v in self.outs.items()})

    def got(self):
        o = self.outs
        return o["h_raw"].cpu(), o["c_out"].cpu(), o["h_out"].cpu(), o["gates"].cpu()

    def check(self):
        """Padding intact, no NaN written, every output inside its bound; returns max err/bound."""
        for b in list(self.ins.values()) + list(self.outs.values()):
            assert b is None or b.intact()
        h_raw, c_out, h_out, gates = self.got()
        r_raw, r_c, r_h, r_g, _ = self.ref
        worst = 0.0
        for got, ref, bound in ((gates, r_g, self.gb), (h_raw, r_raw, self.sb), (c_out, r_c, self.sb),
                                (h_out, r_h, self.sb)):
            assert bool(torch.isfinite(got).all())
            ratio = float(((got - ref).abs() / bound).max())
            worst = max(worst, ratio)
        return worst


SHAPES = [(1, 4, 4), (3, 6, 12), (8, 64, 64), (8, 128, 1024), (9, 64, 64), (17, 130, 36),
          (9, 32, 1024), (32, 256, 256)]


@pytest.mark.parametrize("state", [True, False], ids=["state", "nostate"])
@pytest.mark.parametrize("xmode", ["xproj", "bias", "none"])
@pytest.mark.parametrize("masks", [True, False], ids=["masks", "eval"])
@pytest.mark.parametrize("B,U,K", SHAPES)
def test_step_fwd(cuda, B, U, K, masks, xmode, state):
    """sat_lstm_step_fwd at every shape family (smallest; U % 4 != 0 and a part batch tile; the
    batch <= 8 register kernel's first shape and its K ceiling; the first batch past it; ragged in
    both tile dimensions; an LDS need of 98,432 B; the training shape) x {masks, eval blend} x
    {xproj, bias only, neither} x {c_prev / h_prev given, NULL}.
    Largest err/bound observed: 0.07."""
    from sat_amd import kernels
    c = Fwd(cuda, B, U, K, masks=masks, xmode=xmode, state=state, seed=1000 * B + U + K)
    kernels.lstm_step_fwd(**c.kw)
    worst = c.check()
    _note("test_step_fwd", worst)
    assert worst <= 1.0


@pytest.mark.parametrize("B,U", [(3, 6), (8, 64), (9, 64)])
@pytest.mark.parametrize("segs", [(8, 12, 16), (0, 20, 16), (16, 0, 20), (0, 0, 36)])
def test_step_fwd_segments(cuda, B, U, segs):
    """The row as [rin | rin1 | rin2] in separate buffers, each segment empty in turn (rin NULL
    when empty), on the general kernel (B = 3: U < 64; B = 9) and the register kernel (B = 8,
    U = 64), against the concatenated-row reference.
    Largest err/bound observed: 0.07."""
    from sat_amd import kernels
    c = Fwd(cuda, B, U, 36, masks=False, xmode="bias", state=True, seed=7 * B + segs[0], segs=segs)
    assert (c.kw["rin"] is None) == (segs[0] == 0)
    kernels.lstm_step_fwd(**c.kw)
    worst = c.check()
    _note("test_step_fwd_segments", worst)
    assert worst <= 1.0


@pytest.mark.parametrize("masks", [True, False], ids=["masks", "eval"])
def test_step_fwd_lengths(cuda, masks):
    """The sequence-length copy-through at t = 2 with lengths below, equal to and above t (B = 9:
    the general kernel): an invalid row copies c_prev / h_prev bit for bit and writes h_raw = 0,
    gates = 0 exactly; valid rows meet the bounds.
    Largest err/bound observed: 0.06."""
    from sat_amd import kernels
    lengths = torch.tensor([0, 1, 2, 3, 5, 2, 9, 1, 3])
    c = Fwd(cuda, 9, 64, 64, masks=masks, xmode="xproj", state=True, seed=77, lengths=lengths, t=2)
    kernels.lstm_step_fwd(**c.kw)
    worst = c.check()
    _note("test_step_fwd_lengths", worst)
    assert worst <= 1.0
    h_raw, c_out, h_out, gates = c.got()
    inv = ~c.valid
    assert int(inv.sum()) == 5 and int(c.valid.sum()) == 4
    assert torch.equal(c_out[inv], c.cp.double()[inv]) and torch.equal(h_out[inv], c.hp.double()[inv])
    assert torch.equal(h_raw[inv], torch.zeros(5, 64, dtype=torch.float64))
    assert torch.equal(gates[inv], torch.zeros(5, 64, 4, dtype=torch.float64))
    assert float(gates[c.valid].abs().min()) > 0.0


MULTI = [dict(B=3, U=6, K=12, masks=True, xmode="xproj", state=True),
         dict(B=9, U=64, K=64, masks=False, xmode="bias", state=True),
         dict(B=17, U=130, K=36, masks=True, xmode="none", state=False),
         dict(B=32, U=256, K=256, masks=False, xmode="xproj", state=True)]


@pytest.mark.parametrize("n", [2, 3, 4])
def test_steps_fwd_multi(cuda, n):
    """n problems of different B, U, K and options in ONE sat_lstm_steps_fwd launch are bit-equal
    to n single sat_lstm_steps_fwd(.., 1) launches (not the register kernel), and meet the bounds.
    Largest err/bound observed: 0.07."""
    from sat_amd import kernels
    lens = torch.tensor([5, 0, 3] + [4] * 14)
    extra = [dict(), dict(), dict(lengths=lens, t=3), dict()]
    mk = lambda: [Fwd(cuda, seed=31 + i, **MULTI[i], **extra[i]) for i in range(n)]   # noqa: E731
    together, single = mk(), mk()
    kernels.lstm_steps_fwd([c.kw for c in together])
    for c in single:
        kernels.lstm_steps_fwd([c.kw])
    for a, b in zip(together, single):
        worst = a.check()
        _note("test_steps_fwd_multi", worst)
        assert worst <= 1.0
        for x, y in zip(a.got(), b.got()):
            assert torch.equal(x, y)


def test_steps_fwd_count_refused(cuda):
    """0 or more than 4 problems in one launch: refused before any launch."""
    from sat_amd import kernels
    from sat_amd._lib import SatLibraryError, SAT_ERR_ARGUMENT
    c = Fwd(cuda, 3, 6, 12, masks=False, xmode="bias", state=True, seed=1)
    for steps in ([], [c.kw] * 5):
        with pytest.raises(SatLibraryError) as e:
            kernels.lstm_steps_fwd(steps)
        assert e.value.rc == SAT_ERR_ARGUMENT
    assert all(bool(torch.isnan(o.buf).all()) for o in c.outs.values())


def _off1(dev, *shape):
    """A view of ``shape`` one float past a 16-byte boundary."""
    n = math.prod(shape)
    v = torch.zeros(n + 8, device=dev)[5:5 + n].view(shape)
    assert v.data_ptr() % 16 == 4
    return v


@pytest.mark.parametrize("what", ["xproj", "xproj_sb", "bias", "gates", "W", "rin"])
def test_step_fwd_alignment_refused(cuda, what):
    """The forward's 16-byte loads: a misaligned xproj / bias / gates / W / rin or an xproj stride
    of 4k + 1 is refused by check_fwd (SAT_ERR_ARGUMENT) before any launch, on both entry points."""
    from sat_amd import kernels
    from sat_amd._lib import SatLibraryError, SAT_ERR_ARGUMENT
    B, U, K = 3, 8, 8
    c = Fwd(cuda, B, U, K, masks=False, xmode="bias" if what == "bias" else "xproj", state=True, seed=2)
    kw = dict(c.kw)
    if what == "xproj_sb":
        kw["xproj"] = torch.zeros(B, 4 * U + 5, device=cuda)[:, 4:4 + 4 * U]
        assert kw["xproj"].stride(0) % 4 == 1 and kw["xproj"].data_ptr() % 16 == 0
    elif what == "W":
        kw["W"] = _off1(cuda, K, U, 4)
    elif what == "gates":
        kw["gates"] = _off1(cuda, B, U, 4)
    elif what == "bias":
        kw["bias"] = _off1(cuda, U, 4)
    else:
        kw[what] = _off1(cuda, B, 4 * U if what == "xproj" else K)
    for call in (lambda: kernels.lstm_step_fwd(**kw), lambda: kernels.lstm_steps_fwd([kw])):
        with pytest.raises(SatLibraryError) as e:
            call()
        assert e.value.rc == SAT_ERR_ARGUMENT
    assert all(bool(torch.isnan(o.buf).all()) for o in c.outs.values())


# ------------------------------------------------------------------------------ backward

DQ_VARIANTS = {"dq0": ((128, 0), 1, False), "dq01": ((128, 64), 3, True), "dqcap": ((4, 316), 1, True)}


class Bwd:
    """One reverse step: float32 inputs, float64 reference, device operands, output buffers."""

    def __init__(self, dev, B, U, hoff, variant, seed):
        g = torch.Generator().manual_seed(seed)
        f = lambda *s, scale=1.0: (scale * torch.randn(*s, generator=g)).float()   # noqa: E731
        K = U + hoff
        masks = variant in ("masks", "rec", "nulls", "lengths", "dq01")
        last = variant == "last"
        nulls = variant == "nulls"
        W = f(K, U, 4, scale=0.1)
        dgn = None if last else f(B, U, 4, scale=0.5)
        cp = None if nulls else f(B, U)
        # the reference forward's float64 gates, rounded to float32: forward error stays out
        gates = R.step(None, f(B, 4).double(), f(4, U, 4).double(), None if cp is None else cp.double(),
                       None, None, None, ZC, ZH)[3].float()
        dy = None if nulls else f(B, U)
        dhc = None if nulls else f(B, U)
        dcc = None if nulls else f(B, U)
        mc = (torch.rand(B, U, generator=g) < 0.8).float() if masks else None
        mh = (torch.rand(B, U, generator=g) < 0.8).float() if masks else None
        t = 3
        lengths = None
        if variant == "lengths":    # odd rows and the last row are invalid at t
            lengths = torch.tensor([t if (b % 2 == 1 or b == B - 1) else t + 1 + b for b in range(B)])
        dd = lambda x: None if x is None else x.double()   # noqa: E731
        Wr = W.double()[hoff:hoff + U]
        A = torch.zeros(B, U, dtype=torch.float64)
        rec = None
        if dgn is not None:
            A = A + torch.einsum("bvg,uvg->bu", dgn.double().abs(), Wr.abs())
            if variant == "rec":
                rec = torch.einsum("bvg,uvg->bu", dgn.double(), Wr).float()
        dqs, self.dq_bufs, dq_kw = [], [], {}
        if variant in DQ_VARIANTS:
            (D0, D1), parts, padded = DQ_VARIANTS[variant]
            # padded: partial p of row b at arena[4 + p * pstride + b * bstride + 4 ..], dq0's
            # columns then dq1's, NaN everywhere else; else one contiguous [B][D0] dq0
            bstride = D0 + D1 + 8 if padded else D0
            pstride = B * bstride + 16 if padded else 0
            c0 = 4 if padded else 0
            self.arena = arena = torch.full((4 + (parts - 1) * pstride + B * bstride + 4,), NAN, device=dev)
            block = lambda p: arena[4 + p * pstride:][:B * bstride].view(B, bstride)   # noqa: E731
            for name, D, col in (("0", D0, c0), ("1", D1, c0 + D0)):
                if D == 0:
                    continue
                part, wq = f(parts, B, D, scale=0.3), f(U, D, scale=0.1)
                for p in range(parts):
                    block(p)[:, col:col + D] = part[p].to(dev)
                dqs.append((part.double().sum(0), wq.double()))
                A = A + part.double().abs().sum(0) @ wq.double().abs().T
                wq_buf = Buf(dev, (U, D), wq)
                self.dq_bufs.append(wq_buf)
                dq_kw["dq" + name], dq_kw["wq" + name] = block(0)[:, col:col + D], wq_buf.v
                assert dq_kw["dq" + name].data_ptr() % 16 == 0
            self.arena_nan = int(torch.isnan(arena).sum())
            dq_kw.update(dq_parts=parts, dq_pstride=pstride, dq_bstride=bstride if padded else 0)
        valid = None if lengths is None else t < lengths
        self.ref = R.step_bwd(W.double(), hoff, gates.double(), dd(cp), None if rec is not None else dd(dgn),
                              dd(rec), dd(dy), dqs, dd(dhc), dd(dcc), dd(mc), dd(mh), ZC, ZH, valid=valid)
        ab = lambda x: 0.0 if x is None else x.double().abs()   # noqa: E731
        self.bound = 6e-7 * A + 1e-6 * (1.0 + ab(dy) + ab(dhc) + ab(dcc))
        self.valid = valid
        # with rec the kernel must not read dgates_next: hand it NaN
        dgn_dev = None if dgn is None else Buf(dev, (B, U, 4), None if variant == "rec" else dgn)
        self.ins = dict(W=Buf(dev, (K, U, 4), W), dgates_next=dgn_dev, gates=Buf(dev, (B, U, 4), gates),
                        c_prev=None if cp is None else Buf(dev, (B, U), cp),
                        dy=None if dy is None else Buf(dev, (B, U), dy, strided=True),
                        dh_carry=None if dhc is None else Buf(dev, (B, U), dhc),
                        dc_carry=None if dcc is None else Buf(dev, (B, U), dcc),
                        mask_c=None if mc is None else Buf(dev, (B, U), mc),
                        mask_h=None if mh is None else Buf(dev, (B, U), mh),
                        rec=None if rec is None else Buf(dev, (B, U), rec, strided=True))
        self.outs = dict(dgates=Buf(dev, (B, U, 4)), dh_carry_out=Buf(dev, (B, U)),
                         dc_carry_out=Buf(dev, (B, U)))
        self.kw = dict(B=B, U=U, K=K, hoff=hoff, t=t, zc=ZC, zh=ZH,
                       lengths=None if lengths is None else lengths.to(dev),
                       **{k: _view_of(v) for k, v in self.ins.items()},
                       **{k: v.v for k, v in self.outs.items()}, **dq_kw)

    def got(self):
        o = self.outs
        return o["dgates"].cpu(), o["dh_carry_out"].cpu(), o["dc_carry_out"].cpu()

    def check(self):
        for b in list(self.ins.values()) + list(self.outs.values()) + self.dq_bufs:
            assert b is None or b.intact()
        if hasattr(self, "arena"):
            assert int(torch.isnan(self.arena).sum()) == self.arena_nan
        worst = 0.0
        for got, ref in zip(self.got(), self.ref):
            assert bool(torch.isfinite(got).all())
            bound = self.bound.unsqueeze(-1) if got.dim() == 3 else self.bound
            worst = max(worst, float(((got - ref).abs() / bound).max()))
        return worst


BWD_SHAPES = [(1, 4), (3, 6), (9, 64), (17, 130), (32, 256)]
BWD_VARIANTS = ["masks", "eval", "last", "rec", "nulls", "lengths", "dq0", "dq01", "dqcap"]


@pytest.mark.parametrize("variant", BWD_VARIANTS)
@pytest.mark.parametrize("hoff", [0, 8])
@pytest.mark.parametrize("B,U", BWD_SHAPES)
def test_step_bwd(cuda, B, U, hoff, variant):
    """sat_lstm_step_bwd, K = U + hoff: masks / the eval blend with dgates_next given; the last
    step (dgates_next NULL, eval); rec given with dgates_next filled with NaN (not read); dy,
    dh_carry, dc_carry and c_prev NULL; invalid lengths rows (carries pass through, dgates = 0);
    dq0 alone (contiguous, one part); dq0 + dq1 of widths (128, 64) as sums of 3 partials in a
    NaN-padded arena (dq_pstride, dq_bstride); widths (4, 316), the cap of 320.
    Largest err/bound observed: 0.15."""
    from sat_amd import kernels
    c = Bwd(cuda, B, U, hoff, variant, seed=100 * B + U + hoff)
    kernels.lstm_step_bwd(**c.kw)
    worst = c.check()
    _note("test_step_bwd", worst)
    assert worst <= 1.0
    if variant == "lengths":
        dg, dh, dc = c.got()
        inv = ~c.valid
        assert int(inv.sum()) >= 1
        assert torch.equal(dg[inv], torch.zeros_like(dg[inv]))
        assert torch.equal(dc[inv], c.ins["dc_carry"].cpu()[inv])


def test_step_bwd_query_width_refused(cuda):
    """dq0 + dq1 of 4 + 320 = 324 columns: past the cap, refused before any launch."""
    from sat_amd import kernels
    from sat_amd._lib import SatLibraryError, SAT_ERR_ARGUMENT
    c = Bwd(cuda, 3, 8, 0, "masks", seed=3)
    kw = dict(c.kw, dq0=torch.zeros(3, 4, device=cuda), wq0=torch.zeros(8, 4, device=cuda),
              dq1=torch.zeros(3, 320, device=cuda), wq1=torch.zeros(8, 320, device=cuda))
    with pytest.raises(SatLibraryError) as e:
        kernels.lstm_step_bwd(**kw)
    assert e.value.rc == SAT_ERR_ARGUMENT
    assert all(bool(torch.isnan(o.buf).all()) for o in c.outs.values())


@pytest.mark.parametrize("what", ["gates", "dgates"])
def test_step_bwd_alignment_refused(cuda, what):
    """A misaligned gates / dgates (one float4 per (row, unit)) is refused by check_bwd."""
    from sat_amd import kernels
    from sat_amd._lib import SatLibraryError, SAT_ERR_ARGUMENT
    c = Bwd(cuda, 3, 8, 0, "masks", seed=4)
    kw = dict(c.kw)
    kw[what] = _off1(cuda, 3, 8, 4)
    for call in (lambda: kernels.lstm_step_bwd(**kw), lambda: kernels.lstm_steps_bwd([kw])):
        with pytest.raises(SatLibraryError) as e:
            call()
        assert e.value.rc == SAT_ERR_ARGUMENT
    assert all(bool(torch.isnan(o.buf).all()) for o in c.outs.values())


def test_steps_bwd_multi(cuda):
    """Four reverse steps of different B, U, hoff and options in ONE sat_lstm_steps_bwd launch are
    bit-equal to four single launches and meet the bounds; 0 and 5 problems are refused.
    Largest err/bound observed: 0.06."""
    from sat_amd import kernels
    from sat_amd._lib import SatLibraryError, SAT_ERR_ARGUMENT
    spec = [(3, 6, 8, "dq01"), (9, 64, 0, "lengths"), (17, 130, 8, "rec"), (32, 256, 0, "eval")]
    mk = lambda: [Bwd(cuda, B, U, hoff, v, seed=50 + i) for i, (B, U, hoff, v) in enumerate(spec)]  # noqa: E731
    together, single = mk(), mk()
    kernels.lstm_steps_bwd([c.kw for c in together])
    for c in single:
        kernels.lstm_steps_bwd([c.kw])
    for a, b in zip(together, single):
        worst = a.check()
        _note("test_steps_bwd_multi", worst)
        assert worst <= 1.0
        for x, y in zip(a.got(), b.got()):
            assert torch.equal(x, y)
    for steps in ([], [single[0].kw] * 5):
        with pytest.raises(SatLibraryError) as e:
            kernels.lstm_steps_bwd(steps)
        assert e.value.rc == SAT_ERR_ARGUMENT
