"""sat_encoder_lstm_fwd / _bwd (csrc/encoder_lstm.hip, the persistent BiLSTM and its BPTT) and the
per-step schedule it replaces (sat_lstm_steps_fwd / _bwd driven as model.py and backward.py drive
them), each against tests/lstm_ref.bilstm in float64 -- both schedules tied to the reference, not
merely to each other.  N below, at and just past the BPTT's 8-step LDS-DMA chunk.

Tolerance, from the reference alone: per case lstm_ref.bilstm also runs in float32 on the CPU;
E32 = max |ref32 - ref64|, separately over the forward outputs (H, CS, HS, G) and over the gate
gradients.  The kernels (exp + reciprocal activations of ~3 ulp where libm gives <= 1, another
summation order) must stay within 8 max(E32, 2.5e-7).  The gate gradients are autograd of
sum(H . DY) w.r.t. X_fw / X_bw; the kernels' BPTT is fed their own forward's G and CS.
"""
import pytest
import torch

import lstm_ref as R

pytestmark = pytest.mark.gpu

U = 128
ZC = ZH = 0.1
CASES = [(1, 1), (2, 7), (3, 8), (3, 9), (2, 16), (5, 17)]


def _note(name, what, ratio):
    print(f"RATIO {name} {what} {ratio:.4f}")


def _lengths(B, N):
    """always one full row and (B > 1) one row of length 1; the others a middle value"""
    return torch.tensor(([N, 1] + [N // 2 + 1] * B)[:B])


class Case:
    def __init__(self, B, N, masked, seed):
        g = torch.Generator().manual_seed(seed)
        f = lambda *s, scale=1.0: (scale * torch.randn(*s, generator=g)).float()   # noqa: E731
        self.B, self.N = B, N
        self.X = f(2, B, N, 4 * U)                         # both directions' halves of one buffer
        self.W = [f(U, U, 4, scale=0.1) for _ in range(2)]
        self.init = [f(B, U, scale=0.5) for _ in range(4)]  # c_fw, h_fw, c_bw, h_bw
        self.masks = None
        if masked:
            self.masks = tuple((torch.rand(N, B, U, generator=g) < 0.9).float() for _ in range(4))
        self.lengths = _lengths(B, N)
        self.DY = f(B, N, 2 * U)
        self.ref, self.ref_dg = self._run(torch.float64)
        r32, dg32 = self._run(torch.float32)
        flat = lambda r: torch.cat([t.double().reshape(-1) for t in (r[0], *r[1], *r[2], *r[3])])  # noqa: E731
        self.e32_fwd = float((flat(r32) - flat(self.ref)).abs().max())
        self.e32_bwd = max(float((a.double() - b).abs().max()) for a, b in zip(dg32, self.ref_dg))
        self.tol_fwd = 8.0 * max(self.e32_fwd, 2.5e-7)
        self.tol_bwd = 8.0 * max(self.e32_bwd, 2.5e-7)

    def _run(self, dt):
        X = [self.X[d].to(dt).requires_grad_(True) for d in range(2)]
        masks = None if self.masks is None else tuple(m.to(dt) for m in self.masks)
        out = R.bilstm(X[0], X[1], self.W[0].to(dt), self.W[1].to(dt), self.lengths, masks, ZC, ZH,
                       init=[s.to(dt) for s in self.init])
        (out[0] * self.DY.to(dt)).sum().backward()
        # DG layout: [N][B][4U]
        dg = [x.grad.transpose(0, 1).contiguous() for x in X]
        det = lambda ts: tuple(t.detach() for t in ts)   # noqa: E731
        return (out[0].detach(), det(out[1]), det(out[2]), det(out[3])), dg

    def device(self, dev):
        """Device operands: NaN-filled outputs, state histories NaN except the initial rows."""
        B, N = self.B, self.N
        d = dict(X=self.X.to(dev), W=[w.to(dev) for w in self.W], lengths=self.lengths.to(dev),
                 masks=None if self.masks is None else [m.to(dev) for m in self.masks],
                 H=torch.full((B, N, 2 * U), float("nan"), device=dev), DY=self.DY.to(dev),
                 CS=[torch.full((N + 1, B, U), float("nan"), device=dev) for _ in range(2)],
                 HS=[torch.full((N + 1, B, U), float("nan"), device=dev) for _ in range(2)],
                 G=[torch.full((N, B, 4 * U), float("nan"), device=dev) for _ in range(2)],
                 DG=[torch.full((N, B, 4 * U), float("nan"), device=dev) for _ in range(2)])
        for i in range(2):
            r0 = N if i else 0
            d["CS"][i][r0] = self.init[2 * i].to(dev)
            d["HS"][i][r0] = self.init[2 * i + 1].to(dev)
        return d

    def check_fwd(self, d):
        """max err / E32 over H, CS, HS, G of both directions; exact zeros past the lengths; the
        initial state rows as given."""
        B, N = self.B, self.N
        H, CS, HS, G = self.ref
        worst = float((d["H"].double().cpu() - H).abs().max())
        for i in range(2):
            r0 = N if i else 0
            assert torch.equal(d["CS"][i][r0].cpu(), self.init[2 * i])
            assert torch.equal(d["HS"][i][r0].cpu(), self.init[2 * i + 1])
            worst = max(worst, float((d["CS"][i].double().cpu() - CS[i]).abs().max()),
                        float((d["HS"][i].double().cpu() - HS[i]).abs().max()),
                        float((d["G"][i].double().cpu().view(N, B, U, 4) - G[i]).abs().max()))
        for b, L in enumerate(self.lengths.tolist()):
            assert not bool(d["H"][b, L:].any())
            assert not bool(d["G"][0][L:, b].any()) and not bool(d["G"][1][L:, b].any())
        assert worst == worst                              # no NaN left in any output
        return worst

    def check_bwd(self, d):
        worst = 0.0
        for i in range(2):
            got = d["DG"][i].double().cpu()
            worst = max(worst, float((got - self.ref_dg[i]).abs().max()))
            for b, L in enumerate(self.lengths.tolist()):
                assert not bool(d["DG"][i][L:, b].any())
        assert worst == worst
        return worst


def _mask(d, i, n=None):
    if d["masks"] is None:
        return None
    return d["masks"][i] if n is None else d["masks"][i][n]


def _persistent(c, d):
    from sat_amd import kernels
    B, N = c.B, c.N
    m = [_mask(d, i) for i in range(4)]
    X = d["X"]
    kernels.encoder_lstm_fwd(
        B=B, N=N, U=U, zc=ZC, zh=ZH, X_fw=X[0], X_bw=X[1], x_sb=X.stride(1), x_sn=X.stride(2),
        W_fw=d["W"][0], W_bw=d["W"][1], mc_fw=m[0], mh_fw=m[1], mc_bw=m[2], mh_bw=m[3],
        lengths=d["lengths"], H=d["H"], h_sb=d["H"].stride(0), h_sn=d["H"].stride(1),
        CS_fw=d["CS"][0], HS_fw=d["HS"][0], CS_bw=d["CS"][1], HS_bw=d["HS"][1],
        G_fw=d["G"][0], G_bw=d["G"][1])
    kernels.encoder_lstm_bwd(
        B=B, N=N, U=U, zc=ZC, zh=ZH, W_fw=d["W"][0], W_bw=d["W"][1], G_fw=d["G"][0], G_bw=d["G"][1],
        CS_fw=d["CS"][0], CS_bw=d["CS"][1], mc_fw=m[0], mh_fw=m[1], mc_bw=m[2], mh_bw=m[3],
        lengths=d["lengths"], DY=d["DY"], dy_sb=d["DY"].stride(0), dy_sn=d["DY"].stride(1),
        DG_fw=d["DG"][0], DG_bw=d["DG"][1])


def _per_step(c, d):
    """model.py encoder_fwd's and backward.py's non-persistent schedule: forward step n of the
    forward cell with step N-1-n of the backward cell in one launch; the same pairing reversed."""
    from sat_amd import kernels
    from sat_amd.backward import _LstmBwd
    B, N = c.B, c.N

    def fwd(i, n):
        rev = bool(i)
        out = d["H"][:, :, U:] if rev else d["H"][:, :, :U]
        prev, nxt = (n + 1, n) if rev else (n, n + 1)
        return dict(B=B, U=U, K=U, t=n, xproj=d["X"][i][:, n], rin=d["HS"][i][prev], W=d["W"][i],
                    c_prev=d["CS"][i][prev], h_prev=d["HS"][i][prev],
                    mask_c=_mask(d, 2 * i, n), mask_h=_mask(d, 2 * i + 1, n), zc=ZC, zh=ZH,
                    h_raw=out[:, n], c_out=d["CS"][i][nxt], h_out=d["HS"][i][nxt],
                    gates=d["G"][i][n], lengths=d["lengths"])

    for n in range(N):
        kernels.lstm_steps_fwd([fwd(0, n), fwd(1, N - 1 - n)])
    runs = [_LstmBwd(B, U, d["X"].device) for _ in range(2)]

    def bwd(i, n):
        rev = bool(i)
        half = slice(U, 2 * U) if rev else slice(0, U)
        nt = (n - 1 if n > 0 else None) if rev else (n + 1 if n + 1 < N else None)
        return runs[i].desc(
            B=B, U=U, K=U, hoff=0, t=n, W=d["W"][i],
            dgates_next=None if nt is None else d["DG"][i][nt], gates=d["G"][i][n],
            c_prev=d["CS"][i][n + 1] if rev else d["CS"][i][n], dy=d["DY"][:, n, half],
            mask_c=_mask(d, 2 * i, n), mask_h=_mask(d, 2 * i + 1, n), zc=ZC, zh=ZH,
            dgates=d["DG"][i][n], lengths=d["lengths"])

    for j in range(N):
        kernels.lstm_steps_bwd([bwd(0, N - 1 - j), bwd(1, j)])


_CASES = {}


def _case(B, N, masked):
    key = (B, N, masked)
    if key not in _CASES:
        _CASES[key] = Case(B, N, masked, seed=17 * B + N + 1000 * masked)
    return _CASES[key]


@pytest.mark.parametrize("masked", [True, False], ids=["masks", "eval"])
@pytest.mark.parametrize("B,N", CASES)
def test_encoder_lstm_persistent(cuda, B, N, masked):
    """The persistent kernels: H, CS, HS, G of both directions and DG_fw, DG_bw within
    8 max(E32, 2.5e-7) of float64.  Largest err/E32 observed (forward / gradients) per (B, N):
    (1,1) 0.63 / 0.65, (2,7) 0.65 / 1.20, (3,8) 0.79 / 0.99, (3,9) 0.77 / 1.02,
    (2,16) 0.87 / 0.91, (5,17) 0.84 / 1.07 (the bar is 8)."""
    c = _case(B, N, masked)
    d = c.device(cuda)
    _persistent(c, d)
    ef, eb = c.check_fwd(d), c.check_bwd(d)
    _note("test_encoder_lstm_persistent", f"({B},{N}) fwd", ef / max(c.e32_fwd, 2.5e-7))
    _note("test_encoder_lstm_persistent", f"({B},{N}) bwd", eb / max(c.e32_bwd, 2.5e-7))
    assert ef <= c.tol_fwd, (ef, c.e32_fwd)
    assert eb <= c.tol_bwd, (eb, c.e32_bwd)


@pytest.mark.parametrize("masked", [True, False], ids=["masks", "eval"])
@pytest.mark.parametrize("B,N", CASES)
def test_encoder_lstm_per_step(cuda, B, N, masked):
    """The per-step schedule on the same inputs, against the same reference at the same
    tolerance.  Largest err/E32 observed (forward / gradients) per (B, N): (1,1) 0.84 / 0.51, (2,7) 0.76 / 1.20,
    (3,8) 0.79 / 0.99, (3,9) 0.82 / 1.26, (2,16) 0.73 / 1.04, (5,17) 1.12 / 1.15 (the bar is 8)."""
    c = _case(B, N, masked)
    d = c.device(cuda)
    _per_step(c, d)
    ef, eb = c.check_fwd(d), c.check_bwd(d)
    _note("test_encoder_lstm_per_step", f"({B},{N}) fwd", ef / max(c.e32_fwd, 2.5e-7))
    _note("test_encoder_lstm_per_step", f"({B},{N}) bwd", eb / max(c.e32_bwd, 2.5e-7))
    assert ef <= c.tol_fwd, (ef, c.e32_fwd)
    assert eb <= c.tol_bwd, (eb, c.e32_bwd)


def _off1(t):
    """``t``'s values in a view one float past a 16-byte boundary."""
    v = torch.zeros(t.numel() + 8, device=t.device)[5:5 + t.numel()].view(t.shape)
    assert v.data_ptr() % 16 == 4
    return v


def _args(c, d):
    B, N = c.B, c.N
    m = [_mask(d, i) for i in range(4)]
    X = d["X"]
    fwd = dict(B=B, N=N, U=U, zc=ZC, zh=ZH, X_fw=X[0], X_bw=X[1], x_sb=X.stride(1), x_sn=X.stride(2),
               W_fw=d["W"][0], W_bw=d["W"][1], mc_fw=m[0], mh_fw=m[1], mc_bw=m[2], mh_bw=m[3],
               lengths=d["lengths"], H=d["H"], h_sb=d["H"].stride(0), h_sn=d["H"].stride(1),
               CS_fw=d["CS"][0], HS_fw=d["HS"][0], CS_bw=d["CS"][1], HS_bw=d["HS"][1],
               G_fw=d["G"][0], G_bw=d["G"][1])
    bwd = dict(B=B, N=N, U=U, zc=ZC, zh=ZH, W_fw=d["W"][0], W_bw=d["W"][1], G_fw=d["G"][0],
               G_bw=d["G"][1], CS_fw=d["CS"][0], CS_bw=d["CS"][1], mc_fw=m[0], mh_fw=m[1], mc_bw=m[2],
               mh_bw=m[3], lengths=d["lengths"], DY=d["DY"], dy_sb=d["DY"].stride(0),
               dy_sn=d["DY"].stride(1), DG_fw=d["DG"][0], DG_bw=d["DG"][1])
    return fwd, bwd


@pytest.mark.parametrize("what", ["mc_fw", "mh_fw", "mc_bw", "mh_bw"])
def test_encoder_lstm_fwd_alignment_refused(cuda, what):
    """A misaligned zoneout mask is refused by sat_encoder_lstm_fwd before any launch."""
    from sat_amd import kernels
    from sat_amd._lib import SatLibraryError, SAT_ERR_ARGUMENT
    c = _case(2, 7, True)
    d = c.device(cuda)
    fwd, _ = _args(c, d)
    fwd[what] = _off1(fwd[what])
    with pytest.raises(SatLibraryError) as e:
        kernels.encoder_lstm_fwd(**fwd)
    assert e.value.rc == SAT_ERR_ARGUMENT
    assert bool(torch.isnan(d["H"]).all()) and bool(torch.isnan(d["G"][0]).all())


@pytest.mark.parametrize("what", ["DY", "dy_sb", "dy_sn", "CS_fw", "CS_bw", "mc_fw", "mh_fw", "mc_bw",
                                  "mh_bw"])
def test_encoder_lstm_bwd_alignment_refused(cuda, what):
    """The BPTT's LDS-DMA operands: a misaligned DY / CS / mask, or a DY stride of 4k + 1, is
    refused by sat_encoder_lstm_bwd before any launch."""
    from sat_amd import kernels
    from sat_amd._lib import SatLibraryError, SAT_ERR_ARGUMENT
    c = _case(2, 7, True)
    d = c.device(cuda)
    _, bwd = _args(c, d)
    if what in ("dy_sb", "dy_sn"):
        bwd[what] += 1
        assert bwd[what] % 4 == 1
    else:
        bwd[what] = _off1(bwd[what])
    with pytest.raises(SatLibraryError) as e:
        kernels.encoder_lstm_bwd(**bwd)
    assert e.value.rc == SAT_ERR_ARGUMENT
    assert bool(torch.isnan(d["DG"][0]).all()) and bool(torch.isnan(d["DG"][1]).all())
