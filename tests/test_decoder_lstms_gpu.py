"""sat_decoder_lstms_fwd / _bwd (csrc/decoder_lstm_persistent.hip: both decoder ZoneoutLSTM layers
for all T' steps in one launch, and their BPTT) called directly, against tests/lstm_ref.decoder_stack
in float64; and the per-step schedule they replace (sat_lstm_steps_fwd, X2 by a GEMM) against the
same reference, so the h1' -> LSTM2 wiring has two implementations tied to one restatement.

Cases (B, T') are the smallest that reach each edge of the layout and the schedule: group g owns
utterances g and g + 16, so B = 1 leaves 15 groups empty, 16 fills every group once, 17 gives one
group two utterances, 31 leaves one group with a single one, 32 is full; T' = 1 runs each layer in
an iteration of its own, T' = 2 uses each hand-off slot once, T' >= 3 reuses slots, the BPTT's
parity tag flips every two steps; (17, 40) cycles slots and tags many times.

Inputs: X1 ~ N(0, 1) is LSTM1's hoisted projection, so it alone gives pre-activations of unit
variance.  The weights are N(0, 0.1^2): the state rows have an rms of about 0.25-0.3 (|h| < 1),
so the 256 recurrent rows of LSTM1 add a term of standard deviation 0.1 * 16 * 0.3 ~ 0.5 and
LSTM2's 512 rows with b2 ~ N(0, 0.3^2) give ~0.7.  Measured over the cases below: 1.1 (LSTM1)
and 0.7 (LSTM2), largest |pre-activation| 6.4, so sigmoid and tanh stay on their slopes (no gate
saturates and hides an error) while the recurrent terms still carry a third of the variance.
Initial states ~ N(0, 0.5^2), non-zero; zc != zh.

Tolerance, from the reference alone: per case decoder_stack and its autograd also run in float32
on the CPU; E32 = max |ref32 - ref64|, separately over the eight forward histories and over the
two gate-gradient tensors.  The kernels (exp + reciprocal activations of ~3 ulp where libm gives
<= 1, another summation order, <= 1 ulp from the BPTT's parity tag in the mantissa LSB) must stay
within 8 max(E32, 2.5e-7).  The gate gradients are autograd of sum(H2RAW . DH2) w.r.t. X1 and a
zero X2 added to LSTM2's pre-activations; the BPTT is fed the kernels' own forward G and CS.

That the comparison can fail (CPU only, on a copy of the reference): feeding LSTM2 LSTM1's
zoned-out state h1 instead of its raw output h1' moves the float64 forward result of case (17, 5)
under masks by 1.01, 1.3e5 x its bar 8 E32 = 7.5e-6.

Every output lives in a NaN-filled buffer with NaN guard floats on both sides (the guards must
survive, no NaN may remain inside); every launch is followed by one synchronize and a look at
err[0] and at the outputs, and a test stops at the first that is wrong.
"""
import pytest
import torch

import lstm_ref as R

pytestmark = pytest.mark.gpu

U = 256
ZC, ZH = 0.1, 0.15
W_SCALE, B2_SCALE, INIT_SCALE = 0.1, 0.3, 0.5
GUARD = 64                   # floats on each side of an output: 256 bytes, keeps 16-byte alignment
FLOOR = 2.5e-7
CASES = [(1, 1), (1, 2), (2, 3), (16, 2), (17, 5), (31, 4), (32, 3), (32, 9), (17, 40)]
FWD = ("H1RAW", "C1S", "H1S", "G1", "H2RAW", "C2S", "H2S", "G2")
STATES = ("C1S", "H1S", "C2S", "H2S")
BWD = ("DG1", "DG2")
NAN = float("nan")


def _note(name, what, ratio):
    print(f"RATIO {name} {what} {ratio:.4f}")


class Case:
    def __init__(self, B, T, masked, seed):
        g = torch.Generator().manual_seed(seed)
        f = lambda *s, scale=1.0: (scale * torch.randn(*s, generator=g)).float()   # noqa: E731
        self.B, self.T = B, T
        self.X1 = f(T, B, 4 * U)
        self.W1r = f(U, U, 4, scale=W_SCALE)
        self.W2 = f(2 * U, U, 4, scale=W_SCALE)
        self.b2 = f(U, 4, scale=B2_SCALE)
        self.init = [f(B, U, scale=INIT_SCALE) for _ in range(4)]       # c1, h1, c2, h2
        self.masks = None
        if masked:
            self.masks = tuple((torch.rand(T, B, U, generator=g) < 0.9).float() for _ in range(4))
        self.DH2 = f(T, B, U)
        self.ref, self.ref_dg = self._run(torch.float64)
        r32, dg32 = self._run(torch.float32)
        diff = lambda a, b: max(float((x.double() - y).abs().max()) for x, y in zip(a, b))  # noqa: E731
        self.e32_fwd = diff(r32.values(), self.ref.values())
        self.e32_bwd = diff(dg32.values(), self.ref_dg.values())
        self.tol_fwd = 8.0 * max(self.e32_fwd, FLOOR)
        self.tol_bwd = 8.0 * max(self.e32_bwd, FLOOR)

    def _run(self, dt):
        X1 = self.X1.to(dt).requires_grad_(True)
        X2 = torch.zeros(self.T, self.B, 4 * U, dtype=dt, requires_grad=True)
        masks = None if self.masks is None else tuple(m.to(dt) for m in self.masks)
        out = R.decoder_stack(X1, self.W1r.to(dt), self.W2.to(dt), self.b2.to(dt),
                              [s.to(dt) for s in self.init], masks, ZC, ZH, X2=X2)
        (out[4] * self.DH2.to(dt)).sum().backward()
        return ({n: t.detach() for n, t in zip(FWD, out)}, {"DG1": X1.grad, "DG2": X2.grad})

    def shapes(self):
        T, B = self.T, self.B
        raw, st, g = (T, B, U), (T + 1, B, U), (T, B, 4 * U)
        return dict(H1RAW=raw, C1S=st, H1S=st, G1=g, H2RAW=raw, C2S=st, H2S=st, G2=g, DG1=g, DG2=g)

    def device(self, dev):
        """Device operands.  ``o``: every output as a view into ``whole``, a NaN-filled buffer
        with GUARD floats on both sides; the state histories carry the initial state in row 0."""
        d = dict(X1=self.X1.to(dev), W1r=self.W1r.to(dev), W2=self.W2.to(dev), b2=self.b2.to(dev),
                 masks=[None] * 4 if self.masks is None else [m.to(dev) for m in self.masks],
                 DH2=self.DH2.to(dev), err=torch.zeros(2, 2, dtype=torch.int32, device=dev),
                 o={}, whole={})
        for name, shape in self.shapes().items():
            d["o"][name], d["whole"][name] = _guarded(shape, dev)
        for name, s in zip(STATES, self.init):
            d["o"][name][0] = s.to(dev)
        return d

    def check_guards(self, d, names):
        for name in names:
            w, n = d["whole"][name], d["o"][name].numel()
            assert bool(torch.isnan(w[:GUARD]).all()) and bool(torch.isnan(w[GUARD + n:]).all()), name

    def check_fwd(self, d):
        """max |got - ref64| over the eight histories; guards intact, row 0 as given."""
        self.check_guards(d, FWD)
        for name, s in zip(STATES, self.init):
            assert torch.equal(d["o"][name][0].cpu(), s), name
        worst = max(float((d["o"][n].double().cpu() - self.ref[n]).abs().max()) for n in FWD)
        assert worst == worst
        return worst

    def check_bwd(self, d):
        self.check_guards(d, BWD)
        worst = max(float((d["o"][n].double().cpu() - self.ref_dg[n]).abs().max()) for n in BWD)
        assert worst == worst
        return worst


def _guarded(shape, dev):
    n = 1
    for s in shape:
        n *= s
    whole = torch.full((n + 2 * GUARD,), NAN, device=dev)
    view = whole[GUARD:GUARD + n].view(shape)
    assert view.data_ptr() % 16 == 0
    return view, whole


def _settle(err, outs, what):
    """After a launch: one synchronize, the kernel's error word, every output finite."""
    torch.cuda.synchronize()
    assert int(err[0].item()) == 0, f"{what}: err[0] != 0 (a hand-off timed out)"
    for name, t in outs.items():
        assert bool(torch.isfinite(t).all()), f"{what}: non-finite {name}"


def _fwd_args(c, d, xch):
    o, m = d["o"], d["masks"]
    return dict(B=c.B, T=c.T, U=U, zc=ZC, zh=ZH, X1=d["X1"], W1r=d["W1r"], W2=d["W2"], b2=d["b2"],
                mask1_c=m[0], mask1_h=m[1], mask2_c=m[2], mask2_h=m[3],
                H1RAW=o["H1RAW"], C1S=o["C1S"], H1S=o["H1S"], G1=o["G1"],
                H2RAW=o["H2RAW"], C2S=o["C2S"], H2S=o["H2S"], G2=o["G2"], xch=xch, err=d["err"][0])


def _bwd_args(c, d, ctr):
    o, m = d["o"], d["masks"]
    return dict(B=c.B, T=c.T, U=U, zc=ZC, zh=ZH, W1r=d["W1r"], W2=d["W2"], G1=o["G1"],
                C1S=o["C1S"], G2=o["G2"], C2S=o["C2S"], DH2=d["DH2"],
                mask1_c=m[0], mask1_h=m[1], mask2_c=m[2], mask2_h=m[3],
                DG1=o["DG1"], DG2=o["DG2"], ctr=ctr, err=d["err"][1])


def _scratch(B, dev):
    """Fresh hand-off scratch of both directions, sized by the library for B."""
    from sat_amd import _lib
    lib = _lib.load()
    return (torch.zeros(int(lib.sat_decoder_lstms_scratch(B)), device=dev),
            torch.zeros(int(lib.sat_decoder_lstms_bwd_scratch(B)), dtype=torch.int32, device=dev))


def _forward(c, d, xch):
    from sat_amd import kernels
    kernels.decoder_lstms_fwd(**_fwd_args(c, d, xch))
    _settle(d["err"][0], {n: d["o"][n] for n in FWD}, "sat_decoder_lstms_fwd")


def _backward(c, d, ctr):
    """The BPTT on the forward's own G and CS (already in ``d``)."""
    from sat_amd import kernels
    kernels.decoder_lstms_bwd(**_bwd_args(c, d, ctr))
    _settle(d["err"][1], {n: d["o"][n] for n in BWD}, "sat_decoder_lstms_bwd")


def _both(c, dev, scratch=None):
    xch, ctr = _scratch(c.B, dev) if scratch is None else scratch
    d = c.device(dev)
    _forward(c, d, xch)
    ef = c.check_fwd(d)
    _backward(c, d, ctr)
    eb = c.check_bwd(d)
    return d, ef, eb


_CASES = {}


def _case(B, T, masked):
    key = (B, T, masked)
    if key not in _CASES:
        _CASES[key] = Case(B, T, masked, seed=41 * B + T + 1000 * masked)
    return _CASES[key]


@pytest.mark.parametrize("masked", [True, False], ids=["masks", "eval"])
@pytest.mark.parametrize("B,T", CASES)
def test_decoder_lstms_persistent(cuda, B, T, masked):
    """The persistent kernels on fresh scratch: the eight forward histories and DG1, DG2 within
    8 max(E32, 2.5e-7) of float64.  Largest err/E32 observed (forward / gradients) per (B, T'):
    (1,1) 0.36 / 0.56, (1,2) 0.48 / 0.72, (2,3) 0.40 / 0.74, (16,2) 0.46 / 0.62,
    (17,5) 0.61 / 0.96, (31,4) 0.61 / 0.82, (32,3) 0.57 / 0.75, (32,9) 0.83 / 1.01,
    (17,40) 1.33 / 0.93 (the bar is 8)."""
    c = _case(B, T, masked)
    d, ef, eb = _both(c, cuda)
    _note("test_decoder_lstms_persistent", f"({B},{T}) fwd", ef / max(c.e32_fwd, FLOOR))
    _note("test_decoder_lstms_persistent", f"({B},{T}) bwd", eb / max(c.e32_bwd, FLOOR))
    assert ef <= c.tol_fwd, (ef, c.e32_fwd)
    assert eb <= c.tol_bwd, (eb, c.e32_bwd)


def _bits(d):
    return {n: d["o"][n].cpu() for n in FWD + BWD}


def test_decoder_lstms_reused_scratch(cuda):
    """One scratch pair sized for B = 32 serves (32, 9) and then (17, 2) with other inputs: the
    tags and granules the longer, wider run left behind (another layout, later epochs) must not
    satisfy the second run's polls -- the call zeroes what it uses.  The second run meets the
    bars and is bit-identical to (17, 2) on fresh scratch.  Largest err/E32 observed of the second
    run (forward / gradients): 0.42 / 0.69 (the bar is 8)."""
    shared = _scratch(32, cuda)
    first, second = _case(32, 9, True), _case(17, 2, True)
    _, ef, eb = _both(first, cuda, shared)
    assert ef <= first.tol_fwd and eb <= first.tol_bwd, (ef, eb)
    d1, ef, eb = _both(second, cuda, shared)
    _note("test_decoder_lstms_reused_scratch", "(17,2) fwd", ef / max(second.e32_fwd, FLOOR))
    _note("test_decoder_lstms_reused_scratch", "(17,2) bwd", eb / max(second.e32_bwd, FLOOR))
    assert ef <= second.tol_fwd, (ef, second.e32_fwd)
    assert eb <= second.tol_bwd, (eb, second.e32_bwd)
    d2, _, _ = _both(second, cuda)
    a, b = _bits(d1), _bits(d2)
    for n in a:
        assert torch.equal(a[n], b[n]), n


@pytest.mark.parametrize("B,T", [(17, 5), (32, 9)])
def test_decoder_lstms_deterministic(cuda, monkeypatch, B, T):
    """The same case twice, and once more with SAT_XCD_LOCAL=0 (sc1 hand-off stores everywhere):
    forward histories and gate gradients bit-identical -- neither the order in which hand-offs
    arrive nor the store policy may reach the arithmetic."""
    c = _case(B, T, True)
    runs = [_bits(_both(c, cuda)[0]) for _ in range(2)]
    monkeypatch.setenv("SAT_XCD_LOCAL", "0")
    runs.append(_bits(_both(c, cuda)[0]))
    for other in runs[1:]:
        for n in runs[0]:
            assert torch.equal(runs[0][n], other[n]), n


@pytest.mark.parametrize("masked", [True, False], ids=["masks", "eval"])
@pytest.mark.parametrize("B,T", [(17, 5), (32, 3)])
def test_decoder_lstms_per_step_forward(cuda, B, T, masked):
    """The per-step schedule of decoder.py's non-persistent branch on the same inputs: LSTM1 step
    by step (sat_lstm_steps_fwd), X2 = H1RAW @ W2[:U] + b2 as one GEMM, LSTM2 step by step over
    its recurrent rows -- the same reference, the same bar.  Largest err/E32 observed per (B, T'):
    (17,5) 1.03, (32,3) 0.65 (the bar is 8)."""
    from sat_amd import kernels
    c = _case(B, T, masked)
    d = c.device(cuda)
    o, m = d["o"], d["masks"]

    def layer(X, Wr, mc, mh, HRAW, CS, HS, G):
        for t in range(T):
            kernels.lstm_steps_fwd([dict(
                B=B, U=U, K=U, t=t, xproj=X[t], rin=HS[t], W=Wr, c_prev=CS[t], h_prev=HS[t],
                mask_c=None if mc is None else mc[t], mask_h=None if mh is None else mh[t],
                zc=ZC, zh=ZH, h_raw=HRAW[t], c_out=CS[t + 1], h_out=HS[t + 1], gates=G[t])])
            torch.cuda.synchronize()
        assert bool(torch.isfinite(HRAW).all()) and bool(torch.isfinite(G).all())

    layer(d["X1"], d["W1r"], m[0], m[1], o["H1RAW"], o["C1S"], o["H1S"], o["G1"])
    X2 = kernels.linear(o["H1RAW"].view(T * B, U), d["W2"][:U].view(U, 4 * U), d["b2"].view(4 * U))
    torch.cuda.synchronize()
    layer(X2.view(T, B, 4 * U), d["W2"][U:], m[2], m[3], o["H2RAW"], o["C2S"], o["H2S"], o["G2"])
    ef = c.check_fwd(d)
    _note("test_decoder_lstms_per_step_forward", f"({B},{T}) fwd", ef / max(c.e32_fwd, FLOOR))
    assert ef <= c.tol_fwd, (ef, c.e32_fwd)


def _off1(t):
    """``t``'s values in a view one float past a 16-byte boundary of a larger buffer."""
    big = torch.full((t.numel() + 8,), NAN, device=t.device)
    v = big[5:5 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def _refused(fn, args):
    from sat_amd._lib import SatLibraryError, SAT_ERR_ARGUMENT
    with pytest.raises(SatLibraryError) as e:
        fn(**args)
    assert e.value.rc == SAT_ERR_ARGUMENT
    torch.cuda.synchronize()


def _bend(args, what):
    """One refusal's change to a valid argument set.  None of them, wrongly accepted, could run
    out of bounds: sizes only shrink below the buffers, B = 33 comes with buffers for 33."""
    if what == "U128":
        args["U"] = 128
    elif what == "B0":
        args["B"] = 0
    elif what == "T0":
        args["T"] = 0
    elif what == "three_masks":
        args["mask2_h"] = None
    elif what != "B33":
        args[what[:-4]] = _off1(args[what[:-4]])
    return args


@pytest.mark.parametrize("what", ["U128", "B0", "B33", "T0", "three_masks", "X1_off", "G1_off"])
def test_decoder_lstms_fwd_refused(cuda, what):
    """sat_decoder_lstms_fwd refuses, before any launch: U != 256, B = 0, B = 33, T = 0, three of
    the four masks, X1 or G1 one float off a 16-byte boundary.  Every output stays NaN."""
    from sat_amd import kernels
    c = _case(33 if what == "B33" else 2, 3, True)
    d = c.device(cuda)
    args = _bend(_fwd_args(c, d, _scratch(c.B, cuda)[0]), what)
    _refused(kernels.decoder_lstms_fwd, args)
    for n in FWD:
        w = d["whole"][n]
        keep = GUARD + (c.B * U if n in STATES else 0)       # row 0 of a state history was given
        assert bool(torch.isnan(w[:GUARD]).all()) and bool(torch.isnan(w[keep:]).all()), n
    assert bool(torch.isnan(args["G1"]).all())


@pytest.mark.parametrize("what", ["U128", "B0", "B33", "T0", "three_masks", "G1_off", "DG1_off"])
def test_decoder_lstms_bwd_refused(cuda, what):
    """sat_decoder_lstms_bwd refuses the same, and a DG1 one float off; its inputs here are the
    reference's finite G and CS, so an accepted call would have left numbers in DG1 / DG2."""
    from sat_amd import kernels
    c = _case(33 if what == "B33" else 2, 3, True)
    d = c.device(cuda)
    for n in ("G1", "C1S", "G2", "C2S"):
        d["o"][n].copy_(c.ref[n].float())
    dg1 = d["o"]["DG1"]
    args = _bend(_bwd_args(c, d, _scratch(c.B, cuda)[1]), what)
    _refused(kernels.decoder_lstms_bwd, args)
    for n in BWD:
        assert bool(torch.isnan(d["whole"][n]).all()), n
    assert bool(torch.isnan(args["DG1"]).all()) and bool(torch.isnan(dg1).all())
