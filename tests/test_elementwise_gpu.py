"""The small elementwise / data-movement kernels (csrc/elementwise.hip, sat_gemm_rowdot,
sat_attn_query), each against torch float64 on the CPU at ragged and unaligned sizes.

Tolerances: pure data movement is bit-exact; pointwise arithmetic 4e-7 (sum |terms|) + 1e-7; the
two products the gemm bound 6e-7 (|A| |B|) + 1e-7.  The largest err / bound each arithmetic test
has shown on an MI355X is in its docstring.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float("nan")
SIZES = [1, 5, 255, 256, 257, 4099]
F64 = torch.float64


def _note(name, ratio):
    print(f"RATIO {name} {ratio:.4f}")


def _ratio(got, ref, terms):
    got = got.double().cpu()
    assert bool(torch.isfinite(got).all())
    return float(((got - ref).abs() / (4e-7 * terms + 1e-7)).max()) if got.numel() else 0.0


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


# ------------------------------------------------------------------------------ highway

@pytest.mark.parametrize("n", SIZES)
def test_highway_fwd(cuda, n):
    """y = h t + x (1 - t).  Largest err/bound observed: 0.22."""
    from sat_amd import kernels
    g = torch.Generator().manual_seed(n)
    h, t, x = _randn(g, n), torch.rand(n, generator=g), _randn(g, n)
    y = torch.full((n,), NAN, device=cuda)
    kernels.highway_fwd(h.to(cuda), t.to(cuda), x.to(cuda), y)
    hd, td, xd = h.double(), t.double(), x.double()
    r = _ratio(y, hd * td + xd * (1 - td), (hd * td).abs() + (xd * (1 - td)).abs())
    _note("test_highway_fwd", r)
    assert r <= 1.0


@pytest.mark.parametrize("n", SIZES)
def test_highway_act_fwd(cuda, n):
    """h <- relu(h), t <- sigmoid(t) in place, y = h t + x (1 - t); terms |h| + |x| (the gate's
    rounding reaches y through both).  Largest err/bound observed: 0.23."""
    from sat_amd import kernels
    g = torch.Generator().manual_seed(n + 1)
    h, t, x = _randn(g, n), 3.0 * _randn(g, n), _randn(g, n)
    h[::3] = 0.0
    hd_, td_ = h.to(cuda), t.to(cuda)
    y = torch.full((n,), NAN, device=cuda)
    kernels.highway_act_fwd(hd_, td_, x.to(cuda), y)
    hr, tr, xd = torch.relu(h.double()), torch.sigmoid(t.double()), x.double()
    assert torch.equal(hd_.cpu(), torch.relu(h))
    r = max(_ratio(td_, tr, tr), _ratio(y, hr * tr + xd * (1 - tr), hr + xd.abs()))
    _note("test_highway_act_fwd", r)
    assert r <= 1.0


@pytest.mark.parametrize("n", SIZES)
def test_highway_bwd(cuda, n):
    """Against autograd of relu / sigmoid / combine, h and t taken from the kernel's own forward
    (so the h > 0 gate is the kernel's), exact zeros in h_pre.
    Largest err/bound observed: 0.14."""
    from sat_amd import kernels
    g = torch.Generator().manual_seed(n + 2)
    h_pre, t_pre, x, dy = _randn(g, n), _randn(g, n), _randn(g, n), _randn(g, n)
    h_pre[::4] = 0.0
    h, t = h_pre.to(cuda), t_pre.to(cuda)
    kernels.highway_act_fwd(h, t, x.to(cuda), torch.empty(n, device=cuda))
    # float64 autograd at the kernel's forward values: d/dh_pre through relu's gate h > 0,
    # d/dt_pre = dL/dt * t (1 - t)
    hk = h.double().cpu().requires_grad_(True)
    tk = t.double().cpu().requires_grad_(True)
    xk = x.double().requires_grad_(True)
    (hk * tk + xk * (1 - tk)).backward(dy.double())
    ref_dh = torch.where(hk.detach() > 0, hk.grad, torch.zeros_like(hk.grad))
    ref_dt = tk.grad * tk.detach() * (1 - tk.detach())
    out = [torch.full((n,), NAN, device=cuda) for _ in range(3)]
    kernels.highway_bwd(h, t, x.to(cuda), dy.to(cuda), *out)
    gd = dy.double().abs()
    r = max(_ratio(out[0], ref_dh, gd), _ratio(out[1], ref_dt, gd * (hk.detach().abs() + xk.detach().abs())),
            _ratio(out[2], xk.grad, gd))
    assert torch.equal(out[0].cpu()[::4], torch.zeros(n)[::4])
    _note("test_highway_bwd", r)
    assert r <= 1.0


# ------------------------------------------------------------------------------ act_bwd / axpby / add

def _act_ref(act, y):
    """(act'(y) in terms of the activation output, an upper bound on its magnitude's terms)"""
    if act == 0:
        return torch.ones_like(y), torch.ones_like(y)
    if act == 1:
        return (y > 0).to(F64), torch.ones_like(y)
    if act == 2:
        return 1 - y * y, 1 + y * y
    if act == 3:
        return y * (1 - y), y.abs() * (1 + y.abs())
    return (1 - y.abs()) ** 2, (1 + y.abs()) ** 2


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("beta", [0.0, 1.0, -0.5])
@pytest.mark.parametrize("masked", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("act", [0, 1, 2, 3, 4])
def test_act_bwd(cuda, act, masked, beta, n):
    """dx = beta dx + dy act'(y) [mask]; beta == 0 must not read dx (pre-filled with NaN).
    Largest err/bound observed: 0.27."""
    from sat_amd import kernels
    names = {v: k for k, v in kernels.ACT.items() if k is not None}
    g = torch.Generator().manual_seed(n + 10 * act)
    dy, dx0 = _randn(g, n), _randn(g, n)
    y = {0: _randn(g, n), 1: torch.relu(_randn(g, n)), 2: torch.tanh(_randn(g, n)),
         3: torch.sigmoid(_randn(g, n)), 4: torch.nn.functional.softsign(_randn(g, n))}[act]
    mask = (torch.rand(n, generator=g) < 0.5).float() * 2.0 if masked else None
    dx = dx0.to(cuda) if beta != 0.0 else torch.full((n,), NAN, device=cuda)
    kernels.act_bwd(dy.to(cuda), y.to(cuda), dx, names[act], mask=None if mask is None else mask.to(cuda),
                    beta=beta)
    d, mag = _act_ref(act, y.double())
    gm = dy.double() * (1.0 if mask is None else mask.double())
    ref = gm * d + (beta * dx0.double() if beta != 0.0 else 0.0)
    r = _ratio(dx, ref, gm.abs() * mag + abs(beta) * dx0.double().abs())
    _note("test_act_bwd", r)
    assert r <= 1.0


def test_act_bwd_without_output(cuda):
    """The identity needs no activation output (y = None); acts 1-4 without it are refused."""
    from sat_amd import kernels
    from sat_amd._lib import SatLibraryError
    dy = torch.randn(37)
    dx = torch.full((37,), NAN, device=cuda)
    kernels.act_bwd(dy.to(cuda), None, dx, None)
    assert torch.equal(dx.cpu(), dy)
    for act in ("relu", "tanh", "sigmoid", "softsign"):
        out = torch.full((37,), NAN, device=cuda)
        with pytest.raises(SatLibraryError):
            kernels.act_bwd(dy.to(cuda), None, out, act)
        assert bool(torch.isnan(out).all())


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("a,b", [(1.0, 0.0), (0.5, 1.0), (-2.0, 0.25)])
def test_axpby(cuda, n, a, b):
    """y = a x + b y; b == 0 over a NaN y gives finite output.
    Largest err/bound observed: 0.14."""
    from sat_amd import kernels
    g = torch.Generator().manual_seed(n)
    x, y0 = _randn(g, n), _randn(g, n)
    y = y0.to(cuda) if b != 0.0 else torch.full((n,), NAN, device=cuda)
    kernels.axpby(x.to(cuda), y, a, b)
    ref = a * x.double() + (b * y0.double() if b != 0.0 else 0.0)
    r = _ratio(y, ref, abs(a) * x.double().abs() + abs(b) * y0.double().abs())
    _note("test_axpby", r)
    assert r <= 1.0


@pytest.mark.parametrize("n", [4, 252, 1024, 4100])
def test_add(cuda, n):
    """z = x + y on float4s: one rounding, so bit-equal to torch's float32 sum."""
    from sat_amd import kernels
    g = torch.Generator().manual_seed(n)
    x, y = _randn(g, n), _randn(g, n)
    z = kernels.add(x.to(cuda), y.to(cuda))
    assert torch.equal(z.cpu(), x + y)


def test_add_refused(cuda):
    """n % 4 != 0 and operands off a 16-byte boundary are refused."""
    from sat_amd import kernels
    from sat_amd._lib import SatLibraryError
    with pytest.raises(SatLibraryError):
        kernels.add(torch.zeros(7, device=cuda), torch.zeros(7, device=cuda))
    base = torch.zeros(16, device=cuda)
    with pytest.raises(SatLibraryError):
        kernels.add(base[1:9], torch.zeros(8, device=cuda))
    with pytest.raises(SatLibraryError):
        kernels.add(torch.zeros(8, device=cuda), base[3:11])


@pytest.mark.parametrize("fn", ["highway_fwd", "highway_act_fwd", "highway_bwd", "act_bwd", "axpby", "add"])
def test_empty_is_a_no_op(cuda, fn):
    """n == 0 succeeds (grid_for never returns 0 blocks; sat_add returns early) and writes
    nothing.  Called at the C level with real pointers: an empty torch view has a null one."""
    from sat_amd import _lib, kernels
    buf = torch.full((16,), NAN, device=cuda)
    p, s = buf.data_ptr(), kernels._stream()
    args = {"highway_fwd": (p, p, p, p, 0, s), "highway_act_fwd": (p, p, p, p, 0, s),
            "highway_bwd": (p, p, p, p, p, p, p, 0, s), "act_bwd": (p, p, None, p, 0, 2, 1.0, s),
            "axpby": (p, p, 0, 1.0, 1.0, s), "add": (p, p, p, 0, s)}[fn]
    _lib.call("sat_" + fn, *args)
    assert bool(torch.isnan(buf).all())


# ------------------------------------------------------------------------------ data movement

def _padded3(dev, n0, n1, n2, s1, s0):
    """[n0][n1][n2] view with strides (s0, s1, 1) at float 4 of a NaN buffer."""
    buf = torch.full((4 + n0 * s0 + 4,), NAN, device=dev)
    return buf, buf[4:].as_strided((n0, n1, n2), (s0, s1, 1))


@pytest.mark.parametrize("n2,s1", [(8, 8), (8, 12), (7, 7), (7, 12), (8, 9)])
def test_copy3d(cuda, n2, s1):
    """Vector path (n2 and every stride % 4 == 0) and scalar path (n2 = 7; n2 = 8 with row stride
    9): a transposed-view source into a padded destination, bit-exact, padding still NaN."""
    from sat_amd import kernels
    n0, n1 = 5, 6
    g = torch.Generator().manual_seed(n2 + s1)
    src_t = _randn(g, n1, n0, n2).to(cuda)              # source = its transpose(0, 1) view
    src = src_t.transpose(0, 1)
    buf, dst = _padded3(cuda, n0, n1, n2, s1, n1 * s1 + (4 if s1 % 4 == 0 else 3))
    kernels.copy3d_(dst, src)
    assert torch.equal(dst.cpu(), src.cpu())
    check = buf.clone()
    check[4:].as_strided(dst.shape, dst.stride()).fill_(NAN)
    assert bool(torch.isnan(check).all())
    # a 2-D strided slice (the step-buffer copy) through the same entry
    wide = torch.full((n1, n2 + 8), NAN, device=cuda)
    kernels.copy3d_(wide[:, 4:4 + n2], src_t[:, 0])
    assert torch.equal(wide[:, 4:4 + n2].cpu(), src_t[:, 0].cpu())
    assert bool(torch.isnan(wide[:, :4]).all()) and bool(torch.isnan(wide[:, 4 + n2:]).all())


def test_copy3d_empty(cuda):
    """An empty box copies nothing."""
    from sat_amd import _lib, kernels
    src = torch.zeros(64, device=cuda)
    dst = torch.full((64,), NAN, device=cuda)
    for box in ((3, 0, 8), (0, 2, 8), (3, 2, 0)):
        _lib.call("sat_copy3d", src.data_ptr(), 16, 8, dst.data_ptr(), 16, 8, *box, kernels._stream())
    assert bool(torch.isnan(dst).all())


@pytest.mark.parametrize("R,C", [(1, 1), (31, 33), (32, 32), (100, 7), (257, 129)])
def test_transpose_padded(cuda, R, C):
    """out[c][r] = in[r][c] with ldi > C and ldo > R: bit-exact, the output's padding untouched."""
    from sat_amd import kernels
    g = torch.Generator().manual_seed(R + C)
    x = torch.full((R, C + 3), NAN, device=cuda)
    vals = _randn(g, R, C)
    x[:, :C] = vals.to(cuda)
    out = torch.full((C, R + 5), NAN, device=cuda)
    kernels.transpose(x[:, :C], out[:, :R])
    assert torch.equal(out[:, :R].cpu(), vals.t())
    assert bool(torch.isnan(out[:, R:]).all())


@pytest.mark.parametrize("off", [0, 1, 2, 3])
@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 1023, 1024, 4099])
def test_fill32(cuda, n, off):
    """sat_fill32 at every head / body / tail split: pointer 0-3 floats past a 16-byte boundary,
    the word on each side of the range as it was; int32 too."""
    from sat_amd import kernels
    buf = torch.full((n + 12,), NAN, device=cuda)
    lo = 4 + off
    assert buf[lo:].data_ptr() % 16 == 4 * off
    kernels.fill_(buf[lo:lo + n], 1.5)
    assert torch.equal(buf[lo:lo + n].cpu(), torch.full((n,), 1.5))
    assert bool(torch.isnan(buf[:lo]).all()) and bool(torch.isnan(buf[lo + n:]).all())
    ib = torch.full((n + 12,), 7, device=cuda, dtype=torch.int32)
    kernels.fill_(ib[lo:lo + n], -3)
    assert torch.equal(ib.cpu(), torch.cat([torch.full((lo,), 7), torch.full((n,), -3),
                                            torch.full((12 - lo,), 7)]).to(torch.int32))


@pytest.mark.parametrize("C", [1, 7, 128])
def test_seq_mask(cuda, C):
    """out[b, n, :] = x[b, n, :] for n < lengths[b], else 0: lengths 0, 1, N and above N."""
    from sat_amd import kernels
    B, N = 6, 9
    g = torch.Generator().manual_seed(C)
    x = _randn(g, B, N, C)
    lengths = torch.tensor([0, 1, N, N + 3, 4, N - 1])
    out = torch.full((B, N, C), NAN, device=cuda)
    kernels.seq_mask(x.to(cuda), lengths.to(cuda), out=out)
    keep = (torch.arange(N)[None, :] < lengths[:, None]).unsqueeze(-1)
    assert torch.equal(out.cpu(), torch.where(keep, x, torch.zeros_like(x)))


@pytest.mark.parametrize("offset", [0, 225])
def test_embedding_fwd(cuda, offset):
    """Rows of table[ids - offset]; an id below and one above the table write zeros and set err;
    err stays 0 with valid ids; err = None is accepted."""
    from sat_amd import kernels
    V, D = 11, 37
    g = torch.Generator().manual_seed(offset)
    table = _randn(g, V, D)
    ids = torch.tensor([0, V - 1, 3, 3, 7, 1, 10, 5, 2]) + offset
    td = table.to(cuda)
    err = torch.zeros(1, dtype=torch.int32, device=cuda)
    out = torch.full((ids.numel(), D), NAN, device=cuda)
    kernels.embedding_fwd(td, ids.to(cuda), out, offset=offset, err=err)
    assert torch.equal(out.cpu(), table[ids - offset]) and int(err.item()) == 0
    bad = ids.clone()
    bad[2], bad[6] = offset - 1, offset + V
    out = torch.full((ids.numel(), D), NAN, device=cuda)
    kernels.embedding_fwd(td, bad.to(cuda), out, offset=offset, err=err)
    ref = table[(bad - offset).clamp(0, V - 1)]
    ref[2] = 0.0
    ref[6] = 0.0
    assert torch.equal(out.cpu(), ref) and int(err.item()) == 1
    out = torch.full((ids.numel(), D), NAN, device=cuda)
    kernels.embedding_fwd(td, bad.to(cuda), out, offset=offset, err=None)
    assert torch.equal(out.cpu(), ref)


# ------------------------------------------------------------------------------ the two skinny products

@pytest.mark.parametrize("M,N,K", [(32, 1024, 288), (5, 7, 36), (1, 1, 4), (33, 3, 260)])
@pytest.mark.parametrize("alpha,beta", [(1.0, 0.0), (0.5, 1.0)])
def test_rowdot(cuda, M, N, K, alpha, beta):
    """C = alpha A Bt^T + beta C (sat_gemm_rowdot: 32 outputs per workgroup, 8 lanes x float4 = 32
    columns of K per trip): the decoder step's own shape and ones where M N is no multiple of 32
    and K none of 32; strided rows; beta == 0 over a NaN C.
    Largest err/bound observed: 0.10."""
    from sat_amd import kernels
    g = torch.Generator().manual_seed(M + N + K)
    A, Bt, C0 = _randn(g, M, K), _randn(g, N, K), _randn(g, M, N)
    Ad = torch.full((M, K + 4), NAN, device=cuda)
    Ad[:, :K] = A.to(cuda)
    Bd = torch.full((N, K + 8), NAN, device=cuda)
    Bd[:, :K] = Bt.to(cuda)
    Cd = torch.full((M, N + 3), NAN, device=cuda)
    if beta != 0.0:
        Cd[:, :N] = C0.to(cuda)
    kernels.rowdot(Ad[:, :K], Bd[:, :K], Cd[:, :N], alpha=alpha, beta=beta)
    ref = alpha * A.double() @ Bt.double().T + (beta * C0.double() if beta != 0.0 else 0.0)
    terms = abs(alpha) * A.double().abs() @ Bt.double().abs().T + abs(beta) * C0.double().abs()
    got = Cd[:, :N].double().cpu()
    assert bool(torch.isfinite(got).all()) and bool(torch.isnan(Cd[:, N:]).all())
    r = float(((got - ref).abs() / (6e-7 * terms + 1e-7)).max())
    _note("test_rowdot", r)
    assert r <= 1.0


@pytest.mark.parametrize("B,K,N1,N2", [(32, 256, 128, 128), (11, 37, 70, 5), (3, 5, 9, 0), (8, 64, 64, 64)])
def test_attn_query(cuda, B, K, N1, N2):
    """q = x [W1 | W2] (sat_attn_query: 8 rows x 64 columns per workgroup): the step's own shape,
    one ragged in rows, columns and K, one without W2; strided x and q, q's padding untouched.
    Largest err/bound observed: 0.34."""
    from sat_amd import kernels
    g = torch.Generator().manual_seed(B + K + N1)
    x, W1 = _randn(g, B, K), _randn(g, K, N1)
    W2 = _randn(g, K, N2) if N2 else None
    xd = torch.full((B, K + 3), NAN, device=cuda)
    xd[:, :K] = x.to(cuda)
    q = torch.full((B, N1 + N2 + 5), NAN, device=cuda)
    kernels.attn_query(xd[:, :K], W1.to(cuda), None if W2 is None else W2.to(cuda), q[:, :N1 + N2])
    Wc = W1.double() if W2 is None else torch.cat([W1, W2], dim=1).double()
    ref, terms = x.double() @ Wc, x.double().abs() @ Wc.abs()
    got = q[:, :N1 + N2].double().cpu()
    assert bool(torch.isfinite(got).all()) and bool(torch.isnan(q[:, N1 + N2:]).all())
    r = float(((got - ref).abs() / (6e-7 * terms + 1e-7)).max())
    _note("test_attn_query", r)
    assert r <= 1.0
