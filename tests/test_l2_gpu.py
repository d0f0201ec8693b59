"""The L2 regulariser's kernel on the GPU: sat_l2_regularize called directly on synthetic arenas,
and on a model's own parameter arena with the table params.l2_segments builds for it.

Tolerances (nothing in a bound comes from the GPU).  The loss value: 4 * e32, e32 = the deviation
of l2_ref's float32 evaluation from its float64 one on the same inputs (the rule of
tests/test_optim_gpu.py), computed per case and printed.  The kernel sums in float64 and rounds
once, so its own error is at most half a float32 ulp of the value -- and no float32 output can
promise less.  numpy's pairwise float32 sums are accurate enough that e32 falls below an eighth of
an ulp for some inputs (0.011 .. 4.9 ulp over seeds 1..7 of the cases below, on the CPU); the
bound would then ask for more than the format holds.  So each case's input seed (third field of
CASES) was picked, from that CPU-only table, as one where e32 >= ulp / 4, and _check_loss asserts
4 * e32 >= ulp / 2 of its inputs before it looks at the GPU's value.  e32 / ulp of the cases as
they stand: small 0.60, unaligned 1.10, chunks 1.03, wrap 3.46, many 2.51, many_unaligned 2.55;
the model's initial weights 0.31 (seed 42).  An updated gradient is one float32
fused multiply-add: 1 ulp of the float64 result.  Everything the kernel must not touch is
compared bit for bit.
"""
import numpy as np
import pytest
import torch

import l2_ref

pytestmark = pytest.mark.gpu

F32 = np.float32
POISON = 0x7FC0DEAD          # a quiet NaN with a payload: read it and the sum is NaN
# csrc/optim.hip: l2_segments_kernel runs kL2Blocks = 1024 workgroups, each taking chunks of
# kL2Chunk = 2048 floats (256 threads x 2 float4): one pass of the whole grid covers
GRID_PASS = 1024 * 2048      # floats; a single longer segment makes the chunk loop wrap
CHUNK = 2048

SMALL = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257]
CASES = {
    # every start on a 256-byte boundary, as arena tensors are: float4 body + scalar tail
    "small": (SMALL, 0, 1),
    # starts at 1, 2, 3 (mod 4) floats: no 16-byte alignment, the scalar path
    "unaligned": (SMALL, 1, 7),
    # lengths around one and several chunks of a workgroup pass
    "chunks": ([CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK, 3 * CHUNK + 7], 0, 3),
    # one segment longer than a full grid pass (by three chunks and a tail) between two small
    # ones: workgroups 0..3 take a second chunk of it
    "wrap": ([5, GRID_PASS + 3 * CHUNK + 5, 257], 0, 3),
    # more segments (150) than a workgroup's chunk loop meets in one stretch: the table cursor
    # skips many entries between a workgroup's chunks
    "many": ([int(x) for x in np.random.default_rng(99).integers(1, 300, 150)], 0, 3),
    "many_unaligned": ([int(x) for x in np.random.default_rng(98).integers(1, 300, 131)], 1, 4),
}


class Arena:
    """Synthetic parameter / gradient arenas: segments of the given lengths separated by gaps
    (and one unselected, poisoned 'tensor' between every two), poison everywhere else."""

    def __init__(self, cuda, lengths, misalign, seed):
        r = np.random.default_rng(seed)
        self.ranges = []
        off = 64
        for i, n in enumerate(lengths):
            start = off + ((1 + i % 3) if misalign else 0)
            self.ranges.append((start, n))
            off = (start + n + 63) // 64 * 64 + 64 * (1 + i % 2)     # padding + an unselected run
        self.total = off + 64
        self.sel = np.zeros(self.total, bool)
        for o, n in self.ranges:
            self.sel[o:o + n] = True
        p = np.full(self.total, POISON, np.uint32).view(F32)
        g = np.full(self.total, POISON, np.uint32).view(F32)
        p[self.sel] = r.standard_normal(int(self.sel.sum())).astype(F32)
        g[self.sel] = r.standard_normal(int(self.sel.sum())).astype(F32)
        self.p, self.g = p, g
        self.dp, self.dg = torch.from_numpy(p.copy()).to(cuda), torch.from_numpy(g.copy()).to(cuda)
        self.out = torch.full((2,), float("nan"), device=cuda)
        self.cuda = cuda

    def weights(self):
        return {i: self.p[o:o + n] for i, (o, n) in enumerate(self.ranges)}

    def table(self):
        from sat_amd import kernels as K
        return K.l2_table(self.ranges, self.total, self.cuda)

    def run(self, weight, gw, grads=True, loss_total=None, table=None):
        from sat_amd import kernels as K
        K.l2_regularize(self.dp, self.dg if grads else None,
                        self.table() if table is None else table, weight, gw, self.out[:1],
                        loss_total)
        torch.cuda.synchronize()
        return float(self.out[0])

    def bits(self, t):
        return t.cpu().numpy().view(np.uint32)


def _check_loss(got, weights, weight, selected=lambda n: True):
    want = l2_ref.l2_loss64(weights, float(F32(weight)), selected)
    e32 = l2_ref.e32(weights, weight, selected)
    ulp = float(l2_ref.ulp32(want))
    print(f"l2 gpu {got!r} ref {want!r} err {abs(got - want):.3e} e32 {e32:.3e} ulp {ulp:.3e}")
    assert 4 * e32 >= 0.5 * ulp, "inputs whose float32 evaluation is exact by chance: reseed"
    assert np.isfinite(got) and abs(got - want) <= 4 * e32, (got, want, e32)
    return want


@pytest.mark.parametrize("case", list(CASES))
def test_kernel_on_synthetic_arena(cuda, case):
    lengths, mis, seed = CASES[case]
    a = Arena(cuda, lengths, mis, seed)
    weight, gw = 0.37, 0.011
    got = a.run(weight, gw)
    _check_loss(got, a.weights(), weight)
    assert np.isnan(float(a.out[1])), "out[1] is not the entry's to write"
    # params: every byte unchanged
    assert np.array_equal(a.bits(a.dp), a.p.view(np.uint32))
    g1 = a.dg.cpu().numpy()
    # gaps and unselected runs of the gradients: bit-unchanged
    assert np.array_equal(g1.view(np.uint32)[~a.sel], a.g.view(np.uint32)[~a.sel])
    # selected gradients: g + grad_weight * w, one fused multiply-add
    want = l2_ref.grad64(a.p[a.sel], a.g[a.sel], gw)
    err = np.abs(g1[a.sel].astype(np.float64) - want)
    print(f"{case}: worst grad err / ulp {float((err / l2_ref.ulp32(want)).max()):.3f}")
    assert (err <= l2_ref.ulp32(want)).all()
    # a second run on identical inputs: bit-identical loss and gradients
    b = Arena(cuda, lengths, mis, seed)
    got2 = b.run(weight, gw)
    assert F32(got).tobytes() == F32(got2).tobytes()
    assert np.array_equal(b.bits(b.dg), g1.view(np.uint32))


def test_case_lengths_cover_the_paths():
    assert CASES["wrap"][0][1] > GRID_PASS and len(CASES["many"][0]) >= 130
    assert len(CASES["many_unaligned"][0]) >= 130
    assert set(SMALL) == {1, 3, 4, 5, 63, 64, 65, 255, 256, 257}


def test_loss_only_without_gradients(cuda):
    """grads = NULL (EVAL): the value alone; and grad_weight = 0 with a gradient arena given
    leaves that arena's bits alone as well."""
    a = Arena(cuda, SMALL, 0, seed=5)
    got = a.run(0.37, 0.5, grads=False)
    _check_loss(got, a.weights(), 0.37)
    assert np.array_equal(a.bits(a.dp), a.p.view(np.uint32))
    assert np.array_equal(a.bits(a.dg), a.g.view(np.uint32))
    got0 = a.run(0.37, 0.0, grads=True)
    assert got0 == got
    assert np.array_equal(a.bits(a.dg), a.g.view(np.uint32))


def test_zero_weights_and_empty_table(cuda):
    from sat_amd import kernels as K
    a = Arena(cuda, SMALL, 0, seed=6)
    total = torch.tensor([1.25], device=cuda)
    assert a.run(0.0, 0.0, loss_total=total) == 0.0
    assert np.array_equal(a.bits(a.dg), a.g.view(np.uint32)) and float(total) == 1.25
    a.out.fill_(float("nan"))
    empty = K.l2_table([], a.total, cuda)
    assert tuple(empty.shape) == (0, 2)
    assert a.run(0.37, 0.011, loss_total=total, table=empty) == 0.0     # nseg = 0: SAT_OK
    assert np.array_equal(a.bits(a.dg), a.g.view(np.uint32)) and float(total) == 1.25
    assert np.array_equal(a.bits(a.dp), a.p.view(np.uint32))


def test_loss_total_grows_by_exactly_the_term(cuda):
    a = Arena(cuda, SMALL, 0, seed=7)
    start = F32(0.7316)
    total = torch.tensor([start], device=cuda)
    got = a.run(0.37, 0.011, loss_total=total)
    assert F32(float(total)).tobytes() == F32(start + F32(got)).tobytes()     # one fp32 add


def test_refusals_launch_nothing(cuda):
    from sat_amd import _lib, kernels as K
    a = Arena(cuda, SMALL, 0, seed=8)
    tab = a.table()
    ws = torch.zeros(int(_lib.load().sat_workspace_l2()), dtype=torch.uint8, device=cuda)
    total = torch.tensor([1.25], device=cuda)
    a.out.fill_(7.0)
    good = dict(params=a.dp.data_ptr(), grads=a.dg.data_ptr(), seg=tab.data_ptr(),
                nseg=tab.shape[0], weight=0.37, grad_weight=0.011, out=a.out.data_ptr(),
                loss_total=total.data_ptr(), workspace=ws.data_ptr())
    for over in (dict(params=None), dict(out=None), dict(workspace=None), dict(nseg=-1),
                 dict(seg=None)):
        with pytest.raises(_lib.SatLibraryError) as e:
            _lib.check(_lib.load().sat_l2_regularize(*{**good, **over}.values(), K._stream()),
                       "sat_l2_regularize")
        assert e.value.rc == _lib.SAT_ERR_ARGUMENT, over
    torch.cuda.synchronize()
    assert a.out.tolist() == [7.0, 7.0] and float(total) == 1.25 and not ws.any()
    assert np.array_equal(a.bits(a.dg), a.g.view(np.uint32))
    # the table is validated on the host before it is uploaded
    for bad in ([(-1, 4)], [(0, -4)], [(a.total - 3, 4)], [(64, 8), (70, 4)]):
        with pytest.raises(ValueError):
            K.l2_table(bad, a.total, cuda)


# ------------------------------------------------------------------ a model's arena
def test_model_arena(cuda):
    """The LJSpeech model's parameter arena (seed 42) with the table of params.l2_segments, and
    a gradient arena of the same layout: the term is the reference's over
    params.is_l2_regularized, the regularised tensors' gradients gain LAM * w, every other
    gradient and every padding float keeps its bits."""
    from sat_amd import hparams, kernels as K, params as PR
    LAM = 1e-2
    hp = hparams.ljspeech_hparams()
    lay = PR.Layout(PR.param_specs(hp))
    w = lay.pack(PR.init_params(hp, seed=42))
    g = np.random.default_rng(11).standard_normal(lay.total).astype(F32)
    sel = np.zeros(lay.total, bool)
    for p in lay.specs:
        if PR.is_l2_regularized(p.name):
            sel[lay.offsets[p.name]:lay.offsets[p.name] + int(np.prod(p.shape))] = True
    dw, dg = torch.from_numpy(w).to(cuda), torch.from_numpy(g).to(cuda)
    out = torch.zeros(1, device=cuda)
    table = K.l2_table(PR.l2_segments(lay.specs, lay), lay.total, cuda)
    K.l2_regularize(dw, dg, table, LAM, LAM, out)
    torch.cuda.synchronize()
    ref = _check_loss(float(out), lay.unpack(w, internal=False), LAM, PR.is_l2_regularized)
    assert ref > 1.0
    assert np.array_equal(dw.cpu().numpy().view(np.uint32), w.view(np.uint32))
    g1 = dg.cpu().numpy()
    assert np.array_equal(g1.view(np.uint32)[~sel], g.view(np.uint32)[~sel])
    want = l2_ref.grad64(w[sel], g[sel], LAM)
    assert (np.abs(g1[sel].astype(np.float64) - want) <= l2_ref.ulp32(want)).all()
