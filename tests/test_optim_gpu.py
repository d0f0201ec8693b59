"""clip + Adam (csrc/optim.hip: sat_adam_step, sat_global_norm_sq) called directly on random
p, g, m, v, against oracle.sat_oracle's clip_by_global_norm / learning_rate / adam_tf in float64.

Tolerances.  scalars (norm, scale, lr, lr_t) are float32 roundings of values the prepare kernel
computes in float64: rel 2 * 2^-23.  For p, m, v the same three formulas are also evaluated op by
op in numpy float32 on the CPU (``_chain32``); e32 = that result's max |deviation| from the
float64 reference, per array and step, and the GPU must be within 4 * e32 (its contraction into
FMAs and its sqrtf may round differently from numpy's).  Nothing in a bound comes from the GPU.


A note for whoever changes how optim.hip is compiled.  Over the 1, 3 or 5 elements of the small
cases e32 can by chance fall below half a float32 ulp (n = 3, third step: e32(v) = 7.1e-11 where
half an ulp of v is 4.7e-10), so there the bound holds only because the kernel rounds exactly
where numpy does: measured, the GPU's error exceeds e32 in no case of this file (ratio <= 1.0).
Evaluating the update on the CPU with the two moment updates contracted into FMAs misses that
n = 3 bound (4.0e-10 > 2.8e-10) with a correctly rounded v.  If contraction ever changes the
kernel's roundings, that case needs a floor of half an ulp, not a kernel fix.

e32 as measured on the CPU (max over the case's steps; p / m / v), for the record -- the tests
recompute it:
  n = 1: 2.0e-08 / 4.1e-09 / 7.2e-11      n = 1027:    3.4e-07 / 2.4e-08 / 2.1e-09
  n = 3: 1.0e-07 / 7.1e-09 / 2.0e-10      n = 1310723: 7.1e-07 / 5.9e-08 / 2.6e-09
  n = 5: 5.6e-08 / 7.3e-09 / 7.2e-10      n = 2097157: 7.1e-07 / 5.9e-08 / 2.4e-09
(the other cases are all at n = 1027; their docstrings carry theirs, and every test prints its own).
"""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F32 = np.float32
SIZES = [1, 3, 5, 1027, 1_048_576 + 262_147, 2_097_152 + 5]   # the last two: past the norm
#                                      kernel's grid (1024 x 256 x 4) and the update's (8192 x 256)
NOAM_STEPS = [0, 1999, 3999, 4000, 100000]
REL32 = 2.0 * 2.0 ** -23


def _cfg(lr0=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, clip_norm=1.0, decay=1, step_factor=1,
         grad_scale=1.0):
    from sat_amd import _lib
    c = _lib.SatAdamConfig()
    c.lr0, c.beta1, c.beta2, c.eps, c.clip_norm = lr0, beta1, beta2, eps, clip_norm
    c.decay, c.step_factor, c.grad_scale = decay, step_factor, grad_scale
    return c


def _state(n, seed, steps=1, norm=40.0, grad_scale=1.0, zero_g=False):
    """float32 p, m, v (v >= 0, moments non-zero) and one gradient per step whose scaled global
    norm grad_scale * |g| is ``norm`` (up to float32 rounding of the elements)."""
    r = np.random.default_rng(seed)
    p = r.standard_normal(n).astype(F32)
    m = (0.1 * r.standard_normal(n)).astype(F32)
    v = (0.01 * r.random(n) + 1e-6).astype(F32)
    gs = []
    for _ in range(steps):
        g = r.standard_normal(n)
        g = np.zeros(n) if zero_g else g * (norm / (grad_scale * math.sqrt(float((g * g).sum()))))
        gs.append(g.astype(F32))
    return p, m, v, gs


def _scalars64(g, gs, c):
    """{norm, total scale, lr, lr_t} of a step in float64 from the oracle's formulas, with the
    hyper-parameters as the float32 values the config carries."""
    from oracle import sat_oracle as O
    scaled = torch.from_numpy(g.astype(np.float64)) * float(c.grad_scale)
    if c.clip_norm > 0:
        clipped, norm = O.clip_by_global_norm([scaled], float(c.clip_norm))
        clipped = clipped[0]
    else:
        clipped, norm = scaled, math.sqrt(float((scaled ** 2).sum()))
    scale = float(c.grad_scale) * (float(c.clip_norm) / max(norm, float(c.clip_norm))
                                   if c.clip_norm > 0 else 1.0)
    lr = O.learning_rate(float(c.lr0), gs, c.step_factor) if c.decay else float(c.lr0)
    t = gs + 1
    lr_t = lr * math.sqrt(1 - float(c.beta2) ** t) / (1 - float(c.beta1) ** t)
    return clipped, (norm, scale, lr, lr_t)


def _chain64(p, m, v, grads, gs0, c):
    """The float64 reference over consecutive steps: per step (p, m, v, scalars)."""
    from oracle import sat_oracle as O
    p, m, v = (torch.from_numpy(x.astype(np.float64)) for x in (p, m, v))
    out = []
    for k, g in enumerate(grads):
        clipped, sc = _scalars64(g, gs0 + k, c)
        p, m, v = O.adam_tf(p, clipped, m, v, sc[2], gs0 + k + 1, float(c.beta1), float(c.beta2),
                            float(c.eps))
        out.append((p.numpy(), m.numpy(), v.numpy(), sc))
    return out


def _chain32(p, m, v, grads, ref):
    """The same update op by op in numpy float32 (every product, sum, sqrt and quotient rounded
    once), fed the float32 roundings of the reference's scale and lr_t as the kernel is."""
    b1, b2, eps = ref["b1"], ref["b2"], ref["eps"]
    one = F32(1.0)
    out = []
    for g, (_, _, _, sc) in zip(grads, ref["steps"]):
        scale, lr_t = F32(sc[1]), F32(sc[3])
        gg = g * scale
        m = b1 * m + (one - b1) * gg
        v = b2 * v + (one - b2) * gg * gg
        p = p - lr_t * m / (np.sqrt(v) + eps)
        assert p.dtype == m.dtype == v.dtype == F32
        out.append((p, m, v))
    return out


def reference(p, m, v, grads, gs0, c):
    ref = dict(b1=F32(c.beta1), b2=F32(c.beta2), eps=F32(c.eps),
               steps=_chain64(p, m, v, grads, gs0, c))
    ref["steps32"] = _chain32(p, m, v, grads, ref)
    # e32[k][a]: float32 arithmetic's own error at step k, array a (p, m, v)
    ref["e32"] = [[float(np.abs(a32.astype(np.float64) - a64).max())
                   for a32, a64 in zip(s32, s64[:3])]
                  for s32, s64 in zip(ref["steps32"], ref["steps"])]
    return ref


class Dev:
    """Device state of one sat_adam_step caller; outputs of the step start as sentinels."""

    def __init__(self, cuda, p, m, v, gs0, n_health=0):
        from sat_amd import _lib
        self.p, self.m, self.v = (torch.from_numpy(x.copy()).to(cuda) for x in (p, m, v))
        self.g = torch.full_like(self.p, float("nan"))
        self.n = self.p.numel()
        self.gs = torch.tensor([gs0], dtype=torch.int64, device=cuda)
        self.scalars = torch.full((4,), float("nan"), device=cuda)
        self.ws = torch.empty(int(_lib.load().sat_workspace_adam()), dtype=torch.uint8,
                              device=cuda)
        self.health = torch.zeros(max(n_health, 1), dtype=torch.int32, device=cuda)
        self.n_health = n_health
        self.status = torch.zeros(2, dtype=torch.int32, device=cuda)

    def args(self, c, **over):
        a = dict(params=self.p.data_ptr(), grads=self.g.data_ptr(), m=self.m.data_ptr(),
                 v=self.v.data_ptr(), n=self.n, global_step=self.gs.data_ptr(),
                 scalars=self.scalars.data_ptr(), workspace=self.ws.data_ptr(),
                 cfg=ctypes.byref(c) if c is not None else None,
                 health=self.health.data_ptr() if self.n_health else None,
                 n_health=self.n_health, status=self.status.data_ptr())
        a.update(over)
        return list(a.values())

    def step(self, c, g=None, **over):
        from sat_amd import _lib, kernels as K
        if g is not None:
            self.g.copy_(torch.from_numpy(g))
        _lib.check(_lib.load().sat_adam_step(*self.args(c, **over), K._stream()), "sat_adam_step")
        torch.cuda.synchronize()

    def bits(self):
        """Everything a skipped or refused step must leave alone, as exact bit patterns."""
        return [x.clone().view(torch.int32) if x.dtype == torch.float32 else x.clone()
                for x in (self.p, self.m, self.v, self.scalars, self.gs)]

    def same_bits(self, before):
        return all(torch.equal(a, b) for a, b in zip(self.bits(), before))


def _close32(got, want):
    return abs(got - want) <= REL32 * abs(want)


def _within(got, want, e32):
    """(ok, max error) of a device array against the float64 reference: within 4 * e32."""
    got = got.cpu().numpy()
    err = float(np.abs(got.astype(np.float64) - want).max())
    return bool(np.isfinite(got).all()) and err <= 4 * e32, err


def _run(cuda, n, seed, c, gs0=0, steps=1, norm=40.0, zero_g=False):
    p, m, v, grads = _state(n, seed, steps, norm, float(c.grad_scale), zero_g)
    ref = reference(p, m, v, grads, gs0, c)
    d = Dev(cuda, p, m, v, gs0)
    for k, g in enumerate(grads):
        d.scalars.fill_(float("nan"))
        d.step(c, g)
        p64, m64, v64, sc = ref["steps"][k]
        got_sc = [float(x) for x in d.scalars.cpu()]
        assert int(d.gs.item()) == gs0 + k + 1
        print(f"n={n} gs={gs0 + k} scalars gpu {got_sc} ref {sc} e32 {ref['e32'][k]}")
        assert _close32(got_sc[0], sc[0]) and _close32(got_sc[1], sc[1]), (got_sc, sc)
        assert _close32(got_sc[2], sc[2]) and _close32(got_sc[3], sc[3]), (got_sc, sc)
        for name, got, want, e32 in zip("pmv", (d.p, d.m, d.v), (p64, m64, v64), ref["e32"][k]):
            ok, err = _within(got, want, e32)
            print(f"  {name}: gpu err {err:.3e}  e32 {e32:.3e}")
            assert ok, (name, k, err, e32)
    assert torch.equal(d.g.cpu(), torch.from_numpy(grads[-1])), "the gradient is an input"
    return ref, d


@pytest.mark.parametrize("n", SIZES)
def test_three_steps_from_nonzero_moments(cuda, n):
    """Three consecutive steps (global_step 7, 8, 9: t-dependent bias correction, Noam warm-up
    arm) at every size: the norm kernel's n & 3 tail and both kernels' grid-stride loops.  Clip
    engaged (norm 40).  e32 per size: the module docstring."""
    _run(cuda, n, seed=n, c=_cfg(), gs0=7, steps=3, norm=40.0)


@pytest.mark.parametrize("step_factor", [1, 2])
@pytest.mark.parametrize("gs0", NOAM_STEPS)
def test_noam_schedule_both_arms(cuda, gs0, step_factor):
    """lr = lr0 4000^0.5 min(s 4000^-1.5, s^-0.5), s = global_step * step_factor + 1: the min
    switches arm at s = 4000, and these steps lie on both sides of it at either factor (with
    bias correction up to t = 100001).  e32 (p / m / v) between 1.1e-07 / 1.4e-08 / 8.6e-10 and
    1.2e-07 / 2.5e-08 / 9.2e-10 over the ten cases."""
    s = gs0 * step_factor + 1
    ref, _ = _run(cuda, 1027, seed=gs0 + step_factor, c=_cfg(step_factor=step_factor), gs0=gs0,
                  norm=40.0)
    lr = ref["steps"][0][3][2]
    warm, decayed = 1e-3 * 4000 ** 0.5 * s * 4000 ** -1.5, 1e-3 * 4000 ** 0.5 * s ** -0.5
    assert math.isclose(lr, warm if s < 4000 else decayed, rel_tol=1e-6)
    assert (warm < decayed) == (s < 4000)


def test_noam_cases_cover_both_arms():
    arms = {(sf, gs * sf + 1 < 4000) for gs in NOAM_STEPS for sf in (1, 2)}
    assert arms == {(1, True), (1, False), (2, True), (2, False)}


@pytest.mark.parametrize("norm,grad_scale,clip_norm,decay", [
    (0.25, 1.0, 1.0, 1),       # clip idle
    (40.0, 1.0, 1.0, 0),       # constant lr
    (0.25, 1.0, 1.0, 0),
    (40.0, 1.0, 0.0, 1),       # clipping off
    (40.0, 1.0, -1.0, 1),
    (0.25, 0.125, 1.0, 1),     # the data-parallel scale, clip idle and engaged
    (40.0, 0.125, 1.0, 1),
    (40.0, 0.125, 0.0, 1)])
def test_clip_scale_and_decay_arms(cuda, norm, grad_scale, clip_norm, decay):
    """scalars[0] is the norm of grad_scale * g; scalars[1] the total factor on g: exactly
    grad_scale when the clip is idle or off, grad_scale * clip / norm when engaged.  e32
    (p / m / v) between 1.2e-07 / 1.4e-08 / 8.7e-10 and 2.3e-07 / 4.6e-08 / 2.4e-09."""
    c = _cfg(grad_scale=grad_scale, clip_norm=clip_norm, decay=decay)
    ref, d = _run(cuda, 1027, seed=int(norm * 4) + decay, c=c, gs0=3, steps=2, norm=norm)
    sc = [float(x) for x in d.scalars.cpu()]
    assert abs(ref["steps"][-1][3][0] - norm) <= 1e-6 * norm
    if clip_norm <= 0 or norm < clip_norm:
        assert sc[1] == grad_scale
    else:
        assert _close32(sc[1], grad_scale * clip_norm / ref["steps"][-1][3][0])
    if not decay:
        assert sc[2] == float(F32(1e-3))


def test_zero_gradients(cuda):
    """Norm 0: the clip factor is clip / max(0, clip) = 1, nothing is NaN, and the moments decay.
    e32 (p / m / v): 2.1e-07 / 1.6e-08 / 8.7e-10."""
    ref, d = _run(cuda, 1027, seed=5, c=_cfg(), gs0=2, steps=2, zero_g=True)
    sc = [float(x) for x in d.scalars.cpu()]
    assert sc[0] == 0.0 and sc[1] == 1.0


@pytest.mark.parametrize("n", [0] + SIZES)
def test_global_norm_sq(cuda, n):
    """sat_global_norm_sq: the fp64 partials summed on the host are the float64 sum of squares
    (1e-12 relative: fp64 accumulation of exact float32 squares); n = 0 gives 0."""
    from sat_amd import _lib, kernels as K
    g = _state(max(n, 1), seed=n + 1, norm=3.0)[3][0]
    gd = torch.from_numpy(g).to(cuda)
    part = torch.full((int(_lib.load().sat_workspace_adam()) // 8,), float("nan"),
                      dtype=torch.float64, device=cuda)
    _lib.call("sat_global_norm_sq", gd.data_ptr(), n, part.data_ptr(), K._stream())
    torch.cuda.synchronize()
    got = math.fsum(part[:1024].cpu().tolist())
    want = math.fsum((g[:n].astype(np.float64) ** 2).tolist())
    print(f"n={n} sumsq gpu {got!r} ref {want!r}")
    assert abs(got - want) <= 1e-12 * want
    assert bool(torch.isnan(part[1024:]).all())
    assert torch.equal(gd.cpu(), torch.from_numpy(g))


@pytest.mark.parametrize("index,code,n_health", [(0, 1, 256), (255, 9, 256), (3, -5, 8),
                                                  (0, 1, 1)])
def test_health_guard(cuda, index, code, n_health):
    """A set health word -- first, last of the 256 the entry takes, a negative code -- skips the
    step on the device: with NaN gradients p, m, v, global_step and scalars keep their bits;
    status[0] counts each skipped step and status[1] keeps the first code seen."""
    p, m, v, grads = _state(1027, seed=index + n_health)
    d = Dev(cuda, p, m, v, 11, n_health=n_health)
    d.scalars.copy_(torch.tensor([1.5, 2.5, 3.5, 4.5]))
    d.g.fill_(float("nan"))
    before = d.bits()
    d.health[index] = code
    d.step(_cfg())
    assert d.same_bits(before)
    assert d.status.tolist() == [1, code]
    d.health.zero_()
    d.health[n_health - 1 - index] = code + 100            # another word, another code
    d.step(_cfg())
    assert d.same_bits(before)
    assert d.status.tolist() == [2, code]
    d.step(_cfg(), status=None)                            # status is optional
    assert d.same_bits(before)
    assert d.status.tolist() == [2, code]
    # healthy again: the update runs and is the reference's
    d.health.zero_()
    ref = reference(p, m, v, grads, 11, _cfg())
    d.step(_cfg(), grads[0])
    assert int(d.gs.item()) == 12 and d.status.tolist() == [2, code]
    for got, want, e32 in zip((d.p, d.m, d.v), ref["steps"][0][:3], ref["e32"][0]):
        assert _within(got, want, e32)[0]


def test_no_health_words_updates(cuda):
    """n_health = 0 with health = NULL (and status NULL) is a plain update."""
    p, m, v, grads = _state(1027, seed=21)
    ref = reference(p, m, v, grads, 0, _cfg())
    d = Dev(cuda, p, m, v, 0, n_health=0)
    d.step(_cfg(), grads[0], health=None, n_health=0, status=None)
    assert int(d.gs.item()) == 1
    for got, want, e32 in zip((d.p, d.m, d.v), ref["steps"][0][:3], ref["e32"][0]):
        assert _within(got, want, e32)[0]


def test_refusals(cuda):
    from sat_amd import _lib
    p, m, v, grads = _state(1027, seed=22)
    d = Dev(cuda, p, m, v, 4, n_health=256)
    d.g.copy_(torch.from_numpy(grads[0]))
    d.scalars.copy_(torch.tensor([1.5, 2.5, 3.5, 4.5]))
    before = d.bits()
    big = torch.zeros(257, dtype=torch.int32, device=cuda)
    bad = [dict(health=big.data_ptr(), n_health=257), dict(health=None, n_health=3),
           dict(n_health=-1), dict(n=-1)]
    bad += [{k: None} for k in ("params", "grads", "m", "v", "global_step", "scalars",
                                "workspace", "cfg")]
    for over in bad:
        with pytest.raises(_lib.SatLibraryError) as e:
            d.step(_cfg(), **over)
        assert e.value.rc == _lib.SAT_ERR_ARGUMENT, over
    for gsc in (0.0, -1.0):
        with pytest.raises(_lib.SatLibraryError, match="grad_scale"):
            d.step(_cfg(grad_scale=gsc))
    torch.cuda.synchronize()
    assert d.same_bits(before) and d.status.tolist() == [0, 0]


def test_empty_arena_is_a_no_op(cuda):
    """n = 0: SAT_OK with nothing launched and nothing written -- global_step, scalars and
    status keep their values, health words or not (the update launch would otherwise ask for a
    grid of 0 blocks)."""
    p, m, v, _ = _state(8, seed=23)
    d = Dev(cuda, p, m, v, 6, n_health=4)
    d.scalars.copy_(torch.tensor([1.5, 2.5, 3.5, 4.5]))
    before = d.bits()
    d.step(_cfg(), n=0)
    d.health[2] = 7
    d.step(_cfg(), n=0)
    d.step(_cfg(), n=0, health=None, n_health=0, status=None)
    assert d.same_bits(before) and int(d.gs.item()) == 6 and d.status.tolist() == [0, 0]
    assert bool(torch.isnan(d.g).all())
