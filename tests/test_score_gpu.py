"""The score kernels (csrc/score.hip: edit distance and DTW distortion) against the integer /
float64 reference (score_ref.py), at the edges of the kernel's layout: S rows per strip, 64 lanes
per wave.

Edit distances are compared exactly.  The DTW cost bound is not tuned: each fp32 cell cost carries
at most about (width + 2) 2^-24 relative error, a sum of non-negative terms keeps that relative
error, and the minimum over paths of perturbed sums moves by at most the largest perturbation;
the test allows (width + 4) 2^-23.  Path lengths are compared exactly, which needs the optimal
path to be decided by more than rounding: every case's margin (score_ref.py) must be above 1e-3 of
its mean cell cost.  The frames are Gaussian with a log-normal amplitude per frame (so that cell
costs, and with them the gaps between predecessors, spread as widely at width 256 as at width 1);
a (width, case) whose first seed fell short of the margin has its replacement in SEEDS, found on
the CPU with the reference alone.  Smallest margin over the seeded cases: see MIN_MARGIN below
(the test asserts it for every case).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import score_ref as R
from sat_amd import kernels as K

pytestmark = pytest.mark.gpu

S = K.SCORE_STRIP
CODE_LENGTHS = [0, 1, 2, 63, 64, 65, S - 1, S, S + 1, 2 * S + 3]
DTW_LENGTHS = CODE_LENGTHS[1:]
WIDTHS = [1, 13, 80, 256]
MARGIN = 1e-3               # of the mean cell cost


def _crossed(lengths):
    """(Tp, Tt): every length against the one mirrored in the list (Tp << Tt and Tp >> Tt both
    occur) and against itself."""
    return [(a, b) for a, b in zip(lengths, lengths[::-1])] + [(a, a) for a in lengths]


# (width, case index in _crossed(DTW_LENGTHS)) -> the seed that replaces width * 1000 + case
SEEDS = {(1, 2): 1801002, (1, 3): 2501003, (1, 5): 4801005, (1, 6): 5401006, (1, 11): 101011,
         (1, 12): 101012, (1, 14): 1201014, (1, 15): 2701015, (1, 16): 401016,
         (1, 17): 25501017, (13, 3): 113003, (13, 15): 113015, (13, 16): 113016,
         (13, 17): 113017, (80, 2): 180002, (80, 14): 280014, (80, 17): 780017,
         (256, 13): 356013, (256, 17): 356017}
# the smallest margin / mean cell cost over the 72 seeded cases with the table above (the 300
# small pairs: 1.131e-3)
MIN_MARGIN = 1.013e-3


def _frames(rng, n, width):
    amp = np.exp(rng.standard_normal((n, 1)))
    return (amp * rng.standard_normal((n, width))).astype(np.float32)


def dtw_pair(width, n, m, seed):
    rng = np.random.default_rng(seed)
    return _frames(rng, n, width), _frames(rng, m, width)


@functools.lru_cache(maxsize=None)
def dtw_cases(width):
    """The crossed pairs of one width with their reference results, computed once."""
    out = []
    for k, (n, m) in enumerate(_crossed(DTW_LENGTHS)):
        p, t = dtw_pair(width, n, m, SEEDS.get((width, k), width * 1000 + k))
        out.append((p, t, R.dtw(p, t)))
    return out


@functools.lru_cache(maxsize=None)
def code_cases(alphabet):
    rng = np.random.default_rng(alphabet)
    out = []
    for n, m in _crossed(CODE_LENGTHS):
        a, b = rng.integers(0, alphabet, n), rng.integers(0, alphabet, m)
        out.append((a.astype(np.int32), b.astype(np.int32), R.edit_distance(a, b)))
    return out


def _guarded(dev, n, dtype, guard=64):
    """(buffer, inner view of n elements): sentinel-filled, `guard` elements on either side."""
    fill = {torch.int32: -77, torch.float64: -77.5, torch.uint8: 0xA5}[dtype]
    buf = torch.full((guard + n + guard,), fill, dtype=dtype, device=dev)
    return buf, buf[guard:guard + n], guard, fill


def _guards_intact(buf, guard, fill):
    return bool((buf[:guard] == fill).all()) and bool((buf[-guard:] == fill).all())


def _ragged(seqs, dev, dtype):
    lengths = [len(s) for s in seqs]
    off = np.zeros(len(seqs) + 1, np.int64)
    np.cumsum(lengths, out=off[1:])
    flat = np.concatenate(seqs) if sum(lengths) else np.zeros((0,) + np.shape(seqs[0])[1:])
    return torch.tensor(flat.astype(dtype), device=dev), torch.tensor(off, device=dev), lengths


def _scratch(dev, pairs, max_len):
    from sat_amd import _lib
    nbytes = int(_lib.load().sat_score_scratch_bytes(pairs, max_len))
    assert nbytes > 0
    return _guarded(dev, nbytes, torch.uint8, guard=256)


def run_edit(dev, pairs_ab, max_len=None, check=True):
    """Two runs into guarded buffers: (distance [pairs] numpy, error word)."""
    a, a_off, la = _ragged([x[0] for x in pairs_ab], dev, np.int32)
    b, b_off, lb = _ragged([x[1] for x in pairs_ab], dev, np.int32)
    n = len(pairs_ab)
    ml = max_len or max(1, max(la + lb))
    got = []
    for _ in range(2):
        obuf, out, g, fill = _guarded(dev, n, torch.int32)
        sbuf, scr, sg, sfill = _scratch(dev, n, ml)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        K.edit_distance(a, a_off, b, b_off, max_len=ml, out=out, err=err, scratch=scr,
                        check=check)
        torch.cuda.synchronize()
        assert _guards_intact(obuf, g, fill) and _guards_intact(sbuf, sg, sfill)
        got.append((out.cpu().numpy().copy(), int(err.item())))
    assert np.array_equal(got[0][0], got[1][0]) and got[0][1] == got[1][1]
    return got[0]


def run_dtw(dev, pairs_pt, max_len=None):
    """Two runs into guarded buffers: (cost, path_len) numpy; bit-identical or it fails."""
    p, p_off, lp = _ragged([x[0] for x in pairs_pt], dev, np.float32)
    t, t_off, lt = _ragged([x[1] for x in pairs_pt], dev, np.float32)
    n = len(pairs_pt)
    ml = max_len or max(lp + lt)
    got = []
    for _ in range(2):
        cbuf, cost, g, fill = _guarded(dev, n, torch.float64)
        nbuf, plen, ng, nfill = _guarded(dev, n, torch.int32)
        sbuf, scr, sg, sfill = _scratch(dev, n, ml)
        K.dtw_distortion(p, p_off, t, t_off, max_len=ml, cost=cost, path_len=plen, scratch=scr)
        torch.cuda.synchronize()
        assert _guards_intact(cbuf, g, fill) and _guards_intact(nbuf, ng, nfill)
        assert _guards_intact(sbuf, sg, sfill)
        got.append((cost.cpu().numpy().copy(), plen.cpu().numpy().copy()))
    assert got[0][0].tobytes() == got[1][0].tobytes()
    assert np.array_equal(got[0][1], got[1][1])
    return got[0]


def _check_dtw(width, cases, cost, plen, exact_path=True):
    bound = (width + 4) * 2.0 ** -23
    for k, (p, t, (ref_cost, ref_len, margin, mean)) in enumerate(cases):
        rel = abs(cost[k] - ref_cost) / ref_cost if ref_cost else abs(cost[k])
        print(f"width {width} case {k} ({len(p)} x {len(t)}): cost {cost[k]!r} ref {ref_cost!r} "
              f"rel {rel:.3e} bound {bound:.3e}; path {plen[k]} ref {ref_len}; "
              f"margin/mean {margin / mean:.3e}")
    for k, (p, t, (ref_cost, ref_len, margin, mean)) in enumerate(cases):
        assert abs(cost[k] - ref_cost) <= bound * ref_cost, (k, cost[k], ref_cost)
        if exact_path:
            assert margin > MARGIN * mean, (k, margin, mean)     # the seed table's promise
            assert plen[k] == ref_len, (k, plen[k], ref_len)
        assert max(len(p), len(t)) <= plen[k] <= len(p) + len(t) - 1


# ------------------------------------------------------------------ edit distance
@pytest.mark.parametrize("alphabet", [2, 256])
def test_edit_distance_ragged_batch_is_exact(cuda, alphabet):
    cases = code_cases(alphabet)
    got, err = run_edit(cuda, cases)
    assert err == 0
    assert got.tolist() == [c[2] for c in cases]


def test_edit_distance_one_pair(cuda):
    rng = np.random.default_rng(3)
    a, b = rng.integers(0, 4, S + 1).astype(np.int32), rng.integers(0, 4, 63).astype(np.int32)
    got, err = run_edit(cuda, [(a, b)])
    assert err == 0 and got.tolist() == [R.edit_distance(a, b)]


def test_edit_distance_more_pairs_than_compute_units(cuda):
    rng = np.random.default_rng(4)
    pairs = []
    for _ in range(300):
        n, m = rng.integers(0, 41, 2)
        pairs.append((rng.integers(0, 3, n).astype(np.int32), rng.integers(0, 3, m).astype(np.int32)))
    got, err = run_edit(cuda, pairs)
    assert err == 0
    assert got.tolist() == [R.edit_distance(a, b) for a, b in pairs]


# ------------------------------------------------------------------ DTW
@pytest.mark.parametrize("width", WIDTHS)
def test_dtw_ragged_batch(cuda, width):
    cases = dtw_cases(width)
    cost, plen = run_dtw(cuda, cases)
    _check_dtw(width, cases, cost, plen)


def test_dtw_one_pair(cuda):
    cases = [dtw_cases(13)[5]]
    cost, plen = run_dtw(cuda, cases)
    _check_dtw(13, cases, cost, plen)


def small_dtw_cases(count=300, width=13):
    """`count` pairs of 1..40 frames; a pair whose margin falls short is drawn again from the
    next seed (a rule that looks at the reference only)."""
    lengths = np.random.default_rng(5).integers(1, 41, (count, 2))
    out = []
    for k, (n, m) in enumerate(lengths):
        seed = 50000 + k
        while True:
            p, t = dtw_pair(width, int(n), int(m), seed)
            ref = R.dtw(p, t)
            if ref[2] > MARGIN * ref[3]:
                break
            seed += count
        out.append((p, t, ref))
    return out


def test_dtw_more_pairs_than_compute_units(cuda):
    cases = small_dtw_cases()
    cost, plen = run_dtw(cuda, cases)
    _check_dtw(13, cases, cost, plen)


def test_dtw_exact_ties_cost_and_path_bounds(cuda):
    """Integer-valued frames: ties at every turn.  The cost must still agree (a tie changes the
    path, not its cost); the path length is only held to max(Tp, Tt) <= n <= Tp + Tt - 1."""
    rng = np.random.default_rng(6)
    cases = []
    for n, m in _crossed([1, 2, 64, 65, S + 1]):
        p = rng.integers(0, 3, (n, 2)).astype(np.float32)
        t = rng.integers(0, 3, (m, 2)).astype(np.float32)
        cases.append((p, t, R.dtw(p, t)))
    cost, plen = run_dtw(cuda, cases)
    _check_dtw(2, cases, cost, plen, exact_path=False)


# ------------------------------------------------------------------ refusals
def test_bad_sizes_are_refused_before_any_launch():
    from sat_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(256)      # never dereferenced: every call below fails its host checks
    big = 1 << 40

    def edit(pairs, max_len):
        return lib.sat_edit_distance(fake, 8, fake, fake, 8, fake, pairs, max_len, fake, fake,
                                     fake, big, None)

    def dtw(width, pairs, max_len):
        return lib.sat_dtw_distortion(fake, 8, fake, fake, 8, fake, width, pairs, max_len, fake,
                                      fake, fake, fake, big, None)

    for fn, args, word in ((dtw, (0, 1, 8), b"width"), (dtw, (257, 1, 8), b"width"),
                           (dtw, (80, 1, 0), b"max_len"), (dtw, (80, 0, 8), b"pairs"),
                           (dtw, (80, 1, K.SCORE_MAX_LEN + 1), b"max_len"),
                           (edit, (1, 0), b"max_len"), (edit, (0, 8), b"pairs")):
        assert fn(*args) == _lib.SAT_ERR_ARGUMENT
        assert word in lib.sat_last_error_string()
    assert lib.sat_dtw_distortion(fake, 8, fake, fake, 8, fake, 80, 1, 8, fake, fake, fake, None,
                                  big, None) == _lib.SAT_ERR_ARGUMENT          # null scratch
    assert lib.sat_edit_distance(fake, 8, fake, fake, 8, fake, 1, 8, fake, fake, fake, 16,
                                 None) == _lib.SAT_ERR_ARGUMENT                # scratch too small


def test_scratch_query_is_host_arithmetic():
    from sat_amd import _lib
    lib = _lib.load()
    assert lib.sat_score_scratch_bytes(0, 8) < 0 and lib.sat_score_scratch_bytes(1, 0) < 0
    assert lib.sat_score_scratch_bytes(1, K.SCORE_MAX_LEN + 1) < 0
    one = lib.sat_score_scratch_bytes(1, 1000)
    assert one >= 1000 * 12 and lib.sat_score_scratch_bytes(7, 1000) == 7 * one


def test_edit_distance_overlong_pair_is_refused_alone(cuda):
    from sat_amd import _lib
    cases = code_cases(2)[:6] + code_cases(2)[10:16]       # lengths up to 65, and one of 2S + 3
    want = [c[2] if max(len(c[0]), len(c[1])) <= 65 else -1 for c in cases]
    assert -1 in want and sum(w == -1 for w in want) < len(want) / 2
    got, err = run_edit(cuda, cases, max_len=65, check=False)
    assert err == 1 and got.tolist() == want
    a, a_off, _ = _ragged([c[0] for c in cases], cuda, np.int32)
    b, b_off, _ = _ragged([c[1] for c in cases], cuda, np.int32)
    with pytest.raises(_lib.SatLibraryError):
        K.edit_distance(a, a_off, b, b_off, max_len=65)
    assert int(K.score_error_word(cuda).item()) == 0        # cleared after reporting


def test_dtw_overlong_and_empty_pairs_are_refused_alone(cuda):
    """Through the C entry (the wrapper's host check would refuse the empty pair first)."""
    from sat_amd import _lib
    cases = dtw_cases(13)
    picked = [cases[9], cases[10], cases[0], cases[11]]     # 1x1, 2x2, 1x(2S+3), 63x63
    p, _, lp = _ragged([c[0] for c in picked], cuda, np.float32)
    t, _, lt = _ragged([c[1] for c in picked], cuda, np.float32)
    assert lp == [1, 2, 1, 63] and lt == [1, 2, 2 * S + 3, 63]
    # pair 3 keeps 60 of its 63 true frames; a fifth pair gets the other 3 and no prediction
    ref3 = R.dtw(picked[3][0], picked[3][1][:60])
    assert ref3[2] > MARGIN * ref3[3]
    p_off = torch.tensor(np.cumsum([0, 1, 2, 1, 63, 0]), device=cuda)
    t_off = torch.tensor(np.cumsum([0, 1, 2, 2 * S + 3, 60, 3]), device=cuda)
    n = 5
    cbuf, cost, g, fill = _guarded(cuda, n, torch.float64)
    nbuf, plen, ng, nfill = _guarded(cuda, n, torch.int32)
    sbuf, scr, sg, sfill = _scratch(cuda, n, 63)
    err = torch.zeros(1, dtype=torch.int32, device=cuda)
    _lib.call("sat_dtw_distortion", p.data_ptr(), p.shape[0], p_off.data_ptr(), t.data_ptr(),
              t.shape[0], t_off.data_ptr(), 13, n, 63, cost.data_ptr(), plen.data_ptr(),
              err.data_ptr(), scr.data_ptr(), scr.numel(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert _guards_intact(cbuf, g, fill) and _guards_intact(nbuf, ng, nfill)
    assert _guards_intact(sbuf, sg, sfill)
    cost, plen = cost.cpu().numpy(), plen.cpu().numpy()
    assert int(err.item()) == 1
    assert np.isnan(cost[2]) and plen[2] == -1              # 2S + 3 > max_len
    assert np.isnan(cost[4]) and plen[4] == -1              # empty prediction
    kept = [(picked[0], 0), (picked[1], 1), ((picked[3][0], picked[3][1][:60], ref3), 3)]
    bound = 17 * 2.0 ** -23
    for (_, _, ref), k in kept:
        assert abs(cost[k] - ref[0]) <= bound * ref[0] and plen[k] == ref[1]
