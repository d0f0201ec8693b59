"""Hand-checkable cases of tests/score_ref.py, the reference the GPU score kernels are tested
against, and the loop form of each recurrence against its anti-diagonal form."""
import numpy as np
import pytest

import score_ref as R


def _codes(word):
    return [ord(ch) for ch in word]


@pytest.mark.parametrize("fn", [R.edit_distance_loop, R.edit_distance])
def test_edit_distance_by_hand(fn):
    assert fn(_codes("kitten"), _codes("sitting")) == 3
    assert fn(_codes("sitting"), _codes("kitten")) == 3
    assert fn(_codes("flaw"), _codes("lawn")) == 2
    for n in (0, 1, 7):
        assert fn([], list(range(n))) == n
        assert fn(list(range(n)), []) == n
        assert fn(list(range(n)), list(range(n))) == 0
    assert fn([1, 2, 3], [4, 5, 6, 7]) == 4


@pytest.mark.parametrize("fn", [R.dtw_loop, R.dtw])
def test_dtw_by_hand(fn):
    rng = np.random.default_rng(0)
    x = rng.standard_normal((9, 3)).astype(np.float32)
    cost, cells, _, _ = fn(x, x)
    assert cost == 0.0 and cells == 9          # the diagonal wins every tie
    twice = np.repeat(x, 2, axis=0)
    for p, t in ((x, twice), (twice, x)):
        cost, cells, _, _ = fn(p, t)
        assert cost == 0.0 and cells == 18     # the longer length
    # one frame against many: a single row, every cell on the path
    cost, cells, margin, mean = fn(x[:1], x)
    c = np.sqrt(((x[:1].astype(np.float64) - x.astype(np.float64)) ** 2).sum(-1))
    assert cells == 9 and abs(cost - c.sum()) < 1e-12 and margin == np.inf
    assert abs(mean - c.mean()) < 1e-12
    # 1-D, by hand: p = 0 3, t = 0 1 3: path (0,0) (0,1) (1,2), cost 0 + 1 + 0
    cost, cells, margin, _ = fn(np.array([[0.], [3.]]), np.array([[0.], [1.], [3.]]))
    assert (cost, cells) == (1.0, 3)
    assert margin == 1.0      # at (1, 2): D(0, 1) = 1 against D(1, 1) = 2; (0, 2) costs 4


def test_loop_forms_equal_antidiagonal_forms_on_random_ragged_inputs():
    rng = np.random.default_rng(7)
    for _ in range(25):
        n, m = rng.integers(0, 24, 2)
        k = int(rng.choice([2, 5, 256]))
        a, b = rng.integers(0, k, n), rng.integers(0, k, m)
        assert R.edit_distance_loop(a, b) == R.edit_distance(a, b)
    for _ in range(12):
        n, m = rng.integers(1, 20, 2)
        w = int(rng.choice([1, 3, 13]))
        p = rng.standard_normal((n, w)).astype(np.float32)
        t = rng.standard_normal((m, w)).astype(np.float32)
        a, b = R.dtw_loop(p, t), R.dtw(p, t)
        assert a[1] == b[1]
        assert a[0] == b[0] and a[2] == b[2] and a[3] == b[3]
    # exact ties (integer frames): both forms break them diagonal, (i-1, j), (i, j-1)
    for _ in range(8):
        n, m = rng.integers(1, 16, 2)
        p = rng.integers(0, 2, (n, 2)).astype(np.float32)
        t = rng.integers(0, 2, (m, 2)).astype(np.float32)
        assert R.dtw_loop(p, t)[:2] == R.dtw(p, t)[:2]
