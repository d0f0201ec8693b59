"""Plain integer / float64 references of the synthesis scores (csrc/score.hip).

Each recurrence is written twice: as the textbook double loop, and swept along anti-diagonals
with numpy (every cell of an anti-diagonal depends only on the two before it) for speed.
tests/test_score_ref_cpu.py checks each form against the other.

  edit distance  E(i, j) over prefixes, unit costs.
  DTW            c(i, j) = ||p_i - t_j||_2 in float64 from the inputs as given;
                 D(0, 0) = c(0, 0), D(i, j) = c(i, j) + min(D(i-1, j-1), D(i-1, j), D(i, j-1)),
                 ties in that order; the path length is carried with the minimum.  Beside the
                 cost and the path length the DTW forms return the MARGIN: the smallest gap
                 between the best and the second-best predecessor over the cells of the optimal
                 path (cells with one finite predecessor have an infinite gap), and the mean
                 cell cost of the grid, which the GPU test scales the margin by.
"""
import numpy as np


def edit_distance_loop(a, b) -> int:
    a, b = list(a), list(b)
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        cur = [i] + [0] * len(b)
        for j in range(1, len(b) + 1):
            cur[j] = min(prev[j - 1] + (a[i - 1] != b[j - 1]), prev[j] + 1, cur[j - 1] + 1)
        prev = cur
    return prev[len(b)]


def edit_distance(a, b) -> int:
    """Anti-diagonal form: E[i, j] with i + j = d from the diagonals d - 1 and d - 2."""
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    n, m = len(a), len(b)
    if n == 0 or m == 0:
        return n + m
    E = np.zeros((n + 1, m + 1), np.int64)
    E[:, 0] = np.arange(n + 1)
    E[0, :] = np.arange(m + 1)
    ne = (a[:, None] != b[None, :]).astype(np.int64)
    for d in range(2, n + m + 1):
        i = np.arange(max(1, d - m), min(n, d - 1) + 1)
        j = d - i
        E[i, j] = np.minimum(E[i - 1, j - 1] + ne[i - 1, j - 1],
                             np.minimum(E[i - 1, j], E[i, j - 1]) + 1)
    return int(E[n, m])


def cell_costs(p, t) -> np.ndarray:
    """c[i, j] = ||p_i - t_j||_2 in float64, by direct differences (rows in slabs)."""
    p = np.asarray(p, np.float64).reshape(len(p), -1)
    t = np.asarray(t, np.float64).reshape(len(t), -1)
    c = np.empty((len(p), len(t)))
    for i0 in range(0, len(p), 32):
        d = p[i0:i0 + 32, None, :] - t[None, :, :]
        c[i0:i0 + 32] = np.sqrt((d * d).sum(-1))
    return c


def _trace(choice, gap, n, m):
    """Walks the chosen predecessors back from (n - 1, m - 1): (cells on the path, margin)."""
    i, j, cells, margin = n - 1, m - 1, 1, np.inf
    while i or j:
        margin = min(margin, gap[i, j])
        k = choice[i, j]
        i, j = (i - 1, j - 1) if k == 0 else (i - 1, j) if k == 1 else (i, j - 1)
        cells += 1
    return cells, float(margin)


def dtw_loop(p, t):
    """(cost, path_len, margin, mean cell cost), the double loop."""
    c = cell_costs(p, t)
    n, m = c.shape
    D = np.full((n, m), np.inf)
    L = np.zeros((n, m), np.int64)
    choice = np.zeros((n, m), np.int64)
    gap = np.full((n, m), np.inf)
    for i in range(n):
        for j in range(m):
            if i == 0 and j == 0:
                D[0, 0], L[0, 0] = c[0, 0], 1
                continue
            cand = [D[i - 1, j - 1] if i and j else np.inf, D[i - 1, j] if i else np.inf,
                    D[i, j - 1] if j else np.inf]
            k = 0
            if cand[1] < cand[k]:
                k = 1
            if cand[2] < cand[k]:
                k = 2
            prev = [(i - 1, j - 1), (i - 1, j), (i, j - 1)][k]
            D[i, j], L[i, j], choice[i, j] = c[i, j] + cand[k], L[prev] + 1, k
            rest = sorted(cand)
            gap[i, j] = rest[1] - rest[0] if np.isfinite(rest[1]) else np.inf
    cells, margin = _trace(choice, gap, n, m)
    assert cells == L[n - 1, m - 1]
    return float(D[n - 1, m - 1]), int(L[n - 1, m - 1]), margin, float(c.mean())


def dtw(p, t):
    """(cost, path_len, margin, mean cell cost), anti-diagonal form."""
    c = cell_costs(p, t)
    n, m = c.shape
    # one row and one column of +inf in front; D(-1, -1) = 0 makes D(0, 0) = c(0, 0)
    D = np.full((n + 1, m + 1), np.inf)
    D[0, 0] = 0.0
    L = np.zeros((n + 1, m + 1), np.int64)
    choice = np.zeros((n, m), np.int64)
    gap = np.full((n, m), np.inf)
    for d in range(2, n + m + 1):
        i = np.arange(max(1, d - m), min(n, d - 1) + 1)
        j = d - i
        cand = np.stack([D[i - 1, j - 1], D[i - 1, j], D[i, j - 1]])
        k = np.zeros(len(i), np.int64)
        best = cand[0].copy()
        for q in (1, 2):
            better = cand[q] < best
            k[better] = q
            best = np.where(better, cand[q], best)
        lens = np.stack([L[i - 1, j - 1], L[i - 1, j], L[i, j - 1]])
        D[i, j] = c[i - 1, j - 1] + best
        L[i, j] = lens[k, np.arange(len(i))] + 1
        choice[i - 1, j - 1] = k
        s = np.sort(cand, axis=0)
        with np.errstate(invalid="ignore"):
            g = s[1] - s[0]
        gap[i - 1, j - 1] = np.where(np.isfinite(s[1]), g, np.inf)
    cells, margin = _trace(choice, gap, n, m)
    assert cells == L[n, m]
    return float(D[n, m]), int(L[n, m]), margin, float(c.mean())
