"""Crafted inputs with rows of chosen lengths -- a test helper, not a test.

star_points(d, stars, n, k): n points in d dimensions (float32) whose symmetric kNN graph (k
counting the point itself) has rows of known lengths:

  * "stars": a centre and s satellites, satellite j at radius 0.5 (1 + 0.002 j) along its own
    coordinate axis, so every satellite's nearest neighbour is its centre (0.5 .. 0.63 away, the
    other satellites at least 0.70) and no two distances from one point tie.  The centre's row
    has exactly s edges; for k > 2 the k - 2 satellites of smallest radius are picked by every
    other satellite and have s edges too.
  * clusters of k points (one point and k - 1 more, 0.105 .. 0.13 along distinct axes): rows of
    k - 1 edges.  The last cluster takes the points left over (up to 2 k - 1).

Groups sit 3 apart on an 8 x 8 x ... grid in the last three coordinates, so no edge joins two
groups and every point stays within ~40 of the origin (squared norms of ~1e3: an fp32 ulp there is
1e-4, far below the 1e-3 steps between the squared distances that order the satellites).  The
points are shuffled (seeded), so stars fall among labelled and unlabelled rows alike.
row_lengths(X, k) is the float64 reference of the row lengths: exact kNN, union graph.
"""
from __future__ import annotations

import numpy as np


def star_points(d: int, stars, n: int, k: int = 4, seed: int = 0):
    assert d - 3 >= max([*stars, 2 * k]), "one coordinate axis per satellite, three for the grid"
    pts, grp = [], []

    def origin(g):
        o = np.zeros(d, np.float64)
        o[d - 3], o[d - 2], o[d - 1] = 3.0 * (g % 8), 3.0 * ((g // 8) % 8), 3.0 * (g // 64)
        return o

    g = 0
    for s in stars:
        o = origin(g)
        pts.append(o.copy())
        grp.append(g)
        for j in range(s):
            p = o.copy()
            p[j] += 0.5 * (1.0 + 0.002 * j)
            pts.append(p)
            grp.append(g)
        g += 1
    left = n - len(pts)
    assert left >= k, "room for at least one cluster"
    sizes = [k] * (left // k)
    sizes[-1] += left % k
    for sz in sizes:
        o = origin(g)
        pts.append(o.copy())
        grp.append(g)
        for j in range(1, sz):
            p = o.copy()
            p[j] += 0.1 * (1.0 + 0.05 * j)
            pts.append(p)
            grp.append(g)
        g += 1
    X = np.asarray(pts, np.float32)
    grp = np.asarray(grp)
    perm = np.random.default_rng(seed).permutation(n)
    return np.ascontiguousarray(X[perm]), grp[perm]


def row_lengths(X: np.ndarray, k: int) -> np.ndarray:
    Xd = X.astype(np.float64)
    sq = np.einsum("ij,ij->i", Xd, Xd)
    D = sq[:, None] + sq[None, :] - 2.0 * (Xd @ Xd.T)
    np.fill_diagonal(D, -1.0)
    nb = np.argsort(D, axis=1, kind="stable")[:, 1:k]
    A = np.zeros(D.shape, bool)
    A[np.repeat(np.arange(len(X)), k - 1), nb.ravel()] = True
    A |= A.T
    return A.sum(1)


def row_parts(length: int, nd: int) -> int:
    """Parts the fused backward runs a row of `length` edges in (fused_bwd.hip row_parts): the fewest
    of 1, 2, 4 whose EB P slots hold its first 64 edges; rows of one f32x4 per lane stay whole."""
    eb, pmax = (16 if nd <= 2 else 8), (4 if nd >= 2 else 1)
    p = 1
    while p < pmax and min(length, 64) > eb * p:
        p *= 2
    return p
