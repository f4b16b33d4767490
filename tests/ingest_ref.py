"""Float64 stage reference of the graph build from caller-supplied neighbour lists (ingest.hip,
DESIGN.md §3.14), the list generator the CPU and GPU tests share, and the case table of the GPU
stage test -- a test helper, not a test.  Pure numpy / scipy.

The stage: for row i and its list nbr[i, 0 .. K-2] (the other rows, in the caller's order)
  * an entry outside [0, n) is dropped and counted;
  * the row itself is dropped silently;
  * an entry equal to an earlier entry of the row (entries 0 .. t-1 as given) is dropped and
    counted;
  * d2 = sum_f (x_if - x_jf)^2 in float64 over the fp32 features; an entry whose d2, rounded to
    fp32, is 0 or not finite is dropped silently;
  * kept entries stay in order at columns 1 .. of knn_idx / knn_d2, the tail is (i, 0), column 0 is
    (i, 0); eps_i = epsilon, or for 'auto' sqrt(knn_d2[i, K-1]) (0 when that column is padding);
  * row j's reverse entries are {(i, d2_ij) : j kept in row i}.
The kernel returns d2 as the float64 sum rounded once to fp32: one rounding, far inside the bound
of the fp32 difference form the query kNN returns (tests/query_ref.py d2_bound), which is the
bound the tests hold it to; eps adds half of that and the rounding of sqrtf.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np
import scipy.sparse as sparse
from scipy.sparse.csgraph import connected_components

from tests import query_ref as Q

U32 = Q.U32


def d2_bound(d):
    """Relative bound of the stored fp32 d2 against float64: tests/query_ref.py's."""
    return Q.d2_bound(d)


def eps_bound(d):
    """Relative bound of the 'auto' eps_i = sqrtf(d2): half the d2 bound plus sqrtf's rounding."""
    return (0.5 * d2_bound(d) + U32) * 1.001


@dataclass
class Stage:
    knn_idx: np.ndarray     # n x K int64
    knn_d2: np.ndarray      # n x K float64
    eps: np.ndarray         # n float64
    dropped: int            # counted drops (out of range, repeats)
    kept: np.ndarray        # n: entries kept per row
    reverse: list           # per row j: {i: d2_ij}
    tiny_eps: bool          # some eps_i < 1e-10


def ingest_ref(X, nbr, epsilon) -> Stage:
    X = np.asarray(X, dtype=np.float32).astype(np.float64)
    nbr = np.asarray(nbr, dtype=np.int64)
    n, km1 = nbr.shape
    K = km1 + 1
    idx = np.tile(np.arange(n)[:, None], (1, K))
    d2o = np.zeros((n, K))
    kept = np.zeros(n, dtype=np.int64)
    reverse = [dict() for _ in range(n)]
    dropped = 0
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(n):
            row = nbr[i]
            pos = 0
            for t in range(km1):
                j = int(row[t])
                if j < 0 or j >= n:
                    dropped += 1
                    continue
                if j == i:
                    continue
                if (row[:t] == j).any():
                    dropped += 1
                    continue
                diff = X[i] - X[j]
                dd = float(np.dot(diff, diff))
                f = np.float32(dd)
                if not (f > 0) or not np.isfinite(f):
                    continue
                idx[i, 1 + pos] = j
                d2o[i, 1 + pos] = dd
                reverse[j][i] = dd
                pos += 1
            kept[i] = pos
    if isinstance(epsilon, str):
        assert epsilon == "auto"
        eps = np.sqrt(d2o[:, K - 1])
    else:
        eps = np.full(n, float(epsilon))
    return Stage(idx, d2o, eps, dropped, kept, reverse, bool((eps < 1e-10).any()))


def sym_rows(st: Stage):
    """Per row the symmetric graph the row build makes of a Stage: {col: d2}, the union of the
    row's kept entries and its reverse entries, the larger of the two directed distances."""
    n = st.knn_idx.shape[0]
    rows = []
    for i in range(n):
        r = dict(st.reverse[i])
        for t in range(int(st.kept[i])):
            j = int(st.knn_idx[i, 1 + t])
            r[j] = max(r.get(j, 0.0), float(st.knn_d2[i, 1 + t]))
        rows.append(r)
    return rows


# ------------------------------------------------------------------------------------------------
# the list generator shared by the CPU and GPU tests
# ------------------------------------------------------------------------------------------------
def approx_lists(X, k, seed=0):
    """n x (k - 1) int64: each row takes a random k - 1 of its 3 (k - 1) float64-nearest other rows
    (all n - 1 when there are fewer), in random order, from a seeded PCG64 stream -- what an
    approximate index returns: mostly near rows, not all of the nearest, in no distance order."""
    X = np.asarray(X, dtype=np.float32)
    n = X.shape[0]
    km1 = min(k, n) - 1
    pool = min(3 * km1, n - 1)
    D = Q.dist2(X, X)
    D[np.arange(n), np.arange(n)] = np.inf
    near = np.argsort(D, axis=1, kind="stable")[:, :pool]
    rng = np.random.Generator(np.random.PCG64(seed))
    out = np.empty((n, km1), dtype=np.int64)
    for i in range(n):
        out[i] = near[i, rng.permutation(pool)[:km1]]
    return out


def exact_lists(X, k):
    """n x (k - 1) int64: the float64 k - 1 nearest other rows, by (distance, index)."""
    X = np.asarray(X, dtype=np.float32)
    n = X.shape[0]
    D = Q.dist2(X, X)
    D[np.arange(n), np.arange(n)] = -1.0
    return np.argsort(D, axis=1, kind="stable")[:, 1:min(k, n)]


def with_self(nbr):
    """The reference's knn_ind: the row itself in column 0."""
    nbr = np.asarray(nbr, dtype=np.int64)
    return np.concatenate([np.arange(nbr.shape[0])[:, None], nbr], axis=1)


def components(nbr):
    """Connected components of the symmetrised graph of valid lists."""
    n, km1 = nbr.shape
    r = np.repeat(np.arange(n), km1)
    A = sparse.coo_matrix((np.ones(n * km1), (r, np.asarray(nbr).ravel())), shape=(n, n))
    return connected_components(A, directed=False)[0]


# ------------------------------------------------------------------------------------------------
# the GPU stage test's cases: name -> (n, d, k, builder of (X float32, nbr int64 n x (k-1)))
# ------------------------------------------------------------------------------------------------
def _normal(seed, n, d):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)


def _plain(seed, n, d, k):
    X = _normal(seed, n, d)
    return X, approx_lists(X, k, seed)


def _ns():
    from graphlearninglayer_amd.synth import CONFIGS, synth
    c = CONFIGS["ns"]
    X, _ = synth(c["base"], c["batch"], c["d"], r=c["r"], seed=0)
    return X, approx_lists(X, c["k"], 0)


def _hub(seed, n, d, k):
    """Column 0 of every list is row 0: n - 1 reverse entries on one row, past RCAP = 8 (k-1) + 8."""
    X, nbr = _plain(seed, n, d, k)
    nbr[:, 0] = 0
    return X, nbr


def _bad(seed, n, d, k):
    """Entries of -1, n, a repeat, the row itself and a duplicated point."""
    X = _normal(seed, n, d)
    X[7] = X[3]                      # rows 3 and 7 are the same point: d2 = 0 between them
    nbr = approx_lists(X, k, seed)
    nbr[0, 1] = -1
    nbr[1, 0] = n
    nbr[2, 3] = nbr[2, 0]            # a repeat
    nbr[4, 2] = 4                    # the row itself
    nbr[3, 1] = 7                    # the duplicated point (unless already listed: then a repeat)
    nbr[5, :] = nbr[5, 0]            # one entry, k - 2 repeats
    nbr[6, k - 2] = 2 * n + 5        # the last column out of range: 'auto' eps_6 = 0
    return X, nbr


CASES = {
    "ragged": (130, 7, 4, lambda: _plain(1, 130, 7, 4)),          # scalar loads, ragged
    "ns": (1000, 512, 10, _ns),
    "parts2": (300, 64, 65, lambda: _plain(2, 300, 64, 65)),      # lists in 64-entry parts
    "parts4": (300, 64, 257, lambda: _plain(3, 300, 64, 257)),
    "hub": (200, 16, 3, lambda: _hub(4, 200, 16, 3)),             # reverse overflow past RCAP = 24
    "bad": (150, 12, 6, lambda: _bad(5, 150, 12, 6)),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(X, nbr) of a case; computed once per process, read-only."""
    X, nbr = CASES[name][3]()
    X.setflags(write=False)
    nbr.setflags(write=False)
    return X, nbr


@functools.lru_cache(maxsize=None)
def stage(name, epsilon):
    X, nbr = case(name)
    return ingest_ref(X, nbr, epsilon)


# ------------------------------------------------------------------------------------------------
# the layer cases: shuffled approximate lists on the named configs
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def layer_case(config, seed=0):
    """(X, Y one-hot float32, nbr, k) of a named config (synth.CONFIGS) with approx_lists."""
    from graphlearninglayer_amd.synth import CONFIGS, one_hot, synth
    c = CONFIGS[config]
    X, lab = synth(c["base"], c["batch"], c["d"], r=c["r"], seed=seed)
    Y = one_hot(lab[: c["base"]])
    nbr = approx_lists(X, c["k"], seed)
    for a in (X, Y, nbr):
        a.setflags(write=False)
    return X, Y, nbr, c["k"]
