"""Float64 reference of gll_knn_rerank (rerank.hip) in both modes, and the pools
the GPU test runs.  Pure numpy on top of tests/query_ref.py (dist2, knn_ref, d2_bound): validity,
the ranking by (float64 d^2, index) with ties to the lower index, the (-1, +inf) padding of short
rows and the status counts.  The CPU test pins the reference against query_ref.knn_ref and checks
the pools; the GPU test compares the kernel with it."""
import functools

import numpy as np

from tests import query_ref as R

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def valid_mask(cand, N):
    """Q x c bool: the entry lies in [0, N) and no earlier entry of its row holds the same index."""
    cand = np.asarray(cand, dtype=np.int64)
    ok = (cand >= 0) & (cand < N)
    for q in range(cand.shape[0]):
        seen = set()
        for e, j in enumerate(cand[q].tolist()):
            if ok[q, e]:
                ok[q, e] = j not in seen
                seen.add(j)
    return ok


def _row_dist(xq, Xdb, js):
    """float64 d^2 of one query to rows js; NaN -> +inf (what the kernel ranks)."""
    if len(js) == 0:
        return np.zeros(0)
    with np.errstate(invalid="ignore", over="ignore"):
        dd = R.dist2(xq[None, :], Xdb[np.asarray(js, dtype=np.int64)])[0]
    return np.where(np.isnan(dd), np.inf, dd)


def rerank_ref(Xq, Xdb, cand, k, keep_order=False):
    """(idx int64 Q x k, d2 float64 Q x k, status [0, rows with a non-finite kept distance, 0, short
    rows]).  Pool mode: the k valid candidates nearest by (float64 d^2, index), in that order --
    the kernel's (returned fp32 d^2, index) order wherever order_determined says the two agree; a short row ends in (-1, +inf).  List mode (c == k): idx =
    cand, +inf for an index outside [0, N)."""
    Xq = np.asarray(Xq, dtype=np.float32)
    Xdb = np.asarray(Xdb, dtype=np.float32)
    cand = np.asarray(cand, dtype=np.int64)
    Q, c = cand.shape
    N = Xdb.shape[0]
    idx = np.full((Q, k), -1, dtype=np.int64)
    d2 = np.full((Q, k), np.inf)
    status = [0, 0, 0, 0]
    if keep_order:
        assert c == k
        inr = (cand >= 0) & (cand < N)
        for q in range(Q):
            idx[q] = cand[q]
            d2[q, inr[q]] = _row_dist(Xq[q], Xdb, cand[q, inr[q]])
            status[1] += int(not np.isfinite(d2[q]).all())
        return idx, d2, status
    ok = valid_mask(cand, N)
    for q in range(Q):
        js = cand[q, ok[q]]
        dd = _row_dist(Xq[q], Xdb, js)
        order = np.lexsort((js, dd))[:k]     # by (d^2, index)
        nb = len(order)
        idx[q, :nb], d2[q, :nb] = js[order], dd[order]
        status[1] += int(not np.isfinite(d2[q, :nb]).all())
        status[3] += int(nb < k)
    return idx, d2, status


def order_determined(d2_row, d):
    """The float64 order of a kept list is the order of the returned fp32 values: neighbours in
    the list are equal (the case's sums are exact, or the two rows are the same row of numbers) or
    further apart than the two fp32 values' errors together."""
    a, b = d2_row[:-1], d2_row[1:]
    fin = np.isfinite(b)
    return bool(np.all((a[fin] == b[fin]) | (b[fin] - a[fin] > 2 * R.d2_bound(d) * b[fin])))


def boundary_clear(Xq, Xdb, cand, k):
    """No row's k-th and (k + 1)-th valid candidates are a float64 near-tie (query_ref.tie_gap):
    the kept set does not hang on the order of a float64 sum.  Exact ties are fine: they go to
    the lower index on both sides."""
    ok = valid_mask(cand, Xdb.shape[0])
    for q in range(len(Xq)):
        dd = np.sort(_row_dist(np.asarray(Xq[q], np.float32), np.asarray(Xdb, np.float32),
                               np.asarray(cand, np.int64)[q, ok[q]]))
        if len(dd) > k and np.isfinite(dd[k]):
            gap = dd[k] - dd[k - 1]
            if gap != 0 and gap <= R.tie_gap(Xdb.shape[1]) * dd[k]:
                return False
    return True


# ----------------------------------------------------------------------------------------
# the GPU test's pools: name -> (Xq, Xdb, cand int32 Q x c, k)
# ----------------------------------------------------------------------------------------
def _pool(seed, Q, N, d, c, lo=0):
    rng = np.random.default_rng(seed)
    Xq = rng.standard_normal((Q, d)).astype(np.float32)
    Xdb = rng.standard_normal((N, d)).astype(np.float32)
    return Xq, Xdb, rng.integers(lo, N, size=(Q, c)).astype(np.int32)


def _hard():
    """Repeats, -1, N, INT32_MIN, INT32_MAX, a row with no valid entry, short rows."""
    Xq, Xdb, cand = _pool(61, 7, 40, 9, 24)
    N = 40
    cand[0, 3], cand[0, 9], cand[0, 10] = -1, N, I32_MIN
    cand[1, 0], cand[1, 23] = I32_MAX, I32_MIN
    cand[2, :] = cand[2, 0]                       # one valid entry: a short row
    cand[3, :] = [-1, N, I32_MIN, I32_MAX] * 6    # no valid entry
    cand[4, :] = np.arange(24) % 5                # five valid entries: a short row at k = 6
    cand[5, ::2] = cand[5, 1::2]                  # every entry twice
    return Xq, Xdb, cand, 6


def _lattice():
    """Small-integer coordinates, every database row twice, queries on database rows: exact
    distances and many exact ties (to the lower index)."""
    Xq, Xdb = R._lattice(62, 9, 120, 6)
    rng = np.random.default_rng(63)
    cand = np.stack([rng.permutation(120)[:70] for _ in range(9)]).astype(np.int32)
    return Xq, Xdb, cand, 20


def _nonfinite():
    Xq, Xdb, cand = _pool(64, 6, 50, 12, 30)
    Xq, Xdb = Xq.copy(), Xdb.copy()
    Xq[1, 3] = np.inf
    Xq[2, 0] = np.nan
    Xdb[7, 4] = np.nan
    Xdb[11, 1] = -np.inf
    cand[0, :4] = [7, 11, 7, 3]     # a short row that keeps its two non-finite candidates
    cand[0, 4:] = 3
    cand[4, :] = np.arange(30)      # rows 7 and 11 rank last and are left out
    return Xq, Xdb, cand, 12


def _shape(seed, Q, N, d, c, k):
    Xq, Xdb, cand = _pool(seed, Q, N, d, c, lo=-2)   # -2, -1: a few invalid entries everywhere
    return Xq, Xdb, cand, k


POOLS = {
    "hard": _hard,
    "lattice": _lattice,
    "nonfinite": _nonfinite,
    # d: 1, 3, 4 (one vector), 32 (one sweep of the 8 lanes), 36, 130; c: eight candidates a sweep,
    # 64 a register slot; k: 1, c, 256; Q: four rows a workgroup; N: 1, 2
    "d1_c1": lambda: _shape(70, 1, 30, 1, 1, 1),
    "d3_c7": lambda: _shape(71, 3, 30, 3, 7, 7),
    "d4_c8": lambda: _shape(72, 4, 30, 4, 8, 1),
    "d32_c9": lambda: _shape(73, 5, 30, 32, 9, 9),
    "d36_c64": lambda: _shape(74, 5, 200, 36, 64, 64),
    "d130_c65": lambda: _shape(75, 3, 200, 130, 65, 1),
    "c256_k256": lambda: _shape(76, 4, 600, 4, 256, 256),
    "c512_k256": lambda: _shape(77, 5, 600, 3, 512, 256),
    "c512_k1": lambda: _shape(78, 1, 600, 36, 512, 1),
    "n1": lambda: _shape(79, 5, 1, 4, 9, 1),
    "n2": lambda: _shape(80, 5, 2, 3, 8, 8),
}
# the pools whose rows all hold k valid candidates are also run as lists (their first k columns)


@functools.lru_cache(maxsize=None)
def pool(name):
    """(Xq, Xdb, cand, k, idx_ref, d2_ref, status_ref, det) of a pool; det: the rows whose float64
    order is the order of the returned values (order_determined) -- their lists must equal the
    reference's entry by entry, the others' as sets and in (returned d2, index) order.  Computed
    once per process."""
    Xq, Xdb, cand, k = POOLS[name]()
    idx, d2, status = rerank_ref(Xq, Xdb, cand, k)
    assert boundary_clear(Xq, Xdb, cand, k), name
    det = np.array([order_determined(d2[q], Xdb.shape[1]) for q in range(len(Xq))])
    for a in (Xq, Xdb, cand, idx, d2, det):
        a.setflags(write=False)
    return Xq, Xdb, cand, k, idx, d2, status, det


@functools.lru_cache(maxsize=None)
def shuffled_pool(name):
    """A query case of query_ref with a pool that holds the true k nearest by construction: the
    2k nearest (or all N), each row's columns shuffled.  (Xq, Xdb, k, cand int64)."""
    Xq, Xdb, k, *_ = R.case(name)
    wide = min(2 * k, Xdb.shape[0])
    rng = np.random.default_rng(90)
    cand = R.knn_ref(Xq, Xdb, wide)[0]
    cand = np.stack([row[rng.permutation(wide)] for row in cand])
    # the reference alone satisfies what the GPU test asks of the kernel
    idx, d2, status = rerank_ref(Xq, Xdb, cand, k)
    ref_idx, ref_d2 = R.knn_ref(Xq, Xdb, k)
    assert (idx == ref_idx).all() and (d2 == ref_d2).all() and status == [0, 0, 0, 0], name
    cand.setflags(write=False)
    return Xq, Xdb, k, cand
