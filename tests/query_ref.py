"""Float64 references and derived error bounds for the query kNN and the out-of-sample extension
(query.hip), and the case table the GPU test runs.  Pure numpy: the CPU test
pins these references (scipy's cKDTree, a dense closed form) and evaluates the bounds on the
cases; the GPU test compares the kernels with them.  Every bound is counted from the kernels'
operations with u = 2^-24 (fp32) or 2^-53 (float64); nothing is fitted to a measurement."""
import functools
import itertools
import math

import numpy as np

U32 = 2.0 ** -24
U64 = 2.0 ** -53


# ----------------------------------------------------------------------------------------
# references
# ----------------------------------------------------------------------------------------
def dist2(Xq, Xdb):
    """Q x N float64 sum_f (q_f - x_f)^2 of the fp32 inputs (difference form)."""
    Xq = np.asarray(Xq, dtype=np.float32).astype(np.float64)
    Xdb = np.asarray(Xdb, dtype=np.float32).astype(np.float64)
    out = np.empty((Xq.shape[0], Xdb.shape[0]))
    for i in range(Xq.shape[0]):
        diff = Xdb - Xq[i]
        out[i] = np.einsum("nf,nf->n", diff, diff)
    return out


def knn_ref(Xq, Xdb, k):
    """(idx int64 Q x k, d2 float64 Q x k): the k smallest float64 distances, equal distances to
    the lower index (a stable sort of the distances is a sort on (distance, index))."""
    D = dist2(Xq, Xdb)
    idx = np.argsort(D, axis=1, kind="stable")[:, :k]
    return idx, np.take_along_axis(D, idx, axis=1)


def boundary_gap(Xq, Xdb, k):
    """Per row (d_(k+1) - d_k) / d_(k+1), inf for k = N: the relative float64 gap at the set's
    boundary.  A set comparison is only as exact as this gap is above float64 summation noise."""
    D = np.sort(dist2(Xq, Xdb), axis=1)
    if k >= D.shape[1]:
        return np.full(D.shape[0], np.inf)
    return (D[:, k] - D[:, k - 1]) / np.maximum(D[:, k], 1e-300)


def d2_bound(d):
    """Relative bound of the returned fp32 d^2 against float64.  Lane `sub` of an 8-lane group
    sums features 4 sub + 32 u + (0..3): n = 4 ceil(d / 32) fmaf steps, each term (a - b)^2 with
    the difference rounded once (2 u + u^2 on the square), then 3 additions of the butterfly.
    All terms are non-negative, so the roundings add up relative to the sum: (n + 3 + 2) u to
    first order, (n + 8) u with the higher orders for d <= 4096."""
    return (4 * math.ceil(d / 32) + 8) * U32


def gram_err(d):
    """|D2 - d^2| <= gram_err(d) (|a_q| + |a_j|)^2 for the nominating distances (query.hip
    q_gram_err repeats this count): centring a^ = fl(x - c) moves the distance by
    <= u (|a_q| + |a_j|), its square by <= 2 u (1 + u) (..)^2; each norm is d fmaf roundings plus
    a 6-level lane tree, <= (d + 6) u |a^|^2; the dot product accumulates d products with at most
    d roundings, <= d u |a^_q| |a^_j|, and enters twice; fl(nq + nj) and the closing fmaf add 2 u
    (..)^2.  Since |a_q|^2 + |a_j|^2 + 2 |a_q| |a_j| = (..)^2 the sum is <= (d + 10) u (1 + 2^-10)
    (..)^2 <= (d + 16) u (..)^2 for d <= 4096."""
    return (d + 16) * U32


def extend_ref(idx, d2, P, kn, epsilon, eps_db=None):
    """Float64 extension from a float64 kNN (idx, d2: Q x kn, nearest first): weights
    exp(-4 d2 / (eps_q eps_j)), eps_q = sqrt(d2[:, kn - 1]) for 'auto'.  Returns (Uq, labels, t)
    with t = the exponents' magnitudes 4 d2 / (eps_q eps_j)."""
    P = np.asarray(P, dtype=np.float32).astype(np.float64)
    if epsilon == "auto":
        eq = np.sqrt(d2[:, kn - 1])[:, None]
        ej = np.asarray(eps_db, dtype=np.float32).astype(np.float64)[idx]
    else:
        eq = ej = float(epsilon)
    t = 4.0 * d2 / (eq * ej)
    w = np.exp(-t)
    Uq = np.einsum("qk,qkc->qc", w, P[idx]) / w.sum(axis=1, keepdims=True)
    return Uq, label_ref(Uq), t


def label_ref(U):
    """Lowest index among the maxima; NaN ranks after every number (a row of NaN: 0)."""
    V = np.where(np.isnan(U), -np.inf, U)
    return np.argmax(V, axis=1).astype(np.int64)


def extend_dense(Xq, Xdb, P, kn, epsilon, eps_db=None):
    """The same extension as a dense closed form: W (Q x N) from every distance, zero outside the
    kn nearest, Uq = (W P) / (W 1)."""
    D = dist2(Xq, Xdb)
    order = np.argsort(D, axis=1, kind="stable")
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, np.arange(D.shape[1])[None, :], axis=1)
    if epsilon == "auto":
        eq = np.sqrt(np.take_along_axis(D, order[:, kn - 1:kn], axis=1))
        E = eq * np.asarray(eps_db, dtype=np.float32).astype(np.float64)[None, :]
    else:
        E = float(epsilon) ** 2
    W = np.where(rank < kn, np.exp(-4.0 * D / E), 0.0)
    return (W @ np.asarray(P, dtype=np.float32).astype(np.float64)) / W.sum(axis=1, keepdims=True)


def uq_bound(d, kn, t, P, auto):
    """Bound of |Uq_gpu - Uq_ref| (per entry) for the extension over the same neighbour sets.
    The kernel's exponent differs from the float64 reference's by a relative rho: the returned
    fp32 d^2 (d2_bound), for 'auto' eps_q = sqrtf of the fp32 d^2 (half of d2_bound plus one fp32
    rounding), and three float64 roundings.  A weight then differs by a relative
    delta = expm1(max t * rho) + 4 u64 (one ulp of exp on either side, with slack).  Weights off
    by relative delta move a weighted mean by <= 2 delta / (1 - delta) times the spread of P; the
    two float64 sums (kn products and additions each, in either order) and the division add
    <= 2 (kn + 2) u64 max|P| on each side."""
    rho = d2_bound(d) + ((0.5 * d2_bound(d) + U32) * 1.001 if auto else 0.0) + 3 * U64
    delta = math.expm1(float(np.max(t)) * rho) + 4 * U64
    P = np.asarray(P, dtype=np.float64)
    return 2 * delta / (1 - delta) * float(P.max() - P.min()) + 4 * (kn + 2) * U64 * float(np.abs(P).max())


# ----------------------------------------------------------------------------------------
# the GPU test's cases
# ----------------------------------------------------------------------------------------
def _normal(seed, Q, N, d):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((Q, d)).astype(np.float32),
            rng.standard_normal((N, d)).astype(np.float32))


def _offset(seed, Q, N, d, norm):
    Xq, Xdb = _normal(seed, Q, N, d)
    v = np.random.default_rng(seed + 1).standard_normal(d)
    v = (v / np.linalg.norm(v) * norm).astype(np.float32)
    return Xq + v, Xdb + v


def _far(seed, Q, N, d):
    Xq, Xdb = _normal(seed, Q, N, d)
    v = np.random.default_rng(seed + 1).standard_normal(d)
    Xq[Q - 1] = (v / np.linalg.norm(v) * 1e7).astype(np.float32)
    return Xq, Xdb


def _sphere(Q, N, d):
    """Every database row is q + a signed permutation of (3, 2, 1, 0, ...): every distance is
    exactly 14 in fp32 and in float64, and the centred rows are small integers, so the
    nominating distances tie exactly as well."""
    q = (np.arange(d) % 5 - 2).astype(np.float32)
    rows = []
    for pos in itertools.permutations(range(d), 3):
        for sg in itertools.product((1, -1), repeat=3):
            r = np.zeros(d, dtype=np.float32)
            for p, s, v in zip(pos, sg, (3, 2, 1)):
                r[p] = s * v
            rows.append(q + r)
            if len(rows) == N:
                return np.tile(q, (Q, 1)), np.stack(rows)
    raise ValueError("not enough signed permutations")


def _lattice(seed, Q, N, d):
    """Small-integer coordinates, every database row twice (rows 2 i and 2 i + 1), queries equal to
    database rows: exact distances with many ties, d2 = 0 first."""
    rng = np.random.default_rng(seed)
    B = rng.integers(0, 4, size=(N // 2, d)).astype(np.float32)
    Xdb = np.repeat(B, 2, axis=0)
    return Xdb[rng.integers(0, N, size=Q)].copy(), Xdb


# name: (builder, k, exact) -- exact: idx and d2 must equal the reference bitwise (all sums exact)
CASES = {
    "ragged": (lambda: _normal(1, 33, 300, 7), 5, False),
    "eval_like": (lambda: _normal(2, 64, 1024, 128), 50, False),
    "wide": (lambda: _normal(3, 40, 2100, 130), 65, False),
    "kmax": (lambda: _normal(4, 5, 300, 16), 256, False),
    "all": (lambda: _normal(5, 3, 40, 5), 40, False),
    "one": (lambda: _normal(6, 1, 64, 4), 1, False),
    "offset100": (lambda: _offset(7, 70, 1000, 20, 100.0), 26, False),
    "offset1000": (lambda: _offset(7, 70, 1000, 20, 1000.0), 26, False),
    "far_query": (lambda: _far(8, 4, 500, 16), 10, False),
    "sphere": (lambda: _sphere(2, 300, 8), 10, True),
    "sphere_overflow": (lambda: _sphere(2, 600, 8), 10, True),   # > 512 columns tie at the threshold
    "lattice": (lambda: _lattice(9, 20, 300, 6), 8, True),
}
# relative float64 gap at the set boundary below which a row's set is not compared (float64
# sums in two orders differ by <= 2 (d + 2) u64 relative; no case has such a row, which the CPU
# test asserts, so the GPU test excuses nothing)
def tie_gap(d):
    return 4 * (d + 2) * U64


@functools.lru_cache(maxsize=None)
def case(name):
    """(Xq, Xdb, k, exact, idx_ref, d2_ref) of a case; computed once per process."""
    build, k, exact = CASES[name]
    Xq, Xdb = build()
    idx, d2 = knn_ref(Xq, Xdb, k)
    for a in (Xq, Xdb, idx, d2):
        a.setflags(write=False)
    return Xq, Xdb, k, exact, idx, d2


def _clusters(seed, Q, N, d, C, spread):
    """C well-separated clusters; P = the cluster's one-hot plus noise, so Uq depends on the
    weights while every row's top-2 gap stays near 1."""
    rng = np.random.default_rng(seed)
    cen = rng.standard_normal((C, d)) * 6.0
    ldb, lq = rng.integers(0, C, size=N), rng.integers(0, C, size=Q)
    Xdb = (cen[ldb] + spread * rng.standard_normal((N, d))).astype(np.float32)
    Xq = (cen[lq] + spread * rng.standard_normal((Q, d))).astype(np.float32)
    P = (np.eye(C)[ldb] + 0.1 * rng.random((N, C))).astype(np.float32)
    return Xq, Xdb, P


# name: (builder, k (incl. self: kn = k - 1), epsilon)
EXT_CASES = {
    "fixed": (lambda: _clusters(11, 37, 400, 16, 4, 0.5), 12, 3.0),
    "auto": (lambda: _clusters(12, 37, 400, 16, 4, 0.5), 12, "auto"),
    "auto_wide": (lambda: _clusters(13, 10, 700, 130, 70, 0.5), 80, "auto"),
}


def eps_of(Xdb, k):
    """The database graph's 'auto' eps_i as float32: the distance to the k-th neighbour incl.
    self (the (k - 1)-th other row), GLL.py:205."""
    D = np.sort(dist2(Xdb, Xdb), axis=1)
    return np.sqrt(D[:, k - 1]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def ext_case(name):
    """(Xq, Xdb, P, k, epsilon, eps_db, Uq_ref, labels_ref, bound) of an extension case."""
    build, k, epsilon = EXT_CASES[name]
    Xq, Xdb, P = build()
    kn = k - 1
    eps_db = eps_of(Xdb, k) if epsilon == "auto" else None
    idx, d2 = knn_ref(Xq, Xdb, kn)
    Uq, lab, t = extend_ref(idx, d2, P, kn, epsilon, eps_db)
    bound = uq_bound(Xq.shape[1], kn, t, P, epsilon == "auto")
    for a in (Xq, Xdb, P, Uq, lab):
        a.setflags(write=False)
    return Xq, Xdb, P, k, epsilon, eps_db, Uq, lab, bound
