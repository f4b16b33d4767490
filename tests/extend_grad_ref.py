"""Float64 reference, derived stage bound and case table for the backward of the out-of-sample
extension (extend_grad.hip).  Pure numpy; tests/query_ref.py is only imported.

The neighbour lists are frozen.  For query q, entry i, j = idx[q, i], delta = d2[q, i]:
  t_i = 4 delta_i / (e_q e_j),  w_i = exp(-t_i),  S = sum_i w_i,  u = sum_i w_i P[j_i] / S
  r_i = sum_c g_c (P[j_i, c] - u_c),  beta_i = w_i r_i / S,  a_i = w_i / S
  c_i = -4 beta_i / (e_q e_j);  'auto': c_last += (sum_i beta_i t_i) / (2 delta_last)
  gXq[q] = 2 sum_i c_i (x_q - x_j),  gXdb[j] = -2 sum c_i (x_q - x_j),  gP[j] = sum a_i g[q]
  grad_eps = sum_q sum_i 2 beta_i t_i / eps   (fixed eps)
"""
import functools

import numpy as np

from tests import query_ref as R

U32 = R.U32
U64 = R.U64


# ----------------------------------------------------------------------------------------
# the closed form and its bound
# ----------------------------------------------------------------------------------------
def _f64(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _eps_pair(idx, d2, epsilon, eps_db):
    """(e_q as Q x 1, e_j as Q x kn or scalar, eps as float or None).  A float32 d2 is the
    kernel's input: e_q is then its sqrtf, as gll_extend takes it; a float64 d2 takes the float64
    square root."""
    if isinstance(epsilon, str):
        last = d2[:, -1]
        eq = np.sqrt(last).astype(np.float64)[:, None]     # float32 in: the float32 sqrt
        return eq, _f64(eps_db)[idx], None
    e = float(np.float32(epsilon))
    return np.full((idx.shape[0], 1), e), e, e


def closed_form(Xq, Xdb, P, idx, d2, gU, epsilon, eps_db=None, bounds=False):
    """The gradients of L = sum(gU * Uq) on given lists (idx, d2: Q x kn): a dict with gXq (Q x d),
    gXdb (N x d), gP (N x C) and geps (a float, None for 'auto').  bounds=True adds b_gXq, b_gXdb,
    b_gP, b_geps: the per-entry bound of |kernel - this| (see stage_bound's count)."""
    X, Y, Pd = _f64(Xq), _f64(Xdb), _f64(P)
    g = np.asarray(gU, dtype=np.float64)
    idx = np.asarray(idx).astype(np.int64)
    N, C = Pd.shape
    Q, kn = idx.shape
    delta = np.asarray(d2).astype(np.float64)
    eq, ej, e = _eps_pair(idx, np.asarray(d2), epsilon, eps_db)
    den = eq * ej * np.ones((Q, kn))
    t = 4.0 * delta / den
    w = np.exp(-t)
    S = w.sum(axis=1, keepdims=True)
    Pj = Pd[idx]                                   # Q x kn x C
    u = np.einsum("qk,qkc->qc", w, Pj) / S
    dev = Pj - u[:, None, :]
    r = np.einsum("qc,qkc->qk", g, dev)
    beta = w * r / S
    a = w / S
    c0 = -4.0 * beta / den
    c = c0.copy()
    sbt = (beta * t).sum(axis=1)
    if e is None:
        c[:, -1] += sbt / (2.0 * delta[:, -1])
    diff = X[:, None, :] - Y[idx]                  # Q x kn x d, exact
    out = {
        "gXq": 2.0 * np.einsum("qk,qkd->qd", c, diff),
        "gXdb": np.zeros_like(Y),
        "gP": np.zeros_like(Pd),
        "geps": None if e is None else float((2.0 * sbt / e).sum()),
    }
    np.add.at(out["gXdb"], idx, -2.0 * c[:, :, None] * diff)
    np.add.at(out["gP"], idx, a[:, :, None] * g[:, None, :])
    if bounds:
        out.update(stage_bound(out, idx, N, C, kn, delta, den, t, w, S, Pj, u, dev, g, beta, a, c0,
                               c, sbt, diff, e))
    return out


def stage_bound(ref, idx, N, C, kn, delta, den, t, w, S, Pj, u, dev, g, beta, a, c0, c, sbt, diff, e):
    """|kernel - closed_form| per output entry <= 2^-24 |ref| + 2 u64 E, E the first-order error
    of ONE float64 evaluation of the formulas in any summation order, counted in units of u64 =
    2^-53 from the kernel's operations (the factor 2: the kernel and this reference each make it;
    both are fed the same idx and fp32 d2, and x_q - x_j is exact, so nothing else differs):
      t_i      4 delta exact, e_q e_j and the quotient: 2 roundings
      w_i      exp within 1 ulp = 2 u64, plus the exponent's 2 u64 t_i:  ew = 2 tmax + 2 (row max)
      S        kn - 1 additions of positive terms:                       eS = ew + kn - 1
      u_c      kn products, kn - 1 additions, the quotient, w and S:     Eu_c = (ew + eS + kn + 1) sum_i w_i |P_ic| / S
      r_i      per class a subtraction and a product, C - 1 additions:   Er_i = (C + 1) sum_c |g_c||P_ic - u_c| + sum_c |g_c| Eu_c
      beta_i   a product and a quotient, w, S and r:                     Eb_i = (ew + eS + 2)|beta_i| + a_i Er_i
      a_i      one quotient, w and S:                                    Ea_i = (ew + eS + 1) a_i
      c_i      a product (exact: x 4) and a quotient:                    Ec_i = 4 Eb_i / (e_q e_j) + 2 |c_i|
      'auto'   sum_i beta_i t_i: kn products, kn - 1 additions, t's 2 roundings; the quotient by
               2 delta_last and the addition to c_last:
               Ec_last += (sum_i t_i Eb_i + (kn + 3)|beta_i t_i|) / (2 delta_last) + 2 (|extra| + |c_last|)
      gXq      kn products and kn - 1 additions (x 2 exact):             2 sum_i (|d_if| Ec_i + (kn + 1)|c_i d_if|)
      gXdb     the same over a list of L entries:                        2 sum (|d| Ec + (L + 1)|c d|)
      gP       L products, L - 1 additions:                              sum (Ea_i |g| + (L + 1) a_i |g|)
      grad_eps per row sum_i beta_i t_i as above, x 2 / eps (one rounding), Q - 1 additions:
               (2 / eps) sum_q (sum_i t_i Eb_i + (kn + 3)|beta_i t_i|) + (Q + 2)(2 / eps) sum_q |sum_i beta_i t_i|
    and the single rounding of each output to fp32 adds 2^-24 |ref| (2^-149 where the result is
    subnormal).  grad_eps stays float64 and has no such term."""
    Q = idx.shape[0]
    ew = (2.0 * t.max(axis=1) + 2.0)[:, None]                       # Q x 1
    eS = ew + (kn - 1)
    A = np.einsum("qk,qkc->qc", w, np.abs(Pj)) / S
    Eu = (ew + eS + kn + 1) * A
    ag = np.abs(g)
    Er = (C + 1) * np.einsum("qc,qkc->qk", ag, np.abs(dev)) + (ag * Eu).sum(axis=1, keepdims=True)
    Eb = (ew + eS + 2) * np.abs(beta) + a * Er
    Ea = (ew + eS + 1) * a
    Ec = 4.0 * Eb / den + 2.0 * np.abs(c0)
    Esbt = (t * Eb + (kn + 3) * np.abs(beta * t)).sum(axis=1)
    if e is None:
        extra = sbt / (2.0 * delta[:, -1])
        Ec[:, -1] += Esbt / (2.0 * delta[:, -1]) + 2.0 * (np.abs(extra) + np.abs(c[:, -1]))
    ad, ac = np.abs(diff), np.abs(c)
    L = np.bincount(idx.ravel(), minlength=N).astype(np.float64)
    E_xq = 2.0 * (np.einsum("qk,qkd->qd", Ec, ad) + (kn + 1) * np.einsum("qk,qkd->qd", ac, ad))
    E1, T1 = np.zeros_like(ref["gXdb"]), np.zeros_like(ref["gXdb"])
    np.add.at(E1, idx, 2.0 * Ec[:, :, None] * ad)
    np.add.at(T1, idx, 2.0 * ac[:, :, None] * ad)
    E2, T2 = np.zeros_like(ref["gP"]), np.zeros_like(ref["gP"])
    np.add.at(E2, idx, Ea[:, :, None] * ag[:, None, :])
    np.add.at(T2, idx, a[:, :, None] * ag[:, None, :])
    tiny = 2.0 ** -149
    b = {
        "b_gXq": U32 * np.abs(ref["gXq"]) + 2 * U64 * E_xq + tiny,
        "b_gXdb": U32 * np.abs(ref["gXdb"]) + 2 * U64 * (E1 + (L + 1)[:, None] * T1) + tiny,
        "b_gP": U32 * np.abs(ref["gP"]) + 2 * U64 * (E2 + (L + 1)[:, None] * T2) + tiny,
        "b_geps": None,
    }
    if e is not None:
        b["b_geps"] = 2 * U64 * ((2.0 / e) * Esbt.sum() + (Q + 2) * (2.0 / e) * np.abs(sbt).sum())
    return b


def forward_np(Xq, Xdb, P, idx, epsilon, eps_db=None):
    """Uq of the plain formula in float64 on frozen lists, the distances from the features (for
    finite differences)."""
    X, Y, Pd = (np.asarray(v, dtype=np.float64) for v in (Xq, Xdb, P))
    diff = X[:, None, :] - Y[idx]
    d2 = (diff * diff).sum(axis=2)
    if isinstance(epsilon, str):
        den = np.sqrt(d2[:, -1:]) * np.asarray(eps_db, dtype=np.float64)[idx]
    else:
        den = float(epsilon) ** 2
    w = np.exp(-4.0 * d2 / den)
    return np.einsum("qk,qkc->qc", w, Pd[idx]) / w.sum(axis=1, keepdims=True)


def transposed_lists(idx, N):
    """For every database row j the entries (q, i) with idx[q, i] == j, ordered by q (then i):
    a list of N int64 arrays of shape (L_j, 2).  Indices outside [0, N) belong to no row."""
    idx = np.asarray(idx)
    out = [[] for _ in range(N)]
    for q in range(idx.shape[0]):
        for i in range(idx.shape[1]):
            j = int(idx[q, i])
            if 0 <= j < N:
                out[j].append((q, i))
    return [np.array(v, dtype=np.int64).reshape(-1, 2) for v in out]


# ----------------------------------------------------------------------------------------
# cases: name -> (Xq, Xdb, P, k (incl. self: kn = k - 1), epsilon, eps_db, gU)
# ----------------------------------------------------------------------------------------
def _hub():
    """Row 0 of the database at the origin, rows 1-5 and every query within 0.3 of it, the other
    rows 3 N(0, 1): row 0 is in every query's list, a few rows have lists longer than a wave and
    most rows have an empty one."""
    Q, N, d, C = 300, 500, 12, 3
    rng = np.random.default_rng(21)
    Xdb = (3.0 * rng.standard_normal((N, d))).astype(np.float32)
    Xdb[0] = 0.0
    Xdb[1:6] = (0.3 * rng.standard_normal((5, d))).astype(np.float32)
    Xq = (0.3 * rng.standard_normal((Q, d))).astype(np.float32)
    P = rng.random((N, C)).astype(np.float32)
    return Xq, Xdb, P


def _plain(seed, Q, N, d, C):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((Q, d)).astype(np.float32),
            rng.standard_normal((N, d)).astype(np.float32),
            rng.random((N, C)).astype(np.float32))


def _ext(name):
    Xq, Xdb, P, k, epsilon, eps_db = R.ext_case(name)[:6]
    return (Xq, Xdb, P), k, epsilon


GRAD_CASES = {
    "fixed": lambda: _ext("fixed"),
    "auto": lambda: _ext("auto"),
    "auto_wide": lambda: _ext("auto_wide"),            # kn = 79 > 64, C = 70, d % 4 != 0
    "hub_fixed": lambda: (_hub(), 9, 2.0),             # lists longer than a wave, empty lists
    "hub_auto": lambda: (_hub(), 9, "auto"),
    "long_d": lambda: (_plain(22, 9, 80, 520, 5), 6, 40.0),      # three feature chunks
    "kmax": lambda: (_plain(23, 3, 300, 16, 256), 257, "auto"),  # kn = C = 256: the limits
    "tiny": lambda: (_plain(24, 1, 2, 1, 1), 2, 1.0),            # the smallest call
}


@functools.lru_cache(maxsize=None)
def grad_case(name):
    """(Xq, Xdb, P, k, epsilon, eps_db, gU, idx_ref, d2_ref) of a case: gU random float64, the
    float64 kNN of the kn = k - 1 nearest rows; computed once per process, read-only."""
    (Xq, Xdb, P), k, epsilon = GRAD_CASES[name]()
    Xq, Xdb, P = (np.array(a, dtype=np.float32) for a in (Xq, Xdb, P))
    eps_db = R.eps_of(Xdb, k) if epsilon == "auto" else None
    seed = 1000 + sorted(GRAD_CASES).index(name)
    gU = np.random.default_rng(seed).standard_normal((Xq.shape[0], P.shape[1]))
    idx, d2 = R.knn_ref(Xq, Xdb, k - 1)
    for a in (Xq, Xdb, P, gU, idx, d2) + (() if eps_db is None else (eps_db,)):
        a.setflags(write=False)
    return Xq, Xdb, P, k, epsilon, eps_db, gU, idx, d2
