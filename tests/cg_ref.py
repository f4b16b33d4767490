"""Textbook preconditioned conjugate gradients in numpy -- a test helper, not a test.

The yardstick of the CG solvers' stopping contract (tests/test_gpu_cg_contract.py; pinned on the
CPU by tests/test_cg_ref_cpu.py).  One right-hand-side column per call, in float64 or float32:

    x = 0, r = b, z = M^-1 r, p = z
    repeat:  alpha = (r, z) / (p, A p);  x += alpha p;  r -= alpha A p        <- one iteration
             stop when the rule holds (tested here, after the x and r update)
             z = M^-1 r;  beta = (r, z)_new / (r, z)_old;  p = z + beta p

with the project's stop rules (include/gll.h): ||r||^2 <= rtol^2 ||b||^2 for the layer's Luu
solves (gll_problem.rtol), ||r|| <= atol for gll_cg_csr.  The count is the kernels': one per x
update.  A zero right-hand side (or, under atol, one already inside the tolerance) gives
0 iterations, converged, x = 0.  A breakdown ((p, A p) <= 0 or NaN) stops unconverged, as every
kernel does.

Preconditioners (A = D - N, D the diagonal):
    'jacobi'   M^-1 r = D^-1 r
    'neumann'  y = D^-1 r,  M^-1 r = y + D^-1 (N y)     (the MODE 3 body of cg_ell_kernel)

`luu_from_view` assembles Luu and the right-hand-side operator W_ul from the arrays a workspace
holds (gll_workspace_view), so the matrix under test is the GPU's own fp32 graph.  `route` restates
the host-side kernel choice of cg_route.h cg_route / grid_cg_route, gll_internal.h vr_threads and
api.hip backward_impl / gll_cg_csr, so a test can say which kernel a problem runs.  It stays an
independent restatement: `lib_route` asks the library itself (gll_cg_route), and the tests hold
the two against each other.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import scipy.sparse as sp


@dataclass
class CgResult:
    x: np.ndarray
    iters: int
    converged: bool
    history: list = field(default_factory=list)   # x after every iteration (on request)


def split(A, dtype=np.float64):
    """(A, D, N) of a scipy sparse matrix in `dtype`: A = diag(D) - N."""
    A = sp.csr_matrix(A, dtype=dtype)
    D = A.diagonal().astype(dtype)
    N = (sp.diags(D).astype(dtype) - A).tocsr().astype(dtype)
    return A, D, N


def pcg(A, b, *, rtol=None, atol=None, max_iter=1000, precond="jacobi", dtype=np.float64,
        history=False, parts=None) -> CgResult:
    """Textbook PCG on one column `b`; exactly one of rtol / atol.  `parts`: split(A, dtype) of
    an earlier call on the same matrix."""
    assert (rtol is None) != (atol is None), "one stop rule: rtol (layer) or atol (CSR solver)"
    assert precond in ("jacobi", "neumann")
    dt = np.dtype(dtype).type
    A, D, N = parts if parts is not None else split(A, dtype)
    assert A.dtype == np.dtype(dtype)
    b = np.asarray(b, dtype=dtype).ravel()
    Dinv = np.where(D > 0, dt(1) / np.where(D > 0, D, dt(1)), dt(0)).astype(dtype)

    def minv(r):
        y = Dinv * r
        return y if precond == "jacobi" else y + Dinv * (N @ y)

    x = np.zeros_like(b)
    r = b.copy()
    bb = dt(r @ r)
    tol2 = dt(rtol) * dt(rtol) * bb if rtol is not None else dt(atol) * dt(atol)
    res = CgResult(x, 0, bool(bb <= tol2) if atol is not None else not bb > 0)
    if res.converged:
        return res
    z = minv(r)
    p = z.copy()
    rz = dt(r @ z)
    while res.iters < max_iter:
        res.iters += 1
        Ap = A @ p
        pAp = dt(p @ Ap)
        if not pAp > 0:
            break
        alpha = dt(rz / pAp)
        x = x + alpha * p
        r = r - alpha * Ap
        if history:
            res.history.append(x.copy())
        if dt(r @ r) <= tol2:
            res.converged = True
            break
        z = minv(r)
        rzn = dt(r @ z)
        p = z + dt(rzn / rz) * p
        rz = rzn
    res.x = x
    return res


def pcg_columns(A, B, **kw):
    """pcg on every column of B (m x C): (X m x C, iters[C], converged[C], results)."""
    dtype = kw.get("dtype", np.float64)
    parts = split(A, dtype)
    B = np.asarray(B)
    out = [pcg(None, B[:, c], parts=parts, **kw) for c in range(B.shape[1])]
    X = np.stack([o.x for o in out], axis=1) if out else np.zeros_like(B)
    return (X, np.array([o.iters for o in out]), np.array([o.converged for o in out]), out)


def true_residual(A, X, B):
    """rho_c = ||b_c - A x_c|| / ||b_c|| per column in float64 (0 for a zero column whose x is
    zero), and the absolute norms ||b_c - A x_c||."""
    A = sp.csr_matrix(A, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64)
    B = np.asarray(B, dtype=np.float64)
    rn = np.linalg.norm(B - A @ X, axis=0)
    bn = np.linalg.norm(B, axis=0)
    return np.where(bn > 0, rn / np.where(bn > 0, bn, 1.0), rn), rn


def luu_from_view(row_start, row_len, col, w, deg, tau, base):
    """(Luu, W_ul) in float64 scipy CSR from a workspace's graph arrays (gll_workspace_view:
    padded rows of the symmetric kNN graph, no diagonal): Luu = diag(deg_u + tau) - W_uu over the
    unlabeled rows u >= base, W_ul their weights to the labeled columns; the forward's right-hand
    side is W_ul @ Y."""
    row_start = np.asarray(row_start, dtype=np.int64)
    row_len = np.asarray(row_len, dtype=np.int64)
    n = row_start.shape[0]
    m = n - base
    rs, rl = row_start[base:], row_len[base:]
    rows = np.repeat(np.arange(m, dtype=np.int64), rl)
    first = np.cumsum(rl) - rl
    idx = np.repeat(rs - first, rl) + np.arange(int(rl.sum()), dtype=np.int64)
    cols = np.asarray(col)[idx].astype(np.int64)
    vals = np.asarray(w)[idx].astype(np.float64)
    assert cols.min(initial=0) >= 0 and cols.max(initial=0) < n
    uu = cols >= base
    Wuu = sp.csr_matrix((vals[uu], (rows[uu], cols[uu] - base)), shape=(m, m))
    Wul = sp.csr_matrix((vals[~uu], (rows[~uu], cols[~uu])), shape=(m, base))
    diag = np.asarray(deg, dtype=np.float64)[base:] + float(tau)
    return (sp.diags(diag) - Wuu).tocsr(), Wul


# ------------------------------------------------------------------------------------------
# Which kernel solves a problem: the host-side choice of the library, restated.
# ------------------------------------------------------------------------------------------
FLAG_CG_GRID, FLAG_CG_PERCOL, FLAG_CG_ELL, FLAG_CG_VR, FLAG_BWD_UNFUSED = 1, 8, 512, 1024, 16384
LDS_DYN = 159 * 1024   # cg_route.h kLdsDyn: the dynamic share of the 160 KiB
D_FEAT_DEFAULT = 16    # the route does not depend on d


def vr_threads(n, m, K, flags, knob_rv=0):
    """gll_internal.h vr_threads: virtual rows per thread of the balanced kernel, 0 = not used."""
    if m <= 0 or m > 4 * 512 or (flags & FLAG_CG_ELL):
        return 0
    ln = 1.4 * (K - 1) * float(m) / float(n)
    if ln <= 12.0 and not (flags & FLAG_CG_VR):
        return 0
    rv = int((m * (ln / 8 + 0.5) + 512 - 1) / 512)
    if knob_rv > 0:
        rv = knob_rv
    return 4 if rv <= 4 else (8 if rv <= 8 else (10 if rv <= 10 else 0))


def route(n, base, C, K, flags=0, B=1, knob_rv=0):
    """(kernel, preconditioner) of a Luu solve (cg_route.h cg_route; the adjoint of a single
    graph with fixed eps takes the same choice inside cg_grad_fused_kernel unless
    GLL_FLAG_BWD_UNFUSED or the shape sends it to the two-launch path).  The whole-GPU kernel is
    named when grid_cg_route holds; a system past its capacity falls through at run time."""
    m = n - base
    K = min(K, n)
    if B == 1 and C <= 16 and not (flags & FLAG_CG_PERCOL) and (m > 2048 or (flags & FLAG_CG_GRID)):
        return "cg_gv", "jacobi"
    rv = vr_threads(n, m, K, flags, knob_rv)
    if rv > 0:
        return f"cg_vr<512,{(m + 511) // 512},{rv}>", "jacobi"
    if m <= 64:
        return "cg_ell<64,1,24>", "neumann"
    if m <= 128:
        return "cg_ell<128,1,24>", "neumann"
    if m <= 256:
        return "cg_ell<256,1,24>", "neumann"
    if m <= 512 and (B == 1 or B * C <= 256):
        return "cg_ell<512,1,24>", "neumann"
    if m <= 512:
        return "cg_ell<256,2,24>", "jacobi"
    if m <= 1024:
        return "cg_ell<1024,1,16>", "neumann"
    if m <= 2048:
        return "cg_ell<1024,2,16>", "jacobi"
    if m <= 4096:
        return "cg_ell<1024,4,4>", "jacobi"
    return ("cg_lds<lds>" if 64 * 4 + 5 * m * 4 <= LDS_DYN else "cg_lds<global>"), "jacobi"


def lib_route(n, base, C, K, flags=0, B=1, knob_rv=0, d=D_FEAT_DEFAULT):
    """The library's own choice for the same problem, in route()'s words: gll_cg_route (no GPU)
    decoded to (kernel, preconditioner), plus its raw words.  Sets and restores GLL_KNOB_VR_RV."""
    import ctypes as ct

    from graphlearninglayer_amd import GLL as G
    from graphlearninglayer_amd import _lib
    p = G.make_problem(n, d, base, C, K, 0.07, 1.0, flags=flags)
    out = (ct.c_int32 * 9)()
    _lib.set_knob(_lib.KNOB_VR_RV, knob_rv)
    try:
        rc = _lib.lib().gll_cg_route(ct.byref(p), B, out)
    finally:
        _lib.set_knob(_lib.KNOB_VR_RV, 0)
    grid_first, family, NT, R, S, MODE, vec_in_lds, row, rows = list(out)
    if grid_first:
        name = "cg_gv", "jacobi"
    elif family == 0:
        name = f"cg_ell<{NT},{R},{S}>", "neumann" if MODE == 3 else "jacobi"
    elif family == 1:
        name = f"cg_vr<{NT},{R},{S}>", "jacobi"
    else:
        name = ("cg_lds<lds>" if vec_in_lds else "cg_lds<global>"), "jacobi"
    return rc, name, list(out)


def csr_route(m, C):
    """Kernel of gll_cg_csr (api.hip; always Jacobi)."""
    if m > 2048 and C <= 16:
        return "cg_gv_csr"
    return "cg_csr<lds>" if 64 * 4 + 5 * m * 4 <= LDS_DYN else "cg_csr<workspace>"


# ------------------------------------------------------------------------------------------
# The shapes of the contract tests: the smallest that reach each kernel.  Shared by the CPU test
# (which pins the route restated above and the float32 / float64 agreement of the textbook counts
# on every shape) and the GPU test.
# ------------------------------------------------------------------------------------------
D_FEAT = 16        # synth features
ZERO_COL = 7       # labelled class zeroed: every run has a zero right-hand-side column
RTOLS = (1e-2, 1e-4, 1e-6)


@dataclass(frozen=True)
class Case:
    name: str
    base: int
    m: int
    kernel: str          # what route() must say
    precond: str
    k: int = 10
    C: int = 10
    tau: float = 0.07
    eps: object = 1.0
    flags: int = 0
    B: int = 1
    knob_rv: int = 0
    seed: int = 0

    @property
    def n(self):
        return self.base + self.m


def _ell1(m):
    nt = 64 if m <= 64 else 128 if m <= 128 else 256 if m <= 256 else 512 if m <= 512 else 1024
    return Case(f"ell_neumann_m{m}", m, m, f"cg_ell<{nt},1,{24 if m <= 512 else 16}>", "neumann",
                seed=m)


FORWARD_CASES = (
    # cg_ell, Neumann form, one row per thread: the thread-tail boundaries of each NT
    *[_ell1(m) for m in (60, 64, 65, 129, 257, 500, 513, 1024)],
    # cg_ell, Jacobi form: 256 x 2 (batched, B C > 256), 1024 x 2, 1024 x 4
    Case("ell_jacobi_256x2_B27", 300, 300, "cg_ell<256,2,24>", "jacobi", B=27, seed=100),
    Case("ell_jacobi_1024x2_m1025", 1025, 1025, "cg_ell<1024,2,16>", "jacobi", seed=1),
    Case("ell_jacobi_1024x2_m2048", 2048, 2048, "cg_ell<1024,2,16>", "jacobi", seed=2),
    Case("ell_jacobi_1024x4_m2100", 300, 2100, "cg_ell<1024,4,4>", "jacobi",
         flags=FLAG_CG_PERCOL, seed=3),
    # cg_vr, R = 1..4 rows per thread at RV = 4, 8, 10, 10 (k = 25).  R = 4 needs base 2400: at
    # 250 + 2048 vr_threads wants 17 virtual rows per thread and returns 0 (the register-ELL
    # kernel runs whatever GLL_FLAG_CG_VR says).
    Case("vr_R1_RV4", 250, 500, "cg_vr<512,1,4>", "jacobi", k=25, flags=FLAG_CG_VR, seed=4),
    Case("vr_R2_RV8", 250, 700, "cg_vr<512,2,8>", "jacobi", k=25, flags=FLAG_CG_VR, seed=5),
    Case("vr_R3_RV10", 250, 1250, "cg_vr<512,3,10>", "jacobi", k=25, flags=FLAG_CG_VR, seed=6),
    Case("vr_R4_RV10", 2400, 2048, "cg_vr<512,4,10>", "jacobi", k=25, flags=FLAG_CG_VR, seed=7),
    Case("vr_R3_RV4_spill", 250, 1250, "cg_vr<512,3,4>", "jacobi", k=25, flags=FLAG_CG_VR,
         knob_rv=4, seed=6),
    # cg_lds: vectors in LDS, and in global memory (5 m floats past the 159 KiB dynamic share)
    Case("lds_vectors_in_lds", 300, 4200, "cg_lds<lds>", "jacobi", flags=FLAG_CG_PERCOL, seed=8),
    Case("lds_vectors_in_global", 300, 8200, "cg_lds<global>", "jacobi", flags=FLAG_CG_PERCOL,
         seed=9),
    # whole-GPU cg_gv: automatic past m = 2048, forced below; C = 16 stays, C = 17 leaves
    Case("gv_auto_m2100", 300, 2100, "cg_gv", "jacobi", seed=3),
    Case("gv_forced_m500", 500, 500, "cg_gv", "jacobi", flags=FLAG_CG_GRID, seed=500),
    Case("gv_forced_C16", 500, 500, "cg_gv", "jacobi", C=16, flags=FLAG_CG_GRID, seed=10),
    Case("gv_left_at_C17", 500, 500, "cg_ell<512,1,24>", "neumann", C=17, flags=FLAG_CG_GRID,
         seed=11),
    # eps = 'auto' and tau = 0 on cg_ell and on cg_gv
    Case("ell_auto_eps", 500, 500, "cg_ell<512,1,24>", "neumann", eps="auto", seed=500),
    Case("ell_tau0", 500, 500, "cg_ell<512,1,24>", "neumann", tau=0.0, seed=500),
    Case("gv_auto_eps", 300, 2100, "cg_gv", "jacobi", eps="auto", seed=3),
    Case("gv_tau0", 300, 2100, "cg_gv", "jacobi", tau=0.0, seed=3),
)
CASES = {c.name: c for c in FORWARD_CASES}
# rescue_solve (classic Jacobi PCG by one workgroup): the forced whole-GPU solve with the injected
# barrier failure, GLL_FLAG_CG_GRID | GLL_FLAG_DIAG_GRID_FAIL
FLAG_DIAG_GRID_FAIL = 256
RESCUE_CASE = Case("gv_rescue_m500", 500, 500, "cg_gv", "jacobi",
                   flags=FLAG_CG_GRID | FLAG_DIAG_GRID_FAIL, seed=500)


def features(case: Case, g: int = 0):
    """(X n x 16 float32, Y base x C float32 one-hot with class ZERO_COL zeroed) of graph g."""
    from graphlearninglayer_amd.synth import one_hot, synth
    X, lab = synth(case.base, case.m, D_FEAT, C=case.C, seed=case.seed + g)
    Y = one_hot(lab[: case.base], case.C)
    Y[:, ZERO_COL] = 0.0
    return X, Y


# ------------------------------------------------------------------------------------------
# gll_cg_csr, called directly
# ------------------------------------------------------------------------------------------
CSR_ROUTES = ((300, 1, "cg_csr<lds>"), (300, 3, "cg_csr<lds>"), (300, 17, "cg_csr<lds>"),
              (2049, 4, "cg_gv_csr"), (2049, 17, "cg_csr<lds>"), (8200, 17, "cg_csr<workspace>"))
CSR_ZERO_COL = 1


def csr_case(m, C):
    """(row_ptr, col, val fp32, A float64 scipy CSR, b m x C fp32): a random symmetric, strictly
    diagonally dominant matrix (as test_cg_csr_large_matches_scipy builds one) stored with the
    diagonal entry LAST in every row, the other columns ascending; b standard normal with column
    CSR_ZERO_COL zeroed (C = 1 keeps its only column: nothing would be left to solve)."""
    rng = np.random.default_rng(1000 * C + m)
    T = sp.triu(sp.random(m, m, density=6.0 / m, random_state=rng, format="csr"), k=1)
    A = (T + T.T).tocsr()
    A.sort_indices()
    dg = np.asarray(abs(A).sum(1)).ravel() + 0.5
    cnt = np.diff(A.indptr)
    rp = np.concatenate([[0], np.cumsum(cnt + 1)]).astype(np.int32)
    col = np.empty(rp[-1], dtype=np.int32)
    val = np.empty(rp[-1], dtype=np.float32)
    last = rp[1:] - 1
    body = np.ones(rp[-1], dtype=bool)
    body[last] = False
    col[body], val[body] = A.indices, A.data.astype(np.float32)
    col[last], val[last] = np.arange(m, dtype=np.int32), dg.astype(np.float32)
    assert (col[rp[:-1]] != np.arange(m)).mean() > 0.99       # the diagonal is not first
    A64 = sp.csr_matrix((val.astype(np.float64), col.copy(), rp.copy()), shape=(m, m))
    A64.sort_indices()
    b = rng.standard_normal((m, C)).astype(np.float32)
    if C > 1:
        b[:, CSR_ZERO_COL] = 0.0
    return rp, col, val, A64, b
