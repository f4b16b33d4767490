"""CPU checks of the CG yardstick (tests/cg_ref.py): the textbook solver against a direct sparse
solve, the Neumann preconditioner's definiteness, the restated kernel choice on every shape of
the GPU contract test, and the measured figures that test's bounds lean on, as assertions.

Matrices here are oracle-built (exact float64 kNN, oracle.gll_oracle.graph_from_knn) on the same
synth features (d = 16, class 7 zeroed) the GPU test uses; the GPU test assembles its matrix from
the workspace instead, which differs by fp32 rounding of the weights.

Measured (float64 / float32 textbook, max over the 10 columns, rtol 1e-2 / 1e-4 / 1e-6):
  500 + 500, k 10, tau 0.07, eps 1     Jacobi 4 / 8 / 11    Neumann 2 / 5 / 7
  500 + 500, eps 'auto'                Jacobi 4 / 7 / 11    Neumann 2 / 4 / 6
  250 + 1250, k 25                     Jacobi 6 / 12 / 17   Neumann 4 / 8 / 11
  300 + 2100, tau 0                    Jacobi 9 / 17 / 24   Neumann 5 / 10 / 14
  60 + 60                              Jacobi 4 / 7 / 10    Neumann 2 / 4 / 6
  300 + 4200, tau 1e-3                 Jacobi 13 / 23 / 33  Neumann 8 / 13 / 19
float32 and float64 counts are identical column by column in all 36 runs, and on every shape of
the contract test with the preconditioner its kernel uses -- so that test's iteration slack stays
at +-1 everywhere.  At rtol 1e-2 and 1e-4 the two true residuals agree to three digits; at 1e-6
the float32 run drifts above rtol (1.67e-6 at m = 4200, tau 1e-3; 2.12e-6 at m = 8200), which is
why the GPU test bounds the 1e-6 residual by the float32 textbook's own, not by rtol alone.
"""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle import gll_oracle as O
from oracle.graphlearning_standin import knn_exact
from tests import cg_ref as R

_cache = {}


def oracle_system(case, g=0):
    """(Luu csr float64, rhs m x C float64) of graph g of a case, without the direct solve."""
    key = (case.base, case.m, case.k, case.C, case.tau, str(case.eps), case.seed + g)
    if key not in _cache:
        X, Y = R.features(case, g)
        ind, dist = knn_exact(X.astype(np.float64), case.k, fast=True)
        gr = O.graph_from_knn(ind, dist, case.eps)
        W = gr.csr(gr.W)
        deg = np.asarray(W.sum(axis=1)).ravel()
        b = case.base
        Luu = (sp.diags(deg[b:] + float(case.tau)) - W[b:, b:]).tocsr()
        _cache[key] = (Luu, np.asarray(W[b:, :b] @ Y.astype(np.float64)))
    return _cache[key]


def _counts(A, B, precond, dtype):
    out = []
    for rtol in R.RTOLS:
        X, it, cv, _ = R.pcg_columns(A, B, rtol=rtol, precond=precond, dtype=dtype)
        assert cv.all()
        out.append((it, R.true_residual(A, X, B)[0], X))
    return out


SIX = {   # name: (case, {precond: (max counts at 1e-2, 1e-4, 1e-6)})
    "ns": (R.Case("ns", 500, 500, "", "", seed=0), {"jacobi": (4, 8, 11), "neumann": (2, 5, 7)}),
    "ns_auto": (R.Case("ns_auto", 500, 500, "", "", eps="auto", seed=0),
                {"jacobi": (4, 7, 11), "neumann": (2, 4, 6)}),
    "fullysup": (R.Case("fullysup", 250, 1250, "", "", k=25, seed=0),
                 {"jacobi": (6, 12, 17), "neumann": (4, 8, 11)}),
    "tau0_m2100": (R.Case("tau0", 300, 2100, "", "", tau=0.0, seed=0),
                   {"jacobi": (9, 17, 24), "neumann": (5, 10, 14)}),
    "m60": (R.Case("m60", 60, 60, "", "", seed=0), {"jacobi": (4, 7, 10), "neumann": (2, 4, 6)}),
    "m4200_tau1e-3": (R.Case("m4200", 300, 4200, "", "", tau=1e-3, seed=0),
                      {"jacobi": (13, 23, 33), "neumann": (8, 13, 19)}),
}


def test_textbook_cg_matches_a_direct_solve():
    """Both preconditioners, float64, rtol 1e-12 against spsolve on an oracle-built Luu: the
    error of a CG iterate is at most cond(A) * rtol relative, cond(Luu) <= (2 max deg + tau) / tau
    < 1e3 here -- 1e-9 is a bar with three digits to spare that still sees any wrong term.  The
    zero column is exactly zero after 0 iterations."""
    A, B = oracle_system(SIX["ns"][0])
    Xe = np.asarray(spla.spsolve(A.tocsc(), B))
    for pre in ("jacobi", "neumann"):
        X, it, cv, _ = R.pcg_columns(A, B, rtol=1e-12, precond=pre)
        err = O.rel_err(X, Xe)
        print(f"{pre}: rel err vs spsolve {err:.2e}, iterations {it.tolist()}")
        assert cv.all() and err < 1e-9
        assert it[R.ZERO_COL] == 0 and not X[:, R.ZERO_COL].any()
        assert (np.delete(it, R.ZERO_COL) > 0).all()
    # the absolute rule of the CSR solver: the same solve stated with atol = rtol ||b||
    c = 0
    bn = np.linalg.norm(B[:, c])
    ra = R.pcg(A, B[:, c], atol=1e-6 * bn)
    rr = R.pcg(A, B[:, c], rtol=1e-6)
    assert ra.iters == rr.iters and ra.converged and np.array_equal(ra.x, rr.x)
    assert R.pcg(A, B[:, c], atol=2 * bn).iters == 0     # already inside the tolerance


def test_history_and_max_iter():
    """The iterate after every x update is returned on request; max_iter caps the count, leaves
    `converged` false and returns that iterate; converging on the last permitted iteration counts
    as converged."""
    A, B = oracle_system(SIX["ns"][0])
    full = R.pcg(A, B[:, 0], rtol=1e-6, history=True)
    assert full.converged and len(full.history) == full.iters >= 4
    assert np.array_equal(full.history[-1], full.x)
    cap = R.pcg(A, B[:, 0], rtol=1e-6, max_iter=2)
    assert cap.iters == 2 and not cap.converged and np.array_equal(cap.x, full.history[1])
    last = R.pcg(A, B[:, 0], rtol=1e-6, max_iter=full.iters)
    assert last.converged and last.iters == full.iters


def test_neumann_operator_is_symmetric_positive_definite():
    """M^-1 = D^-1 + D^-1 N D^-1 on an oracle-built Luu (m = 60: dense eigenvalues)."""
    A, _ = oracle_system(SIX["m60"][0])
    _, D, N = R.split(A)
    Minv = np.diag(1 / D) + np.diag(1 / D) @ N.toarray() @ np.diag(1 / D)
    assert np.abs(Minv - Minv.T).max() <= 1e-15 * np.abs(Minv).max()
    ev = np.linalg.eigvalsh((Minv + Minv.T) / 2)
    print(f"Neumann M^-1 eigenvalues in [{ev.min():.3e}, {ev.max():.3e}]")
    assert ev.min() > 0
    # and it is what pcg applies: one Neumann step from x = 0 is alpha M^-1 b
    b = np.arange(1.0, 61.0)
    z = Minv @ b
    x1 = R.pcg(A, b, rtol=1e-30, precond="neumann", max_iter=1).x
    assert np.allclose(x1, (b @ z) / (z @ (A.toarray() @ z)) * z, rtol=1e-12, atol=0)


@pytest.mark.parametrize("name", list(SIX))
def test_measured_counts_and_residuals_are_pinned(name):
    """The module docstring's figures: counts per preconditioner and rtol, float32 == float64
    column by column, the residuals' agreement at the looser bars and the float32 drift at 1e-6."""
    case, want = SIX[name]
    A, B = oracle_system(case)
    for pre in ("jacobi", "neumann"):
        c64, c32 = _counts(A, B, pre, np.float64), _counts(A, B, pre, np.float32)
        got = tuple(int(it.max()) for it, _, _ in c64)
        print(name, pre, got, [f"{r.max():.3e}/{s.max():.3e}" for (_, r, _), (_, s, _) in zip(c64, c32)])
        assert got == want[pre]
        for (i64, r64, _), (i32, r32, _), rtol in zip(c64, c32, R.RTOLS):
            assert np.array_equal(i64, i32)
            assert r64.max() <= rtol                      # float64: no drift worth the name
            if rtol > 1e-6:
                assert abs(r32.max() - r64.max()) <= 2e-3 * r64.max()   # three digits
                assert np.abs(r32 - r64).max() <= 1e-3 * rtol         # drift: 1e-7 of ||b||
                assert r32.max() <= 1.05 * rtol
            else:
                assert r32.max() <= 2.5e-6                # visible drift, bounded
    if name == "m4200_tau1e-3":
        r32 = _counts(A, B, "jacobi", np.float32)[2][1].max()
        assert 1.2e-6 < r32 < 2.0e-6, r32                 # above rtol: the 1e-6 bound cannot be rtol


def test_route_restatement_names_the_intended_kernel_for_every_case():
    for c in R.FORWARD_CASES + (R.RESCUE_CASE,):
        assert R.route(c.n, c.base, c.C, c.k, c.flags, c.B, c.knob_rv) == (c.kernel, c.precond), c.name
    # the issue's 250 + 2048 at k = 25: 17 virtual rows per thread, the balanced kernel is not used
    assert R.vr_threads(2298, 2048, 25, R.FLAG_CG_VR) == 0
    assert R.route(2298, 250, 10, 25, R.FLAG_CG_VR)[0] == "cg_ell<1024,2,16>"
    # every forward kernel of the table is reached by at least one case
    kernels = {c.kernel.split("<")[0] for c in R.FORWARD_CASES}
    assert kernels == {"cg_ell", "cg_vr", "cg_lds", "cg_gv"}
    assert R.csr_route(300, 17) == "cg_csr<lds>" and R.csr_route(2049, 4) == "cg_gv_csr"
    assert R.csr_route(2049, 17) == "cg_csr<lds>" and R.csr_route(8200, 17) == "cg_csr<workspace>"


@pytest.mark.parametrize("name", list(R.CASES))
def test_float32_and_float64_counts_agree_on_every_contract_shape(name):
    """The GPU test allows +-1 iteration against the float64 textbook.  That slack is for the
    summation order at the threshold only if float32 itself does not move the count: checked here
    for every shape (every graph of the batch) with the preconditioner its kernel uses.  Also what
    the max_iter = 2 test needs: every non-zero column takes at least 4 iterations at 1e-6, and
    the counts grow strictly with the tolerance."""
    case = R.CASES[name]
    for g in range(case.B):
        A, B = oracle_system(case, g)
        c64, c32 = _counts(A, B, case.precond, np.float64), _counts(A, B, case.precond, np.float32)
        for (i64, _, _), (i32, _, _) in zip(c64, c32):
            assert np.array_equal(i64, i32), (name, g, i64, i32)
        mx = [int(it.max()) for it, _, _ in c64]
        assert mx[0] < mx[1] < mx[2], mx
        nz = np.delete(c64[2][0], R.ZERO_COL)
        assert nz.min() >= 4 and c64[2][0][R.ZERO_COL] == 0
    print(name, case.precond, "counts", mx)


@pytest.mark.parametrize("m,C,kernel", R.CSR_ROUTES)
def test_csr_cases_float32_and_float64_counts_agree(m, C, kernel):
    """The matrices of the direct gll_cg_csr test (diagonal stored last in its row): Jacobi
    textbook counts under the absolute rule agree between float32 and float64, grow with the
    tolerance, and every live column needs at least 4 iterations at 1e-6 ||b||_max."""
    assert R.csr_route(m, C) == kernel
    rp, col, val, A, b = R.csr_case(m, C)
    assert (A != A.T).nnz == 0 and (col[rp[1:] - 1] == np.arange(m)).all()
    bmax = np.linalg.norm(b.astype(np.float64), axis=0).max()
    mx = []
    for rel in (1e-3, 1e-6):
        _, i64, c64, _ = R.pcg_columns(A, b, atol=rel * bmax)
        _, i32, c32, _ = R.pcg_columns(A, b, atol=rel * bmax, dtype=np.float32)
        assert c64.all() and c32.all() and np.array_equal(i64, i32), (i64, i32)
        mx.append(int(i64.max()))
    live = np.delete(i64, R.CSR_ZERO_COL) if C > 1 else i64
    assert mx[0] < mx[1] and live.min() >= 4 and (C == 1 or i64[R.CSR_ZERO_COL] == 0)
    print(f"csr m {m} C {C}: Jacobi counts {mx}")
