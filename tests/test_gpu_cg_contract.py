"""The CG solvers' stopping contract on the MI355X (-m gpu): true residual, iteration count,
rtol and max_iter, for every CG kernel, against the textbook solver of tests/cg_ref.py.

Everything goes through the C ABI (gll_problem.rtol / max_iter / flags are not reachable from
`apply`).  Features: synth at d = 16, C = 10, tau 0.07, eps 1 unless the case says otherwise, one
labelled class zeroed so every run has a zero right-hand-side column.  The matrix the reference
solves is assembled from the workspace's own arrays (cg_ref.luu_from_view): the GPU's fp32 graph.

Per route (tests/cg_ref.py FORWARD_CASES: the smallest shapes that reach each kernel, the kernel
named by cg_ref.route, the restated host-side choice, plus one bracketed CG launch per solve and
-- the observable part -- the iteration count of that kernel's preconditioner), at rtol 1e-2,
1e-4 and 1e-6, every column:
  1. true residual rho_c = ||b_c - Luu x_c|| / ||b_c|| in float64: <= 1.05 rtol at 1e-2 and 1e-4
     (fp32 drift is ~1e-7 of ||b||); at 1e-6 <= 2 max(rtol, rho_c of the float32 textbook run on
     the same matrix, preconditioner and column) -- drift is visible there, the factor 2 covers
     the summation order and diag = deg + tau rounded to fp32;
  2. GLL_ST_*_ITERS (the maximum over columns) within +-1 of the float64 textbook's maximum with
     the same preconditioner (float32 and float64 textbook counts agree on every shape:
     tests/test_cg_ref_cpu.py) -- a wrong recurrence converges, but later;
  3. iterations(1e-2) < iterations(1e-4) < iterations(1e-6), no non-converged column, no failed
     solve;
  4. the zero column is exactly 0.0 and out64 == double(U32) bitwise.
The cap: max_iter = 2 stops every non-zero column after two x updates (count, non-converged
columns, the textbook's second iterate within 1e-5 -- the project's bar between two CG kernels --
nothing NaN, a finite backward after it); max_iter = textbook maximum + 1 converges everywhere.
The adjoint solves (fused, two-launch, auto-eps, batched; gbar fp32 and fp64) and gll_cg_csr
(called directly, not through refined_solve's float64 refinement) are held to the same rules.

cg_grid_classic_kernel has no row: dispatch_grid reaches it only when cg_gv declines (more than
512 rows per workgroup: m > 131,072 on 256 CUs, sixteen times the largest graph a test here may
build; with GLL_KNOB_GRID_CAP both kernels decline together) or with GLL_FLAG_DIAG_GRID_OVERSUB,
the diagnostic that sizes it at one row per workgroup so that the launch is refused.  It is
still reachable from the ABI, so it is left in place.

Measured on the MI355X (profiles/cg01_gpu_tests.txt holds every figure of the run):
  route (kernel, preconditioner)            iterations at 1e-2 / 1e-4 / 1e-6   worst rho / bound
  cg_ell Neumann, m 60 / 64 / 65 / 129      2 4 6 / 2 4 6 / 3 4 6 / 2 4 6      0.54 / 0.82 / 0.83 / 0.73
  cg_ell Neumann, m 257 / 500 / 513 / 1024  3 4 7 / 3 5 6 / 3 4 6 / 3 4 6      0.92 / 0.91 / 0.72 / 0.91
  cg_ell Jacobi 256 x 2, B = 27 (max)       5 8 12                             0.94
  cg_ell Jacobi 1024 x 2, m 1025 / 2048     4 8 11 / 4 8 11                    0.90 / 0.90
  cg_ell Jacobi 1024 x 4, m 2100            8 15 22                            0.94
  cg_vr R 1 / 2 / 3 / 4 (RV 4 / 8 / 10 / 10)  5 9 13 / 5 10 15 / 6 12 18 / 4 7 10  0.85 / 0.88 / 0.87 / 0.95
  cg_vr R 3, RV forced to 4 (spill)         6 12 18                            0.87
  cg_lds, vectors in LDS / in global        10 19 27 / 13 24 35                0.87 / 0.95
  cg_gv automatic m 2100 / forced m 500     8 15 22 / 4 8 11                   0.94 / 0.92
  cg_gv C = 16 / left at C = 17 (cg_ell)    4 8 12 / 3 4 6                     0.95 / 0.95
  cg_ell auto eps / tau 0                   3 4 6 / 3 5 7                      0.91 / 0.76
  cg_gv auto eps / tau 0                    6 11 17 / 9 17 24                  0.93 / 0.90
  rescue_solve (m 500)                      4 8 11                             0.92
  adjoint fused = two launches (both gbar dtypes) / auto eps / batched
                                            2 5 6 / 2 4 6 / 4 8 12             0.93 / 0.84 / 0.95
  gll_cg_csr, six (m, C): 8 / 16 iterations at 1e-3 / 1e-6 ||b||_max, worst ||r|| / bound 0.88
All 120 iteration counts compared equal the float64 textbook's exactly (the +-1 was not used);
the second iterate under max_iter = 2 is within 4.4e-7 of the textbook's everywhere.  The batch
without a sink reports 10-12 iterations per graph in its own blocks; with a sink the word holds
graph 0's 11.  The whole file runs in 4 s.

What it found: the whole-GPU kernel's pipelined (Ghysels-Vanroose) form, which the Luu solves
ran until this test, returned rho = 4.0-5.8e-6 at m = 2100 and 5.3-9.2e-6 at tau = 0 under
rtol 1e-6 (2.9 and 4.5 times the bound; float32 textbook 1.24e-6 and 1.21e-6), at the right
iteration counts: the recursive residual it stops on had drifted from the true one.  The Luu
solves now run the kernel's Chronopoulos-Gear form, as gll_cg_csr did already (rho 1.25e-6 and
1.15e-6 on the same two cases).
"""
import numpy as np
import pytest
import torch

from graphlearninglayer_amd import GLL
from graphlearninglayer_amd import _lib as L
from oracle import gll_oracle as O
from tests import abi as A
from tests import cg_ref as R

pytestmark = pytest.mark.gpu
ITERATE_TOL = 1e-5     # between two CG kernels (tests/test_gpu_cg.py)
GBAR_ZERO_COL = 3


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    A.need_gpu()


class Session:
    """One case on the device (tests/abi.py Run): its B graphs and workspace blocks, optional
    sink; every call under the case's GLL_KNOB_VR_RV (the workspace layout reads it) with the CG
    and fused-backward launches bracketed."""

    def __init__(self, case, sink=False):
        self.case, self.B = case, case.B
        xy = [R.features(case, g) for g in range(case.B)]
        Xh = np.stack([x for x, _ in xy])
        self.Yh = np.stack([y for _, y in xy])
        one = case.B == 1
        with self._knobbed():
            self.run = A.Run(Xh[0] if one else Xh, self.Yh[0] if one else self.Yh, case.k, case.tau,
                             case.eps, case.flags, rtol=1e-6, max_iter=1000, sink=sink)
        self.sink = self.run.sink

    def _knobbed(self):
        return A.knobs({L.KNOB_VR_RV: self.case.knob_rv})

    def _status(self):
        return [self.run.status(g) for g in range(self.B)]

    def _solutions(self, field):
        """The m x C fp32 array `field` of every graph's view."""
        c = self.case
        with self._knobbed():
            return np.stack([self.run.array(getattr(self.run.view(g), field), c.m * c.C, np.float32,
                                            g).reshape(c.m, c.C) for g in range(self.B)])

    def forward(self, rtol=1e-6, max_iter=1000):
        """(U B x m x C float64, U32, status words per graph or of the sink, CG launches)."""
        c = self.case
        with self._knobbed(), A.launches(L.K_CG, L.K_BWD) as ran:
            U = self.run.forward(rtol=rtol, max_iter=max_iter)
        return U.reshape(self.B, c.m, c.C), self._solutions("U32"), self._status(), ran[0]

    def backward(self, gbar, g_dtype, rtol=1e-6, max_iter=1000):
        """(grad_X, wadj B x m x C fp32, status per graph, (CG launches, fused launches))."""
        c = self.case
        with self._knobbed(), A.launches(L.K_CG, L.K_BWD) as ran:
            gx = self.run.backward(gbar, g_dtype, rtol=rtol, max_iter=max_iter)
        return gx.reshape(self.B, c.n, R.D_FEAT), self._solutions("wadj"), self._status(), tuple(ran)

    def systems(self):
        """[(Luu, W_ul @ Y)] per graph from the workspace arrays a forward left."""
        c, run = self.case, self.run
        out = []
        for g in range(self.B):
            with self._knobbed():
                v = run.view(g)
            rs = run.array(v.row_start, c.n, np.int32, g)
            rl = run.array(v.row_len, c.n, np.int32, g)
            E = int((rs.astype(np.int64) + rl).max())
            col = run.array(v.col, E, np.int32, g)
            w = run.array(v.w, E, np.float32, g)
            deg = run.array(v.deg, c.n, np.float32, g)
            Luu, Wul = R.luu_from_view(rs, rl, col, w, deg, c.tau, c.base)
            out.append((Luu, np.asarray(Wul @ self.Yh[g].astype(np.float64))))
        return out


class Ref:
    """Textbook runs on one system: float64 at the three rtols, float32 at 1e-6, and the float64
    iterate after two x updates."""

    def __init__(self, A, B, precond):
        self.A, self.B = A, np.asarray(B, dtype=np.float64)
        self.it = {}
        for rtol in R.RTOLS:
            _, it, cv, _ = R.pcg_columns(A, self.B, rtol=rtol, precond=precond)
            assert cv.all()
            self.it[rtol] = it
        X32, it32, cv32, _ = R.pcg_columns(A, self.B, rtol=1e-6, precond=precond, dtype=np.float32)
        assert cv32.all()
        self.it32 = it32
        self.rho32 = R.true_residual(A, X32, self.B)[0]
        self.x2 = R.pcg_columns(A, self.B, rtol=1e-6, precond=precond, max_iter=2)[0]
        self.nonzero = int((np.linalg.norm(self.B, axis=0) > 0).sum())


_refs, _adj_refs = {}, {}
def _note(line):
    """One line per route and check (pytest -s): the profiles/ record of a run."""
    print(line)


def _forward_refs(case, ses):
    """Textbook references of a case's forward systems (the graph build is bitwise
    deterministic, so they are computed once per case from the first session's workspace)."""
    if case.name not in _refs:
        _refs[case.name] = [Ref(A, b, case.precond) for A, b in ses.systems()]
    return _refs[case.name]


def _check_solution(tag, refs, X64, X32, rtol, zero_col):
    """Assertions 1 and 4 on the solutions of every graph; returns the worst ratio to the bound."""
    worst = 0.0
    for g, ref in enumerate(refs):
        rho, _ = R.true_residual(ref.A, X32[g], ref.B)
        bound = np.full_like(rho, 1.05 * rtol) if rtol > 1e-6 else 2.0 * np.maximum(rtol, ref.rho32)
        ratio = float((rho / bound).max())
        worst = max(worst, ratio)
        if ratio > 1.0 or g == 0:
            _note(f"{tag} rtol {rtol:g} graph {g}: rho max {rho.max():.3e} (float32 textbook "
                  f"{ref.rho32.max():.3e}), worst rho/bound {ratio:.3f}")
        assert np.isfinite(X32[g]).all()
        assert (rho <= bound).all(), (tag, rtol, g, rho, bound)
        assert not X32[g][:, zero_col].any()                       # exactly 0.0
        if X64 is not None:
            assert np.array_equal(X64[g], X32[g].astype(np.float64))   # out64 == double(U32)
    return worst


def _check_iters(tag, got, ref_it, rtol):
    want = int(np.max(ref_it))
    _note(f"{tag} rtol {rtol:g}: iterations {got} (float64 textbook max {want})")
    assert abs(got - want) <= 1, (tag, rtol, got, want)


# ------------------------------------------------------------------------------------------
# Forward solves, every route
# ------------------------------------------------------------------------------------------
ALL_FORWARD = R.FORWARD_CASES + (R.RESCUE_CASE,)


def _kernel_ran(case, st, ncg):
    """The intended kernel: the restated host-side choice names it, and so does the library's own
    route for the case's problem (gll_cg_route: what cg_dispatch launches from); exactly one CG
    launch was bracketed per forward, and the whole-GPU route was (or, injected, was not) left
    alone."""
    assert R.route(case.n, case.base, case.C, case.k, case.flags, case.B, case.knob_rv) == \
        (case.kernel, case.precond)
    rc, name, words = R.lib_route(case.n, case.base, case.C, case.k, case.flags, case.B,
                                  case.knob_rv)
    assert rc == 0 and name == (case.kernel, case.precond), (rc, name, words)
    assert ncg == 1, ncg
    rescued = sum(s[L.ST_GRID_RESCUED] for s in st)
    assert rescued == (1 if case.flags & R.FLAG_DIAG_GRID_FAIL else 0)
    assert all(s[L.ST_SOLVE_FAILED] == 0 for s in st)


@pytest.mark.parametrize("name", [c.name for c in ALL_FORWARD])
def test_forward_residual_iterations_and_rtol(name):
    case = {c.name: c for c in ALL_FORWARD}[name]
    ses = Session(case)
    runs = {rtol: ses.forward(rtol) for rtol in R.RTOLS}
    refs = _forward_refs(case, ses)
    its, worst = [], 0.0
    for rtol in R.RTOLS:
        U, U32, st, ncg = runs[rtol]
        _kernel_ran(case, st, ncg)
        worst = max(worst, _check_solution(name, refs, U, U32, rtol, R.ZERO_COL))
        for g, ref in enumerate(refs):   # without a sink every graph's block holds its own words
            assert st[g][L.ST_FWD_NONCONV] == 0
            assert abs(st[g][L.ST_FWD_ITERS] - int(ref.it[rtol].max())) <= 1, (g, rtol)
        _check_iters(name, st[0][L.ST_FWD_ITERS], refs[0].it[rtol], rtol)
        its.append(max(s[L.ST_FWD_ITERS] for s in st))
    assert its[0] < its[1] < its[2], its                            # rtol is honoured
    _note(f"{name} ({case.kernel}, {case.precond}): iterations {its}, worst rho/bound {worst:.3f}")


@pytest.mark.parametrize("name", [c.name for c in ALL_FORWARD])
def test_forward_max_iter_cap(name):
    case = {c.name: c for c in ALL_FORWARD}[name]
    ses = Session(case)
    U, U32, st, ncg = ses.forward(1e-6, max_iter=2)
    refs = _forward_refs(case, ses)
    _kernel_ran(case, st, ncg)
    errs = []
    for g, ref in enumerate(refs):
        assert np.delete(ref.it[1e-6], R.ZERO_COL).min() >= 4      # every live column is cut short
        assert st[g][L.ST_FWD_ITERS] == 2
        assert st[g][L.ST_FWD_NONCONV] == ref.nonzero == case.C - 1
        assert np.isfinite(U[g]).all() and np.isfinite(U32[g]).all()
        assert not U[g][:, R.ZERO_COL].any()
        assert np.array_equal(U[g], U32[g].astype(np.float64))
        errs.append(O.rel_err(U[g], ref.x2))
    _note(f"{name} max_iter 2: second iterate vs textbook, worst rel err {max(errs):.2e}")
    assert max(errs) <= ITERATE_TOL
    if name == "ell_neumann_m500":
        with pytest.warns(RuntimeWarning, match="reached max_iter"):
            GLL._warn_from(st[0])
    # the backward after a capped forward: finite, and not reported as a failed solve
    gbar = np.stack([_gbar(case, g) for g in range(case.B)])
    gx, wadj, stb, _ = ses.backward(gbar, L.GLL_DT_F32, 1e-6, max_iter=2)
    assert np.isfinite(gx).all() and np.isfinite(wadj).all()
    assert all(s[L.ST_SOLVE_FAILED] == 0 for s in stb)
    assert all(s[L.ST_BWD_ITERS] == 2 and s[L.ST_BWD_NONCONV] == case.C - 1 for s in stb)
    # converging on the last permitted iteration counts as converged
    cap = max(int(ref.it[1e-6].max()) for ref in refs) + 1
    U, U32, st, _ = ses.forward(1e-6, max_iter=cap)
    assert all(s[L.ST_FWD_NONCONV] == 0 for s in st), (cap, [s[L.ST_FWD_ITERS] for s in st])
    assert all(s[L.ST_FWD_ITERS] <= cap for s in st)


def _gbar(case, g=0):
    from graphlearninglayer_amd.synth import seeded_gbar
    gb = seeded_gbar(case.m, case.C, 77 + case.seed + g)
    gb[:, GBAR_ZERO_COL] = 0.0
    return gb


# ------------------------------------------------------------------------------------------
# Status words of a batch: own blocks, and a sticky sink
# ------------------------------------------------------------------------------------------
def test_batched_status_sink_holds_graph_zero_and_capped_columns_and_is_sticky():
    """gll.h: with a status_sink the *_ITERS words hold the iterations of graph 0 and of every
    column that hit max_iter; the words accumulate across calls.  Without one, each graph's own
    workspace block holds its own words (checked per graph in the tests above)."""
    case = R.CASES["ell_jacobi_256x2_B27"]
    own = Session(case)
    _, _, st_own, _ = own.forward(1e-6)
    its = [s[L.ST_FWD_ITERS] for s in st_own]
    ses = Session(case, sink=True)
    U, _, st_ws, _ = ses.forward(1e-6)
    sink = ses.sink.cpu().tolist()
    _note(f"batched sink: own-block iterations {its}, sink word {sink[L.ST_FWD_ITERS]}")
    assert sink[L.ST_FWD_ITERS] == its[0] and sink[L.ST_FWD_NONCONV] == 0
    assert max(its) > its[0]      # other graphs take more (textbook: 11 against 12): not a maximum
    assert np.array_equal(U, A.host(own.run.U))                   # the sink changes no result
    assert all(s[L.ST_FWD_ITERS] == 0 and s[L.ST_FWD_NONCONV] == 0 for s in st_ws)
    # capped: every live column of every graph reports, twice over two calls
    live = case.B * (case.C - 1)
    ses.sink.zero_()
    ses.forward(1e-6, max_iter=2)
    s1 = ses.sink.cpu().tolist()
    assert s1[L.ST_FWD_ITERS] == 2 and s1[L.ST_FWD_NONCONV] == live
    ses.forward(1e-6, max_iter=3)
    s2 = ses.sink.cpu().tolist()
    assert s2[L.ST_FWD_ITERS] == 3 and s2[L.ST_FWD_NONCONV] == 2 * live   # max / add: sticky
    gbar = np.stack([_gbar(case, g) for g in range(case.B)])
    ses.backward(gbar, L.GLL_DT_F64, 1e-6, max_iter=2)
    s3 = ses.sink.cpu().tolist()
    assert s3[L.ST_BWD_ITERS] == 2 and s3[L.ST_BWD_NONCONV] == live
    assert s3[L.ST_FWD_NONCONV] == 2 * live
    with pytest.warns(RuntimeWarning, match="reached max_iter"):
        GLL._warn_from(s3)


# ------------------------------------------------------------------------------------------
# Adjoint solves
# ------------------------------------------------------------------------------------------
ADJOINT = {   # name: (forward case, extra flags, (CG launches, fused launches), preconditioner)
    "fused": ("ell_neumann_m500", 0, (0, 1), "neumann"),
    "two_launches": ("ell_neumann_m500", R.FLAG_BWD_UNFUSED, (1, 0), "neumann"),
    "auto_eps": ("ell_auto_eps", 0, (1, 0), "neumann"),
    "batched": ("ell_jacobi_256x2_B27", 0, (1, 0), "jacobi"),
}


@pytest.mark.parametrize("g_dtype", ["f32", "f64"])
@pytest.mark.parametrize("name", list(ADJOINT))
def test_adjoint_residual_iterations_rtol_and_cap(name, g_dtype):
    """wadj (read from the view) of gll_backward(_batched) under the forward's four rules and the
    max_iter cap.  The right-hand side is gbar as the kernels read it: rounded to fp32."""
    import dataclasses
    fwd_name, extra, launches, precond = ADJOINT[name]
    case = dataclasses.replace(R.CASES[fwd_name], flags=R.CASES[fwd_name].flags | extra)
    assert R.route(case.n, case.base, case.C, case.k, case.flags, case.B)[1] == precond
    dt = L.GLL_DT_F32 if g_dtype == "f32" else L.GLL_DT_F64
    ses = Session(case)
    gbar = np.stack([_gbar(case, g) for g in range(case.B)])
    ses.forward()
    if name not in _adj_refs:   # shared by the two gbar dtypes: the kernels read both as fp32
        _adj_refs[name] = [Ref(A, gbar[g].astype(np.float32), precond)
                           for g, (A, _) in enumerate(ses.systems())]
    refs = _adj_refs[name]
    tag = f"adjoint {name} {g_dtype}"
    its, worst = [], 0.0
    for rtol in R.RTOLS:
        ses.forward()        # zeroes the block's status words (the adjoint words accumulate)
        gx, wadj, st, ran = ses.backward(gbar, dt, rtol)
        assert ran == launches, ran
        assert np.isfinite(gx).all()
        worst = max(worst, _check_solution(tag, refs, None, wadj, rtol, GBAR_ZERO_COL))
        for g, ref in enumerate(refs):
            assert st[g][L.ST_BWD_NONCONV] == 0 and st[g][L.ST_SOLVE_FAILED] == 0
            assert abs(st[g][L.ST_BWD_ITERS] - int(ref.it[rtol].max())) <= 1, (g, rtol)
        _check_iters(tag, st[0][L.ST_BWD_ITERS], refs[0].it[rtol], rtol)
        its.append(max(s[L.ST_BWD_ITERS] for s in st))
    assert its[0] < its[1] < its[2], its
    _note(f"{tag}: iterations {its}, worst rho/bound {worst:.3f}")
    # the cap
    ses.forward()
    gx, wadj, st, ran = ses.backward(gbar, dt, 1e-6, max_iter=2)
    assert ran == launches and np.isfinite(gx).all() and np.isfinite(wadj).all()
    errs = []
    for g, ref in enumerate(refs):
        assert np.delete(ref.it[1e-6], GBAR_ZERO_COL).min() >= 4
        assert st[g][L.ST_BWD_ITERS] == 2 and st[g][L.ST_BWD_NONCONV] == case.C - 1
        assert st[g][L.ST_SOLVE_FAILED] == 0 and st[g][L.ST_FWD_NONCONV] == 0
        assert not wadj[g][:, GBAR_ZERO_COL].any()
        errs.append(O.rel_err(wadj[g], ref.x2))
    _note(f"{tag} max_iter 2: second iterate vs textbook, worst rel err {max(errs):.2e}")
    assert max(errs) <= ITERATE_TOL
    with pytest.warns(RuntimeWarning, match="adjoint CG.*reached max_iter"):
        GLL._warn_from(st[0])
    ses.forward()
    cap = max(int(ref.it[1e-6].max()) for ref in refs) + 1
    _, _, st, _ = ses.backward(gbar, dt, 1e-6, max_iter=cap)
    assert all(s[L.ST_BWD_NONCONV] == 0 for s in st)


# ------------------------------------------------------------------------------------------
# gll_cg_csr, called directly (refined_solve's float64 refinement would repair its defects)
# ------------------------------------------------------------------------------------------
def _cg_csr(rp, col, val, b, atol, max_iter, ws="auto", counters=True, it_nc=None):
    """gll_cg_csr: (return code, x, iters, nonconv, CG launches).  `it_nc`: device counters to
    accumulate into (default: fresh zeroed ones)."""
    lib = L.lib()
    m, C = b.shape
    d = [torch.from_numpy(a).cuda() for a in (rp, col, val, b)]
    x = A.nan(m, C, dtype=torch.float32)
    if it_nc is None:
        it_nc = torch.zeros(2, dtype=torch.int32, device="cuda")
    wsd = None
    if ws == "auto":
        wsd = torch.empty(max(lib.gll_cg_csr_workspace_bytes(m, C), 4), dtype=torch.uint8, device="cuda")
    with A.launches(L.K_CG) as ran:
        rc = lib.gll_cg_csr(m, C, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                            x.data_ptr(), float(atol), int(max_iter),
                            it_nc.data_ptr() if counters else None,
                            it_nc[1:].data_ptr() if counters else None,
                            wsd.data_ptr() if wsd is not None else None, A.stream())
    it, nc = it_nc.cpu().tolist()
    return rc, x.cpu().numpy(), it, nc, ran[0]


@pytest.mark.parametrize("m,C,kernel", R.CSR_ROUTES)
def test_cg_csr_direct_contract(m, C, kernel):
    assert R.csr_route(m, C) == kernel
    rp, col, val, A, b = R.csr_case(m, C)
    bmax = float(np.linalg.norm(b.astype(np.float64), axis=0).max())
    live = C - 1 if C > 1 else 1
    tag = f"cg_csr m {m} C {C} ({kernel})"
    its = []
    for rel in (1e-3, 1e-6):
        atol = rel * bmax
        rc, x, it, nc, ncg = _cg_csr(rp, col, val, b, atol, 100000)
        assert rc == 0 and ncg == 1 and nc == 0 and np.isfinite(x).all()
        _, i64, cv, _ = R.pcg_columns(A, b, atol=atol)
        X32, i32, cv32, _ = R.pcg_columns(A, b, atol=atol, dtype=np.float32)
        assert cv.all() and cv32.all() and np.array_equal(i64, i32)
        rn = R.true_residual(A, x, b)[1]
        rn32 = R.true_residual(A, X32, b)[1]
        bound = np.full_like(rn, 1.05 * atol) if rel > 1e-6 else 2.0 * np.maximum(atol, rn32)
        _note(f"{tag} atol {rel:g} ||b||max: ||r|| max {rn.max():.3e} (float32 textbook "
              f"{rn32.max():.3e}, atol {atol:.3e}), worst ||r||/bound {(rn / bound).max():.3f}; "
              f"iterations {it} (float64 textbook max {i64.max()})")
        assert (rn <= bound).all(), (rn, bound)
        assert abs(it - int(i64.max())) <= 1
        if C > 1:
            assert not x[:, 1].any()
        its.append(it)
    assert its[0] < its[1]
    # the cap: two x updates, the last iterate is returned; the counters accumulate
    atol = 1e-6 * bmax
    x2 = R.pcg_columns(A, b, atol=atol, max_iter=2)[0]
    assert np.delete(i64, 1).min() >= 4 if C > 1 else i64.min() >= 4
    acc = torch.zeros(2, dtype=torch.int32, device="cuda")
    rc, x, it, nc, _ = _cg_csr(rp, col, val, b, atol, 2, it_nc=acc)
    err = O.rel_err(x, x2)
    _note(f"{tag} max_iter 2: second iterate vs textbook rel err {err:.2e}")
    assert rc == 0 and it == 2 and nc == live and np.isfinite(x).all() and err <= ITERATE_TOL
    rc, _, it, nc, _ = _cg_csr(rp, col, val, b, atol, 3, it_nc=acc)
    assert rc == 0 and it == 3 and nc == 2 * live      # iters: maximum; nonconv: sum -- not zeroed
    rc, _, it, nc, _ = _cg_csr(rp, col, val, b, atol, int(i64.max()) + 1)
    assert rc == 0 and nc == 0
    # NULL counters are accepted and change nothing
    rc, xn, _, _, _ = _cg_csr(rp, col, val, b, atol, 100000, counters=False)
    rc2, xc, _, _, _ = _cg_csr(rp, col, val, b, atol, 100000)
    assert rc == 0 and rc2 == 0 and np.array_equal(xn, xc)


def test_cg_csr_null_workspace():
    """NULL workspace: accepted while 5 m floats fit in LDS (m = 300), GLL_ERR_INVALID_ARG on the
    whole-GPU route (m = 2049, C = 4), before anything is launched."""
    rp, col, val, A, b = R.csr_case(300, 3)
    atol = 1e-6 * float(np.linalg.norm(b, axis=0).max())
    rc, x, it, nc, ncg = _cg_csr(rp, col, val, b, atol, 100000, ws=None)
    rcw, xw, itw, _, _ = _cg_csr(rp, col, val, b, atol, 100000)
    assert rc == 0 and nc == 0 and ncg == 1 and it == itw and np.array_equal(x, xw)
    rp, col, val, A, b = R.csr_case(2049, 4)
    rc, x, it, nc, ncg = _cg_csr(rp, col, val, b, 1e-3, 100000, ws=None)
    assert rc == -1 and ncg == 0 and it == 0 and nc == 0 and np.isnan(x).all()
