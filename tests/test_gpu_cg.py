"""The CG solvers on the HIP path (run on the MI355X: -m gpu): the whole-GPU CG (forced, large,
oversubscribed, its sync words, the rescue, busy CUs, past capacity), the balanced virtual-row
CG, gll_cg_csr and the batched two-row CG, against the float64 oracle (tests/test_gpu_parity.py
has the parity bar; tests/test_gpu_cg_contract.py pins the stopping contract).
"""
import numpy as np
import pytest
import torch

from graphlearninglayer_amd import GLL
from oracle import gll_oracle as O
from tests import abi as A
from tests.parity_runs import (TOL, batched_knn_lists, forward_c_abi, fwd_bwd_batched_c_abi,
                                fwd_bwd_c_abi, fwd_bwds_c_abi, gpu_knn, run_layer)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    A.need_gpu()


def test_grid_cg_forced_at_ns_matches_oracle():
    """The whole-GPU cooperative CG (gridcg.hip) on the NS graph vs the float64 oracle."""
    from graphlearninglayer_amd import _lib
    from graphlearninglayer_amd.synth import CONFIGS, one_hot, synth
    c = CONFIGS["ns"]
    X, lab = synth(c["base"], c["batch"], c["d"], r=c["r"], seed=0)
    Y = one_hot(lab[: c["base"]])
    Ug, itg, ncg = forward_c_abi(X, Y, c["k"], 0.07, 1.0, flags=_lib.FLAG_CG_GRID)
    Ue, ite, nce = forward_c_abi(X, Y, c["k"], 0.07, 1.0)
    # (iteration counts differ by preconditioner: the register-ELL kernel runs the Neumann
    # form at NS, about half the Jacobi iterations of the whole-GPU kernel)
    assert ncg == 0 and nce == 0 and itg > 0 and ite > 0
    ind = gpu_knn(X, c["k"], 1.0)["knn_idx"].cpu().numpy().astype(np.int64)
    Uo, _ = O.forward(X, Y, tau=0.07, epsilon=1.0, K=c["k"], knn=(ind, None))
    assert O.rel_err(Ug, Uo) <= TOL
    assert O.rel_err(Ug, Ue) <= 1e-5


def test_grid_cg_large_system_fwd_bwd_matches_oracle():
    """m = 6000 > 4096 selects the grid CG automatically (forward and adjoint)."""
    from graphlearninglayer_amd.synth import one_hot, seeded_gbar, synth
    base, m, d, k = 2000, 6000, 64, 10
    X, lab = synth(base, m, d, r=1.0, seed=5)
    Y = one_hot(lab[:base])
    g = seeded_gbar(m, 10, 7)
    U, grad = run_layer(X, Y, 0.07, 1.0, k, g)
    ind = gpu_knn(X, k, 1.0)["knn_idx"].cpu().numpy().astype(np.int64)
    Uo, st = O.forward(X, Y, tau=0.07, epsilon=1.0, K=k, knn=(ind, None))
    go = O.backward(st, g)
    assert O.rel_err(U, Uo) <= TOL
    assert O.rel_err(grad, go) <= TOL


def test_cg_csr_large_matches_scipy():
    """gll_cg_csr for m > 2048 (grid CG) against a direct sparse solve."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    rng = np.random.default_rng(3)
    m, C = 5000, 4
    M = sp.random(m, m, density=6.0 / m, random_state=rng, format="csr")
    M = M + M.T
    M = (sp.diags(np.asarray(abs(M).sum(1)).ravel() + 0.5) + M).tocsr()   # SPD, dominant
    b = rng.standard_normal((m, C))
    x = GLL.stable_conjgrad(M, b, tol=1e-8)
    xe = spla.spsolve(M.tocsc(), b)
    assert np.max(np.abs(x - xe)) <= 1e-6 * np.max(np.abs(xe))


def _grid_case():
    from graphlearninglayer_amd.synth import one_hot, synth
    base, m, d, k = 2000, 6000, 64, 10
    X, lab = synth(base, m, d, r=1.0, seed=5)
    return X, one_hot(lab[:base]), k


def test_grid_cg_oversubscribed_launch_is_refused():
    """A whole-GPU CG grid larger than the co-resident capacity is refused at launch (the
    cooperative launch's guarantee) and surfaces as an error -- never as a U computed by a
    grid whose barrier waited on workgroups that were not resident."""
    from graphlearninglayer_amd import _lib
    X, Y, k = _grid_case()
    with pytest.raises(RuntimeError, match="gll_forward failed"):
        forward_c_abi(X, Y, k, 0.07, 1.0, flags=_lib.FLAG_CG_GRID | _lib.FLAG_DIAG_GRID_OVERSUB)
    torch.cuda.synchronize()   # the device is still healthy: a normal call works
    U, it, nc = forward_c_abi(X, Y, k, 0.07, 1.0)
    assert np.isfinite(U).all() and nc == 0


def test_grid_cg_sync_words_reset_between_solves():
    """The whole-GPU CG's sync words are zeroed by row_build before a forward and returned to
    zero by the last workgroup out of every solve (gridcg.hip gv_exit) -- no memset launch.  Three
    backward calls on one workspace after a forward give bitwise equal gradients with no failed
    or rescued barrier; after a forward whose barrier failed (injected: the rescue solve ran), a
    normal backward on the same workspace runs its grid solve cleanly (GLL.py:53,93)."""
    from graphlearninglayer_amd import _lib
    from graphlearninglayer_amd.synth import seeded_gbar
    X, Y, k = _grid_case()
    n, d = X.shape
    base, C = Y.shape
    g = seeded_gbar(n - base, C, 3)
    U, grads, st = fwd_bwds_c_abi(X, Y, k, 0.07, 1.0, g, backward_calls=3)
    for gx in grads[1:]:
        np.testing.assert_array_equal(gx, grads[0])
    assert st[_lib.ST_SOLVE_FAILED] == 0 and st[_lib.ST_GRID_RESCUED] == 0
    run = A.Run(X, Y, k, 0.07, 1.0, _lib.FLAG_DIAG_GRID_FAIL)
    assert run.workspace_bytes(flags=0) == run.wb
    Ud = run.forward()
    rescued = run.status()[_lib.ST_GRID_RESCUED]
    assert rescued >= 1
    gx = run.backward(g, labels=False, flags=0)
    st2 = run.status()
    assert st2[_lib.ST_GRID_RESCUED] == rescued and st2[_lib.ST_SOLVE_FAILED] == 0
    assert O.rel_err(Ud, U) <= 1e-5
    assert O.rel_err(gx, grads[0]) <= 1e-5


def test_grid_cg_barrier_failure_is_rescued():
    """An (injected) grid-barrier failure of the whole-GPU CG (gridcg.hip): the first workgroup
    to see it solves the system alone (rescue_solve) and the others write nothing -- U still
    matches the float64 oracle, GLL_ST_GRID_RESCUED counts the rescue and is reported as a
    RuntimeWarning, and no error is raised (GLL.py:53)."""
    from graphlearninglayer_amd import _lib
    X, Y, k = _grid_case()
    st = []
    U, it, nc = forward_c_abi(X, Y, k, 0.07, 1.0,
                               flags=_lib.FLAG_CG_GRID | _lib.FLAG_DIAG_GRID_FAIL, status=st)
    assert st[_lib.ST_GRID_RESCUED] == 1 and st[_lib.ST_SOLVE_FAILED] == 0 and nc == 0
    ind = gpu_knn(X, k, 1.0)["knn_idx"].cpu().numpy().astype(np.int64)
    Uo, _ = O.forward(X, Y, tau=0.07, epsilon=1.0, K=k, knn=(ind, None))
    assert O.rel_err(U, Uo) <= TOL
    with pytest.warns(RuntimeWarning, match="solved by one workgroup"):
        GLL._warn_from(st)


def test_grid_cg_correct_beside_a_kernel_holding_the_cus():
    """The whole-GPU CG launches ordinarily (no cooperative residency promise).  With a large
    GEMM holding the CUs on another stream when the stress solve starts, its workgroups become
    resident as the GEMM's retire; the solve completes (or is rescued) and U and grad_X match
    the float64 oracle (GLL.py:53,93)."""
    from graphlearninglayer_amd.synth import CONFIGS, one_hot, seeded_gbar, synth
    c = CONFIGS["stress"]
    X, lab = synth(c["base"], c["batch"], c["d"], r=c["r"], seed=8)
    Y = one_hot(lab[: c["base"]])
    g = seeded_gbar(c["batch"], 10, 9)
    a = torch.randn(8192, 8192, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(4):
            a = a @ a * 1e-4   # ~tens of ms of GEMM on every CU
    U, grad = run_layer(X, Y, 0.07, "auto", c["k"], g)
    torch.cuda.synchronize()
    ind = gpu_knn(X, c["k"])["knn_idx"].cpu().numpy()
    Uo, st = O.forward(X, Y, 0.07, "auto", c["k"], knn=(ind, None))
    assert O.rel_err(U, Uo) < TOL
    assert O.rel_err(grad, O.backward(st, g)) < TOL


def test_grid_cg_past_capacity_falls_back_to_per_column(monkeypatch):
    """More rows than the co-resident workgroups can hold (capacity shrunk to 4 workgroups
    through the GLL_KNOB_GRID_CAP test knob): the whole-GPU CG declines and the per-column kernels with the
    Krylov vectors in the workspace solve the system -- no size limit, same answer."""
    X, Y, k = _grid_case()
    from graphlearninglayer_amd import _lib
    with A.knobs({_lib.KNOB_GRID_CAP: 4}):
        U, it, nc = forward_c_abi(X, Y, k, 0.07, 1.0)
    ind = gpu_knn(X, k, 1.0)["knn_idx"].cpu().numpy().astype(np.int64)
    Uo, _ = O.forward(X, Y, tau=0.07, epsilon=1.0, K=k, knn=(ind, None))
    assert nc == 0 and O.rel_err(U, Uo) <= TOL


@pytest.mark.parametrize("cfg,flags", [("fullysup", 0), ("ns", "vr"), ("plumbing", "vr")])
def test_balanced_cg_matches_register_ell_and_oracle(cfg, flags):
    """The balanced virtual-row CG (solve.hip cg_vr_kernel: the automatic choice at K = 25, the
    FullySup shape; forced elsewhere) against the register-ELL kernel and the float64 oracle,
    forward and adjoint (GLL.py:53,93)."""
    from graphlearninglayer_amd import _lib
    from graphlearninglayer_amd.synth import CONFIGS, one_hot, synth
    c = CONFIGS[cfg]
    X, lab = synth(c["base"], c["batch"], c["d"], r=c["r"], seed=2)
    Y = one_hot(lab[: c["base"]])
    fv = _lib.FLAG_CG_VR if flags == "vr" else 0
    st_v, st_e = [], []
    Uv, itv, ncv = forward_c_abi(X, Y, c["k"], 0.07, 1.0, flags=fv, status=st_v)
    Ue, ite, nce = forward_c_abi(X, Y, c["k"], 0.07, 1.0, flags=_lib.FLAG_CG_ELL, status=st_e)
    assert ncv == 0 and nce == 0 and itv > 0 and ite > 0, (itv, ite)   # Jacobi vs Neumann
    ind = gpu_knn(X, c["k"], 1.0)["knn_idx"].cpu().numpy().astype(np.int64)
    Uo, _ = O.forward(X, Y, tau=0.07, epsilon=1.0, K=c["k"], knn=(ind, None))
    assert O.rel_err(Uv, Uo) <= TOL
    assert O.rel_err(Uv, Ue) <= 1e-5


def test_balanced_cg_spill_path_matches_oracle(monkeypatch):
    """Virtual rows past the register capacity (forced to 4 per thread through the GLL_KNOB_VR_RV test knob, so
    most of the FullySup U block spills) are summed from the CSR by their rows' threads: same
    answer, forward and adjoint, deterministic."""
    from graphlearninglayer_amd.synth import CONFIGS, one_hot, seeded_gbar, synth
    c = CONFIGS["fullysup"]
    X, lab = synth(c["base"], c["batch"], c["d"], r=c["r"], seed=4)
    Y = one_hot(lab[: c["base"]])
    g = seeded_gbar(c["batch"], 10, 9)
    from graphlearninglayer_amd import _lib
    with A.knobs({_lib.KNOB_VR_RV: 4}):
        U1, gr1 = run_layer(X, Y, 0.07, 1.0, c["k"], g)
        U2, gr2 = run_layer(X, Y, 0.07, 1.0, c["k"], g)
    np.testing.assert_array_equal(U1, U2)
    np.testing.assert_array_equal(gr1, gr2)
    ind = gpu_knn(X, c["k"], 1.0)["knn_idx"].cpu().numpy().astype(np.int64)
    Uo, st = O.forward(X, Y, tau=0.07, epsilon=1.0, K=c["k"], knn=(ind, None))
    assert O.rel_err(U1, Uo) <= TOL
    assert O.rel_err(gr1, O.backward(st, g)) <= TOL


def test_balanced_cg_vrm_clamp_at_wide_k_matches_oracle():
    """Advisor (round 5): at k = 129 a U row may need ceil((5(K-1)+8)/8) = 81 virtual-row slots,
    past the 63 the CG's 6-bit slot field holds (vr_max_per_row clamps), so long rows keep their
    tail in the CSR.  Forcing the balanced kernel (GLL_FLAG_CG_VR, 10 virtual rows per thread)
    at k = 129 runs the clamp and the spill path together; forward and adjoint against the
    oracle."""
    from graphlearninglayer_amd import _lib
    from graphlearninglayer_amd.synth import one_hot, seeded_gbar, synth
    X, lab = synth(500, 500, 64, C=10, r=1.0, seed=6)
    Y = one_hot(lab[:500])
    g = seeded_gbar(500, 10, 5)
    with A.knobs({_lib.KNOB_VR_RV: 10}):
        U, gr = fwd_bwd_c_abi(X, Y, 129, 0.07, 1.0, g, flags=_lib.FLAG_CG_VR)
    ind = gpu_knn(X, 129, 1.0)["knn_idx"].cpu().numpy().astype(np.int64)
    Uo, st = O.forward(X, Y, tau=0.07, epsilon=1.0, K=129, knn=(ind, None))
    assert O.rel_err(U, Uo) <= TOL
    assert O.rel_err(gr, O.backward(st, g)) <= TOL


@pytest.mark.parametrize("m,k,eps", [(333, 10, 1.0), (500, 10, "auto"), (449, 11, 1.0)])
def test_batched_two_row_cg_ragged_and_hub_rows_match_oracle(m, k, eps):
    """The batched 256 x 2 CG (B x C > 256 column workgroups, 256 < m <= 512; solve.hip
    cg_dispatch) with ragged row counts (m = 333, 449: dead threads in the last waves), and in
    every third graph a hub -- 40 rows placed around one U row, whose U block then passes the 24
    register slots (its tail comes from the LDS overflow) -- every such graph's U and grad_X
    against the float64 oracle on its own kNN lists (GLL.py:53,93)."""
    from graphlearninglayer_amd.synth import one_hot, seeded_gbar, synth
    B, base, d = 32, 200, 64
    Xs, Ys, Gs = [], [], []
    rng = np.random.default_rng(7)
    for g in range(B):
        X, lab = synth(base, m, d, r=1.0, seed=500 + g)
        if g % 3 == 0:   # a hub: rows 260..299 around row 250 (all U rows)
            X[260:300] = X[250] + 0.02 * rng.standard_normal((40, d)).astype(np.float32)
            X[260:300] /= np.linalg.norm(X[260:300], axis=1, keepdims=True)
        Xs.append(X)
        Ys.append(one_hot(lab[:base]))
        Gs.append(seeded_gbar(m, 10, 600 + g))
    Xs, Ys, G = np.stack(Xs), np.stack(Ys), np.stack(Gs)
    U, gx, run = fwd_bwd_batched_c_abi(Xs, Ys, k, 0.07, eps, G)
    inds = batched_knn_lists(run)
    for g in range(0, B, 3):
        Uo, st = O.forward(Xs[g], Ys[g], tau=0.07, epsilon=eps, K=k, knn=(inds[g], None))
        assert O.rel_err(U[g], Uo) <= TOL, g
        assert O.rel_err(gx[g], O.backward(st, G[g])) <= TOL, g
