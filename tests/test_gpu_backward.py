"""The backward's kernel choices on the HIP path (run on the MI355X: -m gpu): chunked against
whole-row gradient, the fused backward against two launches, its hand-off with uneven column
solves, and the row order a backward may read.  The parity bar is that of
tests/test_gpu_parity.py.
"""
import numpy as np
import pytest

from oracle import gll_oracle as O
from tests import abi as A
from tests.parity_runs import TOL, fwd_bwd_c_abi, fwd_bwds_c_abi, gpu_knn

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    A.need_gpu()


@pytest.mark.parametrize("cfg,eps", [("ns", 1.0), ("ns", "auto"), ("fullysup", 1.0),
                                     ("stress", 1.0), ("stress", "auto")])
def test_chunked_grad_matches_row_kernel_bitwise(cfg, eps):
    """The feature-chunked gradient kernel (grad.hip grad_chunk_kernel: features split over the
    XCDs; automatic at stress, forced here elsewhere) sums every element in the same edge order as
    the whole-row kernel: bitwise equal, and within the parity bar of the oracle
    (GLL.py:111-159)."""
    from graphlearninglayer_amd import _lib
    from graphlearninglayer_amd.synth import CONFIGS, one_hot, seeded_gbar, synth
    c = CONFIGS[cfg]
    X, lab = synth(c["base"], c["batch"], c["d"], r=c["r"], seed=6)
    Y = one_hot(lab[: c["base"]])
    g = seeded_gbar(c["batch"], 10, 3)
    Uc, gc, ran_c = fwd_bwd_c_abi(X, Y, c["k"], 0.07, eps, g, flags=_lib.FLAG_GRAD_CHUNK,
                                   counts=True)
    Ur, gr, ran_r = fwd_bwd_c_abi(X, Y, c["k"], 0.07, eps, g, flags=_lib.FLAG_GRAD_ROWS,
                                   counts=True)
    # the two sides ran different kernels: the edge pass + grad_chunk_kernel against the whole-row
    # form (grad_spmm_kernel, or at NS with fixed eps the fused backward's gradient role)
    from tests import grad_ref
    shape = (c["base"] + c["batch"], c["d"], c["base"], 10, c["k"], 1, eps == "auto", True)
    want_c = grad_ref.route(*shape, _lib.FLAG_GRAD_CHUNK)
    want_r = grad_ref.route(*shape, _lib.FLAG_GRAD_ROWS)
    assert want_c.family == "chunk" and want_r.family == (
        "fused" if (cfg, eps) == ("ns", 1.0) else "spmm")
    assert ran_c.counts == want_c.counts == (1, 1, 0, 1), ran_c
    assert ran_r.counts == want_r.counts, ran_r
    np.testing.assert_array_equal(Uc, Ur)
    np.testing.assert_array_equal(gc, gr)
    if cfg == "stress":   # the chunked kernel's automatic case; the oracle check runs elsewhere
        return
    ind = gpu_knn(X, c["k"], eps)["knn_idx"].cpu().numpy().astype(np.int64)
    Uo, st = O.forward(X, Y, tau=0.07, epsilon=eps, K=c["k"], knn=(ind, None))
    assert O.rel_err(gc, O.backward(st, g)) <= TOL


@pytest.mark.parametrize("cfg", ["plumbing", "ns", "wide_base"])
def test_fused_backward_equals_two_launches_bitwise(cfg):
    """The fused backward (adjoint CG + feature gradient in one launch, fused_bwd.hip
    cg_grad_fused_kernel: single small graphs, fixed eps) against the same two kernels as two
    launches (GLL_FLAG_BWD_UNFUSED): bitwise equal, and equal again on a second backward over
    the same workspace (the hand-off counters re-arm); against the float64 oracle at 1e-4.
    The gradient waves take the rows in class order (round 6); `wide_base`
    (1,400 labeled + 500 unlabeled rows at d = 128) sorts 30 64-row chunks in 248 workgroups,
    the most the 256 CUs hold co-resident (at 3,500 + 500 rows the launch needs 510, the fused
    kernel declines and both sides of this comparison would be the two-launch path).  Which
    side ran which kernels is asserted from the bracketed launches."""
    from graphlearninglayer_amd import _lib
    from graphlearninglayer_amd.synth import CONFIGS, one_hot, seeded_gbar, synth
    c = CONFIGS[cfg] if cfg in CONFIGS else dict(base=1400, batch=500, d=128, k=10, r=1.0)
    X, lab = synth(c["base"], c["batch"], c["d"], r=c["r"], seed=6)
    Y = one_hot(lab[: c["base"]])
    g = seeded_gbar(c["batch"], 10, 17)
    Uf, gf, stf, ran_f = fwd_bwds_c_abi(X, Y, c["k"], 0.07, 1.0, g, backward_calls=3,
                                         counts=True)
    Uu, gu, stu, ran_u = fwd_bwds_c_abi(X, Y, c["k"], 0.07, 1.0, g, flags=_lib.FLAG_BWD_UNFUSED,
                                         counts=True)
    # (edge pass, gradient, fused backward, CG) launches: one fused launch per backward against
    # a CG and a gradient launch
    assert ran_f == [(0, 0, 1, 0)] * 3, ran_f
    assert ran_u == [(0, 1, 0, 1)], ran_u
    np.testing.assert_array_equal(Uf, Uu)
    for gx in gf:
        np.testing.assert_array_equal(gx, gu[0])
    assert stf[_lib.ST_SOLVE_FAILED] == 0 and stf[_lib.ST_BWD_NONCONV] == 0
    assert stf[_lib.ST_BWD_ITERS] == stu[_lib.ST_BWD_ITERS] > 0
    ind = gpu_knn(X, c["k"], 1.0)["knn_idx"].cpu().numpy().astype(np.int64)
    Uo, st = O.forward(X, Y, tau=0.07, epsilon=1.0, K=c["k"], knn=(ind, None))
    assert O.rel_err(gf[0], O.backward(st, g)) <= TOL


@pytest.mark.parametrize("live", [(3,), (0, 9), (4, 5, 6)])
def test_fused_backward_handoff_with_uneven_column_solves(live):
    """The fused backward's hand-off with column solves of very different
    lengths: dL/dU is zero in all but the `live` columns, so those columns' adjoint solves run
    their iterations while the zero columns finish at once and raise the counter first; the 125
    gradient workgroups (one per CU, every XCD) poll while a single column is still iterating.
    Bitwise equal to the two-launch backward, on three backwards over one workspace (re-arm), and
    to the float64 oracle at 1e-4."""
    from graphlearninglayer_amd import _lib
    from graphlearninglayer_amd.synth import CONFIGS, one_hot, seeded_gbar, synth
    c = CONFIGS["ns"]
    X, lab = synth(c["base"], c["batch"], c["d"], r=c["r"], seed=21)
    Y = one_hot(lab[: c["base"]])
    g = np.zeros((c["batch"], 10))
    full = seeded_gbar(c["batch"], 10, 23)
    for q, col in enumerate(live):
        g[:, col] = full[:, col] * 10.0 ** (3 * q)   # scales 1, 1e3, 1e6
    Uf, gf, stf, ran_f = fwd_bwds_c_abi(X, Y, c["k"], 0.07, 1.0, g, backward_calls=3,
                                         counts=True)
    Uu, gu, stu, ran_u = fwd_bwds_c_abi(X, Y, c["k"], 0.07, 1.0, g, flags=_lib.FLAG_BWD_UNFUSED,
                                         counts=True)
    assert ran_f == [(0, 0, 1, 0)] * 3, ran_f      # the fused kernel, every backward
    assert ran_u == [(0, 1, 0, 1)], ran_u          # a CG launch and a gradient launch
    for gx in gf:
        np.testing.assert_array_equal(gx, gu[0])
    assert stf[_lib.ST_SOLVE_FAILED] == 0 and stf[_lib.ST_BWD_NONCONV] == 0
    assert stf[_lib.ST_BWD_ITERS] == stu[_lib.ST_BWD_ITERS] > 0
    ind = gpu_knn(X, c["k"], 1.0)["knn_idx"].cpu().numpy().astype(np.int64)
    Uo, st = O.forward(X, Y, tau=0.07, epsilon=1.0, K=c["k"], knn=(ind, None))
    assert O.rel_err(gf[0], O.backward(st, g)) <= TOL


def test_backward_never_reads_an_order_its_forward_did_not_write():
    """gll_backward takes its own gll_problem, so its flags may differ from the forward's: a
    forward with GLL_FLAG_ROW_ORDER_OFF writes no locality order, and the backward then must not
    gather rows through the workspace's stale perm (here all zeros: every position would map to
    row 0, leaving the other rows of grad_X unwritten).  grad_X equals the row-order result
    bitwise (GLL.py:146-159)."""
    from graphlearninglayer_amd import _lib
    from graphlearninglayer_amd.synth import CONFIGS, one_hot, seeded_gbar, synth
    c = CONFIGS["stress"]
    X, lab = synth(c["base"], c["batch"], c["d"], r=c["r"], seed=5)
    Y = one_hot(lab[: c["base"]])
    g = seeded_gbar(c["batch"], 10, 6)
    off = _lib.FLAG_ROW_ORDER_OFF
    U0, g0 = fwd_bwd_c_abi(X, Y, c["k"], 0.07, 1.0, g, flags=off)
    U1, g1 = fwd_bwd_c_abi(X, Y, c["k"], 0.07, 1.0, g, flags=off, bwd_flags=0, ws_fill=0)
    np.testing.assert_array_equal(U0, U1)
    np.testing.assert_array_equal(g0, g1)
