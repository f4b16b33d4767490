"""The fused backward's row parts (fused_bwd.hip cg_grad_fused_kernel): rows of more
than EB edges run as 2 or 4 waves, each over a part of the row's features.  (run on the MI355X:
-m gpu)

Inputs are tests/star_graphs.py: clusters (rows of k - 1 edges) and stars whose rows have exactly
16, 17, 32, 33, 64, 65 and 130 edges -- each side of every threshold of the rule, and a row past
the 64-edge loop.  The seven stars alone are 357 satellites and 7 centres, 364 rows, so the shapes
have n = 400 and base = 200 (the rest are clusters).
Every test first asserts those lengths from the device graph.  Each shape runs three ways through
the C ABI -- parts on, parts off (GLL_KNOB_GRAD_SPLIT) and as two launches (GLL_FLAG_BWD_UNFUSED)
-- and grad_X must agree bitwise, on a second backward over the same workspace too; which kernels
ran is asserted from the bracketed launches (tests/launch_counts.py) in every case.
"""
import ctypes as ct

import numpy as np
import pytest
import torch

from oracle import gll_oracle as O
from tests import abi as A
from tests.star_graphs import row_lengths, row_parts, star_points

pytestmark = pytest.mark.gpu
TOL = 1e-4   # the parity bar of tests/test_gpu_parity.py
K = 4
STARS = (16, 17, 32, 33, 64, 65, 130)
TAU, EPS = 0.07, 1.0


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    A.need_gpu()


def _problem(n, d, base, flags=0):
    from graphlearninglayer_amd import GLL
    return GLL.make_problem(n, d, base, 10, K, TAU, EPS, flags=flags)


def _run(X, Y, gbar, flags=0, knob=0, backward_calls=2):
    """gll_forward, then `backward_calls` x gll_backward on one workspace with
    GLL_KNOB_GRAD_SPLIT = knob: [grad_X], [status words after each backward], [launches]."""
    from graphlearninglayer_amd import _lib
    from tests.launch_counts import counted
    run = A.Run(X, Y, K, TAU, EPS, flags)
    grads, sts, ran = [], [], []
    with A.knobs({_lib.KNOB_GRAD_SPLIT: knob}):
        run.forward()
        for _ in range(backward_calls):
            with counted() as got:
                grads.append(run.backward(gbar, labels=False))
            sts.append(run.status())
            ran.append(got.counts)
    return grads, sts, ran


def _device_plan(n, d, base):
    """gll_fused_plan for the current device: (threads, ND, grid, base grid, gradient waves, spare
    waves, split, LDS bytes), or None when the backward takes two launches."""
    from graphlearninglayer_amd import _lib
    out = (ct.c_int32 * 8)()
    prob = _problem(n, d, base)
    rc = _lib.lib().gll_fused_plan(ct.byref(prob), 1, -1, out)
    return list(out) if rc == 0 else None


def _case(d, n, base, stars=STARS, seed=3, both_sides=True):
    from graphlearninglayer_amd import GLL
    from graphlearninglayer_amd.synth import one_hot, seeded_gbar
    X, grp = star_points(d, stars, n, K, seed=seed)
    Y = one_hot((grp[:base] % 10).astype(np.int64))
    g = seeded_gbar(n - base, 10, 17)
    # the intended row lengths, from the device graph, before anything else
    rp = GLL.device_graph(torch.from_numpy(X).cuda(), K, EPS)["row_ptr"].cpu().numpy()
    lens = np.diff(rp)
    np.testing.assert_array_equal(lens, row_lengths(X, K))
    for s in stars:
        rows = np.nonzero(lens == s)[0]
        assert len(rows) >= 1, f"no row of {s} edges"
    long_rows = np.nonzero(lens > 16)[0]
    if both_sides:
        assert (long_rows < base).any() and (long_rows >= base).any(), "stars on both sides of base"
    assert (lens[lens < 16] >= K - 1).all() and (lens == K - 1).sum() >= K
    return X, Y, g, lens


def _check_three_ways(X, Y, g, lens, nd, expect_split):
    from graphlearninglayer_amd import _lib
    g_on, st_on, ran_on = _run(X, Y, g, knob=1)
    g_off, st_off, ran_off = _run(X, Y, g, knob=2)
    g_two, st_two, ran_two = _run(X, Y, g, flags=_lib.FLAG_BWD_UNFUSED, backward_calls=1)
    # (edge pass, gradient, fused backward, CG) launches of each backward
    assert ran_on == [(0, 0, 1, 0)] * 2, ran_on
    assert ran_off == [(0, 0, 1, 0)] * 2, ran_off
    assert ran_two == [(0, 1, 0, 1)], ran_two
    assert np.isfinite(g_two[0]).all()
    for gx in (*g_on, *g_off):
        np.testing.assert_array_equal(gx, g_two[0])
    for st in (*st_on, *st_off):
        assert st[_lib.ST_SOLVE_FAILED] == 0 and st[_lib.ST_BWD_NONCONV] == 0
    assert [st[_lib.ST_GRAD_SPLIT] for st in st_on] == [expect_split] * 2
    assert [st[_lib.ST_GRAD_SPLIT] for st in st_off] == [0] * 2
    assert st_two[0][_lib.ST_GRAD_SPLIT] == 0
    return g_on[0]


def _expected_split(lens, n, d, base):
    """Rows the rule splits, and a check that the launch has a wave for every item."""
    plan = _device_plan(n, d, base)
    assert plan is not None, "the shape must take the fused route"
    nd = plan[1]
    parts = np.array([row_parts(int(v), nd) for v in lens])
    assert plan[6] == (1 if nd >= 2 else 0)
    assert parts.sum() <= plan[4], (parts.sum(), plan)
    return nd, int((parts > 1).sum())


@pytest.mark.parametrize("d", [512, 1024, 260])
def test_row_parts_bitwise_across_row_lengths(d):
    """Star sizes 16 .. 130 at d = 512 (two f32x4 per lane: 2 parts of one f32x4, 4 of one f32x2),
    d = 1024 (four: EB = 8, parts of two and one f32x4) and d = 260 (the second vector masked but
    for four floats; the last of four parts owns no feature at all)."""
    n, base = 400, 200
    X, Y, g, lens = _case(d, n, base)
    nd, split = _expected_split(lens, n, d, base)
    assert nd == (2 if d <= 512 else 4)
    assert split == int((lens > (16 if nd == 2 else 8)).sum()) > 0
    _check_three_ways(X, Y, g, lens, nd, split)


def test_row_parts_one_vector_rows_stay_whole():
    """d <= 256: one f32x4 per lane, the rule gives every row one part."""
    n, base, d = 400, 200, 256
    X, Y, g, lens = _case(d, n, base)
    nd, split = _expected_split(lens, n, d, base)
    assert (nd, split) == (1, 0)
    _check_three_ways(X, Y, g, lens, nd, 0)


def test_row_parts_ragged_n_and_oracle():
    """n = 667 (not a multiple of the 8 waves of a workgroup; m = 367 runs the 512-thread
    kernel the NS shape runs), and the gradient against the float64 oracle at the parity bar."""
    from graphlearninglayer_amd import GLL
    n, base, d = 667, 300, 512
    X, Y, g, lens = _case(d, n, base, seed=5)
    plan = _device_plan(n, d, base)
    assert plan is not None and plan[0] == 512 and n % (plan[0] // 64) != 0
    nd, split = _expected_split(lens, n, d, base)
    gx = _check_three_ways(X, Y, g, lens, nd, split)
    ind = GLL.device_graph(torch.from_numpy(X).cuda(), K, EPS)["knn_idx"].cpu().numpy()
    _, st = O.forward(X, Y, tau=TAU, epsilon=EPS, K=K, knn=(ind.astype(np.int64), None))
    err = O.rel_err(gx, O.backward(st, g))
    print(f"grad_X vs the float64 oracle: {err:.3e}")
    assert err <= TOL


def _spare_workgroups(n, d, m):
    """Gradient workgroups past one per row in the launch of (n, d, m <= 64: one wave each); -1
    when the base grid does not fit the device, a large number when the launch is not capped."""
    plan = _device_plan(n, d, n - m)
    if plan is None:
        return -1
    return plan[2] - 10 - n if plan[2] < 10 + 2 * n else 1 << 30


def _shape_at_the_capacity(d):
    """(n, m) whose launch fills the device's co-resident capacity with one or two gradient
    workgroups to spare.  The capacity falls in steps as n grows (the workgroup's LDS grows with
    n), so the spare count falls with n: bisect for the last n with a spare workgroup, over a few
    m (which move the steps), until the count there is 1 or 2."""
    n_max = (4 << 20) // (4 * d)   # the fused route's X limit
    for m in range(60, 8, -4):
        lo, hi = 64 + m, n_max
        if _spare_workgroups(lo, d, m) < 1 or _spare_workgroups(hi, d, m) >= 1:
            continue
        while hi - lo > 1:   # spare(lo) >= 1 > spare(hi)
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if _spare_workgroups(mid, d, m) >= 1 else (lo, mid)
        if _spare_workgroups(lo, d, m) in (1, 2):
            return lo, m
    return None


def test_row_parts_fall_back_when_items_exceed_the_waves():
    """n chosen at run time so the launch fills the device's co-resident capacity with one or two
    spare gradient waves, and three stars of 17 (nine rows of 17 edges at k = 4) ask for more:
    every workgroup keeps one wave per row, GLL_ST_GRAD_SPLIT reads 0 and the gradient is
    bitwise the two-launch one."""
    d, stars = 512, (17, 17, 17)
    found = _shape_at_the_capacity(d)
    if found is None:
        pytest.skip("no n <= 2048 whose launch leaves one or two spare gradient workgroups at "
                    "this device's co-resident capacity")
    n, m = found
    base = n - m
    plan = _device_plan(n, d, base)
    print(f"n = {n}, m = {m}: plan {plan}")
    X, Y, g, lens = _case(d, n, base, stars=stars, seed=7, both_sides=False)
    parts = np.array([row_parts(int(v), plan[1]) for v in lens])
    assert plan[0] == 64 and plan[6] == 1 and parts.sum() > plan[4] >= n, (parts.sum(), plan)
    _check_three_ways(X, Y, g, lens, plan[1], 0)
