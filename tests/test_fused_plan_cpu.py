"""Host sizing of the fused backward's launch (fused_bwd.hip fused_grid through gll_fused_plan): the
grid, the spare gradient waves that take the parts of long rows, and the LDS -- no GPU needed, the
co-resident capacity is an argument."""
import ctypes as ct

import pytest

from graphlearninglayer_amd import GLL, _lib

UNSUPPORTED = -2   # include/gll.h GLL_ERR_UNSUPPORTED


def _plan(n, d, base, capacity, k=10, eps=1.0, flags=0, aligned=1):
    prob = GLL.make_problem(n, d, base, 10, k, 0.07, eps, flags=flags)
    out = (ct.c_int32 * 8)()
    rc = _lib.lib().gll_fused_plan(ct.byref(prob), aligned, capacity, out)
    return rc, list(out)


@pytest.fixture()
def knob():
    yield lambda v: _lib.set_knob(_lib.KNOB_GRAD_SPLIT, v)
    _lib.set_knob(_lib.KNOB_GRAD_SPLIT, 0)


def test_ns_launch_fills_the_capacity():
    """NS (1000 rows, m = 500, d = 512) on 256 CUs, one workgroup each: the base grid is 10 solves
    + 125 gradient workgroups; two waves per row would be 260 workgroups, so the launch is the 256
    the device holds: 1968 gradient waves, 968 spare."""
    rc, p = _plan(1000, 512, 500, 256)
    assert rc == 0
    assert p[:7] == [512, 2, 256, 135, 1968, 968, 1]
    # 128 words + P and y of 500 rows + the solves' overflow entries, (m + n)(K - 1) of them
    assert p[7] == 512 + 2 * 4 * 500 + 8 * 1500 * 9
    # a roomier device: never more than two waves per row
    rc, p = _plan(1000, 512, 500, 1024)
    assert rc == 0 and p[2:6] == [260, 135, 2000, 1000]


def test_base_grid_is_the_route_condition():
    assert _plan(1000, 512, 500, 135)[1][2:6] == [135, 135, 1000, 0]
    assert _plan(1000, 512, 500, 136)[1][2:6] == [136, 135, 1008, 8]
    assert _plan(1000, 512, 500, 134)[0] == UNSUPPORTED
    assert _plan(1000, 512, 500, 0)[0] == UNSUPPORTED


def test_knob_off_keeps_one_wave_per_row(knob):
    knob(2)
    assert _plan(1000, 512, 500, 256)[1][:7] == [512, 2, 135, 135, 1000, 0, 0]
    knob(1)
    assert _plan(1000, 512, 500, 256)[1][:7] == [512, 2, 256, 135, 1968, 968, 1]


@pytest.mark.parametrize("d, nd, split", [(128, 1, 0), (256, 1, 0), (260, 2, 1), (512, 2, 1),
                                          (516, 4, 1), (1024, 4, 1)])
def test_vectors_per_lane_and_split(d, nd, split):
    """Rows of one f32x4 per lane (d <= 256) stay whole: the launch keeps today's shape."""
    rc, p = _plan(400, d, 200, 512, k=4)
    assert rc == 0
    assert p[:2] == [256, nd] and p[6] == split
    assert p[2] == (10 + 200 if split else 10 + 100) and p[3] == 110
    assert p[4] == (p[2] - 10) * 4 and p[5] == p[4] - 400


@pytest.mark.parametrize("m, nt", [(60, 64), (64, 64), (65, 128), (200, 256), (367, 512), (512, 512)])
def test_threads_follow_the_unlabelled_rows(m, nt):
    n = 600
    rc, p = _plan(n, 512, n - m, 4096)
    nw = nt // 64
    assert rc == 0 and p[0] == nt
    assert p[3] == 10 + -(-n // nw) and p[2] == 10 + -(-2 * n // nw)
    assert p[4] == (p[2] - 10) * nw >= 2 * n


def test_shapes_that_take_two_launches():
    U = UNSUPPORTED
    assert _plan(1000, 512, 500, 256, eps="auto")[0] == U           # auto eps: the edge pass
    assert _plan(1000, 512, 500, 256, flags=_lib.FLAG_BWD_UNFUSED)[0] == U
    assert _plan(1000, 512, 400, 256)[0] == U                       # m > 512
    assert _plan(1000, 512, 500, 256, aligned=0)[0] == U            # X not 16-B aligned
    assert _plan(4000, 512, 3500, 4096)[0] == U                     # X past 4 MB: chunked gradient
