"""The two scopes of tests/abi.py for process-wide state: knobs (no GPU needed) and launches."""
import ctypes as ct

import pytest
import torch

from graphlearninglayer_amd import GLL
from graphlearninglayer_amd import _lib as L
from tests import abi as A


def _select_route(n=520, d=64, K=10):
    """gll_select_route of one 520 x 64 graph: the automatic form is the latency one, so
    GLL_KNOB_SEL_FORM = 2 (occupancy) changes the row of the table it reports."""
    p = GLL.make_problem(n, d, 0, 1, K, 0.0, "auto")
    out = (ct.c_int32 * 12)()
    assert L.lib().gll_select_route(ct.byref(p), 1, 1, n, out) == 0
    return list(out)


def test_knobs_restore_after_an_exception():
    auto = _select_route()
    with A.knobs({L.KNOB_SEL_FORM: 2}):
        forced = _select_route()
    assert forced != auto and _select_route() == auto
    with pytest.raises(ZeroDivisionError):
        with A.knobs({L.KNOB_SEL_FORM: 2}):
            assert _select_route() == forced
            1 / 0
    assert _select_route() == auto


@pytest.mark.gpu
def test_launches_counts_its_own_block_not_pairs_left_unread():
    """A K_CG bracket enabled by hand and never read leaves its pairs pending past the disable;
    launches(K_CG) drops them and counts the forward inside it alone -- as many CG launches as a
    clean bracket of the same call.  The smallest graph the layer takes."""
    A.need_gpu()
    from graphlearninglayer_amd.synth import one_hot, synth
    X, lab = synth(3, 9, 16, r=1.0, seed=12)
    run = A.Run(X, one_hot(lab[:3]), 10, 0.07, 1.0)
    with A.launches(L.K_CG) as clean:
        run.forward()
    assert clean[0] >= 1

    def unread_bracket():
        L.prof_enable(L.K_CG, 1)
        try:
            run.forward()
            torch.cuda.synchronize()
        finally:
            L.prof_enable(L.K_CG, 0)

    unread_bracket()
    assert L.prof_read(L.K_CG)[1] == clean[0]      # the premise: the pairs outlive the disable
    unread_bracket()
    with A.launches(L.K_CG) as got:
        run.forward()
    assert got == clean
