"""The graph build from caller-supplied neighbour lists without a GPU: the float64 stage reference
of tests/ingest_ref.py pinned to the oracle, the shared list generator, and the C ABI's layout and
argument checks for GLL_FLAG_KNN_GIVEN (include/gll.h)."""
import ctypes as ct

import numpy as np
import pytest
import torch

from graphlearninglayer_amd import GLL as G
from graphlearninglayer_amd import _lib
from graphlearninglayer_amd.synth import seeded_gbar
from oracle import gll_oracle as O
from tests import ingest_ref as IR
from tests import query_ref as Q

GIVEN = _lib.FLAG_KNN_GIVEN


# ------------------------------------------------------------------------------------------------
# the stage reference
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,epsilon", [("ragged", 1.0), ("ragged", "auto"), ("parts2", 1.0),
                                          ("parts2", "auto"), ("hub", 1.0)])
def test_stage_reference_is_the_oracles_graph_on_valid_lists(name, epsilon):
    """Same edges, distances and eps as oracle.graph_from_knn on [self | lists] with float64
    distances.  (hub: row 0 lists itself, which both drop; its repeats move the stage's last
    column, so it is compared at fixed eps, where the last column plays no part.)"""
    X, nbr = IR.case(name)
    st = IR.ingest_ref(X, nbr, epsilon)
    ind = IR.with_self(nbr)
    Xd = X.astype(np.float64)
    dist = np.sqrt(((Xd[:, None, :] - Xd[ind]) ** 2).sum(-1))
    if name == "hub":
        # a repeat is not a valid list for the oracle (coo -> csr sums it): rows that listed row 0
        # twice keep one copy there, as the stage does
        for i in range(nbr.shape[0]):
            rep = np.flatnonzero(nbr[i, 1:] == nbr[i, 0]) + 1
            dist[i, 1 + rep] = 0.0
            ind[i, 1 + rep] = i
    g = O.graph_from_knn(ind, dist, epsilon)
    rows = IR.sym_rows(st)
    got = [(i, j, np.sqrt(v)) for i, r in enumerate(rows) for j, v in sorted(r.items())]
    assert [(a, b) for a, b, _ in got] == list(zip(g.rows.tolist(), g.cols.tolist()))
    np.testing.assert_allclose([v for _, _, v in got], g.dist, rtol=1e-14)
    np.testing.assert_allclose(st.eps, g.eps, rtol=1e-14)


def test_stage_reference_drop_rules():
    X, nbr = IR.case("bad")
    n, km1 = nbr.shape
    st = IR.stage("bad", "auto")
    # counted: -1, n, the repeat in row 2, k - 2 repeats in row 5, the out-of-range last column
    # (+ 1 if row 3 already listed row 7)
    extra = int((nbr[3] == 7).sum()) - 1
    assert st.dropped == 1 + 1 + 1 + (km1 - 1) + 1 + extra
    # padded form: kept entries first, then (i, 0)
    for i in range(n):
        kpt = int(st.kept[i])
        assert (st.knn_idx[i, 1 + kpt:] == i).all() and (st.knn_d2[i, 1 + kpt:] == 0).all()
        assert (st.knn_d2[i, 1:1 + kpt] > 0).all()
        assert len(set(st.knn_idx[i, 1:1 + kpt].tolist())) == kpt
    assert st.kept[0] == km1 - 1 and st.kept[1] == km1 - 1 and st.kept[2] == km1 - 1
    assert st.kept[4] == km1 - 1 and st.kept[5] == 1
    assert 7 not in st.knn_idx[3, 1:].tolist()          # the duplicated point: d2 = 0, silent
    assert st.eps[6] == 0.0 and st.tiny_eps             # a padded last column
    # the caller's order is kept
    want = [j for t, j in enumerate(nbr[2].tolist()) if j not in nbr[2, :t].tolist()]
    assert st.knn_idx[2, 1:1 + len(want)].tolist() == want
    # reverse entries are the transposed kept entries
    for j in range(n):
        assert set(st.reverse[j]) == {i for i in range(n)
                                      if j in st.knn_idx[i, 1:1 + int(st.kept[i])].tolist()}


def test_bounds_come_from_the_query_kernels():
    assert IR.d2_bound(512) == Q.d2_bound(512) == (4 * 16 + 8) * 2.0 ** -24
    assert IR.eps_bound(512) < IR.d2_bound(512)


# ------------------------------------------------------------------------------------------------
# the list generator: one component, finite oracle outputs
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ["plumbing", "ns", "fullysup"])
def test_generated_lists_give_one_connected_graph(config):
    X, Y, nbr, k = IR.layer_case(config)
    n = X.shape[0]
    assert nbr.shape == (n, k - 1)
    assert ((nbr >= 0) & (nbr < n)).all() and (nbr != np.arange(n)[:, None]).all()
    assert all(len(set(r.tolist())) == k - 1 for r in nbr)
    assert IR.components(nbr) == 1 and Y.shape[0] > 0     # one component, with every labelled row
    exact = IR.exact_lists(X, k)
    differ = sum(set(a.tolist()) != set(b.tolist()) for a, b in zip(nbr, exact))
    assert differ > n // 2            # approximate: most rows miss some of their nearest
    assert (nbr != np.sort(nbr, axis=1)).any()


@pytest.mark.parametrize("epsilon", [1.0, "auto"])
@pytest.mark.parametrize("tau", [0.0, 0.07])
def test_oracle_is_finite_on_generated_lists(epsilon, tau):
    X, Y, nbr, k = IR.layer_case("plumbing")
    U, st = O.forward(X, Y, tau, epsilon, k, knn=(IR.with_self(nbr), None))
    g = O.backward(st, seeded_gbar(U.shape[0], U.shape[1]))
    assert np.isfinite(U).all() and np.isfinite(g).all()


# ------------------------------------------------------------------------------------------------
# the library without a GPU
# ------------------------------------------------------------------------------------------------
def _nbytes(n, d, base, C, K, flags=0):
    return _lib.lib().gll_workspace_bytes(ct.byref(G.make_problem(n, d, base, C, K, 0.07, 1.0,
                                                                   flags=flags)))


@pytest.mark.parametrize("shape", [(1000, 512, 500, 10, 10), (1500, 128, 250, 10, 25),
                                   (60250, 128, 250, 10, 50)])
def test_workspace_loses_its_dense_term(shape):
    n, d, base, C, K = shape
    ks = 2 if ((n + 63) // 64 <= 16 and 256 < d <= 512) else 1
    dense = ks * n * ((n + 3) & ~3) * 4 + n * ((d + 63) // 64 * 64) * 4
    whole, given = _nbytes(n, d, base, C, K), _nbytes(n, d, base, C, K, GIVEN)
    assert 0 < given <= whole - dense


def test_workspace_at_half_a_million_rows():
    nb = _nbytes(500_000, 128, 250, 10, 50, GIVEN)
    assert 0 < nb < 8 * 2 ** 30
    assert _nbytes(500_000, 128, 250, 10, 50) > 8 * 2 ** 30      # the searched route: 8 GiB panels


@pytest.mark.parametrize("other", [_lib.FLAG_KNN_PANEL, _lib.FLAG_GRAM_INLINE, _lib.FLAG_D2_F32,
                                   _lib.FLAG_ROW_ORDER_OFF])
def test_search_flags_do_not_combine_with_given_lists(other):
    assert _nbytes(1000, 64, 100, 10, 10, GIVEN | other) == 0
    assert _nbytes(1000, 64, 100, 10, 10, other) > 0
    assert _nbytes(1000, 64, 100, 10, 10, GIVEN | _lib.FLAG_CG_PERCOL) > 0   # a solver flag is fine


def test_entry_points_check_the_flag_and_the_lists_before_any_gpu_call():
    lib = _lib.lib()
    one = ct.c_void_p(16)     # a non-null pointer nobody follows: every check below comes first
    searched = G.make_problem(100, 16, 50, 10, 5, 0.0, 1.0)
    given = G.make_problem(100, 16, 50, 10, 5, 0.0, 1.0, flags=GIVEN)
    g0 = G.make_problem(100, 16, 0, 1, 5, 0.0, 1.0, flags=GIVEN)
    s0 = G.make_problem(100, 16, 0, 1, 5, 0.0, 1.0)
    # the flag is refused by the searched entry points ...
    assert lib.gll_forward(ct.byref(given), one, one, 0, one, one, None) == -1
    assert lib.gll_forward_batched(ct.byref(given), 1, one, one, 0, one, one, None) == -1
    assert lib.gll_graph(ct.byref(g0), one, one, None) == -1
    # ... and required by the lists ones
    assert lib.gll_forward_lists_batched(ct.byref(searched), 1, one, one, one, 0, one, one, None) == -1
    assert lib.gll_graph_lists(ct.byref(s0), one, one, one, None) == -1
    # null lists
    assert lib.gll_forward_lists_batched(ct.byref(given), 1, one, None, one, 0, one, one, None) == -1
    assert lib.gll_graph_lists(ct.byref(g0), one, None, one, None) == -1
    # the search stage's views and routes do not exist on this route
    out = (ct.c_int32 * 16)()
    assert lib.gll_select_route(ct.byref(given), 1, 1, 100, out) == -1
    assert lib.gll_gram_route(ct.byref(given), 1, 1, 256, out) == -1


def test_status_word_is_public_and_free():
    assert _lib.ST_LIST_DROPPED == 13 and _lib.ST_LIST_DROPPED < _lib.ST_NWORDS
    taken = {_lib.ST_TINY_EPS, _lib.ST_FWD_NONCONV, _lib.ST_FWD_ITERS, _lib.ST_BWD_NONCONV,
             _lib.ST_BWD_ITERS, _lib.ST_KNN_RESCAN, _lib.ST_SOLVE_FAILED, _lib.ST_KNN_MERGE,
             _lib.ST_GRID_RESCUED, _lib.ST_GRAD_SPLIT, 8, 9, 11}
    assert _lib.ST_LIST_DROPPED not in taken


# ------------------------------------------------------------------------------------------------
# argument errors of the Python layer: raised on metadata, before any device is asked for
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fn", ["apply", "apply_python", "ce_loss", "margin_loss", "objective"])
def test_neighbors_argument_errors(fn):
    X = torch.zeros(40, 8)
    Y = torch.zeros(10, 3)
    f = getattr(G.LaplaceLearningSparseHard, fn)
    extra = () if fn.startswith("apply") else (torch.zeros(30, dtype=torch.int64),)

    def call(nb):
        if fn == "apply_python":
            return f(X, Y, 0.0, 1.0, 5, nb)
        return f(X, Y, *extra, 0.0, 1.0, 5, False, neighbors=nb) if fn != "objective" else \
            f(X, Y, *extra, 0.0, 1.0, 5, neighbors=nb)

    for bad in (torch.zeros(40, 3, dtype=torch.int64),      # width neither k nor k - 1
                torch.zeros(40, 6, dtype=torch.int64),
                torch.zeros(39, 4, dtype=torch.int64),      # wrong row count
                torch.zeros(40, 4, dtype=torch.float32),    # not integers
                torch.zeros(2, 40, 4, dtype=torch.int64)):  # a batch for a single graph
        with pytest.raises(ValueError, match="neighbors"):
            call(bad)
    with pytest.raises(ValueError, match="neighbors"):
        G.device_graph(X, 5, 1.0, neighbors=torch.zeros(40, 7, dtype=torch.int32))
