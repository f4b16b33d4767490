"""CPU side of the re-rank of caller-supplied candidates (rerank.hip): the float64
reference of tests/rerank_ref.py against query_ref.knn_ref and on the rules it encodes, the pools
the GPU test runs, gll_knn_rerank's argument checks (before any launch) and the front end's
ValueErrors (from the metadata alone)."""
import inspect

import numpy as np
import pytest
import torch

from graphlearninglayer_amd import GLL, _lib, utils
from tests import query_ref as R
from tests import rerank_ref as RR

OK, INVALID, UNSUPPORTED = 0, -1, -2


def test_header_symbol_is_exported_and_bound():
    lib = _lib.lib()
    assert "gll_knn_rerank" in _lib.EXPORTS and hasattr(lib, "gll_knn_rerank")
    assert _lib.RR_KEEP_ORDER == 1 and _lib.RERANK_MAX_C == 512 and _lib.QST_SHORT_ROW == 3
    assert list(inspect.signature(GLL.knn_query).parameters)[-2:] == ["candidates", "keep_order"]
    assert "neighbors" in inspect.signature(GLL.extend).parameters
    assert "neighbors" in inspect.signature(utils.laplace_predict).parameters


@pytest.mark.parametrize("name", ["ragged", "all", "lattice", "sphere", "kmax"])
def test_pool_of_every_column_is_the_search(name):
    Xq, Xdb, k, exact, idx_ref, d2_ref = R.case(name)
    N = Xdb.shape[0]
    rng = np.random.default_rng(5)
    for cand in (np.tile(np.arange(N), (len(Xq), 1)),
                 np.stack([rng.permutation(N) for _ in range(len(Xq))])):
        idx, d2, status = RR.rerank_ref(Xq, Xdb, cand, k)
        assert (idx == idx_ref).all() and (d2 == d2_ref).all() and status == [0, 0, 0, 0]
    # the search's own lists, kept in order: the same lists again
    idx, d2, status = RR.rerank_ref(Xq, Xdb, idx_ref, k, keep_order=True)
    assert (idx == idx_ref).all() and (d2 == d2_ref).all() and status == [0, 0, 0, 0]


@pytest.mark.parametrize("name", ["ragged", "eval_like", "kmax", "all", "one", "offset1000",
                                  "sphere_overflow", "lattice"])
def test_shuffled_pools_hold_the_true_lists(name):
    Xq, Xdb, k, cand = RR.shuffled_pool(name)   # asserts reference == knn_ref while it builds
    assert cand.shape == (len(Xq), min(2 * k, len(Xdb)))
    assert cand.shape[1] < 4 or not (cand == np.sort(cand, axis=1)).all()


def test_validity_padding_and_status_rules():
    Xdb = np.arange(12, dtype=np.float32).reshape(6, 2)
    Xq = np.zeros((4, 2), dtype=np.float32)
    cand = np.array([[5, 5, 2, -1, 6, 2],
                     [RR.I32_MIN, RR.I32_MAX, -1, 6, 7, 8],
                     [3, 1, 1, 1, 1, 1],
                     [4, 3, 2, 1, 0, 0]])
    ok = RR.valid_mask(cand, 6)
    assert ok.tolist() == [[True, False, True, False, False, False], [False] * 6,
                           [True, True, False, False, False, False],
                           [True, True, True, True, True, False]]
    idx, d2, status = RR.rerank_ref(Xq, Xdb, cand, 3)
    assert idx.tolist() == [[2, 5, -1], [-1, -1, -1], [1, 3, -1], [0, 1, 2]]
    assert np.isinf(d2[0, 2]) and np.isinf(d2[1]).all() and d2[3].tolist() == [1.0, 13.0, 41.0]
    assert status == [0, 0, 0, 3]
    # list mode: nothing dropped, a repeat twice, an index out of range kept with +inf
    idx, d2, status = RR.rerank_ref(Xq, Xdb, cand, 6, keep_order=True)
    assert (idx == cand).all()
    assert d2[0].tolist() == [221.0, 221.0, 41.0, np.inf, np.inf, 41.0] and np.isinf(d2[1]).all()
    assert status == [0, 2, 0, 0]
    # exact ties go to the lower index; NaN ranks as +inf
    Xt = np.array([[1, 0], [0, 1], [-1, 0], [np.nan, 0], [0, -1]], dtype=np.float32)
    idx, d2, status = RR.rerank_ref(np.zeros((1, 2), np.float32), Xt, np.array([[4, 3, 2, 1, 0]]), 5)
    assert idx.tolist() == [[0, 1, 2, 4, 3]] and np.isinf(d2[0, 4]) and status == [0, 1, 0, 0]


@pytest.mark.parametrize("name", list(RR.POOLS))
def test_pools_are_well_posed(name):
    Xq, Xdb, cand, k, idx, d2, status, det = RR.pool(name)   # asserts clear set boundaries
    assert det.any() and (det.all() or name not in ("hard", "lattice", "nonfinite"))
    Q, c = cand.shape
    assert cand.dtype == np.int32 and Q <= 64 and len(Xdb) <= 600 and 1 <= k <= c <= 512
    assert idx.shape == (Q, k)
    short = (idx == -1).any(axis=1)
    assert status[3] == short.sum()
    assert (np.isinf(d2[idx == -1])).all()
    if name == "hard":
        assert status == [0, 0, 0, 3] and (idx[3] == -1).all() and (idx[2, 1:] == -1).all()
    if name == "nonfinite":
        assert status == [0, 3, 0, 1]
    if name == "lattice":
        assert (np.diff(d2, axis=1) == 0).sum() > 50 and (d2 == np.round(d2)).all()


def test_argument_limits_without_a_gpu():
    lib = _lib.lib()

    def r(Q=8, N=100, d=16, c=20, k=5, flags=0, null=False, xq=256):
        p = None if null else 256   # never dereferenced: every check comes before any HIP call
        return lib.gll_knn_rerank(Q, N, d, c, k, flags, xq, p, p, p, p, p, None)

    n0 = lib.gll_query_launches()
    for kw in (dict(Q=0), dict(N=0), dict(d=0), dict(k=0), dict(c=4), dict(flags=2), dict(flags=3),
               dict(flags=1), dict(flags=1, c=6, k=5), dict(null=True), dict(xq=258)):
        assert r(**kw) == INVALID, kw
    for kw in (dict(c=513), dict(c=300, k=257), dict(d=4097), dict(N=(2 ** 31 - 1) // 2 + 1),
               dict(Q=(2 ** 31 - 1) // 2 + 1), dict(flags=1, c=257, k=257)):
        assert r(**kw) == UNSUPPORTED, kw
    assert lib.gll_query_launches() == n0     # nothing was launched


def test_front_end_value_errors_come_from_the_metadata():
    Xq, Xdb, P = torch.zeros(6, 4), torch.zeros(30, 4), torch.zeros(30, 3)
    good = torch.zeros(6, 8, dtype=torch.int64)
    for cand in (good.float(), good.bool(), good[:5], good[0], good[:, :4], torch.zeros(6, 513, dtype=torch.int32)):
        with pytest.raises(ValueError):
            GLL.knn_query(Xq, Xdb, 5, candidates=cand)
    with pytest.raises(ValueError):
        GLL.knn_query(Xq, Xdb, 5, candidates=good, keep_order=True)      # c != k
    with pytest.raises(ValueError):
        GLL.knn_query(Xq, Xdb, 5, keep_order=True)                       # no candidates
    with pytest.raises(ValueError):
        GLL.knn_query(Xq, Xdb, 5, candidates=good, flags=_lib.QF_SMALL_PANELS)
    with pytest.raises(TypeError):
        GLL.knn_query(Xq, Xdb, 5, candidates=[[0] * 8] * 6)
    for nb in (good.float(), good.bool(), good[:5], good[0], good[:, :3], torch.zeros(6, 513, dtype=torch.int32)):
        with pytest.raises(ValueError):
            GLL.extend(Xq, Xdb, P, k=6, epsilon=1.0, neighbors=nb)       # kn = 5
    from collections import namedtuple
    fit = namedtuple("Fit", "X P eps epsilon")(Xdb, P, torch.ones(30), 1.0)
    with pytest.raises(ValueError):
        utils.laplace_predict(fit, Xq, knn_num=6, neighbors=good.float())
