"""CPU checks of the query kNN / out-of-sample extension (query.hip): the float64
references of tests/query_ref.py pinned to independent implementations, the derived bounds
evaluated on the GPU test's case table, and the C ABI's argument checks and workspace size
through ctypes (no GPU call)."""
import ctypes as ct

import numpy as np
import pytest
import torch

from graphlearninglayer_amd import _lib
from tests import query_ref as R

OK, INVALID, UNSUPPORTED = 0, -1, -2


def test_header_symbols_are_exported_and_bound():
    lib = _lib.lib()
    for name in ("gll_query_workspace_bytes", "gll_knn_query", "gll_extend", "gll_query_launches"):
        assert name in _lib.EXPORTS
        assert hasattr(lib, name)
    assert _lib.QF_SMALL_PANELS == 1
    assert lib.gll_query_launches() >= 0
    import graphlearninglayer_amd as pkg
    assert callable(pkg.knn_query) and callable(pkg.extend)
    assert "knn_query" in pkg.__all__ and "extend" in pkg.__all__


@pytest.mark.parametrize("name", ["ragged", "eval_like", "wide", "offset1000", "far_query"])
def test_knn_reference_matches_ckdtree_on_tie_free_inputs(name):
    from scipy.spatial import cKDTree
    Xq, Xdb, k, exact, idx, d2 = R.case(name)
    assert not exact
    # the tree ranks the same float64 points (the fp32 inputs widened): same sets where no two
    # distances tie
    dist, ind = cKDTree(Xdb.astype(np.float64)).query(Xq.astype(np.float64), k=k)
    ind = ind.reshape(len(Xq), k)
    assert (np.sort(ind, axis=1) == np.sort(idx, axis=1)).all()
    assert np.allclose(dist.reshape(len(Xq), k) ** 2, d2, rtol=1e-12, atol=0)


def test_case_table_has_no_boundary_ties_unless_exact():
    """The GPU test compares every row's set with no allowance: the inexact cases must have a
    float64 boundary gap far above the noise of a float64 sum in another order, and the exact
    cases must have sums that are exact in fp32 (integers below 2^24)."""
    for name in R.CASES:
        Xq, Xdb, k, exact, idx, d2 = R.case(name)
        assert idx.shape == (len(Xq), k) and k <= min(len(Xdb), 256)
        if exact:
            assert (Xq == np.round(Xq)).all() and (Xdb == np.round(Xdb)).all()
            assert (d2 == np.round(d2)).all() and d2.max() < 2 ** 20
        else:
            gap = R.boundary_gap(Xq, Xdb, k)
            assert gap.min() > R.tie_gap(Xq.shape[1]), (name, gap.min())
    Xq, Xdb, k, _, idx, d2 = R.case("sphere")
    assert (d2 == 14.0).all() and (idx == np.arange(k)[None, :]).all()
    _, Xdb6, _, _, idx6, _ = R.case("sphere_overflow")
    assert len(Xdb6) > 512 and (idx6 == np.arange(10)[None, :]).all()
    Xq, Xdb, k, _, idx, d2 = R.case("lattice")
    assert (d2[:, 0] == 0).all() and (d2[:, 1] == 0).all()      # the row and its twin
    assert (idx[:, 0] % 2 == 0).all() and (idx[:, 1] == idx[:, 0] + 1).all()
    assert (Xdb[0::2] == Xdb[1::2]).all()


def test_far_query_cannot_be_certified():
    """The far query's boundary gap is below what the Gram bound resolves at its distance from
    the centre: the certificate must fail there (the GPU test expects status[0] > 0)."""
    Xq, Xdb, k, _, idx, d2 = R.case("far_query")
    d = Xq.shape[1]
    D = np.sort(R.dist2(Xq[-1:], Xdb), axis=1)[0]
    ai = np.linalg.norm(Xq[-1].astype(np.float64) - Xdb[0].astype(np.float64))
    assert R.gram_err(d) * (2 * ai + np.sqrt(D[k - 1])) ** 2 > D[-1] - D[k - 1]


def test_bounds_are_what_the_header_states():
    assert R.d2_bound(128) == (4 * 4 + 8) * 2.0 ** -24
    assert R.d2_bound(7) == 12 * 2.0 ** -24 and R.d2_bound(130) == 28 * 2.0 ** -24
    assert R.gram_err(128) == 144 * 2.0 ** -24
    # far below the split-bf16 Gram's 2^-13
    assert R.gram_err(4096) < 2.0 ** -11.9 and R.gram_err(128) < 2.0 ** -16


def test_d2_bound_holds_for_an_fp32_emulation_of_the_kernel_order():
    """The kernel's summation order emulated in numpy float32 (lane sub: features 4 sub + 32 u +
    t in ascending order, then the 3-level butterfly) stays within d2_bound of float64."""
    rng = np.random.default_rng(0)
    for d in (7, 128, 130, 517):
        a = rng.standard_normal((50, d)).astype(np.float32)
        b = rng.standard_normal((50, d)).astype(np.float32)
        lanes = np.zeros((50, 8), dtype=np.float32)
        for f in range(d):
            sub = (f // 4) % 8
            df = (a[:, f] - b[:, f]).astype(np.float32)
            # fmaf: one rounding of df * df + acc
            lanes[:, sub] = (df.astype(np.float64) * df.astype(np.float64)
                             + lanes[:, sub].astype(np.float64)).astype(np.float32)
        v = lanes
        for off in (1, 2, 4):
            v = (v + v[:, np.arange(8) ^ off]).astype(np.float32)
        exact = ((a.astype(np.float64) - b.astype(np.float64)) ** 2).sum(axis=1)
        assert (np.abs(v[:, 0].astype(np.float64) - exact) <= R.d2_bound(d) * exact).all()


@pytest.mark.parametrize("name", list(R.EXT_CASES))
def test_extension_reference_matches_the_dense_closed_form(name):
    Xq, Xdb, P, k, epsilon, eps_db, Uq, lab, bound = R.ext_case(name)
    dense = R.extend_dense(Xq, Xdb, P, k - 1, epsilon, eps_db)
    assert np.allclose(dense, Uq, rtol=1e-12, atol=1e-14)
    assert (R.label_ref(dense) == lab).all()


@pytest.mark.parametrize("name", list(R.EXT_CASES))
def test_extension_cases_have_a_top2_gap_above_twice_the_bound(name):
    """So the GPU label comparison excuses zero rows."""
    Xq, Xdb, P, k, epsilon, eps_db, Uq, lab, bound = R.ext_case(name)
    assert 0 < bound < 1e-2, bound
    top = np.sort(Uq, axis=1)
    assert ((top[:, -1] - top[:, -2]) > 2 * bound).all()
    assert np.isfinite(Uq).all()


def test_label_rule():
    U = np.array([[0.1, 0.7, 0.7], [np.nan, 0.2, 0.1], [np.nan, np.nan, np.nan], [np.nan, -1.0, np.nan]])
    assert R.label_ref(U).tolist() == [1, 1, 0, 1]


def test_argument_limits_without_a_gpu():
    lib = _lib.lib()
    nb = lib.gll_query_workspace_bytes

    def q(Q=8, N=100, d=16, k=5, flags=0, null=False):
        p = None if null else 256   # never dereferenced: every check comes before any HIP call
        return lib.gll_knn_query(Q, N, d, k, flags, p, p, p, p, p, p, None)

    assert nb(8, 100, 16, 5, 0) > 0
    for kw in (dict(Q=0), dict(N=0), dict(d=0), dict(k=0), dict(k=101), dict(flags=2), dict(null=True)):
        assert q(**kw) == INVALID, kw
    for kw in (dict(k=257, N=1000), dict(d=4097), dict(N=(2 ** 31 - 1) // 2 + 1)):
        assert q(**kw) == UNSUPPORTED, kw
        args = dict(Q=8, N=100, d=16, k=5, flags=0)
        args.update(kw)
        assert nb(args["Q"], args["N"], args["d"], args["k"], args["flags"]) == 0
    for bad in ((0, 100, 16, 5, 0), (8, 0, 16, 5, 0), (8, 100, 0, 5, 0), (8, 100, 16, 0, 0),
                (8, 100, 16, 101, 0), (8, 100, 16, 5, 2)):
        assert nb(*bad) == 0
    assert nb(8, 256, 4096, 256, 1) > 0 and nb(1, 1, 1, 1, 0) > 0      # the limits themselves
    assert nb(1, (2 ** 31 - 1) // 2, 1, 1, 0) > 0
    # a misaligned feature pointer
    assert lib.gll_knn_query(8, 100, 16, 5, 0, 258, 256, 256, 256, 256, 256, None) == INVALID

    def e(Q=8, N=100, kn=5, C=3, eps=1.0, eps_db=None, null=False):
        p = None if null else 256
        return lib.gll_extend(Q, N, kn, C, p, p, p, eps_db, ct.c_float(eps), p, p, p, None)

    for kw in (dict(Q=0), dict(N=0), dict(kn=0), dict(C=0), dict(null=True), dict(eps=0.0),
               dict(eps=-1.0), dict(eps=float("nan"))):
        assert e(**kw) == INVALID, kw
    for kw in (dict(kn=257), dict(C=257), dict(N=(2 ** 31 - 1) // 2 + 1)):
        assert e(**kw) == UNSUPPORTED, kw


def test_workspace_is_monotone_up_to_the_panel_cap_and_constant_past_it():
    lib = _lib.lib()
    N, d, k = 50250, 128, 50
    ld = (N + 3) & ~3
    cap = ((128 << 20) // (4 * ld)) // 64 * 64
    assert cap == 640 and cap % 64 == 0
    sizes = [lib.gll_query_workspace_bytes(Q, N, d, k, 0) for Q in (1, 2, 63, 64, 65, cap - 1, cap)]
    assert all(a < b for a, b in zip(sizes, sizes[1:]))
    past = {lib.gll_query_workspace_bytes(Q, N, d, k, 0) for Q in (cap, cap + 1, 4096, 10_000, 10 ** 7)}
    assert past == {sizes[-1]}
    # the panel, two norm vectors and alignment: never Q x N
    assert cap * ld * 4 <= sizes[-1] <= cap * ld * 4 + 4 * (N + cap) + 3 * 256
    assert sizes[-1] <= (128 << 20) + 4 * (N + cap) + 3 * 256
    small = [lib.gll_query_workspace_bytes(Q, N, d, k, _lib.QF_SMALL_PANELS) for Q in (1, 64, 65, 4096)]
    assert small[0] < small[1] == small[2] == small[3] == 64 * ld * 4 + ((4 * N + 255) & ~255) + 256
    # a database so small that the byte cap allows more rows than the row cap
    assert lib.gll_query_workspace_bytes(2 ** 21, 8, 4, 2, 0) == \
        lib.gll_query_workspace_bytes(2 ** 20, 8, 4, 2, 0)


def test_front_end_rejects_bad_arguments_before_the_device():
    from graphlearninglayer_amd import GLL
    Xq, Xdb = torch.zeros(3, 4), torch.zeros(10, 4)
    for k in (0, 11, 257, 2.5):
        with pytest.raises(ValueError):
            GLL.knn_query(Xq, Xdb, k)
    with pytest.raises(ValueError):
        GLL.knn_query(torch.zeros(3, 5), Xdb, 2)
    with pytest.raises(ValueError):
        GLL.knn_query(torch.zeros(3), Xdb, 2)
    with pytest.raises(ValueError):
        GLL.knn_query(Xq, torch.zeros(0, 4), 1)
    with pytest.raises(ValueError):
        GLL.knn_query(Xq, Xdb, 2, flags=4)
    P = torch.zeros(10, 3)
    with pytest.raises(ValueError, match="eps_db"):
        GLL.extend(Xq, Xdb, P, k=5, epsilon="auto")
    with pytest.raises(ValueError):
        GLL.extend(Xq, Xdb, P, k=5, epsilon="auto", eps_db=torch.ones(9))
    for k in (1, 12, 258):
        with pytest.raises(ValueError):
            GLL.extend(Xq, Xdb, P, k=k, epsilon=1.0)
    with pytest.raises(ValueError):
        GLL.extend(Xq, Xdb, torch.zeros(9, 3), k=5, epsilon=1.0)
    with pytest.raises(ValueError):
        GLL.extend(Xq, Xdb, torch.zeros(10, 257), k=5, epsilon=1.0)
