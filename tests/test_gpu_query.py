"""The query kNN and the out-of-sample extension on the GPU (query.hip) against
the float64 references and derived bounds of tests/query_ref.py: exact sets with no near-tie
allowance, the returned fp32 distances within their bound, bitwise repeatability and independence
of panels, batch and alignment, non-finite input, the extension within its bound with every label
equal, the launch budget and the memory contract (never a Q x N array)."""
import ctypes as ct

import numpy as np
import pytest
import torch

from tests import abi as A
from tests import query_ref as R

pytestmark = pytest.mark.gpu


def _L():
    from graphlearninglayer_amd import _lib
    return _lib


def _G():
    from graphlearninglayer_amd import GLL
    return GLL


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    A.need_gpu()


def _query(Xq, Xdb, k, flags=0):
    idx, d2, st = _G().knn_query(A.dev(Xq), A.dev(Xdb), k, flags=flags, return_status=True)
    return idx.cpu().numpy(), d2.cpu().numpy(), st.cpu().numpy()


def _raw_query(Xq_t, Xdb_t, k, flags=0):
    """gll_knn_query on the tensors' own storage (the front end would re-align them)."""
    L = _L()
    Q, d = Xq_t.shape
    N = Xdb_t.shape[0]
    idx = torch.empty((Q, k), dtype=torch.int32, device="cuda")
    d2 = torch.empty((Q, k), dtype=torch.float32, device="cuda")
    st = torch.zeros(4, dtype=torch.int32, device="cuda")
    ws = torch.empty(L.lib().gll_query_workspace_bytes(Q, N, d, k, flags), dtype=torch.uint8, device="cuda")
    L.check(L.lib().gll_knn_query(Q, N, d, k, flags, Xq_t.data_ptr(), Xdb_t.data_ptr(), idx.data_ptr(),
                                  d2.data_ptr(), st.data_ptr(), ws.data_ptr(),
                                  torch.cuda.current_stream().cuda_stream), "gll_knn_query")
    return idx.cpu().numpy(), d2.cpu().numpy(), st.cpu().numpy()


def _check_lists(idx, d2, Xq, Xdb, k, idx_ref, d2_ref):
    N, d = Xdb.shape
    assert idx.shape == (len(Xq), k) and d2.shape == (len(Xq), k)
    assert idx.min() >= 0 and idx.max() < N
    # the set: exactly the reference's, every row, no allowance
    assert (np.sort(idx, axis=1) == np.sort(idx_ref, axis=1)).all()
    # the list is ordered by (returned d2, idx)
    assert (np.diff(d2, axis=1) >= 0).all()
    same = np.diff(d2, axis=1) == 0
    assert (np.diff(idx, axis=1)[same] > 0).all()
    # returned d2 against float64, entry by entry (matched through the index)
    o, orf = np.argsort(idx, axis=1), np.argsort(idx_ref, axis=1)
    got = np.take_along_axis(d2, o, axis=1).astype(np.float64)
    ref = np.take_along_axis(d2_ref, orf, axis=1)
    err = np.abs(got - ref)
    print("max d2 err / bound:", float((err / np.maximum(R.d2_bound(d) * ref, 1e-300)).max()))
    assert (err <= R.d2_bound(d) * ref).all()


@pytest.mark.parametrize("name", list(R.CASES))
def test_knn_query_exact_against_float64(name):
    Xq, Xdb, k, exact, idx_ref, d2_ref = R.case(name)
    idx, d2, st = _query(Xq, Xdb, k)
    print(name, "status", st.tolist())
    _check_lists(idx, d2, Xq, Xdb, k, idx_ref, d2_ref)
    assert st[_L().QST_NONFINITE] == 0
    if exact:   # every sum is exact: the lists are the reference's, bit for bit
        assert (idx == idx_ref).all()
        assert d2.tobytes() == d2_ref.astype(np.float32).tobytes()
    if name == "sphere":
        assert (d2 == np.float32(14.0)).all() and (idx == np.arange(k)[None, :]).all()
    if name in ("far_query", "sphere_overflow"):   # certificate failure / list overflow: rescan
        assert st[_L().QST_RESCAN] > 0
    if name in ("ragged", "eval_like", "offset100", "offset1000"):   # centring: certified rows
        assert st[_L().QST_RESCAN] == 0


@pytest.mark.parametrize("name", ["ragged", "offset100", "wide", "sphere_overflow"])
def test_small_panels_are_bitwise_the_single_panel(name):
    Xq, Xdb, k, *_ = R.case(name)
    a = _query(Xq, Xdb, k)
    b = _query(Xq, Xdb, k, flags=_L().QF_SMALL_PANELS)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert a[2].tolist() == b[2].tolist()


def test_row_of_a_call_equals_the_call_on_that_row_and_runs_repeat():
    Xq, Xdb, k, *_ = R.case("offset100")
    idx, d2, _ = _query(Xq, Xdb, k)
    again = _query(Xq, Xdb, k)
    assert idx.tobytes() == again[0].tobytes() and d2.tobytes() == again[1].tobytes()
    for q in (0, 33, 69):
        i1, f1, _ = _query(Xq[q:q + 1], Xdb, k)
        assert i1.tobytes() == idx[q:q + 1].tobytes() and f1.tobytes() == d2[q:q + 1].tobytes()


@pytest.mark.parametrize("name", ["eval_like", "ragged"])
def test_misaligned_storage_gives_the_aligned_bits(name):
    Xq, Xdb, k, *_ = R.case(name)
    aq, adb = A.dev(Xq), A.dev(Xdb)
    assert aq.data_ptr() % 16 == 0 and adb.data_ptr() % 16 == 0
    ref = _raw_query(aq, adb, k)

    def shifted(a):
        buf = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
        v = buf[1:].view(a.shape)
        v.copy_(torch.from_numpy(np.array(a, order="C")))
        assert v.data_ptr() % 16 == 4
        return v

    for mq, mdb in ((shifted(Xq), adb), (aq, shifted(Xdb)), (shifted(Xq), shifted(Xdb))):
        got = _raw_query(mq, mdb, k)
        assert got[0].tobytes() == ref[0].tobytes() and got[1].tobytes() == ref[1].tobytes()


def test_self_query_matches_the_graph_build():
    n, d, K = 500, 32, 10
    X = np.random.default_rng(21).standard_normal((n, d)).astype(np.float32)
    assert R.boundary_gap(X, X, K).min() > R.tie_gap(d)
    g = _G().device_graph(A.dev(X), K)
    gi, gd = g["knn_idx"].cpu().numpy().astype(np.int64), g["knn_d2"].cpu().numpy().astype(np.float64)
    idx, d2, _ = _query(X, X, K)
    o, og = np.argsort(idx, axis=1), np.argsort(gi, axis=1)
    assert (np.take_along_axis(idx, o, axis=1) == np.take_along_axis(gi, og, axis=1)).all()
    a = np.take_along_axis(d2, o, axis=1).astype(np.float64)
    b = np.take_along_axis(gd, og, axis=1)
    # the graph build's fp32 sums carry (d / 8 + 3) 2^-24 relative (select.hip), ours d2_bound
    assert (np.abs(a - b) <= (R.d2_bound(d) + (d / 8 + 3) * R.U32) * np.maximum(a, b)).all()


def test_non_finite_features_keep_every_index_in_range():
    L = _L()
    rng = np.random.default_rng(31)
    Xq = rng.standard_normal((9, 12)).astype(np.float32)
    Xdb = rng.standard_normal((600, 12)).astype(np.float32)
    Xq[2, 3] = np.inf
    Xq[5, 0] = np.nan
    bad_db = Xdb.copy()
    bad_db[17, 4] = np.nan
    bad_db[40, 1] = -np.inf
    bad_centre = Xdb.copy()
    bad_centre[0, 0] = np.nan     # every centred row is NaN: more than 512 columns tie
    for q, db, k in ((Xq, Xdb, 7), (Xq[:2], bad_db, 7), (Xq, bad_centre, 70), (Xq, bad_db, 256)):
        idx, d2, st = _query(q, db, k)
        assert idx.min() >= 0 and idx.max() < len(db)
        assert st[L.QST_NONFINITE] >= 1
    idx, d2, st = _query(Xq, Xdb, 7)
    assert st[L.QST_NONFINITE] == 2
    clean = [0, 1, 3, 4, 6, 7, 8]   # the finite rows are untouched by their neighbours in the call
    ref = R.knn_ref(Xq[clean], Xdb, 7)[0]
    assert (np.sort(idx[clean], axis=1) == np.sort(ref, axis=1)).all()
    # the extension gathers through whatever indices it is given without following a bad one
    P = torch.rand(600, 3, device="cuda")
    bad_idx = torch.tensor([[0, 5, -1], [599, 600, 3]], dtype=torch.int32, device="cuda")
    dd = torch.ones(2, 3, device="cuda")
    Uq = torch.zeros(2, 3, dtype=torch.float64, device="cuda")
    lab = torch.zeros(2, dtype=torch.int64, device="cuda")
    st = torch.zeros(4, dtype=torch.int32, device="cuda")
    L.check(L.lib().gll_extend(2, 600, 3, 3, bad_idx.data_ptr(), dd.data_ptr(), P.data_ptr(), None,
                               ct.c_float(1.0), Uq.data_ptr(), lab.data_ptr(), st.data_ptr(),
                               torch.cuda.current_stream().cuda_stream), "gll_extend")
    assert torch.isnan(Uq).all() and st.cpu()[L.QST_ZERO_SUM] == 2 and lab.cpu().tolist() == [0, 0]


@pytest.mark.parametrize("name", list(R.EXT_CASES))
def test_extend_within_the_derived_bound_and_every_label_equal(name):
    Xq, Xdb, P, k, epsilon, eps_db, Uq_ref, lab_ref, bound = R.ext_case(name)
    Uq, lab, st = _G().extend(A.dev(Xq), A.dev(Xdb), A.dev(P), k=k, epsilon=epsilon,
                              eps_db=None if eps_db is None else A.dev(eps_db), return_status=True)
    assert Uq.dtype == torch.float64 and lab.dtype == torch.int64
    err = np.abs(Uq.cpu().numpy() - Uq_ref).max()
    print(name, "max |Uq - ref|", err, "bound", bound)
    assert err <= bound
    assert (lab.cpu().numpy() == lab_ref).all()     # zero rows excused
    assert st.cpu()[_L().QST_ZERO_SUM] == 0


def test_extend_zero_weight_sum_is_nan_and_counted():
    Xq, Xdb, P, k, *_ = R.ext_case("fixed")
    Uq, lab, st = _G().extend(A.dev(Xq), A.dev(Xdb), A.dev(P), k=k, epsilon=1e-3, return_status=True)
    assert torch.isnan(Uq).all() and (lab == 0).all()
    assert st.cpu()[_L().QST_ZERO_SUM] == len(Xq)
    Uq0, lab0 = _G().extend(A.dev(Xq[:0]), A.dev(Xdb), A.dev(P), k=k, epsilon=1.0)
    assert Uq0.shape == (0, P.shape[1]) and lab0.shape == (0,)
    i0, f0 = _G().knn_query(A.dev(Xq[:0]), A.dev(Xdb), 3)
    assert i0.shape == (0, 3) and i0.dtype == torch.int64 and f0.shape == (0, 3) and i0.is_cuda


@pytest.mark.parametrize("epsilon", ["auto", 2.0])
def test_laplace_predict_is_extend_on_the_fit(epsilon):
    from graphlearninglayer_amd import utils
    rng = np.random.default_rng(41)
    C, base, n, d, kk = 4, 20, 300, 16, 10
    cen = rng.standard_normal((C, d)) * 3.0
    lab = np.concatenate([np.arange(base) % C, rng.integers(0, C, size=n - base)])
    X = (cen[lab] + 0.5 * rng.standard_normal((n, d))).astype(np.float32)
    Xq = (cen[np.arange(40) % C] + 0.5 * rng.standard_normal((40, d))).astype(np.float32)
    fit = utils.laplace_fit(X, lab[:base], knn_num=kk, epsilon=epsilon)
    assert fit.X.is_cuda and fit.X.dtype == torch.float32 and fit.X.shape == (n, d)
    assert fit.P.is_cuda and fit.P.dtype == torch.float32 and fit.P.shape == (n, C)
    assert fit.eps.shape == (n,)
    U = utils.laplace(X, lab[:base], knn_num=kk, epsilon=epsilon)
    # a second run of the same solve (its float64 degree sums use atomics: last bits may differ)
    assert np.allclose(fit.P[base:].cpu().numpy(), U, rtol=0, atol=1e-6)
    assert (fit.P[:base].cpu().numpy() == np.eye(C, dtype=np.float32)[lab[:base]]).all()
    Uq, labels = utils.laplace_predict(fit, Xq, knn_num=kk)
    Ue, le = _G().extend(A.dev(Xq), fit.X, fit.P, k=kk, epsilon=epsilon, eps_db=fit.eps)
    assert Uq.cpu().numpy().tobytes() == Ue.cpu().numpy().tobytes() and (labels == le).all()
    assert (labels.cpu().numpy() == np.arange(40) % C).mean() > 0.9
    acc = utils.gl_accuracy_inductive(X[:base], lab[:base], Xq, np.arange(40) % C,
                                      unlabeled_data=X[base:], epsilon=epsilon, knn_num=kk)
    assert acc > 90.0


def test_launches_per_call():
    """three launches a panel (norms, Gram, select), one for the extension."""
    lib = _L().lib()
    Xq, Xdb, k, *_ = R.case("offset100")     # 70 rows: one panel, or two of 64
    aq, adb = A.dev(Xq), A.dev(Xdb)
    n0 = lib.gll_query_launches()
    _G().knn_query(aq, adb, k)
    n1 = lib.gll_query_launches()
    _G().knn_query(aq, adb, k, flags=_L().QF_SMALL_PANELS)
    n2 = lib.gll_query_launches()
    _G().extend(aq, adb, torch.rand(len(Xdb), 3, device="cuda"), k=k, epsilon=1.0)
    n3 = lib.gll_query_launches()
    assert (n1 - n0, n2 - n1, n3 - n2) == (3, 6, 4)


def test_evaluation_shape_stays_within_its_workspace():
    Q, N, d, k = 4096, 50250, 128, 50
    rng = np.random.default_rng(51)
    cen = rng.standard_normal((10, d)).astype(np.float32)
    Xdb = cen[rng.integers(0, 10, size=N)] + 0.3 * rng.standard_normal((N, d)).astype(np.float32)
    Xq = cen[rng.integers(0, 10, size=Q)] + 0.3 * rng.standard_normal((Q, d)).astype(np.float32)
    aq, adb = A.dev(Xq), A.dev(Xdb)
    ws = _L().lib().gll_query_workspace_bytes(Q, N, d, k, 0)
    assert ws < 140 * 2 ** 20 < Q * N * 4
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    idx, d2 = _G().knn_query(aq, adb, k)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    outputs = Q * k * (8 + 4)                 # idx int64, d2 float32
    staging = Q * k * 4 + 512 + 4096          # the kernel's int32 idx, the status words, rounding
    print("peak above inputs", peak, "workspace", ws)
    assert peak <= ws + outputs + staging
    rows = rng.choice(Q, size=64, replace=False)
    ref_idx, ref_d2 = R.knn_ref(Xq[rows], Xdb, k)
    assert R.boundary_gap(Xq[rows], Xdb, k).min() > R.tie_gap(d)
    _check_lists(idx[rows].cpu().numpy(), d2[rows].cpu().numpy(), Xq[rows], Xdb, k, ref_idx, ref_d2)
