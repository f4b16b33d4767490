"""The re-rank of caller-supplied candidates on the GPU (rerank.hip) and the
extension on lists and pools built on it: gll_knn_rerank against the float64 reference of
tests/rerank_ref.py on hard pools (no tolerance on selection, the returned distances within
query_ref.d2_bound, the status words equal), bitwise against the search (lists kept, shuffled
pools, extend(neighbors=) in Uq, labels and every gradient), moved queries against extend_ref and
float64 autograd, row independence, repeatability, alignment and the launch counts."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import abi as A
from tests import query_ref as R
from tests import rerank_ref as RR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY = {}


def _L():
    from graphlearninglayer_amd import _lib
    return _lib


def _G():
    from graphlearninglayer_amd import GLL
    return GLL


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    A.need_gpu()
    yield
    try:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "xl01_parity.json"), "w") as fh:
            json.dump(PARITY, fh, indent=1, sort_keys=True)
    except OSError:
        pass


def _shifted(a):
    """The array on the device, its base one float past a 16-B boundary: scalar loads."""
    buf = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
    v = buf[1:].view(a.shape)
    v.copy_(torch.from_numpy(np.array(a, order="C")))
    assert v.data_ptr() % 16 == 4
    return v


def _raw(xq, xdb, cand, k, flags=0):
    """gll_knn_rerank on the tensors' own storage (the front end would re-align the features)."""
    L = _L()
    Q, d = xq.shape
    idx = torch.full((Q, k), -7, dtype=torch.int32, device="cuda")
    d2 = torch.full((Q, k), -7.0, dtype=torch.float32, device="cuda")
    st = torch.zeros(4, dtype=torch.int32, device="cuda")
    L.check(L.lib().gll_knn_rerank(Q, xdb.shape[0], d, cand.shape[1], k, flags, xq.data_ptr(),
                                   xdb.data_ptr(), cand.data_ptr(), idx.data_ptr(), d2.data_ptr(),
                                   st.data_ptr(), torch.cuda.current_stream().cuda_stream),
            "gll_knn_rerank")
    return idx.cpu().numpy(), d2.cpu().numpy(), st.cpu().numpy().tolist()


def _check_d2(d2, d2_ref, d):
    fin = np.isfinite(d2_ref)
    assert not np.isfinite(d2[~fin]).any()       # +inf or NaN where the reference ranks +inf
    err = np.abs(d2[fin].astype(np.float64) - d2_ref[fin])
    print("max d2 err / bound:", float((err / np.maximum(R.d2_bound(d) * d2_ref[fin], 1e-300)).max(initial=0)))
    assert (err <= R.d2_bound(d) * d2_ref[fin]).all()


# ------------------------------------------------------------------------------------------
# 1. the kernel against the float64 reference
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(RR.POOLS))
def test_pool_mode_against_float64(name):
    Xq, Xdb, cand, k, idx_ref, d2_ref, st_ref, det = RR.pool(name)
    d = Xdb.shape[1]
    xq, xdb, cd = A.dev(Xq), A.dev(Xdb), A.dev(cand)
    assert xq.data_ptr() % 16 == 0 and xdb.data_ptr() % 16 == 0
    idx, d2, st = _raw(xq, xdb, cd, k)
    print(name, "status", st, "reference", st_ref)
    # selection: the reference's sets, every row, no allowance; invalid entries never chosen
    assert (np.sort(idx, axis=1) == np.sort(idx_ref, axis=1)).all()
    assert ((idx == -1) == (idx_ref == -1)).all()            # the padding sits at the tail
    assert (idx[det] == idx_ref[det]).all()                  # and the reference's order
    # every list is in (returned d2, index) order, NaN as +inf
    key = np.where(np.isnan(d2), np.inf, d2)
    real = idx[:, 1:] != -1
    assert (key[:, 1:] >= key[:, :-1]).all()
    assert (np.diff(idx, axis=1)[(key[:, 1:] == key[:, :-1]) & real] > 0).all()
    o, orf = np.argsort(idx, axis=1, kind="stable"), np.argsort(idx_ref, axis=1, kind="stable")
    _check_d2(np.take_along_axis(d2, o, axis=1), np.take_along_axis(d2_ref, orf, axis=1), d)
    assert np.isposinf(d2[idx == -1]).all()
    assert st == st_ref
    # scalar loads (a base one float off) give the vector loads' bits; two runs are equal
    for mq, mdb in ((_shifted(Xq), xdb), (xq, _shifted(Xdb)), (_shifted(Xq), _shifted(Xdb)), (xq, xdb)):
        again = _raw(mq, mdb, cd, k)
        assert again[0].tobytes() == idx.tobytes() and again[1].tobytes() == d2.tobytes()
        assert again[2] == st


@pytest.mark.parametrize("name", list(RR.POOLS))
def test_list_mode_against_float64_and_the_pool_bits(name):
    Xq, Xdb, cand, k, *_ = RR.pool(name)
    k = min(k, 256)
    d, N = Xdb.shape[1], Xdb.shape[0]
    lst = np.ascontiguousarray(cand[:, :k])
    idx_ref, d2_ref, st_ref = RR.rerank_ref(Xq, Xdb, lst, k, keep_order=True)
    xq, xdb = A.dev(Xq), A.dev(Xdb)
    idx, d2, st = _raw(xq, xdb, A.dev(lst), k, _L().RR_KEEP_ORDER)
    assert (idx == lst).all()                     # as they are: repeats and indices out of range
    _check_d2(d2, d2_ref, d)
    assert np.isposinf(d2[(lst < 0) | (lst >= N)]).all()
    assert st == st_ref
    again = _raw(_shifted(Xq), _shifted(Xdb), A.dev(lst), k, _L().RR_KEEP_ORDER)
    assert again[0].tobytes() == idx.tobytes() and again[1].tobytes() == d2.tobytes()
    # a pair (q, j) has one distance, whichever mode and slot computed it
    pi, pd, _ = _raw(xq, xdb, A.dev(cand), min(cand.shape[1], 256))
    for q in range(len(Xq)):
        by_j = {int(j): f.tobytes() for j, f in zip(pi[q], pd[q]) if j >= 0}
        for j, f in zip(lst[q], d2[q]):
            if int(j) in by_j:
                assert by_j[int(j)] == f.tobytes()


def test_k_may_exceed_the_database():
    """N = 1, 2 with k up to 256: every row is short, the tail is (-1, +inf)."""
    for N, c, k in ((1, 512, 256), (2, 9, 9), (2, 256, 256)):
        Xq, Xdb, cand = RR._pool(100 + N, 5, N, 4, c, lo=-1)
        idx_ref, d2_ref, st_ref = RR.rerank_ref(Xq, Xdb, cand, k)
        idx, d2, st = _raw(A.dev(Xq), A.dev(Xdb), A.dev(cand), k)
        assert (idx == idx_ref).all() and st == st_ref and st[3] == 5
        _check_d2(d2, d2_ref, 4)


# ------------------------------------------------------------------------------------------
# 2. bitwise against the search
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ragged", "eval_like", "kmax", "all", "one", "offset1000",
                                  "sphere_overflow", "lattice"])
def test_lists_and_shuffled_pools_return_the_search_bits(name):
    Xq, Xdb, k, cand = RR.shuffled_pool(name)
    xq, xdb = A.dev(Xq), A.dev(Xdb)
    idx, d2 = _G().knn_query(xq, xdb, k)
    li, ld, ls = _G().knn_query(xq, xdb, k, candidates=idx, keep_order=True, return_status=True)
    assert li.dtype == torch.int64 and ld.dtype == torch.float32
    assert A.raw_bytes(li) == A.raw_bytes(idx) and A.raw_bytes(ld) == A.raw_bytes(d2) and ls.cpu().tolist() == [0, 0, 0, 0]
    for pool in (A.dev(cand), torch.from_numpy(np.array(cand)).int()):    # int64 on the device, int32 on the host
        pi, pd, ps = _G().knn_query(xq, xdb, k, candidates=pool, return_status=True)
        assert A.raw_bytes(pi) == A.raw_bytes(idx) and A.raw_bytes(pd) == A.raw_bytes(d2) and ps.cpu().tolist() == [0, 0, 0, 0]


def _ext_inputs(name, grad):
    Xq, Xdb, P, k, epsilon, eps_db, *_ = R.ext_case(name)
    xq, xdb, p = (A.dev(a).requires_grad_(grad) for a in (Xq, Xdb, P))
    eps = epsilon
    if epsilon != "auto" and grad:
        eps = torch.tensor(float(epsilon), dtype=torch.float64, device="cuda", requires_grad=True)
    return xq, xdb, p, eps, None if eps_db is None else A.dev(eps_db), k


@pytest.mark.parametrize("name", list(R.EXT_CASES))
def test_extend_on_the_search_lists_is_extend(name):
    gU = A.dev(np.random.default_rng(7).standard_normal(R.ext_case(name)[6].shape))

    def run(neighbors):
        xq, xdb, p, eps, e, k = _ext_inputs(name, True)
        Uq, lab, st = _G().extend(xq, xdb, p, k=k, epsilon=eps, eps_db=e, return_status=True,
                                  neighbors=neighbors)
        assert Uq.grad_fn is not None
        (Uq * gU).sum().backward()
        grads = [xq.grad, xdb.grad, p.grad, eps.grad if torch.is_tensor(eps) else None]
        assert st.cpu().tolist()[1:] == [0, 0, 0]          # (word 0 counts the search's rescans)
        return [A.raw_bytes(t) for t in (Uq, lab, *grads)]

    Xq, Xdb, P, k, *_ = R.ext_case(name)
    kn = k - 1
    idx = _G().knn_query(A.dev(Xq), A.dev(Xdb), kn)[0]
    wide = _G().knn_query(A.dev(Xq), A.dev(Xdb), 2 * kn)[0]
    perm = torch.from_numpy(np.random.default_rng(8).permutation(2 * kn)).cuda()
    ref = run(None)
    assert run(idx) == ref                        # list mode: the caller's order is the search's
    assert run(wide[:, perm]) == ref              # pool mode: the pool holds the kn nearest
    # and without grad
    xq, xdb, p, eps, e, k = _ext_inputs(name, False)
    a = _G().extend(xq, xdb, p, k=k, epsilon=eps, eps_db=e)
    b = _G().extend(xq, xdb, p, k=k, epsilon=eps, eps_db=e, neighbors=idx.cpu())
    assert b[0].grad_fn is None and A.raw_bytes(a[0]) == A.raw_bytes(b[0]) == ref[0] and torch.equal(a[1], b[1])


# ------------------------------------------------------------------------------------------
# 3. moved queries: frozen lists that are no longer distance-ordered
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _moved(name):
    Xq, Xdb, P, k, epsilon, eps_db, *_ = R.ext_case(name)
    kn = k - 1
    idx = R.knn_ref(Xq, Xdb, kn)[0]
    Xm = (Xq + 0.3 * np.random.default_rng(9).standard_normal(Xq.shape)).astype(np.float32)
    D = R.dist2(Xm, Xdb)
    d2 = np.take_along_axis(D, idx, axis=1)
    assert (np.diff(d2, axis=1) < 0).any(axis=1).mean() > 0.9       # out of order
    assert (np.sort(R.knn_ref(Xm, Xdb, kn)[0], axis=1) != np.sort(idx, axis=1)).any()   # and stale
    Uq, lab, t = R.extend_ref(idx, d2, P, kn, epsilon, eps_db)
    bound = R.uq_bound(Xq.shape[1], kn, t, P, epsilon == "auto")
    gU = np.random.default_rng(10).standard_normal(Uq.shape)
    return Xm, idx, Uq, lab, bound, gU


def _torch_grads(name, dtype, device):
    Xq, Xdb, P, k, epsilon, eps_db, *_ = R.ext_case(name)
    Xm, idx, _, _, _, gU = _moved(name)
    t = lambda a: torch.from_numpy(np.array(a)).to(device=device, dtype=dtype).requires_grad_(True)
    xq, xdb, p = t(Xm), t(Xdb), t(P)
    eps = epsilon
    if epsilon != "auto":
        eps = torch.tensor(float(epsilon), dtype=dtype, device=device, requires_grad=True)
    e = None if eps_db is None else torch.from_numpy(np.array(eps_db)).to(device=device, dtype=dtype)
    Uq = _G().extend_torch(xq, xdb, p, torch.from_numpy(np.array(idx)).to(device), eps, e)
    (Uq * torch.from_numpy(np.array(gU)).to(device=device, dtype=dtype)).sum().backward()
    out = [xq.grad, xdb.grad, p.grad, eps.grad.reshape(1) if torch.is_tensor(eps) else None]
    return [None if g is None else g.double().cpu().numpy() for g in out]


@pytest.mark.parametrize("name", list(R.EXT_CASES))
def test_moved_queries_on_frozen_lists(name):
    Xq, Xdb, P, k, epsilon, eps_db, *_ = R.ext_case(name)
    Xm, idx, Uq_ref, lab_ref, bound, gU = _moved(name)
    xq, xdb, p = (A.dev(a).requires_grad_(True) for a in (Xm, Xdb, P))
    eps = epsilon
    if epsilon != "auto":
        eps = torch.tensor(float(epsilon), dtype=torch.float64, device="cuda", requires_grad=True)
    Uq, lab, st = _G().extend(xq, xdb, p, k=k, epsilon=eps, return_status=True,
                              eps_db=None if eps_db is None else A.dev(eps_db), neighbors=A.dev(idx))
    err = np.abs(Uq.detach().cpu().numpy() - Uq_ref).max()
    print(name, "max |Uq - ref|", err, "bound", bound)
    assert err <= bound and (lab.cpu().numpy() == lab_ref).all() and st.cpu().tolist() == [0, 0, 0, 0]
    (Uq * A.dev(gU)).sum().backward()
    ours = [xq.grad, xdb.grad, p.grad, None if epsilon == "auto" else eps.grad.reshape(1)]
    ref = _torch_grads(name, torch.float64, "cpu")
    f32 = _torch_grads(name, torch.float32, "cuda")
    for key, r, o, f in zip(("gXq", "gXdb", "gP", "geps"), ref, ours, f32):
        if r is None:
            assert o is None
            continue
        o = o.double().cpu().numpy()
        scale = np.abs(r).max()
        mine, theirs = np.abs(o - r).max() / scale, np.abs(f - r).max() / scale
        print(name, key, "err", mine, "float32 torch err", theirs, "ratio", mine / max(theirs, 1e-300))
        PARITY.setdefault(name, {})[key] = dict(err=mine, torch_float32_err=theirs,
                                                ratio=mine / max(theirs, 1e-300))
        assert mine <= 8 * theirs
    # a pool re-ranked at the moved queries is the search at the moved queries while it holds them
    kn = k - 1
    pool = _G().knn_query(A.dev(Xq), xdb.detach(), min(4 * kn, 256))[0]
    si, sd = _G().knn_query(A.dev(Xm), xdb.detach(), kn)
    pi, pd = _G().knn_query(A.dev(Xm), xdb.detach(), kn, candidates=pool)
    held = (np.sort(R.knn_ref(Xm, Xdb, kn)[0], axis=1)[:, :, None] == pool.cpu().numpy()[:, None, :]).any(2).all(1)
    assert held.mean() > 0.5
    h = torch.from_numpy(held).cuda()
    assert A.raw_bytes(pi[h]) == A.raw_bytes(si[h]) and A.raw_bytes(pd[h]) == A.raw_bytes(sd[h])


# ------------------------------------------------------------------------------------------
# 4. reproducibility and launches
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hard", "nonfinite", "d36_c64", "c512_k256"])
def test_row_of_a_call_equals_the_call_on_that_row(name):
    Xq, Xdb, cand, k, *_ = RR.pool(name)
    xq, xdb, cd = A.dev(Xq), A.dev(Xdb), A.dev(cand)
    idx, d2, _ = _raw(xq, xdb, cd, k)
    for q in range(len(Xq)):
        i1, f1, _ = _raw(xq[q:q + 1].clone(), xdb, cd[q:q + 1].clone(), k)
        assert i1.tobytes() == idx[q:q + 1].tobytes() and f1.tobytes() == d2[q:q + 1].tobytes()


def test_launches_per_call():
    """the re-rank is one launch, the extension on lists two; the search route
    launches what it did (three a panel + the extension)."""
    lib = _L().lib()
    Xq, Xdb, P, k, epsilon, eps_db, *_ = R.ext_case("auto")
    xq, xdb, p, e = A.dev(Xq), A.dev(Xdb), A.dev(P), A.dev(eps_db)
    idx = _G().knn_query(xq, xdb, k - 1)[0]
    wide = _G().knn_query(xq, xdb, 3 * (k - 1))[0]
    n = [lib.gll_query_launches()]
    g0 = lib.gll_extend_grad_launches()
    _G().knn_query(xq, xdb, k - 1, candidates=idx, keep_order=True)
    n.append(lib.gll_query_launches())
    _G().knn_query(xq, xdb, k - 1, candidates=wide)
    n.append(lib.gll_query_launches())
    _G().extend(xq, xdb, p, k=k, epsilon=epsilon, eps_db=e, neighbors=idx)
    n.append(lib.gll_query_launches())
    _G().extend(xq.clone().requires_grad_(True), xdb, p, k=k, epsilon=epsilon, eps_db=e, neighbors=wide)
    n.append(lib.gll_query_launches())
    _G().extend(xq, xdb, p, k=k, epsilon=epsilon, eps_db=e)
    n.append(lib.gll_query_launches())
    _G().knn_query(xq, xdb, k - 1)
    n.append(lib.gll_query_launches())
    assert np.diff(n).tolist() == [1, 1, 2, 2, 4, 3]
    assert lib.gll_extend_grad_launches() == g0
    # the backward on lists is the backward: one launch for Xq
    a = xq.clone().requires_grad_(True)
    Uq, _ = _G().extend(a, xdb, p, k=k, epsilon=epsilon, eps_db=e, neighbors=idx)
    q0 = lib.gll_query_launches()
    Uq.sum().backward()
    assert lib.gll_extend_grad_launches() - g0 == 1 and lib.gll_query_launches() == q0


def test_short_pool_rows_and_bad_list_entries_are_nan_and_counted():
    L = _L()
    Xq, Xdb, P, k, epsilon, eps_db, *_ = R.ext_case("fixed")
    xq, xdb, p = A.dev(Xq), A.dev(Xdb), A.dev(P)
    kn, N = k - 1, len(Xdb)
    idx = _G().knn_query(xq, xdb, kn)[0]
    clean = _G().extend(xq, xdb, p, k=k, epsilon=epsilon)[0]
    pool = torch.cat([idx, idx], dim=1)           # 2 kn columns, kn valid
    pool[3, :kn + 2] = idx[3, 0]                  # row 3: kn - 1 valid entries
    Uq, lab, st = _G().extend(xq, xdb, p, k=k, epsilon=epsilon, neighbors=pool, return_status=True)
    keep = [q for q in range(len(Xq)) if q != 3]
    assert torch.isnan(Uq[3]).all() and A.raw_bytes(Uq[keep]) == A.raw_bytes(clean[keep])
    assert st.cpu().tolist() == [0, 0, 1, 1]      # the short row, and its NaN weight sum
    bad = idx.clone()
    bad[5, 2], bad[6, 0] = N, -1                  # list mode keeps them and does not follow them
    Uq, lab, st = _G().extend(xq, xdb, p, k=k, epsilon=epsilon, neighbors=bad, return_status=True)
    keep = [q for q in range(len(Xq)) if q not in (5, 6)]
    assert torch.isnan(Uq[[5, 6]]).all() and A.raw_bytes(Uq[keep]) == A.raw_bytes(clean[keep])
    assert st.cpu().tolist() == [0, 2, 2, 0]
    i0, f0 = _G().knn_query(xq[:0], xdb, 3, candidates=idx[:0])
    assert i0.shape == (0, 3) and i0.dtype == torch.int64 and f0.shape == (0, 3)


# ------------------------------------------------------------------------------------------
# 5. laplace_predict
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epsilon", ["auto", 2.0])
def test_laplace_predict_on_lists_and_pools(epsilon):
    from graphlearninglayer_amd import utils
    rng = np.random.default_rng(41)
    C, base, n, d, kk = 4, 20, 300, 16, 10
    cen = rng.standard_normal((C, d)) * 3.0
    lab = np.concatenate([np.arange(base) % C, rng.integers(0, C, size=n - base)])
    X = (cen[lab] + 0.5 * rng.standard_normal((n, d))).astype(np.float32)
    Xq = (cen[np.arange(40) % C] + 0.5 * rng.standard_normal((40, d))).astype(np.float32)
    fit = utils.laplace_fit(X, lab[:base], knn_num=kk, epsilon=epsilon)
    xq = A.dev(Xq)
    Uq, labels = utils.laplace_predict(fit, xq, knn_num=kk)
    idx = _G().knn_query(xq, fit.X, kk - 1)[0]
    pool = _G().knn_query(xq, fit.X, 4 * (kk - 1))[0]
    for nb in (idx, pool):
        a = xq.clone().requires_grad_(True)
        Un, ln = utils.laplace_predict(fit, a, knn_num=kk, neighbors=nb)
        assert A.raw_bytes(Un) == A.raw_bytes(Uq) and torch.equal(ln, labels) and Un.grad_fn is not None
        Un.sum().backward()
        assert torch.isfinite(a.grad).all()
    # the attack loop: the pool searched once, re-ranked at every step's features
    Xs = (Xq + 0.05 * rng.standard_normal(Xq.shape)).astype(np.float32)
    near = R.knn_ref(Xs, X, kk - 1)[0]
    assert (near[:, :, None] == pool.cpu().numpy()[:, None, :]).any(2).all()   # the pool holds them
    step = A.dev(Xs)
    Us, ls = utils.laplace_predict(fit, step, knn_num=kk)
    Up, lp = utils.laplace_predict(fit, step, knn_num=kk, neighbors=pool)
    assert A.raw_bytes(Up) == A.raw_bytes(Us) and torch.equal(lp, ls)
