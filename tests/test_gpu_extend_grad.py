"""The backward of the out-of-sample extension on the GPU (extend_grad.hip):
gll_extend_backward on the GPU's own lists against the float64 closed form of
tests/extend_grad_ref.py within its derived bound, GLL.extend + backward against float64 autograd of
the formula at the margin the SupCon parity uses, bitwise repeatability and independence of `what`,
flags, batch and alignment, the launch counts, IEEE behaviour for a zero weight sum and for indices
out of range, and the chain into the layer's own backward."""
import ctypes as ct
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import abi as A
from tests import extend_grad_ref as E
from tests import query_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = list(E.GRAD_CASES)
PARITY = {}
KEYS = ("gXq", "gXdb", "gP", "geps")


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
        with open(os.path.join(ROOT, "profiles", "eg01_parity.json"), "w") as fh:
            json.dump(PARITY, fh, indent=1, sort_keys=True)
    except OSError:
        pass


def _what(epsilon):
    L = _L()
    return L.EG_XQ | L.EG_XDB | L.EG_P | (0 if epsilon == "auto" else L.EG_EPS)


@functools.lru_cache(maxsize=None)
def _gpu_case(name):
    """The case on the device with the GPU's own lists: (xq, xdb, p, e32, idx int32, d2, gu, eps)."""
    Xq, Xdb, P, k, epsilon, eps_db, gU, idx_ref, d2_ref = E.grad_case(name)
    xq, xdb, p, gu = A.dev(Xq), A.dev(Xdb), A.dev(P), A.dev(gU)
    e32 = None if eps_db is None else A.dev(eps_db)
    idx, d2 = _G().knn_query(xq, xdb, k - 1)
    assert (np.sort(idx.cpu().numpy(), axis=1) == np.sort(idx_ref, axis=1)).all()
    return xq, xdb, p, e32, idx.int().contiguous(), d2, gu, 0.0 if epsilon == "auto" else float(epsilon)


def _stage(name, what, flags=0, rows=None, idx=None):
    """gll_extend_backward on the case (query rows `rows` only, lists `idx` instead of the GPU's)."""
    xq, xdb, p, e32, gidx, d2, gu, eps = _gpu_case(name)
    idx = gidx if idx is None else idx
    if rows is not None:
        xq, idx, d2, gu = (t[rows].contiguous() for t in (xq, idx, d2, gu))
    out = _G()._extend_backward_device(xq, xdb, idx, d2, p, e32, eps, gu, what, flags)
    torch.cuda.synchronize()
    return dict(zip(KEYS + ("status",), out))


# ------------------------------------------------------------------------------------------
# 1. stage: the kernels against the closed form on the same lists
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_stage_within_the_derived_bound_and_what_bits_agree(name):
    L = _L()
    Xq, Xdb, P, k, epsilon, eps_db, gU, *_ = E.grad_case(name)
    xq, xdb, p, e32, idx, d2, gu, eps = _gpu_case(name)
    what = _what(epsilon)
    got = _stage(name, what)
    ref = E.closed_form(Xq, Xdb, P, idx.cpu().numpy(), d2.cpu().numpy(), gU, epsilon, eps_db, bounds=True)
    assert got["status"].cpu().tolist() == [0, 0, 0, 0]
    for key in ("gXq", "gXdb", "gP"):
        g = got[key].cpu().numpy().astype(np.float64)
        ratio = float((np.abs(g - ref[key]) / ref["b_" + key]).max())
        print(name, key, "measured / bound", ratio)
        assert np.isfinite(g).all() and ratio <= 1.0
    if epsilon != "auto":
        ge = float(got["geps"].cpu()[0])
        print(name, "geps measured / bound", abs(ge - ref["geps"]) / ref["b_geps"])
        assert abs(ge - ref["geps"]) <= ref["b_geps"]
    else:
        assert got["geps"] is None
    # every bit alone writes the bits of the call that selects them all
    for bit, key in ((L.EG_XQ, "gXq"), (L.EG_XDB, "gXdb"), (L.EG_P, "gP"), (L.EG_EPS, "geps")):
        if what & bit:
            one = _stage(name, bit)
            assert A.raw_bytes(one[key]) == A.raw_bytes(got[key]), key
            assert all(one[o] is None for o in KEYS if o != key)


def test_misaligned_storage_gives_the_aligned_bits():
    name = "fixed"
    xq, xdb, p, e32, idx, d2, gu, eps = _gpu_case(name)
    ref = _stage(name, 15)

    def shifted(t):
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4
        return v

    assert xq.data_ptr() % 16 == 0 and xdb.data_ptr() % 16 == 0
    for mq, mdb in ((shifted(xq), xdb), (xq, shifted(xdb)), (shifted(xq), shifted(xdb))):
        out = _G()._extend_backward_device(mq, mdb, idx, shifted(d2), shifted(p), e32, eps, gu, 15)
        for key, t in zip(KEYS, out):
            assert A.raw_bytes(t) == A.raw_bytes(ref[key]), key


# ------------------------------------------------------------------------------------------
# 2. end to end: GLL.extend + backward against float64 autograd on exact float64 lists
# ------------------------------------------------------------------------------------------
def _torch_grads(name, dtype, device):
    """autograd of extend_torch on the case's exact float64 lists, everything in `dtype`."""
    Xq, Xdb, P, k, epsilon, eps_db, gU, idx, d2 = E.grad_case(name)
    t = lambda a: torch.from_numpy(np.array(a)).to(device=device, dtype=dtype).requires_grad_(True)
    xq, xdb, p = t(Xq), t(Xdb), t(P)
    eps = epsilon
    if epsilon != "auto":
        eps = torch.tensor(float(epsilon), dtype=dtype, device=device, requires_grad=True)
    e = None if eps_db is None else torch.from_numpy(np.array(eps_db)).to(device=device, dtype=dtype)
    Uq = _G().extend_torch(xq, xdb, p, torch.from_numpy(np.array(idx)).to(device), eps, e)
    (Uq * torch.from_numpy(np.array(gU)).to(device=device, dtype=dtype)).sum().backward()
    out = [xq.grad, xdb.grad, p.grad, eps.grad.reshape(1) if torch.is_tensor(eps) else None]
    return [None if g is None else g.double().cpu().numpy() for g in out]


@pytest.mark.parametrize("name", CASES)
def test_end_to_end_against_float64_autograd(name):
    Xq, Xdb, P, k, epsilon, eps_db, gU, *_ = E.grad_case(name)
    ref = _torch_grads(name, torch.float64, "cpu")
    f32 = _torch_grads(name, torch.float32, "cuda")
    xq, xdb, p = (A.dev(a).requires_grad_(True) for a in (Xq, Xdb, P))
    eps = epsilon
    if epsilon != "auto":
        eps = torch.tensor(float(epsilon), dtype=torch.float64, device="cuda", requires_grad=True)
    Uq, labels = _G().extend(xq, xdb, p, k=k, epsilon=eps,
                             eps_db=None if eps_db is None else A.dev(eps_db))
    assert Uq.grad_fn is not None and Uq.dtype == torch.float64 and not labels.requires_grad
    (Uq * A.dev(gU)).sum().backward()
    assert xq.grad.dtype == torch.float32 and xdb.grad.shape == xdb.shape and p.grad.shape == p.shape
    ours = [xq.grad, xdb.grad, p.grad, None if epsilon == "auto" else eps.grad.reshape(1)]
    if epsilon != "auto":
        assert eps.grad.dtype == torch.float64 and eps.grad.shape == eps.shape
    for key, r, o, f in zip(KEYS, ref, ours, f32):
        if r is None:
            assert o is None
            continue
        o = o.double().cpu().numpy()
        if name == "tiny" and key != "gP":
            # C = 1: u = P[j] whatever the weights, so these gradients are identically zero and
            # both sides of the comparison are rounding noise around 0
            assert np.abs(o).max() <= 1e-12 and np.abs(r).max() <= 1e-12
            continue
        scale = np.abs(r).max()
        mine, theirs = np.abs(o - r).max() / scale, np.abs(f - r).max() / scale
        print(name, key, "err", mine, "float32 torch err", theirs, "ratio", mine / max(theirs, 1e-300))
        PARITY.setdefault(name, {})[key] = dict(err=mine, torch_float32_err=theirs,
                                                ratio=mine / max(theirs, 1e-300))
        assert mine <= 8 * theirs


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float64])
def test_gradients_come_back_in_each_inputs_dtype(dtype):
    Xq, Xdb, P, k, epsilon, eps_db, gU, *_ = E.grad_case("fixed")
    xq = A.dev(Xq).to(dtype).requires_grad_(True)
    xdb = A.dev(Xdb).to(dtype).requires_grad_(True)
    p = A.dev(P).to(dtype).requires_grad_(True)
    Uq, _ = _G().extend(xq, xdb, p, k=k, epsilon=epsilon)
    (Uq * A.dev(gU)).sum().backward()
    assert xq.grad.dtype == dtype and xdb.grad.dtype == dtype and p.grad.dtype == dtype
    # the values are those of the same call on the float32 casts torch makes
    a, b, c = (t.detach().float().requires_grad_(True) for t in (xq, xdb, p))
    U2, _ = _G().extend(a, b, c, k=k, epsilon=epsilon)
    (U2 * A.dev(gU)).sum().backward()
    assert A.raw_bytes(U2) == A.raw_bytes(Uq)
    assert torch.equal(a.grad.to(dtype), xq.grad) and torch.equal(c.grad.to(dtype), p.grad)
    # only what requires grad is computed; eps_db never gets a gradient
    e = A.dev(E.grad_case("auto")[5]).requires_grad_(True)
    Xa, Xda, Pa, ka, *_ = E.grad_case("auto")
    q = A.dev(Xa).requires_grad_(True)
    U3, _ = _G().extend(q, A.dev(Xda), A.dev(Pa), k=ka, epsilon="auto", eps_db=e)
    U3.sum().backward()
    assert e.grad is None and q.grad is not None


# ------------------------------------------------------------------------------------------
# 3. bitwise properties
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hub_fixed", "hub_auto"])
def test_runs_repeat_and_small_lists_give_the_default_bits(name):
    L = _L()
    what = _what(E.grad_case(name)[4])
    a, b = _stage(name, what), _stage(name, what)
    s = _stage(name, what, flags=L.EGF_SMALL_LISTS)
    for key in KEYS:
        assert A.raw_bytes(a[key]) == A.raw_bytes(b[key]) == A.raw_bytes(s[key]), key
    # nine rows of the hub case list more than 64 queries, none more than 512
    assert a["status"].cpu()[L.EGST_LONG_LIST] == 0 and s["status"].cpu()[L.EGST_LONG_LIST] == 9
    lens = np.bincount(_gpu_case(name)[4].cpu().numpy().ravel(), minlength=500)
    assert lens[0] == 300 and (lens == 0).sum() == 486
    empty = torch.from_numpy(lens == 0).cuda()
    assert (a["gXdb"][empty] == 0).all() and (a["gP"][empty] == 0).all()


@pytest.mark.parametrize("name", ["auto", "auto_wide", "long_d"])
def test_row_of_a_call_equals_the_call_on_that_row(name):
    L = _L()
    full = _stage(name, L.EG_XQ)["gXq"]
    Q = full.shape[0]
    for q in sorted({0, Q // 2, Q - 1}):
        one = _stage(name, L.EG_XQ, rows=slice(q, q + 1))["gXq"]
        assert A.raw_bytes(one) == A.raw_bytes(full[q:q + 1]), q


def test_forward_without_grad_is_what_it_was_and_counts_as_before():
    lib = _L().lib()
    Xq, Xdb, P, k, epsilon, eps_db, gU, *_ = E.grad_case("auto")
    xq, xdb, p, e = A.dev(Xq), A.dev(Xdb), A.dev(P), A.dev(eps_db)
    q0, g0 = lib.gll_query_launches(), lib.gll_extend_grad_launches()
    U0, l0 = _G().extend(xq, xdb, p, k=k, epsilon=epsilon, eps_db=e)
    q1 = lib.gll_query_launches()
    assert U0.grad_fn is None and not U0.requires_grad and q1 - q0 == 4
    # the same through the C ABI, as before this backward existed
    idx, d2 = _G().knn_query(xq, xdb, k - 1)
    Uc = torch.empty_like(U0)
    lc = torch.empty_like(l0)
    st = torch.zeros(4, dtype=torch.int32, device="cuda")
    _L().check(lib.gll_extend(len(Xq), len(Xdb), k - 1, P.shape[1], idx.int().data_ptr(), d2.data_ptr(),
                              p.data_ptr(), e.data_ptr(), ct.c_float(0.0), Uc.data_ptr(), lc.data_ptr(),
                              st.data_ptr(), torch.cuda.current_stream().cuda_stream), "gll_extend")
    assert A.raw_bytes(Uc) == A.raw_bytes(U0) and torch.equal(lc, l0)
    q2 = lib.gll_query_launches()
    U1, l1 = _G().extend(xq.clone().requires_grad_(True), xdb, p, k=k, epsilon=epsilon, eps_db=e)
    assert lib.gll_query_launches() - q2 == 4 and lib.gll_extend_grad_launches() == g0
    assert U1.grad_fn is not None and A.raw_bytes(U1) == A.raw_bytes(U0) and torch.equal(l1, l0)
    with torch.no_grad():
        U2, _ = _G().extend(xq.clone().requires_grad_(True), xdb, p, k=k, epsilon=epsilon, eps_db=e)
    assert U2.grad_fn is None and A.raw_bytes(U2) == A.raw_bytes(U0)


# ------------------------------------------------------------------------------------------
# 4. launches: the row kernel; + count, scan, fill and the database kernel for
#    gXdb / gP; + the reduce for grad_eps
# ------------------------------------------------------------------------------------------
def test_launches_per_what():
    L = _L()
    lib = L.lib()
    expect = {L.EG_XQ: 1, L.EG_XDB: 5, L.EG_P: 5, L.EG_XDB | L.EG_P: 5, L.EG_XQ | L.EG_XDB | L.EG_P: 5,
              L.EG_EPS: 2, L.EG_XQ | L.EG_EPS: 2, 15: 6}
    for what, n in expect.items():
        n0, q0 = lib.gll_extend_grad_launches(), lib.gll_query_launches()
        _stage("fixed", what)
        assert lib.gll_extend_grad_launches() - n0 == n, what
        assert lib.gll_query_launches() == q0
    # through autograd: Xq alone is one launch
    Xq, Xdb, P, k, epsilon, *_ = E.grad_case("fixed")
    xq = A.dev(Xq).requires_grad_(True)
    Uq, _ = _G().extend(xq, A.dev(Xdb), A.dev(P), k=k, epsilon=epsilon)
    n0 = lib.gll_extend_grad_launches()
    Uq.sum().backward()
    assert lib.gll_extend_grad_launches() - n0 == 1


# ------------------------------------------------------------------------------------------
# 5. IEEE and safety
# ------------------------------------------------------------------------------------------
def test_zero_weight_sum_is_nan_in_its_own_rows_only():
    Xq, Xdb, P, k, epsilon, eps_db, gU, *_ = E.grad_case("fixed")
    far = np.concatenate([Xq, np.full((1, Xq.shape[1]), 1.0e4, dtype=np.float32)])
    gfar = np.concatenate([gU, np.ones((1, gU.shape[1]))])

    def run(xq_np, g_np):
        xq, xdb, p = (A.dev(a).requires_grad_(True) for a in (xq_np, Xdb, P))
        eps = torch.tensor(float(epsilon), dtype=torch.float64, device="cuda", requires_grad=True)
        Uq, _, st = _G().extend(xq, xdb, p, k=k, epsilon=eps, return_status=True)
        (Uq * A.dev(g_np)).sum().backward()
        return Uq, st, xq.grad, xdb.grad, p.grad, eps.grad

    Uq, st, gq, gdb, gp, ge = run(far, gfar)
    U0, _, gq0, gdb0, gp0, ge0 = run(Xq, gU)
    assert torch.isnan(Uq[-1]).all() and st.cpu()[_L().QST_ZERO_SUM] == 1
    assert torch.isnan(gq[-1]).all() and torch.isnan(ge).all() and torch.isfinite(ge0).all()
    assert A.raw_bytes(gq[:-1]) == A.raw_bytes(gq0)
    listed = _G().knn_query(A.dev(far[-1:]), A.dev(Xdb), k - 1)[0][0]
    mask = torch.zeros(len(Xdb), dtype=torch.bool, device="cuda")
    mask[listed] = True
    assert torch.isnan(gdb[mask]).all() and torch.isnan(gp[mask]).all()
    assert A.raw_bytes(gdb[~mask]) == A.raw_bytes(gdb0[~mask]) and A.raw_bytes(gp[~mask]) == A.raw_bytes(gp0[~mask])
    assert torch.isfinite(gdb0).all() and torch.isfinite(gp0).all()


def test_indices_out_of_range_are_not_followed():
    name = "fixed"
    xq, xdb, p, e32, idx, d2, gu, eps = _gpu_case(name)
    Q, N = xq.shape[0], xdb.shape[0]
    bad = idx.clone()
    bad[3, 2] = -1
    bad[7, 0] = N
    got = _stage(name, 15, idx=bad)
    clean = _stage(name, 15)
    keep = [q for q in range(Q) if q not in (3, 7)]
    less = _stage(name, 15, rows=keep)
    assert got["status"].cpu()[_L().EGST_ZERO_SUM] == 2
    assert torch.isnan(got["gXq"][[3, 7]]).all() and torch.isnan(got["geps"]).all()
    assert A.raw_bytes(got["gXq"][keep]) == A.raw_bytes(clean["gXq"][keep]) == A.raw_bytes(less["gXq"])
    mask = torch.zeros(N, dtype=torch.bool, device="cuda")
    for q, i in ((3, 2), (7, 0)):
        rest = [c for c in range(idx.shape[1]) if c != i]
        mask[idx[q, rest].long()] = True
    # the rows those two queries still list are NaN; every other row -- the rows of the two
    # replaced entries included, unless listed otherwise -- is what the call without them gives
    for key in ("gXdb", "gP"):
        assert torch.isnan(got[key][mask]).all()
        assert torch.isfinite(got[key][~mask]).all()
        assert A.raw_bytes(got[key][~mask]) == A.raw_bytes(less[key][~mask]), key


# ------------------------------------------------------------------------------------------
# 6. chain into the layer's backward, and laplace_predict
# ------------------------------------------------------------------------------------------
def _chain_data():
    rng = np.random.default_rng(41)
    C, base, n, d, kk = 4, 20, 300, 16, 10
    cen = rng.standard_normal((C, d)) * 3.0
    lab = np.concatenate([np.arange(base) % C, rng.integers(0, C, size=n - base)])
    X = (cen[lab] + 0.5 * rng.standard_normal((n, d))).astype(np.float32)
    Xq = (cen[np.arange(40) % C] + 0.5 * rng.standard_normal((40, d))).astype(np.float32)
    gU = rng.standard_normal((40, C))
    return X, Xq, lab, gU, base, C, kk


def test_query_loss_reaches_the_graph_features_through_apply():
    F = _G().LaplaceLearningSparseHard
    X, Xq, lab, gU, base, C, kk = _chain_data()
    Y = A.dev(np.eye(C, dtype=np.float32)[lab[:base]])
    tau, eps = 0.01, 2.0
    x1 = A.dev(X).requires_grad_(True)
    U = F.apply(x1, Y, tau, eps, kk)
    P = torch.cat([Y.double(), U]).float()
    Uq, _ = _G().extend(A.dev(Xq), x1.detach(), P, k=kk, epsilon=eps)
    (Uq * A.dev(gU)).sum().backward()
    # by hand: gP of the extension, its unlabeled rows fed to apply's backward
    x2 = A.dev(X).requires_grad_(True)
    U2 = F.apply(x2, Y, tau, eps, kk)
    P2 = torch.cat([Y.double(), U2.detach()]).float().requires_grad_(True)
    Uq2, _ = _G().extend(A.dev(Xq), x2.detach(), P2, k=kk, epsilon=eps)
    (Uq2 * A.dev(gU)).sum().backward()
    U2.backward(P2.grad[base:].double())
    assert A.raw_bytes(Uq) == A.raw_bytes(Uq2)
    assert torch.isfinite(x1.grad).all() and x1.grad.abs().max() > 0
    assert A.raw_bytes(x1.grad) == A.raw_bytes(x2.grad)


@pytest.mark.parametrize("epsilon", ["auto", 2.0])
def test_laplace_predict_passes_the_gradient_of_extend(epsilon):
    from graphlearninglayer_amd import utils
    X, Xq, lab, gU, base, C, kk = _chain_data()
    fit = utils.laplace_fit(X, lab[:base], knn_num=kk, epsilon=epsilon)
    a = A.dev(Xq).requires_grad_(True)
    Ua, _ = utils.laplace_predict(fit, a, knn_num=kk)
    (Ua * A.dev(gU)).sum().backward()
    b = A.dev(Xq).requires_grad_(True)
    Ub, _ = _G().extend(b, fit.X, fit.P, k=kk, epsilon=epsilon, eps_db=fit.eps)
    (Ub * A.dev(gU)).sum().backward()
    assert Ua.grad_fn is not None and A.raw_bytes(Ua) == A.raw_bytes(Ub) and A.raw_bytes(a.grad) == A.raw_bytes(b.grad)
    assert torch.isfinite(a.grad).all() and a.grad.abs().max() > 0
    # the fit's arrays take gradients when the caller asks for them
    fit2 = fit._replace(X=fit.X.clone().requires_grad_(True), P=fit.P.clone().requires_grad_(True))
    Uc, _ = utils.laplace_predict(fit2, A.dev(Xq), knn_num=kk)
    (Uc * A.dev(gU)).sum().backward()
    assert fit2.X.grad.shape == fit.X.shape and fit2.P.grad.shape == fit.P.shape
    assert torch.isfinite(fit2.X.grad).all() and fit2.P.grad.abs().max() > 0
