"""The fused score/objective head on the HIP path (run on the MI355X: -m gpu).

LaplaceLearningSparseHard.objective must reproduce, from apply's U, the float64 formulas of
tests/objective_ref.py (include/gll.h gll_objective_head_batched), be the cross-entropy head
bitwise at weights (1, 0, 0), scatter the chosen score into a device store and feed the layer's
backward the same dL/dU.  Inputs: tests/ce_head_ref.py.  u = 2^-53:
  * row_loss: |a - b| <= 8 u max(|b|, 1): the same float64 argument, two log implementations;
  * row_entropy: 8 (C + 1) u max(1, sum_c |u_c log(u_c + 1e-8)|): that allowance per term plus a
    C-term float64 sum;
  * row_l2: (C + 4) u max(1, sq_i);
  * loss: (4 m + 8) u mean_i(|w_ce ce_i| + |w_ent ent_i| + |w_l2 sq_i|): the same float64 terms in
    another order -- the head sums w_ce ce_i + w_ent ent_i - w_l2 sq_i row by row, the reference
    weights three sums, so the scale is the magnitude of the terms, not of their signed sum;
  * gbar: 2^-24 |b| + 24 u sum|terms|: one rounding to fp32 plus the float64 evaluation;
  * gradients: O.rel_err < 1e-4, the project's parity bar (tests/test_gpu_ce_head.py).
NaN / inf only where the reference has the same (the `_close` rule of test_gpu_ce_head.py); at
T1, T2, T4 and T7 nothing may be non-finite.
"""
import ctypes as ct

import numpy as np
import pytest
import torch

from oracle import gll_oracle as O
from tests import abi as A
from tests import ce_head_ref as R
from tests import grad_ref
from tests import objective_ref as OB
from tests.launch_counts import counted

pytestmark = pytest.mark.gpu
TOL = 1e-4
U53 = 2.0 ** -53
FINITE_TAGS = ("T1", "T2", "T4", "T7")
W_IDS = ["ce", "ent", "l2", "mix"]


def _gll():
    from graphlearninglayer_amd import GLL
    return GLL


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    A.need_gpu()


def _layer(python=False):
    L = _gll().LaplaceLearningSparseHard
    if python:
        return L.objective_python, L.ce_loss_python, L.apply_python
    return L.objective, L.ce_loss, L.apply


def _close(a, b, bound):
    """|a - b| <= bound elementwise, NaN only where b has NaN, inf only where b has the same."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    special = ~np.isfinite(b)
    ok_special = np.array_equal(a[special], b[special], equal_nan=True)
    fin = ~special
    bound = np.broadcast_to(bound, b.shape)
    return ok_special and bool(np.all(np.abs(a[fin] - b[fin]) <= bound[fin]))


def _loss_bound(ref, m):
    fin = np.isfinite(ref.row_abs)
    return (4 * m + 8) * U53 * float(np.mean(ref.row_abs[fin])) if fin.any() else 0.0


# ------------------------------------------------------------------------------------------
# 1. same-U parity with the float64 reference
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("python", [False, True], ids=["native", "ctypes"])
@pytest.mark.parametrize("weights", OB.WEIGHTS, ids=W_IDS)
@pytest.mark.parametrize("tag,eps,tau", R.SETTINGS + [R.PAST_SWITCH])
def test_same_U_parity_with_the_reference(tag, eps, tau, weights, python):
    X, Y, t = R.inputs(tag)
    k = R.CASES[tag].k
    objective, _, apply = _layer(python)
    Xt, Yt, tt = A.dev(X), A.dev(Y), A.dev(t)
    loss, pred, labels, row_loss, correct, row_ent, row_l2 = objective(Xt, Yt, tt, tau, eps, k,
                                                                       weights=weights)
    U = A.host(apply(Xt, Yt, tau, eps, k))
    m, C = U.shape
    assert loss.shape == () and loss.dtype == torch.float64 and loss.is_cuda
    assert pred.dtype == torch.float64 and labels.dtype == torch.int64
    for r in (row_loss, row_ent, row_l2):
        assert r.shape == (m,) and r.dtype == torch.float64
    assert correct.shape == () and correct.dtype == torch.int64
    assert not pred.requires_grad and loss.grad_fn is None
    np.testing.assert_array_equal(A.host(pred), U)
    ref = OB.objective(U, t, weights)
    a_row, a_ent, a_l2, a_loss = A.host(row_loss), A.host(row_ent), A.host(row_l2), float(loss)
    b_row = 8 * U53 * np.maximum(np.abs(ref.row_ce), 1.0)
    b_ent = 8 * (C + 1) * U53 * np.maximum(1.0, ref.ent_abs)
    b_l2 = (C + 4) * U53 * np.maximum(1.0, ref.sq)
    b_loss = _loss_bound(ref, m)
    with np.errstate(invalid="ignore"):
        print(f"{tag} eps={eps} tau={tau} w={weights}: loss {a_loss:.17g} vs {ref.loss:.17g} "
              f"(bound {b_loss:.2e}); max diff / bound: row_loss "
              f"{np.nanmax(np.abs(a_row - ref.row_ce) / b_row):.3f}, row_entropy "
              f"{np.nanmax(np.append(np.abs(a_ent - ref.row_entropy) / b_ent, 0)):.3f}, row_l2 "
              f"{np.nanmax(np.abs(a_l2 - ref.row_l2) / b_l2):.3f}; non-finite entropy rows "
              f"{int((~np.isfinite(ref.row_entropy)).sum())} / {m}; min U {U.min():.3g}")
    if tag in FINITE_TAGS:
        for name, v in (("row_loss", a_row), ("row_entropy", a_ent), ("row_l2", a_l2),
                        ("ref row_entropy", ref.row_entropy), ("ref row_loss", ref.row_ce)):
            assert np.isfinite(v).all(), name
        assert np.isfinite(a_loss)
    assert _close(a_row, ref.row_ce, b_row)
    assert _close(a_ent, ref.row_entropy, b_ent)
    assert _close(a_l2, ref.row_l2, b_l2)
    assert _close(a_loss, ref.loss, b_loss)
    assert int(correct) == int((A.host(labels) == t).sum())
    Us = np.sort(U, axis=1)
    tie = Us[:, -1] == Us[:, -2]
    np.testing.assert_array_equal(A.host(labels)[~tie], ref.pred_label[~tie])


# ------------------------------------------------------------------------------------------
# 2. gbar through the C ABI
# ------------------------------------------------------------------------------------------
def _abi_head(tag, eps, tau, weights, targets="own", want_gbar=True, score=0, score_len=0,
              indices=None, sentinel=-7.5):
    """gll_forward + gll_objective_head_batched over ctypes; every output as numpy.  targets:
    'own' (the case's), None (NULL) or an array."""
    from graphlearninglayer_amd import _lib
    X, Y, t = R.inputs(tag)
    t = t if isinstance(targets, str) else targets
    c = R.CASES[tag]
    m = c.batch
    lib = _lib.lib()
    run = A.Run(X, Y, c.k, tau, eps)
    prob, ws, s = run.problem(), run.ws, A.stream()
    tt = None if t is None else A.dev(np.asarray(t, dtype=np.int64))
    U = run.forward()
    f64 = dict(dtype=torch.float64, device="cuda")
    loss = torch.empty(1, **f64)
    gbar = torch.full((m, c.C), 7.0, dtype=torch.float32, device="cuda") if want_gbar else None
    row, ent, l2 = (torch.empty(m, **f64) for _ in range(3))
    lab = torch.empty(m, dtype=torch.int64, device="cuda")
    cor = torch.empty(1, dtype=torch.int64, device="cuda")
    store = torch.full((max(score_len, 1),), sentinel, dtype=torch.float32, device="cuda")
    ind = None if indices is None else A.dev(np.asarray(indices, dtype=np.int64))
    sb = lib.gll_objective_head_scratch_bytes(ct.byref(prob), 1)
    scratch = torch.empty(max(sb, 1), dtype=torch.uint8, device="cuda")
    _lib.check(lib.gll_objective_head_batched(
        ct.byref(prob), 1, ws.data_ptr(), None if tt is None else tt.data_ptr(), *weights,
        loss.data_ptr(), gbar.data_ptr() if want_gbar else None, row.data_ptr(), ent.data_ptr(),
        l2.data_ptr(), lab.data_ptr(), cor.data_ptr(), score,
        store.data_ptr() if score else None, score_len, None if ind is None else ind.data_ptr(),
        scratch.data_ptr() if sb else None, s), "gll_objective_head")
    torch.cuda.synchronize()
    return dict(U=U, loss=A.host(loss)[0], gbar=A.host(gbar) if want_gbar else None, row=A.host(row),
                ent=A.host(ent), l2=A.host(l2), labels=A.host(lab), correct=int(cor), store=A.host(store))


def _check_gbar(out, ref, label):
    bound = 2.0 ** -24 * np.abs(ref.gbar) + 24 * U53 * ref.gbar_abs
    got = out["gbar"].astype(np.float64)
    fin = np.isfinite(ref.gbar)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.abs(got[fin] - ref.gbar[fin]) / np.where(bound[fin] > 0, bound[fin], 1.0)
    print(f"{label}: gbar max diff / bound {ratio.max() if ratio.size else 0:.3f}; "
          f"non-finite reference entries {int((~fin).sum())} / {fin.size}")
    assert _close(got, ref.gbar, bound)


@pytest.mark.parametrize("weights", OB.WEIGHTS, ids=W_IDS)
@pytest.mark.parametrize("tag,eps,tau", [("T1", 1.0, 0.07), ("T4", "auto", 0.07), ("T5", 1.0, 0.07),
                                         ("T5", "auto", 0.07), R.PAST_SWITCH])
def test_gbar_through_the_c_abi(tag, eps, tau, weights):
    out = _abi_head(tag, eps, tau, weights)
    _, _, t = R.inputs(tag)
    ref = OB.objective(out["U"], t, weights)     # float64 formula on the GPU's own U (= double(U32))
    _check_gbar(out, ref, f"{tag} eps={eps} w={weights}")
    if tag in FINITE_TAGS:
        assert np.isfinite(out["gbar"]).all()
    if weights[1] == 0.0 and weights[2] == 0.0:
        assert (out["gbar"][ref.gbar == 0] == 0).all()
    assert _close(out["loss"], ref.loss, _loss_bound(ref, len(t)))
    # without gbar the other outputs do not move
    bare = _abi_head(tag, eps, tau, weights, want_gbar=False)
    for key in ("loss", "row", "ent", "l2"):
        A.same_bits(bare[key], out[key], key)
    for key in ("labels", "correct"):
        np.testing.assert_array_equal(bare[key], out[key], err_msg=key)


@pytest.mark.parametrize("tag,eps,tau", [("T1", 1.0, 0.07), R.PAST_SWITCH])
def test_masked_and_absent_targets(tag, eps, tau):
    w = (1.0, 0.3, 0.1)
    _, _, t = R.inputs(tag)
    m, C = len(t), R.CASES[tag].C
    full = _abi_head(tag, eps, tau, w)
    # some rows masked, far-out values among them: a target never forms an address
    tm = t.copy()
    tm[::4] = -1
    tm[1:9:4] = C
    tm[2] = 2 ** 40
    tm[6] = -(2 ** 40)
    masked = (tm < 0) | (tm >= C)
    part = _abi_head(tag, eps, tau, w, targets=tm)
    ref = OB.objective(part["U"], tm, w)
    assert (part["row"][masked] == 0).all()
    A.same_bits(part["row"][~masked], full["row"][~masked])
    A.same_bits(part["ent"], full["ent"])           # the regularisers see every row
    A.same_bits(part["l2"], full["l2"])
    A.same_bits(part["gbar"][~masked], full["gbar"][~masked])
    np.testing.assert_array_equal(part["labels"], full["labels"])
    assert part["correct"] == ref.correct == int((part["labels"][~masked] == t[~masked]).sum())
    _check_gbar(part, ref, f"{tag} partly masked")
    assert _close(part["loss"], ref.loss, _loss_bound(ref, m))
    # every row masked, by value and by targets == NULL: the same numbers, the regularisers alone
    allm = _abi_head(tag, eps, tau, w, targets=np.full(m, -1))
    null = _abi_head(tag, eps, tau, w, targets=None)
    ref0 = OB.objective(allm["U"], None, w)
    for key in ("loss", "row", "ent", "l2", "gbar"):
        A.same_bits(allm[key], null[key], key)
    np.testing.assert_array_equal(allm["labels"], null["labels"])
    assert allm["correct"] == null["correct"] == 0 and (null["row"] == 0).all()
    _check_gbar(null, ref0, f"{tag} targets NULL")
    assert _close(null["loss"], ref0.loss, _loss_bound(ref0, m))
    assert np.abs(null["gbar"]).max() > 0
    # ... and with the ce weight alone nothing is left
    none = _abi_head(tag, eps, tau, (1.0, 0.0, 0.0), targets=None)
    assert none["loss"] == 0.0 and (none["gbar"] == 0).all() and none["correct"] == 0


# ------------------------------------------------------------------------------------------
# 3. pinned to the existing head
# ------------------------------------------------------------------------------------------
def _scalar(v, grad):
    if isinstance(v, str) or not grad:
        return v
    return torch.tensor(float(v), dtype=torch.float64, device="cuda", requires_grad=True)


def _step(tag, eps, tau, head, need=(True, False, False, False), python=False, weights=None,
          count=False):
    """One step with X (and, per `need`, label_matrix, tau, eps) requiring grad.  head: 'objective',
    'ce' or 'torch' (apply followed by the torch formulas)."""
    X, Y, t = R.inputs(tag)
    k = R.CASES[tag].k
    objective, ce, apply = _layer(python)
    Xt = A.dev(X).requires_grad_(need[0])
    Yt = A.dev(Y).requires_grad_(need[1])
    tt, et, tg = _scalar(tau, need[2]), _scalar(eps, need[3]), A.dev(t)
    w = (1.0, 0.0, 0.0) if weights is None else weights
    outs = ()
    if head == "objective":
        outs = objective(Xt, Yt, tg, tt, et, k) if weights is None else \
            objective(Xt, Yt, tg, tt, et, k, weights=weights)
        loss = outs[0]
    elif head == "ce":
        outs = ce(Xt, Yt, tg, tt, et, k)
        loss = outs[0]
    else:
        U = apply(Xt, Yt, tt, et, k)
        m = U.shape[0]
        loss = 0.0
        if w[0] != 0.0:
            loss = loss + w[0] * _gll().custom_ce_loss(U, tg)
        if w[1] != 0.0:
            loss = loss + w[1] * (-torch.sum(U * torch.log(U + 1e-8)) / m)    # losses.py:100-101
        if w[2] != 0.0:
            loss = loss + w[2] * (-torch.sum(U ** 2) / m)                     # losses.py:111-112
    launches = None
    if count:   # the backward's launches alone
        torch.cuda.synchronize()
        with counted() as got:
            loss.backward()
        launches = got.counts
    else:
        loss.backward()
    torch.cuda.synchronize()

    def g(v):
        return None if not torch.is_tensor(v) or v.grad is None else A.host(v.grad)
    return dict(loss=A.host(loss), X=g(Xt), Y=g(Yt), tau=g(tt), eps=g(et),
                outs=[A.host(o) for o in outs], launches=launches)


@pytest.mark.parametrize("python", [False, True], ids=["native", "ctypes"])
@pytest.mark.parametrize("tag,eps,tau", [("T1", 1.0, 0.07), ("T2", "auto", 0.0), R.NS,
                                         R.PAST_SWITCH])
def test_unit_ce_weight_is_the_ce_head_bitwise(tag, eps, tau, python):
    need = (True, True, True, not isinstance(eps, str))
    a = _step(tag, eps, tau, "objective", need, python)
    b = _step(tag, eps, tau, "ce", need, python)
    assert len(a["outs"]) == 7 and len(b["outs"]) == 5
    for q, name in enumerate(("loss", "pred", "pred_labels", "row_loss", "correct")):
        A.same_bits(a["outs"][q], b["outs"][q], name)
    for key in ("X", "Y", "tau", "eps"):
        if b[key] is None:
            assert a[key] is None, key
        else:
            A.same_bits(a[key], b[key], "grad " + key)
    assert a["X"] is not None and a["Y"] is not None and a["tau"] is not None
    # explicit weights (1, 0, 0) and integers are the default
    c = _step(tag, eps, tau, "objective", need, python, weights=(1, 0, 0))
    A.same_bits(c["loss"], a["loss"])
    A.same_bits(c["X"], a["X"])


# ------------------------------------------------------------------------------------------
# 4. gradients: the fused route against apply -> torch formulas -> backward
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", OB.WEIGHTS, ids=W_IDS)
@pytest.mark.parametrize("tag,eps,tau", [("T1", 1.0, 0.07), ("T2", "auto", 0.0),
                                         ("T4", "auto", 0.07), R.PAST_SWITCH, R.NS])
def test_feature_gradient_matches_the_unfused_route(tag, eps, tau, weights):
    """The cases whose predictions stay clear of the 1e-8 offset: at T5 the entropy term is NaN
    on both routes and a relative error says nothing."""
    a = _step(tag, eps, tau, "objective", weights=weights)
    b = _step(tag, eps, tau, "torch", weights=weights)
    e = O.rel_err(a["X"], b["X"])
    print(f"{tag} eps={eps} tau={tau} w={weights}: grad_X rel err fused vs unfused {e:.2e}; "
          f"loss {float(a['loss']):.12g} vs {float(b['loss']):.12g}")
    assert a["X"].shape == b["X"].shape and a["X"].dtype == np.float32
    assert np.isfinite(b["X"]).all() and np.abs(b["X"]).max() > 0
    assert e < TOL


def test_parameter_gradients_match_the_unfused_route():
    need, w = (True, True, True, True), (1.0, 0.3, 0.1)
    a = _step("T1", 1.0, 0.07, "objective", need, weights=w)
    b = _step("T1", 1.0, 0.07, "torch", need, weights=w)
    errs = {key: O.rel_err(a[key], b[key]) for key in ("X", "Y", "tau", "eps")}
    print("T1 all inputs, w = (1, 0.3, 0.1): rel err fused vs unfused " +
          ", ".join(f"{key} {v:.2e}" for key, v in errs.items()))
    for key, v in errs.items():
        assert v < TOL, key
    p = _step("T1", 1.0, 0.07, "objective", need, python=True, weights=w)
    for key in ("loss", "X", "Y", "tau", "eps"):
        A.same_bits(a[key], p[key], key)


# ------------------------------------------------------------------------------------------
# 5. scatter
# ------------------------------------------------------------------------------------------
SENTINEL = -7.5


def _scatter_inputs(tag, N, seed=0):
    _, _, t = R.inputs(tag)
    m, C = len(t), R.CASES[tag].C
    rng = np.random.default_rng(seed)
    ind = rng.permutation(N)[:m].astype(np.int64)
    tm = t.copy()
    tm[3::7] = -1            # masked rows
    tm[5] = C
    ind[0], ind[10 % m], ind[m - 1] = -1, N, -(2 ** 40)      # out of range
    ind[4 % m] = 2 ** 40
    return tm, ind


@pytest.mark.parametrize("python", [False, True], ids=["native", "ctypes"])
@pytest.mark.parametrize("score", ["entropy", "l2"])
@pytest.mark.parametrize("tag,N", [("T1", 300), ("T2", 65), ("T5", 1000), ("T7", 5000)])
def test_scatter(tag, N, score, python):
    eps, tau = 1.0, 0.07
    X, Y, _ = R.inputs(tag)
    k = R.CASES[tag].k
    tm, ind = _scatter_inputs(tag, N)
    C = R.CASES[tag].C
    objective = _layer(python)[0]
    store = torch.full((N,), SENTINEL, dtype=torch.float32, device="cuda")
    outs = objective(A.dev(X), A.dev(Y), A.dev(tm), tau, eps, k, weights=(1.0, 0.3, 0.1),
                     score=score, score_out=store, indices=A.dev(ind))
    row = A.host(outs[3] if score == "entropy" else outs[6]).astype(np.float32)
    got = A.host(store)
    live = (tm >= 0) & (tm < C) & (ind >= 0) & (ind < N)
    assert 0 < live.sum() < len(tm) - 4
    want = np.full(N, SENTINEL, dtype=np.float32)
    want[ind[live]] = row[live]
    A.same_bits(got, want)                       # written rows bitwise, every other entry untouched
    assert (got[ind[live]] != SENTINEL).all()
    # the outputs do not depend on the scatter
    plain = objective(A.dev(X), A.dev(Y), A.dev(tm), tau, eps, k, weights=(1.0, 0.3, 0.1))
    for a, b in zip(outs, plain):
        A.same_bits(A.host(a), A.host(b))


@pytest.mark.parametrize("score", ["entropy", "l2"])
def test_scatter_with_duplicate_indices_stores_one_candidate(score):
    X, Y, t = R.inputs("T1")
    m, N = len(t), 40
    ind = np.arange(m, dtype=np.int64) % 8 + 3            # 8 slots, 8 candidates each
    store = torch.full((N,), SENTINEL, dtype=torch.float32, device="cuda")
    L = _gll().LaplaceLearningSparseHard
    outs = L.objective(A.dev(X), A.dev(Y), A.dev(t), 0.07, 1.0, R.CASES["T1"].k, score=score,
                       score_out=store, indices=A.dev(ind))
    row = A.host(outs[3] if score == "entropy" else outs[6]).astype(np.float32)
    got = A.host(store)
    for slot in range(N):
        cands = row[ind == slot]
        if cands.size:
            assert (A.bits(cands) == A.bits(got[slot:slot + 1])[0]).any(), slot
        else:
            assert got[slot] == SENTINEL


def test_scatter_argument_checks():
    X, Y, t = R.inputs("T1")
    L = _gll().LaplaceLearningSparseHard
    k = R.CASES["T1"].k
    Xt, Yt, tt = A.dev(X), A.dev(Y), A.dev(t)
    ind = torch.arange(len(t), device="cuda")
    good = torch.zeros(100, device="cuda")
    for fn in (L.objective, L.objective_python):
        with pytest.raises(ValueError):
            fn(Xt, Yt, tt, 0.07, 1.0, k, score="l2", score_out=good)
        with pytest.raises(ValueError):
            fn(Xt, Yt, tt, 0.07, 1.0, k, score="l2", indices=ind)
        with pytest.raises(ValueError):
            fn(Xt, Yt, tt, 0.07, 1.0, k, score="l2", score_out=good.double(), indices=ind)
        with pytest.raises(ValueError):
            fn(Xt, Yt, tt, 0.07, 1.0, k, score="l2", score_out=torch.zeros(200, device="cuda")[::2],
               indices=ind)
        with pytest.raises(ValueError):
            fn(Xt, Yt, tt, 0.07, 1.0, k, score="l2", score_out=good.cpu(), indices=ind)
        with pytest.raises(ValueError):
            fn(Xt, Yt, tt, 0.07, 1.0, k, score="l2", score_out=good, indices=ind[:-1])
        with pytest.raises(ValueError):
            fn(Xt, Yt, tt, 0.07, 1.0, k, score="best", score_out=good, indices=ind)
        with pytest.raises(ValueError):
            fn(Xt, Yt, tt, 0.07, 1.0, k, weights=(1.0, 2.0))
    assert (good == 0).all()
    # CPU inputs: every output on the CPU, the store stays on the layer's device
    Xc = torch.from_numpy(np.array(X)).requires_grad_(True)
    outs = L.objective(Xc, torch.from_numpy(np.array(Y)), torch.from_numpy(np.array(t)), 0.07, 1.0,
                       k, score="l2", score_out=good, indices=ind.cpu())
    assert all(o.device.type == "cpu" for o in outs)
    outs[0].backward()
    assert Xc.grad.device.type == "cpu"
    A.same_bits(A.host(good[:len(t)]), outs[6].numpy().astype(np.float32))


# ------------------------------------------------------------------------------------------
# 6. batched
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [True, False], ids=["shared_labels", "per_graph_labels"])
def test_batched_graphs_equal_single_calls(shared):
    tags, eps, tau, k = ("T1", "T1s1", "T1s2"), 1.0, 0.07, R.CASES["T1"].k
    w = (1.0, 0.3, 0.1)
    Xs = np.stack([R.inputs(g)[0] for g in tags])
    Ys = np.stack([R.inputs(tags[0] if shared else g)[1] for g in tags])
    ts = np.stack([np.roll(R.inputs(g)[2], q) for q, g in enumerate(tags)])   # per-graph targets
    ts[1, ::5] = -1
    m, N = ts.shape[1], 3 * ts.shape[1] + 10
    ind = np.random.default_rng(1).permutation(N)[:3 * m].reshape(3, m).astype(np.int64)
    ind[2, 7] = N
    L = _gll().LaplaceLearningSparseHard
    Yb = A.dev(Ys[0]) if shared else A.dev(Ys)
    store = torch.full((N,), SENTINEL, dtype=torch.float32, device="cuda")
    Xb = A.dev(Xs).requires_grad_(True)
    outb = L.objective(Xb, Yb, A.dev(ts), tau, eps, k, weights=w, score="l2", score_out=store,
                       indices=A.dev(ind))
    assert outb[0].shape == (3,) and outb[4].shape == (3,) and outb[1].shape == (3, m, Ys.shape[2])
    for q in (2, 3, 5, 6):
        assert outb[q].shape == (3, m)
    outb[0].sum().backward()
    gb = A.host(Xb.grad)
    Xa = A.dev(Xs).requires_grad_(True)          # apply's own batched backward: bitwise the single?
    Ua = L.apply(Xa, Yb, tau, eps, k)
    Ua.backward(torch.ones_like(Ua))
    single_store = torch.full((N,), SENTINEL, dtype=torch.float32, device="cuda")
    for g in range(3):
        X1 = A.dev(Xs[g]).requires_grad_(True)
        out1 = L.objective(X1, A.dev(Ys[g]), A.dev(ts[g]), tau, eps, k, weights=w, score="l2",
                           score_out=single_store, indices=A.dev(ind[g]))
        out1[0].backward()
        for q, (a, b) in enumerate(zip(out1, outb)):
            A.same_bits(A.host(a), A.host(b[g]), f"graph {g} output {q}")
        Xs1 = A.dev(Xs[g]).requires_grad_(True)
        U1 = L.apply(Xs1, A.dev(Ys[g]), tau, eps, k)
        U1.backward(torch.ones_like(U1))
        apply_bitwise = np.array_equal(A.host(Xa.grad[g]), A.host(Xs1.grad))
        e = O.rel_err(gb[g], A.host(X1.grad))
        print(f"graph {g}: apply batched == single bitwise: {apply_bitwise}; "
              f"objective batched vs single grad_X rel err {e:.2e}")
        if apply_bitwise:
            np.testing.assert_array_equal(gb[g], A.host(X1.grad))
        else:   # other kernel variants in the batched launch: test_gpu_parity's bar for them
            assert e <= 1e-5
        # this graph's loss alone: the others get an exact-zero gradient
        Xc = A.dev(Xs).requires_grad_(True)
        L.objective(Xc, Yb, A.dev(ts), tau, eps, k, weights=w)[0][g].backward()
        gc = A.host(Xc.grad)
        for other in range(3):
            if other != g:
                assert (gc[other] == 0).all()
        np.testing.assert_array_equal(gc[g], gb[g])
    # one store took all B x m indices: the same entries as the three single calls
    A.same_bits(A.host(store), A.host(single_store))
    live = (ts >= 0) & (ind < N)
    assert (A.host(store)[ind[live]] != SENTINEL).all()
    assert int((A.host(store) != SENTINEL).sum()) == int(live.sum())
    # the ctypes path runs the same kernels on the same numbers
    pstore = torch.full((N,), SENTINEL, dtype=torch.float32, device="cuda")
    outp = L.objective_python(A.dev(Xs), Yb, A.dev(ts), tau, eps, k, weights=w, score="l2",
                              score_out=pstore, indices=A.dev(ind))
    for a, b in zip(outp, outb):
        A.same_bits(A.host(a), A.host(b))
    A.same_bits(A.host(pstore), A.host(store))


# ------------------------------------------------------------------------------------------
# 7. launch counts
# ------------------------------------------------------------------------------------------
def test_launch_counts():
    from graphlearninglayer_amd import _lib

    def launches(head, tag, eps, tau):
        with A.launches(_lib.K_LOSS) as ran:
            got = _step(tag, eps, tau, head, weights=(1.0, 0.3, 0.1) if head != "ce" else None,
                        count=True)["launches"]
        return got, ran[0]

    for tag, eps, tau in (("T1", 1.0, 0.07), ("T2", "auto", 0.0), R.NS):
        c = R.CASES[tag]
        for head in ("objective", "ce", "torch"):
            _step(tag, eps, tau, head)   # warm
        ob, ce, ap = (launches(h, tag, eps, tau) for h in ("objective", "ce", "torch"))
        print(f"{tag}: (edge, grad, bwd, cg), loss launches: objective {ob}, ce_loss {ce}, "
              f"apply {ap}")
        # what a backward of this shape launched before the head existed: the route model the
        # gradient tests pin (tests/grad_ref.py), fp32 dL/dU for the heads, float64 for apply
        auto = isinstance(eps, str)
        for got, dt in ((ob, "f32"), (ce, "f32"), (ap, "f64")):
            want = grad_ref.route(c.base + c.batch, c.d, c.base, c.C, c.k, 1, auto, True,
                                  g_dtype=dt).counts
            assert got[0] == want, (tag, got, want)
        assert ob[0] == ce[0]
        assert ob[1] == 1 and ce[1] == 1 and ap[1] == 0
        if tag == "NS":
            assert ob[0] == (0, 0, 1, 0)   # the saved gbar still takes the one-launch backward
    # past the switch the head is a row pass and a reduce under one bracket, and needs scratch
    p = _gll().make_problem(4132, 16, 32, 3, 6, 0.07, 1.0)
    assert _lib.lib().gll_objective_head_scratch_bytes(ct.byref(p), 1) > 0
    p = _gll().make_problem(4096 + 32, 16, 32, 3, 6, 0.07, 1.0)
    assert _lib.lib().gll_objective_head_scratch_bytes(ct.byref(p), 1) == 0


# ------------------------------------------------------------------------------------------
# 8. a FullySup-shaped step in score mode
# ------------------------------------------------------------------------------------------
def test_fullysup_shaped_steps_with_the_score_store():
    from graphlearninglayer_amd.base_data import DeviceBaseLoader, DeviceScoreStore
    from graphlearninglayer_amd.synth import CONFIGS, synth
    c = CONFIGS["fullysup"]
    base, bsz, d, k = c["base"], c["batch"], c["d"], c["k"]
    assert (base, bsz, d, k) == (250, 1250, 128, 25)
    X, lab = synth(base, 2 * bsz, d, r=c["r"], seed=0)      # 250 base rows + a training set of 2500
    dev = torch.device("cuda", torch.cuda.current_device())
    data = torch.from_numpy(X[base:]).to(dev)
    labels = torch.from_numpy(lab[base:]).to(dev)
    N = data.shape[0]
    store = DeviceScoreStore(labels, device=dev, seed=0)
    loader = DeviceBaseLoader(torch.from_numpy(X[:base]), torch.from_numpy(lab[:base]), device=dev,
                              seed=0)
    L = _gll().LaplaceLearningSparseHard
    order = torch.randperm(N, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    for step in range(2):
        idx = order[step * bsz:(step + 1) * bsz]
        feats = data[idx].clone().requires_grad_(True)
        base_x, _ = next(iter(loader))
        Xin = torch.cat((base_x, feats), 0)
        loss, pred, _, _, correct, _, row_l2 = L.objective(
            Xin, loader.label_matrix(), labels[idx], 0.07, 1.0, k, score="l2",
            score_out=store.scores, indices=idx)
        loss.backward()
        assert feats.grad is not None and bool(torch.isfinite(feats.grad).all())
        A.same_bits(A.host(store.scores[idx]), A.host(row_l2).astype(np.float32))
        want = (1.0 - torch.sum(pred ** 2, 1)).float()      # FullySup.py:171 on the same pred
        assert float((store.scores[idx] - want).abs().max()) <= 2.0 ** -23
    host = store.scores.cpu()                               # two steps covered the training set
    sel =store.select_indices(base, class_uniform_sample=True, mode="score")
    want = OB.select_by_score(host.tolist(), lab[base:].tolist(), base, True)
    assert sel.dtype == torch.int64 and sel.device == dev
    assert sel.tolist() == want
    flat = store.select_indices(base, mode="score")
    assert flat.tolist() == OB.select_by_score(host.tolist(), lab[base:].tolist(), base, False)
    loader.update(data[sel], labels[sel])                   # the hand-off (FullySup.py:278)
    assert len(loader) == base
    bx, by = next(iter(loader))
    assert bx.shape == (base, d) and sorted(by.tolist()) == sorted(labels[sel].tolist())
