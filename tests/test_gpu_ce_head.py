"""The fused cross-entropy head on the HIP path (run on the MI355X: -m gpu).

LaplaceLearningSparseHard.ce_loss must reproduce what its callers compute from apply's U in
PyTorch -- custom_ce_loss (losses.py:128-136), the per-row -log(U[i, t_i] + 1e-8) and
U.argmax(1) (FullySup.py:156-171) -- and feed the layer's backward the same dL/dU.  Inputs:
tests/ce_head_ref.py (conditioning asserted on the CPU in test_ce_head_cpu.py).  u = 2^-53:
  * row_loss: |a - b| <= 8 u max(|b|, 1): the same float64 argument, two log implementations;
  * loss: |a - b| <= (4 m + 8) u mean|row_loss|: the same float64 terms in another order;
  * gradients: O.rel_err < 1e-4, the project's parity bar (the two routes differ by the fp32
    rounding of gbar and the CG's 1e-6);
  * loss against the float64 oracle: 1e-4 ||U||_inf mean(1 / (p_t + 1e-8)), the 1e-4 bar on U
    carried through d(-log p)/dp.
"""
import ctypes as ct

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import gll_oracle as O
from tests import abi as A
from tests import ce_head_ref as R
from tests.golden_io import Case

pytestmark = pytest.mark.gpu
TOL = 1e-4
U53 = 2.0 ** -53


def _gll():
    from graphlearninglayer_amd import GLL
    return GLL


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    A.need_gpu()


def _layer(python=False):
    L = _gll().LaplaceLearningSparseHard
    return (L.ce_loss_python, L.apply_python) if python else (L.ce_loss, L.apply)


def _torch_head(U, t):
    """What the callers compute from U in PyTorch (on U's device)."""
    loss = _gll().custom_ce_loss(U, t)
    row = -torch.log(U[torch.arange(U.shape[0], device=U.device), t] + 1e-8)
    return loss, row, U.argmax(1)


def _close(a, b, bound):
    """|a - b| <= bound elementwise, NaN only where b has NaN, inf only where b has the same."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    special = ~np.isfinite(b)
    ok_special = np.array_equal(a[special], b[special], equal_nan=True)
    fin = ~special
    bound = np.broadcast_to(bound, b.shape)
    return ok_special and bool(np.all(np.abs(a[fin] - b[fin]) <= bound[fin]))


# ------------------------------------------------------------------------------------------
# 1. same-U parity with PyTorch
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("python", [False, True], ids=["native", "ctypes"])
@pytest.mark.parametrize("tag,eps,tau", R.SETTINGS + [R.PAST_SWITCH])
def test_same_U_parity_with_pytorch(tag, eps, tau, python):
    X, Y, t = R.inputs(tag)
    k = R.CASES[tag].k
    ce, apply = _layer(python)
    Xt, Yt, tt = A.dev(X), A.dev(Y), A.dev(t)
    loss, pred, labels, row_loss, correct = ce(Xt, Yt, tt, tau, eps, k)
    U = apply(Xt, Yt, tau, eps, k)
    m = len(t)
    assert loss.shape == () and loss.dtype == torch.float64 and loss.is_cuda
    assert pred.dtype == torch.float64 and labels.dtype == torch.int64
    assert row_loss.shape == (m,) and row_loss.dtype == torch.float64
    assert correct.shape == () and correct.dtype == torch.int64
    assert not pred.requires_grad and loss.grad_fn is None
    np.testing.assert_array_equal(A.host(pred), A.host(U))
    tl, tr, ta = _torch_head(U, tt)
    tl, tr, ta = float(tl), A.host(tr), A.host(ta)
    a_row, a_loss = A.host(row_loss), float(loss)
    row_bound = 8 * U53 * np.maximum(np.abs(tr), 1.0)
    fin = np.isfinite(tr)
    loss_bound = (4 * m + 8) * U53 * float(np.mean(np.abs(tr[fin]))) if fin.any() else 0.0
    print(f"{tag} eps={eps} tau={tau}: loss {a_loss:.17g} vs {tl:.17g} (bound {loss_bound:.2e}); "
          f"max row_loss diff {np.nanmax(np.abs(a_row - tr)) if fin.any() else 0:.2e}; "
          f"min p_t {float(np.exp(-np.nanmax(tr))):.3g}; correct {int(correct)} / {m}")
    assert _close(a_row, tr, row_bound)
    assert _close(a_loss, tl, loss_bound)
    Us = np.sort(A.host(U), axis=1)
    tie = Us[:, -1] == Us[:, -2]
    assert tie.sum() <= 0.01 * m
    np.testing.assert_array_equal(A.host(labels)[~tie], ta[~tie])
    assert int(correct) == int((A.host(labels) == t).sum())


# ------------------------------------------------------------------------------------------
# 2. gbar through the C ABI
# ------------------------------------------------------------------------------------------
def _abi_head(tag, eps, tau, targets=None, want_gbar=True):
    """gll_forward + gll_ce_head_batched over ctypes; every output as numpy."""
    from graphlearninglayer_amd import _lib
    X, Y, t = R.inputs(tag)
    t = t if targets is None else targets
    c = R.CASES[tag]
    m = c.batch
    lib = _lib.lib()
    run = A.Run(X, Y, c.k, tau, eps)
    prob, ws, s = run.problem(), run.ws, A.stream()
    tt = A.dev(np.asarray(t, dtype=np.int64))
    U = run.forward()
    loss = torch.empty(1, dtype=torch.float64, device="cuda")
    gbar = torch.full((m, c.C), 7.0, dtype=torch.float32, device="cuda") if want_gbar else None
    row = torch.empty(m, dtype=torch.float64, device="cuda")
    lab = torch.empty(m, dtype=torch.int64, device="cuda")
    cor = torch.empty(1, dtype=torch.int64, device="cuda")
    sb = lib.gll_ce_head_scratch_bytes(ct.byref(prob), 1)
    scratch = torch.empty(max(sb, 1), dtype=torch.uint8, device="cuda")
    _lib.check(lib.gll_ce_head_batched(ct.byref(prob), 1, ws.data_ptr(), tt.data_ptr(),
                                       loss.data_ptr(), gbar.data_ptr() if want_gbar else None,
                                       row.data_ptr(), lab.data_ptr(), cor.data_ptr(),
                                       scratch.data_ptr() if sb else None, s), "gll_ce_head")
    torch.cuda.synchronize()
    return dict(U=U, loss=float(loss), gbar=A.host(gbar) if want_gbar else None, row=A.host(row),
                labels=A.host(lab), correct=int(cor))


@pytest.mark.parametrize("tag,eps,tau", [("T1", 1.0, 0.07), ("T5", 1.0, 0.07),
                                         ("T5", "auto", 0.07), R.PAST_SWITCH])
def test_gbar_through_the_c_abi(tag, eps, tau):
    out = _abi_head(tag, eps, tau)
    _, _, t = R.inputs(tag)
    ref = R.ce_head(out["U"], t)     # float64 formula on the GPU's own U (= double(U32))
    want = ref.gbar.astype(np.float32)
    hot = ref.gbar != 0
    assert hot.sum() == len(t)
    rel = np.abs(out["gbar"][hot].astype(np.float64) - ref.gbar[hot]) / np.abs(ref.gbar[hot])
    print(f"{tag} eps={eps}: gbar max relative error at the target column {rel.max():.2e} "
          f"({(out['gbar'][hot] == want[hot]).mean() * 100:.0f}% bitwise float32 of the formula)")
    assert rel.max() <= 2.0 ** -23
    assert (out["gbar"][~hot] == 0).all()
    # without gbar the other outputs do not move
    bare = _abi_head(tag, eps, tau, want_gbar=False)
    for key in ("loss", "row", "labels", "correct"):
        np.testing.assert_array_equal(bare[key], out[key], err_msg=key)


# ------------------------------------------------------------------------------------------
# 3. gradients: the fused route against apply -> custom_ce_loss -> backward
# ------------------------------------------------------------------------------------------
def _scalar(v, grad):
    if isinstance(v, str) or not grad:
        return v
    return torch.tensor(float(v), dtype=torch.float64, device="cuda", requires_grad=True)


def _grads(tag, eps, tau, fused, need=(True, False, False, False), python=False):
    X, Y, t = R.inputs(tag)
    k = R.CASES[tag].k
    ce, apply = _layer(python)
    Xt = A.dev(X).requires_grad_(need[0])
    Yt = A.dev(Y).requires_grad_(need[1])
    tt, et, tg = _scalar(tau, need[2]), _scalar(eps, need[3]), A.dev(t)
    if fused:
        loss = ce(Xt, Yt, tg, tt, et, k)[0]
    else:
        loss = _gll().custom_ce_loss(apply(Xt, Yt, tt, et, k), tg)
    loss.backward()
    torch.cuda.synchronize()

    def g(v):
        return None if not torch.is_tensor(v) or v.grad is None else A.host(v.grad)
    return dict(loss=float(loss.detach()), X=g(Xt), Y=g(Yt), tau=g(tt), eps=g(et))


@pytest.mark.parametrize("tag,eps,tau", [("T1", 1.0, 0.07), ("T2", "auto", 0.0),
                                         ("T4", "auto", 0.07), ("T5", 1.0, 0.07),
                                         ("T5", "auto", 0.07), R.PAST_SWITCH, R.NS])
def test_feature_gradient_matches_the_unfused_route(tag, eps, tau):
    a = _grads(tag, eps, tau, True)
    b = _grads(tag, eps, tau, False)
    e = O.rel_err(a["X"], b["X"])
    print(f"{tag} eps={eps} tau={tau}: grad_X rel err fused vs unfused {e:.2e}; "
          f"loss {a['loss']:.12g} vs {b['loss']:.12g}")
    assert a["X"].shape == b["X"].shape and a["X"].dtype == np.float32
    assert e < TOL


def test_parameter_gradients_match_the_unfused_route():
    need = (True, True, True, True)
    a = _grads("T1", 1.0, 0.07, True, need)
    b = _grads("T1", 1.0, 0.07, False, need)
    errs = {key: O.rel_err(a[key], b[key]) for key in ("X", "Y", "tau", "eps")}
    print("T1 all inputs: rel err fused vs unfused " +
          ", ".join(f"{key} {v:.2e}" for key, v in errs.items()) +
          f"; grad_tau {float(a['tau']):.8g}, grad_eps {float(a['eps']):.8g}")
    for key, v in errs.items():
        assert v < TOL, key
    # the ctypes path runs the same kernels on the same numbers
    p = _grads("T1", 1.0, 0.07, True, need, python=True)
    for key in ("loss", "X", "Y", "tau", "eps"):
        np.testing.assert_array_equal(a[key], p[key], err_msg=key)


# ------------------------------------------------------------------------------------------
# 4. loss against the float64 oracle
# ------------------------------------------------------------------------------------------
def _oracle_loss_check(tagline, X, Y, t, tau, eps, k):
    Xt, Yt, tt = A.dev(X), A.dev(Y), A.dev(t)
    loss = float(_gll().LaplaceLearningSparseHard.ce_loss(Xt, Yt, tt, tau, eps, k)[0])
    ind = _gll().device_graph(Xt, k, eps)["knn_idx"].cpu().numpy().astype(np.int64)
    Uo, _ = O.forward(X, Y, tau, eps, k, knn=(ind, None))
    ref = R.ce_head(Uo, t)
    pt = Uo[np.arange(len(t)), t]
    bound = TOL * float(np.abs(Uo).max()) * float(np.mean(1.0 / (pt + 1e-8)))
    print(f"{tagline}: loss {loss:.12g} vs oracle {ref.loss:.12g}, diff {abs(loss - ref.loss):.2e} "
          f"(bound {bound:.2e}); oracle min p_t {pt.min():.3g}")
    assert abs(loss - ref.loss) <= bound


def test_loss_against_the_oracle_T2():
    X, Y, t = R.inputs("T2")
    _oracle_loss_check("T2", X, Y, t, 0.0, "auto", R.CASES["T2"].k)


def test_loss_against_the_oracle_ns():
    c = Case("ns_eps1p0_tau0p07_f32")
    assert c.x_ok
    _oracle_loss_check("NS", c.X, c.Y, c.labels[c.meta["base"]:], c.tau, c.eps, c.k)


# ------------------------------------------------------------------------------------------
# 5. batched
# ------------------------------------------------------------------------------------------
def test_batched_graphs_equal_single_calls():
    tags, eps, tau, k = ("T1", "T1s1", "T1s2"), 1.0, 0.07, R.CASES["T1"].k
    Xs = np.stack([R.inputs(g)[0] for g in tags])
    Ys = np.stack([R.inputs(g)[1] for g in tags])
    ts = np.stack([np.roll(R.inputs(g)[2], q) for q, g in enumerate(tags)])   # per-graph targets
    L = _gll().LaplaceLearningSparseHard
    Xb = A.dev(Xs).requires_grad_(True)
    lossb, predb, labb, rowb, corb = L.ce_loss(Xb, A.dev(Ys), A.dev(ts), tau, eps, k)
    assert lossb.shape == (3,) and corb.shape == (3,) and rowb.shape == ts.shape
    assert labb.shape == ts.shape and predb.shape == (3, ts.shape[1], Ys.shape[2])
    lossb.sum().backward()
    gb = A.host(Xb.grad)
    # apply's own batched backward on the same loss: bitwise the single call or not?
    Xa = A.dev(Xs).requires_grad_(True)
    Ua = L.apply(Xa, A.dev(Ys), tau, eps, k)
    sum(_gll().custom_ce_loss(Ua[g], A.dev(ts[g])) for g in range(3)).backward()
    for g in range(3):
        X1 = A.dev(Xs[g]).requires_grad_(True)
        loss, pred, lab, row, cor = L.ce_loss(X1, A.dev(Ys[g]), A.dev(ts[g]), tau, eps, k)
        loss.backward()
        assert float(loss.detach()) == float(lossb[g].detach()) and int(cor) == int(corb[g])
        np.testing.assert_array_equal(A.host(row), A.host(rowb[g]))
        np.testing.assert_array_equal(A.host(lab), A.host(labb[g]))
        np.testing.assert_array_equal(A.host(pred), A.host(predb[g]))
        Xs1 = A.dev(Xs[g]).requires_grad_(True)
        _gll().custom_ce_loss(L.apply(Xs1, A.dev(Ys[g]), tau, eps, k), A.dev(ts[g])).backward()
        apply_bitwise = np.array_equal(A.host(Xa.grad[g]), A.host(Xs1.grad))
        e = O.rel_err(gb[g], A.host(X1.grad))
        print(f"graph {g}: apply batched == single bitwise: {apply_bitwise}; "
              f"ce_loss batched vs single grad_X rel err {e:.2e}")
        if apply_bitwise:
            np.testing.assert_array_equal(gb[g], A.host(X1.grad))
        else:   # other kernel variants in the batched launch: test_gpu_parity's bar for them
            assert e <= 1e-5
    # one graph's loss alone: the others get an exact-zero gradient
    Xc = A.dev(Xs).requires_grad_(True)
    L.ce_loss(Xc, A.dev(Ys), A.dev(ts), tau, eps, k)[0][1].backward()
    gc = A.host(Xc.grad)
    assert (gc[0] == 0).all() and (gc[2] == 0).all()
    np.testing.assert_array_equal(gc[1], gb[1])


# ------------------------------------------------------------------------------------------
# 6. masked targets
# ------------------------------------------------------------------------------------------
def test_masked_targets():
    X, Y, t = R.inputs("T1")
    C = R.CASES["T1"].C
    tm = t.copy()
    tm[::4] = -1
    tm[1:9:4] = C
    tm[2] = 2 ** 40       # far outside: must never index U
    tm[6] = -(2 ** 40)
    out = _abi_head("T1", 1.0, 0.07, targets=tm)
    ref = R.ce_head(out["U"], tm)
    masked = (tm < 0) | (tm >= C)
    assert masked.sum() >= len(t) // 4 + 2
    assert (out["row"][masked] == 0).all() and (out["gbar"][masked] == 0).all()
    np.testing.assert_array_equal(out["labels"], ref.pred_label)
    assert out["correct"] == ref.correct == int((out["labels"][~masked] == t[~masked]).sum())
    row_bound = 8 * U53 * np.maximum(np.abs(ref.row_loss), 1)
    assert np.all(np.abs(out["row"] - ref.row_loss) <= row_bound)
    m = len(t)
    assert abs(out["loss"] - ref.loss) <= (4 * m + 8) * U53 * np.mean(np.abs(ref.row_loss))
    assert abs(out["loss"] - out["row"].sum() / m) <= (4 * m + 8) * U53 * np.mean(out["row"])
    hot = ref.gbar != 0
    rel = np.abs(out["gbar"][hot] - ref.gbar[hot]) / np.abs(ref.gbar[hot])
    assert rel.max() <= 2.0 ** -23 and (out["gbar"][~hot] == 0).all()
    # the same through autograd: masked rows pull no gradient, the others keep the divisor m
    L = _gll().LaplaceLearningSparseHard
    Xt = A.dev(X).requires_grad_(True)
    loss, _, _, row, cor = L.ce_loss(Xt, A.dev(Y), A.dev(tm), 0.07, 1.0, R.CASES["T1"].k)
    loss.backward()
    assert float(loss) == out["loss"] and int(cor) == out["correct"]
    Xr = A.dev(X).requires_grad_(True)
    U = L.apply(Xr, A.dev(Y), 0.07, 1.0, R.CASES["T1"].k)
    U.backward(A.dev(ref.gbar))
    e = O.rel_err(A.host(Xt.grad), A.host(Xr.grad))
    print(f"masked: grad_X rel err against apply fed the reference gbar {e:.2e}")
    assert e < TOL


# ------------------------------------------------------------------------------------------
# 7. launch accounting
# ------------------------------------------------------------------------------------------
def test_launch_accounting():
    from graphlearninglayer_amd import _lib
    kids = (_lib.K_GRAM, _lib.K_SELECT, _lib.K_FINALIZE, _lib.K_CG, _lib.K_EDGE, _lib.K_GRAD,
            _lib.K_BWD, _lib.K_LOSS)

    def counts(fused, tag, eps, tau):
        out = {}
        for kid in kids:   # one kernel id at a time: a bracket pair is armed per thread
            with A.launches(kid) as ran:
                _grads(tag, eps, tau, fused)
            out[kid] = ran[0]
        return out

    # T1 / T2: adjoint CG + gradient launches (fixed / auto eps); NS: the fused backward
    for tag, eps, tau in (("T1", 1.0, 0.07), ("T2", "auto", 0.0), R.NS):
        _grads(tag, eps, tau, True)   # warm
        a, b = counts(True, tag, eps, tau), counts(False, tag, eps, tau)
        print(f"{tag}: launches ce_loss {a}, apply {b}")
        assert a[_lib.K_LOSS] == 1 and b[_lib.K_LOSS] == 0
        for kid in kids[:-1]:
            assert a[kid] == b[kid], _lib.kernel_name(kid)
        assert sum(a[kid] for kid in kids[:-1]) >= 5
        if tag == "NS":
            assert a[_lib.K_BWD] == 1   # the saved gbar still takes the one-launch backward
    # m = 2048 still takes one launch and no scratch
    from graphlearninglayer_amd.synth import one_hot, synth
    X, lab = synth(16, 2048, 16, C=3, r=0.75, seed=0)
    with A.launches(_lib.K_LOSS) as ran, torch.no_grad():
        _gll().LaplaceLearningSparseHard.ce_loss(A.dev(X), A.dev(one_hot(lab[:16], 3)),
                                                 A.dev(lab[16:]), 0.07, 1.0, 6)
    assert ran == [1]
    p = _gll().make_problem(2064, 16, 16, 3, 6, 0.07, 1.0)
    assert _lib.lib().gll_ce_head_scratch_bytes(ct.byref(p), 1) == 0


# ------------------------------------------------------------------------------------------
# 8. no grad
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("python", [False, True], ids=["native", "ctypes"])
def test_no_grad_and_consumed_graph(python):
    X, Y, t = R.inputs("T1")
    k = R.CASES["T1"].k
    ce, _ = _layer(python)
    Xt = A.dev(X).requires_grad_(True)
    full = ce(Xt, A.dev(Y), A.dev(t), 0.07, 1.0, k)
    assert full[0].requires_grad and not any(o.requires_grad for o in full[1:])
    with torch.no_grad():
        ng = ce(Xt, A.dev(Y), A.dev(t), 0.07, 1.0, k)
    plain = ce(A.dev(X), A.dev(Y), A.dev(t), 0.07, 1.0, k)   # no input requires grad
    for outs in (ng, plain):
        assert not outs[0].requires_grad and outs[0].grad_fn is None
        for a, b in zip(outs, full):
            np.testing.assert_array_equal(A.host(a), A.host(b))
    full[0].backward()
    with pytest.raises(RuntimeError):
        full[0].backward()
    # argument handling: shapes and dtypes of targets
    with pytest.raises(ValueError):
        ce(A.dev(X), A.dev(Y), A.dev(t[:-1]), 0.07, 1.0, k)
    with pytest.raises(TypeError):
        ce(A.dev(X), A.dev(Y), A.dev(t.astype(np.float32)), 0.07, 1.0, k)
    i32 = ce(A.dev(X), A.dev(Y), A.dev(t.astype(np.int32)), 0.07, 1.0, k)
    assert float(i32[0]) == float(full[0])
    # CPU input: every output comes back on the CPU, the gradient too
    Xc = torch.from_numpy(np.array(X)).requires_grad_(True)
    outs = ce(Xc, torch.from_numpy(np.array(Y)), torch.from_numpy(np.array(t)), 0.07, 1.0, k)
    assert all(o.device.type == "cpu" for o in outs)
    outs[0].backward()
    assert Xc.grad.device.type == "cpu" and float(outs[0]) == float(full[0])
    np.testing.assert_array_equal(Xc.grad.numpy(), A.host(Xt.grad))


# ------------------------------------------------------------------------------------------
# 9. a three-step SGD loop behind a small network
# ------------------------------------------------------------------------------------------
def test_three_step_sgd_loop():
    X, Y, t = R.inputs("T1")
    k = R.CASES["T1"].k
    L = _gll().LaplaceLearningSparseHard

    def train(fused):
        torch.manual_seed(0)
        net = torch.nn.Linear(16, 16).cuda()
        opt = torch.optim.SGD(net.parameters(), lr=0.1)
        Xt, Yt, tt = A.dev(X), A.dev(Y), A.dev(t)
        losses = []
        for _ in range(3):
            opt.zero_grad()
            feat = F.normalize(net(Xt), dim=1)
            if fused:
                loss = L.ce_loss(feat, Yt, tt, 0.07, 1.0, k)[0]
            else:
                loss = _gll().custom_ce_loss(L.apply(feat, Yt, 0.07, 1.0, k), tt)
            loss.backward()
            opt.step()
            losses.append(float(loss))
        return np.concatenate([A.host(p).ravel() for p in net.parameters()]), losses

    pa, la = train(True)
    pb, lb = train(False)
    e = float(np.linalg.norm(pa - pb) / np.linalg.norm(pb))
    print(f"SGD: losses fused {la}, unfused {lb}; final parameters differ by {e:.2e} (normwise)")
    assert e <= TOL
