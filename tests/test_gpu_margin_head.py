"""The fused Carlini-Wagner margin head on the HIP path (run on the MI355X: -m gpu).

LaplaceLearningSparseHard.margin_loss must reproduce what the attack loop of
adversarial.py:688-751 computes from apply's U in PyTorch -- the two best classes of every row and
clamp(max - U[idx, other], min=0).sum() / m (GLL.cw_margin) -- and feed the layer's backward the
same dL/dU.  Yardstick: tests/margin_ref.py (pinned on the CPU in test_margin_head_cpu.py).
u = 2^-53:
  * labels, second, moved: exact;
  * row_margin: bitwise -- the difference of two fp32 values is exact in float64;
  * gbar: exactly +-float32(1 / m) or 0;
  * loss: |a - b| <= (4 m + 8) u mean|row_margin|: the same float64 terms in another order
    (test_gpu_ce_head.py's form);
  * gradients: O.rel_err < 1e-4, the project's parity bar.
"""
import ctypes as ct
import functools

import numpy as np
import pytest
import torch

from oracle import gll_oracle as O
from tests import abi as A
from tests import ce_head_ref as R
from tests import margin_ref as M
from tests.margin_ref import LAYER_CASES, WELL_SEPARATED

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
    return (L.margin_loss_python, L.apply_python) if python else (L.margin_loss, L.apply)


def _loss_close(got, ref, row_margin):
    """The summation bound; a NaN reference wants a NaN."""
    if np.isnan(ref):
        return bool(np.isnan(got))
    m = len(row_margin)
    return abs(got - ref) <= (4 * m + 8) * U53 * float(np.mean(np.abs(row_margin)))


def _same_bits_nan_where_nan(a, b):
    """Bitwise equal float64 arrays, NaN where NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nan = np.isnan(b)
    return np.array_equal(np.isnan(a), nan) and \
        np.array_equal(a[~nan].view(np.int64), b[~nan].view(np.int64))


# ------------------------------------------------------------------------------------------
# 1. stage test on planted rows, through the C ABI
# ------------------------------------------------------------------------------------------
STAGE_BASE, STAGE_D, STAGE_K = 2, 4, 3


@functools.lru_cache(maxsize=None)
def _planted(m, C, g):
    """(U32 rows m x C, other m, the yardstick's result) of graph g; shared, read-only.  Row
    i takes pattern i % 8 on top of random normals (negatives included): 0 plain; 1 an exact tie
    at first place; 2 an exact tie at second place; 3 every entry equal; 4 other = the best
    class (a == other); 5 other = -1; 6 other = C; 7 other far outside (+-2^40).  The last row of
    m >= 3 holds a NaN: graph 1 points other at it (a NaN margin and loss), the others elsewhere.
    """
    rng = np.random.default_rng(1000 * m + 10 * C + g)
    U = rng.standard_normal((m, C)).astype(np.float32)
    other = rng.integers(0, C, size=m).astype(np.int64)
    for i in range(m):
        pat, top = i % 8, np.float32(np.max(U[i]) + 1)
        j = rng.permutation(C)
        if pat == 1 and C >= 2:
            U[i, j[0]] = U[i, j[1]] = top
            other[i] = max(j[0], j[1]) if i % 16 == 1 else other[i]   # the tied runner-up
        elif pat == 2 and C >= 3:
            U[i, j[0]] = top + 1
            U[i, j[1]] = U[i, j[2]] = top
        elif pat == 3:
            U[i, :] = U[i, 0]
        elif pat == 5:
            other[i] = -1
        elif pat == 6:
            other[i] = C
        elif pat == 7:
            other[i] = 2 ** 40 if i % 16 == 7 else -(2 ** 40)
    if m >= 3 and (C > 1 or g == 1):
        c = int(rng.integers(0, C))
        U[m - 1, c] = np.nan
        other[m - 1] = c if g == 1 else (c + 1) % C
    lab = M.margin_head(U).labels
    sel = np.arange(m) % 8 == 4
    other[sel] = lab[sel]
    ref = M.margin_head(U, other)
    for a in (U, other, *ref[1:5]):
        a.setflags(write=False)
    return U, other, ref


def _stage_call(lib, prob, B, ws, others, want_gbar, m, C):
    """gll_margin_head_batched over ctypes on a prepared workspace; every output as numpy."""
    from graphlearninglayer_amd import _lib
    dev = "cuda"
    loss = torch.full((B,), 7.0, dtype=torch.float64, device=dev)
    moved = torch.full((B,), -7, dtype=torch.int64, device=dev)
    gbar = torch.full((B, m, C), 7.0, dtype=torch.float32, device=dev) if want_gbar else None
    row = torch.full((B, m), 7.0, dtype=torch.float64, device=dev)
    lab = torch.full((B, m), -7, dtype=torch.int64, device=dev)
    sec = torch.full((B, m), -7, dtype=torch.int64, device=dev)
    sb = lib.gll_margin_head_scratch_bytes(ct.byref(prob), B)
    scratch = torch.empty(max(sb, 1), dtype=torch.uint8, device=dev)
    ot = A.dev(np.stack(others))
    _lib.check(lib.gll_margin_head_batched(
        ct.byref(prob), B, ws.data_ptr(), ot.data_ptr(), loss.data_ptr(),
        gbar.data_ptr() if want_gbar else None, row.data_ptr(), lab.data_ptr(), sec.data_ptr(),
        moved.data_ptr(), scratch.data_ptr() if sb else None,
        torch.cuda.current_stream().cuda_stream), "gll_margin_head")
    torch.cuda.synchronize()
    return dict(loss=A.host(loss), moved=A.host(moved), gbar=A.host(gbar) if want_gbar else None,
                row=A.host(row), labels=A.host(lab), second=A.host(sec), scratch_bytes=sb)


def _stage_workspace(m, C, graphs):
    """B workspace blocks of a small valid problem with the planted U32 rows of `graphs` written
    at P + base * C (gll_workspace_solve_view); no forward runs."""
    from graphlearninglayer_amd import _lib
    B = len(graphs)
    # Run only for the problem and B zeroed blocks: its (zero) features and labels are never read
    run = A.Run(np.zeros((B, STAGE_BASE + m, STAGE_D)), np.zeros((B, STAGE_BASE, C)), STAGE_K, 0.07,
                1.0, ws_fill=0)
    ws, nb = run.ws, run.wb
    for q, g in enumerate(graphs):
        off = run.solve_view(q).P - ws.data_ptr() + STAGE_BASE * C * 4
        assert q * nb <= off and off + m * C * 4 <= (q + 1) * nb and off % 4 == 0
        ws[off: off + m * C * 4].view(torch.float32).copy_(A.dev(_planted(m, C, g)[0]).reshape(-1))
    return _lib.lib(), run.problem(), ws


def _check_stage(out, q, ref, m, C, tagline):
    np.testing.assert_array_equal(out["labels"][q], ref.labels, err_msg=tagline + " labels")
    np.testing.assert_array_equal(out["second"][q], ref.second, err_msg=tagline + " second")
    assert int(out["moved"][q]) == ref.moved, tagline
    assert _same_bits_nan_where_nan(out["row"][q], ref.row_margin), tagline + " row_margin"
    if out["gbar"] is not None:
        g = out["gbar"][q]
        assert np.array_equal(g, ref.gbar), tagline + " gbar"
        assert np.all((g == 0) | (np.abs(g) == np.float32(1.0 / m)))
    assert _loss_close(float(out["loss"][q]), ref.loss, ref.row_margin), \
        f"{tagline}: loss {float(out['loss'][q])!r} vs {ref.loss!r}"


@pytest.mark.parametrize("m", [1, 3, 1030, 4097])
@pytest.mark.parametrize("C", [1, 2, 4, 5, 16, 17, 128, 129, 256])
def test_stage_planted_rows(C, m):
    """B = 3 in one call and each of its graphs as a single call (B = 1)."""
    lib, prob, ws = _stage_workspace(m, C, (0, 1, 2))
    nb = ws.numel() // 3
    others = [_planted(m, C, g)[1] for g in range(3)]
    batched = _stage_call(lib, prob, 3, ws, others, True, m, C)
    assert (batched["scratch_bytes"] > 0) == (m > 4096)
    bare = _stage_call(lib, prob, 3, ws, others, False, m, C)
    for g in range(3):
        ref = _planted(m, C, g)[2]
        _check_stage(batched, g, ref, m, C, f"C={C} m={m} B=3 graph {g}")
        single = _stage_call(lib, prob, 1, ws[g * nb: (g + 1) * nb], others[g: g + 1], True, m, C)
        _check_stage(single, 0, ref, m, C, f"C={C} m={m} B=1 graph {g}")
        for key in ("loss", "moved", "row", "labels", "second", "gbar"):   # bitwise the single call
            assert batched[key][g: g + 1].tobytes() == single[key].tobytes(), (key, g)
    for key in ("loss", "moved", "row", "labels", "second"):   # without gbar nothing else moves
        assert bare[key].tobytes() == batched[key].tobytes(), key
    if m >= 3:
        assert np.isnan(batched["loss"][1]) and np.isfinite(batched["loss"][[0, 2]]).all()


def test_stage_other_null_and_no_unlabeled_row():
    from graphlearninglayer_amd import _lib
    m, C = 1030, 17
    lib, prob, ws = _stage_workspace(m, C, (0,))
    ref = M.margin_head(_planted(m, C, 0)[0])
    loss = torch.full((1,), 7.0, dtype=torch.float64, device="cuda")
    moved = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    gbar = torch.full((m, C), 7.0, dtype=torch.float32, device="cuda")
    row = torch.full((m,), 7.0, dtype=torch.float64, device="cuda")
    lab = torch.full((m,), -7, dtype=torch.int64, device="cuda")
    sec = torch.full((m,), -7, dtype=torch.int64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.gll_margin_head_batched(ct.byref(prob), 1, ws.data_ptr(), None, loss.data_ptr(),
                                           gbar.data_ptr(), row.data_ptr(), lab.data_ptr(),
                                           sec.data_ptr(), moved.data_ptr(), None, s),
               "gll_margin_head")
    np.testing.assert_array_equal(A.host(lab), ref.labels)
    np.testing.assert_array_equal(A.host(sec), ref.second)
    assert float(loss) == 0.0 and int(moved) == 0
    assert not A.host(gbar).any() and not A.host(row).any()
    # only loss given: every other output NULL
    loss.fill_(7.0)
    ot = A.dev(_planted(m, C, 0)[1])
    _lib.check(lib.gll_margin_head_batched(ct.byref(prob), 1, ws.data_ptr(), ot.data_ptr(),
                                           loss.data_ptr(), None, None, None, None, None, None, s),
               "gll_margin_head")
    full = _planted(m, C, 0)[2]
    assert _loss_close(float(loss), full.loss, full.row_margin)
    # m == 0: loss 0 and moved 0
    # as above: only the problem and two zeroed blocks are used
    empty = A.Run(np.zeros((2, 8, STAGE_D)), np.zeros((2, 8, 3)), STAGE_K, 0.07, 1.0, ws_fill=0)
    p0, w0 = empty.problem(), empty.ws
    l0 = torch.full((2,), 7.0, dtype=torch.float64, device="cuda")
    m0 = torch.full((2,), -7, dtype=torch.int64, device="cuda")
    _lib.check(lib.gll_margin_head_batched(ct.byref(p0), 2, w0.data_ptr(), None, l0.data_ptr(),
                                           None, None, None, None, m0.data_ptr(), None, s),
               "gll_margin_head")
    assert (A.host(l0) == 0).all() and (A.host(m0) == 0).all()


# ------------------------------------------------------------------------------------------
# 2. the layer against PyTorch on the same U
# ------------------------------------------------------------------------------------------
def _torch_top2(U):
    """adversarial.py:688-692 on U's device: argmax, the -1e6 edit, argmax again."""
    idx = torch.arange(U.shape[0], device=U.device)
    edit = U.clone()
    init_pred = edit.max(1)[1]
    edit[idx, init_pred] = -1000000
    return init_pred, edit.max(1)[1]


@pytest.mark.parametrize("python", [False, True], ids=["native", "ctypes"])
@pytest.mark.parametrize("tag,eps,tau", LAYER_CASES)
def test_same_U_parity_with_pytorch(tag, eps, tau, python):
    X, Y, _ = R.inputs(tag)
    k = R.CASES[tag].k
    mg, apply = _layer(python)
    Xt, Yt = A.dev(X), A.dev(Y)
    clean = mg(Xt, Yt, None, tau, eps, k)           # the attack's set-up step
    assert float(clean[0]) == 0.0 and int(clean[5]) == 0 and not A.host(clean[4]).any()
    other = clean[3]
    loss, pred, labels, second, row_margin, moved = mg(Xt, Yt, other, tau, eps, k)
    U = apply(Xt, Yt, tau, eps, k)
    m = U.shape[0]
    assert loss.shape == () and loss.dtype == torch.float64 and loss.is_cuda
    assert pred.dtype == torch.float64 and labels.dtype == torch.int64 and second.dtype == torch.int64
    assert row_margin.shape == (m,) and row_margin.dtype == torch.float64
    assert moved.shape == () and moved.dtype == torch.int64
    assert not pred.requires_grad and loss.grad_fn is None
    np.testing.assert_array_equal(A.host(pred), A.host(U))
    np.testing.assert_array_equal(A.host(clean[1]), A.host(U))
    np.testing.assert_array_equal(A.host(clean[2]), A.host(labels))
    np.testing.assert_array_equal(A.host(clean[3]), A.host(second))
    idx = torch.arange(m, device=U.device)
    t_row = A.host(torch.clamp(U.max(1)[0] - U[idx, other], min=0))
    t_loss = float(_gll().cw_margin(U, other))
    ta, ts = (A.host(v) for v in _torch_top2(U))
    print(f"{tag} eps={eps} tau={tau}: loss {float(loss):.17g} vs {t_loss:.17g} "
          f"(bound {(4 * m + 8) * U53 * np.mean(np.abs(t_row)):.2e}); moved {int(moved)} / {m}")
    assert _same_bits_nan_where_nan(A.host(row_margin), t_row)
    assert _loss_close(float(loss), t_loss, t_row)
    Us = np.sort(A.host(U), axis=1)
    tie1 = Us[:, -1] == Us[:, -2]
    tie2 = tie1 | (Us[:, -2] == Us[:, -3])
    assert tie2.sum() <= 0.01 * m
    if (tag, eps, tau) in WELL_SEPARATED:
        assert not tie2.any()
    np.testing.assert_array_equal(A.host(labels)[~tie1], ta[~tie1])
    np.testing.assert_array_equal(A.host(second)[~tie2], ts[~tie2])
    assert int(moved) == int((A.host(labels) == A.host(other)).sum())
    # the yardstick on the same U
    ref = M.margin_head(A.host(U), A.host(other))
    np.testing.assert_array_equal(A.host(labels), ref.labels)
    np.testing.assert_array_equal(A.host(second), ref.second)


# ------------------------------------------------------------------------------------------
# 3. gradients: the fused route against apply -> cw_margin -> backward
# ------------------------------------------------------------------------------------------
def _scalar(v, grad):
    if isinstance(v, str) or not grad:
        return v
    return torch.tensor(float(v), dtype=torch.float64, device="cuda", requires_grad=True)


@functools.lru_cache(maxsize=None)
def _clean(tag, eps, tau):
    """(labels, second) of a clean call, on the device."""
    X, Y, _ = R.inputs(tag)
    with torch.no_grad():
        out = _gll().LaplaceLearningSparseHard.margin_loss(A.dev(X), A.dev(Y), None, tau, eps,
                                                           R.CASES[tag].k)
    return out[2], out[3]


def _grads(tag, eps, tau, fused, need=(True, False, False, False), python=False, other=None,
           head="margin"):
    X, Y, t = R.inputs(tag)
    k = R.CASES[tag].k
    mg, apply = _layer(python)
    Xt = A.dev(X).requires_grad_(need[0])
    Yt = A.dev(Y).requires_grad_(need[1])
    tt, et = _scalar(tau, need[2]), _scalar(eps, need[3])
    other = _clean(tag, eps, tau)[1] if other is None else other
    if head == "ce":
        loss = _gll().LaplaceLearningSparseHard.ce_loss(Xt, Yt, A.dev(t), tt, et, k)[0]
    elif fused:
        loss = mg(Xt, Yt, other, tt, et, k)[0]
    else:
        loss = _gll().cw_margin(apply(Xt, Yt, tt, et, k), other)
    loss.backward()
    torch.cuda.synchronize()

    def g(v):
        return None if not torch.is_tensor(v) or v.grad is None else A.host(v.grad)
    return dict(loss=float(loss.detach()), X=g(Xt), Y=g(Yt), tau=g(tt), eps=g(et))


@pytest.mark.parametrize("tag,eps,tau", LAYER_CASES)
def test_feature_gradient_matches_the_unfused_route(tag, eps, tau):
    a = _grads(tag, eps, tau, True)
    b = _grads(tag, eps, tau, False)
    e = O.rel_err(a["X"], b["X"])
    print(f"{tag} eps={eps} tau={tau}: grad_X rel err fused vs unfused {e:.2e}; "
          f"loss {a['loss']:.12g} vs {b['loss']:.12g}")
    assert a["X"].shape == b["X"].shape and a["X"].dtype == np.float32
    assert np.abs(b["X"]).max() > 0
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


def test_other_equal_to_labels_gives_an_exactly_zero_gradient():
    labels = _clean("T1", 1.0, 0.07)[0]
    X, Y, _ = R.inputs("T1")
    Xt = A.dev(X).requires_grad_(True)
    out = _gll().LaplaceLearningSparseHard.margin_loss(Xt, A.dev(Y), labels, 0.07, 1.0,
                                                       R.CASES["T1"].k)
    assert float(out[0].detach()) == 0.0 and not A.host(out[4]).any() and int(out[5]) == len(labels)
    out[0].backward()
    assert Xt.grad is not None and not A.host(Xt.grad).any()


# ------------------------------------------------------------------------------------------
# 4. launch accounting
# ------------------------------------------------------------------------------------------
def test_launch_accounting():
    from graphlearninglayer_amd import _lib
    kids = (_lib.K_GRAM, _lib.K_SELECT, _lib.K_FINALIZE, _lib.K_CG, _lib.K_EDGE, _lib.K_GRAD,
            _lib.K_BWD, _lib.K_LOSS)

    def counts(tag, eps, tau, **kw):
        out = {}
        for kid in kids:   # one kernel id at a time: a bracket pair is armed per thread
            with A.launches(kid) as ran:
                _grads(tag, eps, tau, **kw)
            out[kid] = ran[0]
        return out

    # T1 / T2: adjoint CG + gradient launches (fixed / auto eps); NS: the fused backward
    for tag, eps, tau in (("T1", 1.0, 0.07), ("T2", "auto", 0.0), R.NS):
        _grads(tag, eps, tau, True)   # warm (and the cached clean call)
        a = counts(tag, eps, tau, fused=True)
        b = counts(tag, eps, tau, fused=False)
        c = counts(tag, eps, tau, fused=True, head="ce")
        print(f"{tag}: launches margin_loss {a}, apply {b}, ce_loss {c}")
        assert a[_lib.K_LOSS] == 1 and b[_lib.K_LOSS] == 0
        for kid in kids[:-1]:
            assert a[kid] == b[kid], _lib.kernel_name(kid)
        assert a == c                 # forward and backward launch what ce_loss's do
        assert sum(a[kid] for kid in kids[:-1]) >= 5
        if tag == "NS":
            assert a[_lib.K_BWD] == 1   # the saved gbar still takes the one-launch backward


# ------------------------------------------------------------------------------------------
# 5. lifecycle
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("python", [False, True], ids=["native", "ctypes"])
def test_no_grad_and_consumed_graph(python):
    X, Y, _ = R.inputs("T1")
    k = R.CASES["T1"].k
    mg, _ = _layer(python)
    other = _clean("T1", 1.0, 0.07)[1]
    Xt = A.dev(X).requires_grad_(True)
    full = mg(Xt, A.dev(Y), other, 0.07, 1.0, k)
    assert len(full) == 6
    assert full[0].requires_grad and not any(o.requires_grad for o in full[1:])
    with torch.no_grad():
        ng = mg(Xt, A.dev(Y), other, 0.07, 1.0, k)
    plain = mg(A.dev(X), A.dev(Y), other, 0.07, 1.0, k)   # no input requires grad
    for outs in (ng, plain):
        assert not outs[0].requires_grad and outs[0].grad_fn is None
        for a, b in zip(outs, full):
            np.testing.assert_array_equal(A.host(a), A.host(b))
    full[0].backward()
    with pytest.raises(RuntimeError):
        full[0].backward()
    # argument handling: shape and dtype of other
    with pytest.raises(ValueError):
        mg(A.dev(X), A.dev(Y), other[:-1], 0.07, 1.0, k)
    with pytest.raises(TypeError):
        mg(A.dev(X), A.dev(Y), other.float(), 0.07, 1.0, k)
    i32 = mg(A.dev(X), A.dev(Y), other.int(), 0.07, 1.0, k)
    assert float(i32[0]) == float(full[0])
    # CPU input: every output comes back on the CPU, the gradient too
    Xc = torch.from_numpy(np.array(X)).requires_grad_(True)
    outs = mg(Xc, torch.from_numpy(np.array(Y)), other.cpu(), 0.07, 1.0, k)
    assert all(o.device.type == "cpu" for o in outs)
    outs[0].backward()
    assert Xc.grad.device.type == "cpu" and float(outs[0]) == float(full[0])
    np.testing.assert_array_equal(Xc.grad.numpy(), A.host(Xt.grad))


def test_batched_graphs_equal_single_calls():
    tags, eps, tau, k = ("T1", "T1s1", "T1s2"), 1.0, 0.07, R.CASES["T1"].k
    Xs = np.stack([R.inputs(g)[0] for g in tags])
    Ys = np.stack([R.inputs(g)[1] for g in tags])
    L = _gll().LaplaceLearningSparseHard
    with torch.no_grad():
        clean = L.margin_loss(A.dev(Xs), A.dev(Ys), None, tau, eps, k)
    other = clean[3]
    assert other.shape == (3, Xs.shape[1] - Ys.shape[1])
    outb = L.margin_loss(A.dev(Xs), A.dev(Ys), other, tau, eps, k)
    assert outb[0].shape == (3,) and outb[5].shape == (3,) and outb[4].shape == other.shape
    for g in range(3):
        out1 = L.margin_loss(A.dev(Xs[g]), A.dev(Ys[g]), other[g], tau, eps, k)
        for a, b in zip(out1, outb):
            np.testing.assert_array_equal(A.host(a), A.host(b[g]))
    with pytest.raises(ValueError):
        L.margin_loss(A.dev(Xs), A.dev(Ys), other[0], tau, eps, k)


def test_three_step_cw_adam_loop():
    """adversarial.py:688-751 around the layer: top-2 once, then Adam steps on w with the margin
    of the best class over the clean runner-up.  Both routes must run through without error and
    stay finite; between them only the runner-up labels and the first step's loss are compared."""
    X, Y, _ = R.inputs("T1")
    c = R.CASES["T1"]
    L = _gll().LaplaceLearningSparseHard

    def attack(fused):
        Xt, Yt = A.dev(X), A.dev(Y)
        base_data, data = Xt[:c.base], Xt[c.base:]
        with torch.no_grad():
            if fused:
                next_pred = L.margin_loss(Xt, Yt, None, 0.07, 1.0, c.k)[3]
            else:
                next_pred = _torch_top2(L.apply(Xt, Yt, 0.07, 1.0, c.k))[1]
        w = data.clone().requires_grad_(True)
        opt = torch.optim.Adam([w], lr=0.01)
        losses = []
        for _ in range(3):
            opt.zero_grad()
            loss1 = torch.pow(w - data, 2).sum() / len(data)
            full = torch.vstack((base_data, w))
            if fused:
                loss2 = L.margin_loss(full, Yt, next_pred, 0.07, 1.0, c.k)[0]
            else:
                loss2 = _gll().cw_margin(L.apply(full, Yt, 0.07, 1.0, c.k), next_pred)
            loss = loss1 + loss2
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        return A.host(w), losses, A.host(next_pred)

    wa, la, na = attack(True)
    wb, lb, nb = attack(False)
    np.testing.assert_array_equal(na, nb)      # T1 is well separated: no tie to disagree on
    e = float(np.linalg.norm(wa - wb) / np.linalg.norm(wb))
    print(f"CW: losses fused {la}, unfused {lb}; perturbed points differ by {e:.2e} (normwise)")
    assert np.isfinite(la).all() and np.isfinite(wa).all()
    # the first step sees the same U: the same terms, summed in another order (margins <= 1).
    # Later steps are not compared: Adam's first update is lr * sign(grad), which turns rounding
    # noise in near-zero gradient entries into full-size steps on either route.
    assert abs(la[0] - lb[0]) <= (4 * c.batch + 8) * U53
