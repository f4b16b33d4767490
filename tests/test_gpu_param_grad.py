"""Gradients of label_matrix, tau and a fixed epsilon on the HIP path (run on the MI355X: -m gpu).

The float64 reference (tests/param_grad_ref.py, pinned to finite differences on the CPU) is fed
the GPU's own kNN lists, as in test_gpu_parity.py.  Bars:
  * grad_Y: ||a - b||_inf / ||b||_inf < 1e-4, the project's parity bar;
  * grad_tau, grad_eps: |g - g_ref| <= 1e-4 * sum |terms_ref| -- the same bar on the magnitude
    that does not cancel (w, U and W are each held to 1e-4).  On the fixture cases the
    reference's |g| / sum |terms| is 0.19 / 0.23 / 0.18 (tau) and 0.078 / 0.097 (eps), so the
    bar is at most 0.13 % of the value: a wrong sign or factor of two cannot pass.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import gll_oracle as O
from tests import abi as A
from tests.golden_io import Case
from tests.param_grad_ref import reference

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _gll():
    from graphlearninglayer_amd import GLL
    return GLL


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    A.need_gpu()


def _scalar(v, grad=True, dtype=torch.float64, dev="cuda"):
    """tau / epsilon as a tensor; 'auto' stays the string."""
    if isinstance(v, str):
        return v
    return torch.tensor(float(v), dtype=dtype, device=dev, requires_grad=grad)


def _run(X, Y, tau, eps, k, gbar, need=(True, True, True, True), python=False):
    """One forward+backward; returns U and the gradients (None where not requested) as numpy.
    need: which of X, label_matrix, tau, epsilon require grad (tau / eps then go in as float64
    tensors on the GPU, otherwise as Python numbers)."""
    GLL = _gll()
    fn = GLL.LaplaceLearningSparseHard.apply_python if python else GLL.LaplaceLearningSparseHard.apply
    Xt = torch.from_numpy(np.ascontiguousarray(X)).cuda().requires_grad_(need[0])
    Yt = torch.from_numpy(np.ascontiguousarray(Y)).cuda().requires_grad_(need[1])
    tt = _scalar(tau) if need[2] else tau
    et = _scalar(eps) if need[3] else eps
    U = fn(Xt, Yt, tt, et, k)
    U.backward(torch.from_numpy(np.ascontiguousarray(gbar)).cuda())
    torch.cuda.synchronize()

    def g(t):
        return None if not torch.is_tensor(t) or t.grad is None else t.grad.detach().cpu().numpy()
    return dict(U=U.detach().cpu().numpy(), X=g(Xt), Y=g(Yt), tau=g(tt), eps=g(et),
                tensors=(Xt, Yt, tt, et))


def _knn(X, k, eps):
    g = _gll().device_graph(torch.from_numpy(np.ascontiguousarray(X)).cuda(), k, eps)
    return g


def _check_against_reference(tag, out, X, Y, tau, eps, k, gbar):
    """The three bars of the module docstring; prints every figure before it asserts."""
    ind = _knn(X, k, eps)["knn_idx"].cpu().numpy().astype(np.int64)
    _, _, ref = reference(X, Y, tau, eps, k, gbar, ind)
    eY = O.rel_err(out["Y"], ref.grad_Y)
    e_tau = abs(float(out["tau"]) - ref.grad_tau) / ref.tau_terms
    line = (f"{tag}: grad_Y rel err {eY:.2e}; grad_tau {float(out['tau']):.8g} vs "
            f"{ref.grad_tau:.8g}, err / sum|terms| {e_tau:.2e} "
            f"(|g| / sum|terms| {abs(ref.grad_tau) / ref.tau_terms:.3f})")
    e_eps = None
    if ref.grad_eps is not None:
        e_eps = abs(float(out["eps"]) - ref.grad_eps) / ref.eps_terms
        line += (f"; grad_eps {float(out['eps']):.8g} vs {ref.grad_eps:.8g}, err / sum|terms| "
                 f"{e_eps:.2e} (|g| / sum|terms| {abs(ref.grad_eps) / ref.eps_terms:.3f})")
    print(line)
    assert out["Y"].shape == ref.grad_Y.shape
    assert eY < TOL, f"grad_Y: {eY:.3e}"
    assert e_tau <= TOL, f"grad_tau: {e_tau:.3e}"
    if e_eps is not None:
        assert e_eps <= TOL, f"grad_eps: {e_eps:.3e}"


@functools.lru_cache(maxsize=None)
def _fixture_run(name, python=False):
    """All four inputs requiring grad on a golden case (shared by the tests below; read-only)."""
    c = Case(name)
    assert c.x_ok
    fixed = not isinstance(c.eps, str)
    return c, _run(c.X, c.Y, c.tau, c.eps, c.k, c.gbar, (True, True, True, fixed), python)


# ------------------------------------------------------------------------------------------
# 1. fixture parity: the fused backward, the two-launch route (auto eps), C = 3
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["plumbing_eps1p0_tau0p07_f32", "plumbing_epsauto_tau0p07_f32",
                                  "ns_eps1p0_tau0p07_f32_C3"])
def test_fixture_parity(name):
    c, out = _fixture_run(name)
    if isinstance(c.eps, str):
        assert c.eps == "auto" and out["eps"] is None   # the string still works beside a tensor tau
    Xt, Yt, tt, et = out["tensors"]
    assert Yt.grad.dtype == Yt.dtype and Yt.grad.shape == Yt.shape and Yt.grad.device == Yt.device
    assert tt.grad.dtype == tt.dtype and tt.grad.shape == tt.shape and tt.grad.device == tt.device
    _check_against_reference(name, out, c.X, c.Y, c.tau, c.eps, c.k, c.gbar)


# ------------------------------------------------------------------------------------------
# 2. the feature gradient does not move
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["plumbing_eps1p0_tau0p07_f32", "plumbing_epsauto_tau0p07_f32"])
def test_feature_gradient_unchanged_bitwise(name):
    c, out = _fixture_run(name)
    only_x = _run(c.X, c.Y, c.tau, c.eps, c.k, c.gbar, (True, False, False, False))
    np.testing.assert_array_equal(out["U"], only_x["U"])
    np.testing.assert_array_equal(out["X"], only_x["X"])
    assert only_x["Y"] is None


# ------------------------------------------------------------------------------------------
# 3. labels only
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_labels_only(dtype):
    c, full = _fixture_run("plumbing_eps1p0_tau0p07_f32")
    out = _run(c.X, c.Y.astype(dtype), c.tau, c.eps, c.k, c.gbar, (False, True, False, False))
    Xt, Yt, _, _ = out["tensors"]
    assert Xt.grad is None
    assert Yt.grad is not None and Yt.grad.dtype == Yt.dtype and Yt.grad.shape == Yt.shape
    assert out["Y"].dtype == dtype
    np.testing.assert_array_equal(out["Y"], full["Y"].astype(dtype))   # fp32 kernel output
    ind = _knn(c.X, c.k, c.eps)["knn_idx"].cpu().numpy().astype(np.int64)
    _, _, ref = reference(c.X, c.Y, c.tau, c.eps, c.k, c.gbar, ind)
    assert O.rel_err(out["Y"], ref.grad_Y) < TOL


# ------------------------------------------------------------------------------------------
# 4. the native node and the Python function agree bitwise
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["plumbing_eps1p0_tau0p07_f32", "plumbing_epsauto_tau0p07_f32"])
def test_native_and_python_paths_agree_bitwise(name):
    _, a = _fixture_run(name)
    _, b = _fixture_run(name, python=True)
    for key in ("U", "X", "Y", "tau", "eps"):
        if a[key] is None:
            assert b[key] is None, key
        else:
            np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    assert a["Y"] is not None and a["tau"] is not None


# ------------------------------------------------------------------------------------------
# 5. determinism and batching
# ------------------------------------------------------------------------------------------
def test_two_runs_and_batch_of_one_are_bitwise_equal():
    c, a = _fixture_run("plumbing_eps1p0_tau0p07_f32")
    b = _run(c.X, c.Y, c.tau, c.eps, c.k, c.gbar)
    one = _run(c.X[None], c.Y[None], c.tau, c.eps, c.k, c.gbar[None])
    for key in ("Y", "tau", "eps"):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
        np.testing.assert_array_equal(a[key], one[key].reshape(a[key].shape), err_msg=key)


def test_batched_graphs_equal_single_calls():
    from graphlearninglayer_amd.synth import CONFIGS, one_hot, seeded_gbar, synth
    cfg = CONFIGS["plumbing"]
    B, tau, eps, k = 3, 0.07, 1.0, cfg["k"]
    Xs, Ys = [], []
    for g in range(B):
        X, lab = synth(cfg["base"], cfg["batch"], cfg["d"], r=cfg["r"], seed=40 + g)
        Xs.append(X)
        Ys.append(one_hot(np.roll(lab[: cfg["base"]], g)))   # distinct labels per graph
    Xs, Ys = np.stack(Xs), np.stack(Ys)
    G = np.stack([seeded_gbar(cfg["batch"], 10, 500 + g) for g in range(B)])
    singles = [_run(Xs[g], Ys[g], tau, eps, k, G[g]) for g in range(B)]
    bat = _run(Xs, Ys, tau, eps, k, G)
    assert bat["Y"].shape == Ys.shape
    for g in range(B):
        np.testing.assert_array_equal(bat["Y"][g], singles[g]["Y"])
    for key in ("tau", "eps"):
        want = float(np.sum([np.float64(s[key]) for s in singles]))
        assert abs(float(bat[key]) - want) <= 1e-12 * abs(want), key
    # one 2-D label matrix shared by the batch: its gradient is the sum over the graphs
    shared_singles = [_run(Xs[g], Ys[0], tau, eps, k, G[g], (False, True, False, False))
                      for g in range(B)]
    shared = _run(Xs, Ys[0], tau, eps, k, G, (False, True, False, False))
    assert shared["Y"].shape == Ys[0].shape
    want = np.sum([s["Y"].astype(np.float64) for s in shared_singles], axis=0)
    assert O.rel_err(shared["Y"], want) <= 1e-6


# ------------------------------------------------------------------------------------------
# 6. a hub row: longer than a wave and than the row slot (bump region)
# ------------------------------------------------------------------------------------------
def test_hub_row():
    from graphlearninglayer_amd.synth import one_hot, seeded_gbar, synth
    n, base, d, k, C, tau, eps = 400, 40, 32, 5, 4, 0.07, 1.0
    X, lab = synth(base, n - base, d, C=C, r=0.75, seed=9)
    rng = np.random.default_rng(17)
    X[0] = 0.0
    X[0, 0] = 1.0
    hub = X[0] + 0.3 * rng.standard_normal((300, d))
    X[40:340] = (hub / np.linalg.norm(hub, axis=1, keepdims=True)).astype(np.float32)
    Y = one_hot(lab[:base], C)
    gbar = seeded_gbar(n - base, C, 23)
    g = _knn(X, k, eps)
    rp = g["row_ptr"].cpu().numpy()
    row0 = int(rp[1] - rp[0])
    print(f"hub row 0: {row0} entries (slot width {5 * (k - 1) + 8})")
    assert row0 > 64
    out = _run(X, Y, tau, eps, k, gbar)
    _check_against_reference("hub", out, X, Y, tau, eps, k, gbar)


# ------------------------------------------------------------------------------------------
# 7. m > 2048: Wadj as the whole-GPU CG writes it
# ------------------------------------------------------------------------------------------
def test_whole_gpu_cg_route():
    from graphlearninglayer_amd.synth import one_hot, seeded_gbar, synth
    base, m, d, k, C, tau, eps = 256, 2304, 64, 8, 4, 0.07, 1.0
    X, lab = synth(base, m, d, C=C, r=1.0, seed=13)
    Y = one_hot(lab[:base], C)
    gbar = seeded_gbar(m, C, 29)
    out = _run(X, Y, tau, eps, k, gbar)
    _check_against_reference("grid_cg", out, X, Y, tau, eps, k, gbar)


# ------------------------------------------------------------------------------------------
# 8. argument handling
# ------------------------------------------------------------------------------------------
def test_argument_handling():
    GLL = _gll()
    c, full = _fixture_run("plumbing_eps1p0_tau0p07_f32")
    X = torch.from_numpy(c.X).cuda()
    Y = torch.from_numpy(c.Y).cuda()
    gbar = torch.from_numpy(c.gbar).cuda()
    for fn in (GLL.LaplaceLearningSparseHard.apply, GLL.LaplaceLearningSparseHard.apply_python):
        for bad in (0.0, -1.0):
            with pytest.raises(ValueError):
                fn(X, Y, c.tau, torch.tensor(bad, device="cuda", requires_grad=True), c.k)
        # floats: exactly the node of before -- X and label_matrix edges only, the same U and X.grad
        Xr = X.clone().requires_grad_(True)
        U = fn(Xr, Y, c.tau, c.eps, c.k)
        np.testing.assert_array_equal(U.detach().cpu().numpy(), full["U"])
        (gx,) = torch.autograd.grad(U, Xr, gbar)
        np.testing.assert_array_equal(gx.cpu().numpy(), full["X"])
        assert fn(X, Y, c.tau, c.eps, c.k).grad_fn is None   # nothing requires grad: no node
        # a CPU tau beside GPU features: its gradient comes back on the CPU, in its dtype and shape
        tau = torch.tensor([c.tau], dtype=torch.float32, requires_grad=True)
        U = fn(X, Y, tau, c.eps, c.k)
        U.backward(gbar)
        assert tau.grad.device.type == "cpu" and tau.grad.dtype == torch.float32
        assert tau.grad.shape == (1,)
        assert float(tau.grad) == float(np.float32(full["tau"]))
    Xr = X.clone().requires_grad_(True)
    U = GLL.LaplaceLearningSparseHard.apply(Xr, Y, c.tau, c.eps, c.k)
    assert len(U.grad_fn.next_functions) == 2
    assert U.grad_fn.next_functions[1][0] is None   # label_matrix needs no gradient


# ------------------------------------------------------------------------------------------
# 9. the extra pass runs only when a parameter gradient is requested
# ------------------------------------------------------------------------------------------
def test_param_kernel_launches_only_on_request():
    from graphlearninglayer_amd import _lib
    c = Case("plumbing_eps1p0_tau0p07_f32")
    # raw: one bracket read three times, its milliseconds too; pairs left unread are dropped first
    _lib.prof_read(_lib.K_PARAM)
    _lib.prof_enable(_lib.K_PARAM, 1)
    try:
        _run(c.X, c.Y, c.tau, c.eps, c.k, c.gbar, (True, False, False, False))
        assert _lib.prof_read(_lib.K_PARAM)[1] == 0
        _run(c.X, c.Y, c.tau, c.eps, c.k, c.gbar, (True, True, False, False))
        assert _lib.prof_read(_lib.K_PARAM)[1] == 1
        _run(c.X, c.Y, c.tau, c.eps, c.k, c.gbar, (True, True, True, True))
        ms, cnt = _lib.prof_read(_lib.K_PARAM)
        assert cnt == 1 and ms > 0.0
    finally:
        _lib.prof_enable(_lib.K_PARAM, 0)
        _lib.prof_read(_lib.K_PARAM)
