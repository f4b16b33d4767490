"""CPU checks of the label_matrix / tau / epsilon gradients: the float64 yardstick itself
(tests/param_grad_ref.py against central finite differences of the oracle with the kNN frozen)
and the argument validation of the two C ABI calls (no GPU call is made)."""
import ctypes as ct
import os
import re

import numpy as np
import pytest

from graphlearninglayer_amd import GLL as G
from graphlearninglayer_amd import _lib
from graphlearninglayer_amd.synth import one_hot, seeded_gbar, synth
from oracle import gll_oracle as O
from oracle.graphlearning_standin import knn_exact
from tests.param_grad_ref import param_grads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, BASE, C, K, TAU = 96, 24, 3, 6, 0.07


@pytest.fixture(scope="module")
def case():
    X, lab = synth(BASE, N - BASE, 16, C=C, r=0.75, seed=5)
    X = X.astype(np.float64)
    Y = one_hot(lab[:BASE], C).astype(np.float64)
    # soft labels: a generic point, not a corner of the simplex
    Y = 0.8 * Y + 0.2 * np.random.default_rng(3).random(Y.shape)
    gbar = seeded_gbar(N - BASE, C, 7)
    return X, Y, gbar, knn_exact(X, K)


def _loss(X, Y, tau, eps, gbar, knn):
    U, _ = O.forward(X, Y, tau, eps, K, knn=knn)
    return float(np.sum(gbar * U))


@pytest.mark.parametrize("eps", [0.9, "auto"])
def test_closed_form_matches_finite_differences(case, eps):
    """Central differences of <gbar, U> with the kNN lists and distances frozen.  The loss is
    linear in Y (the difference is exact up to the float64 solve) and smooth in tau and eps.
    With h = 1e-5 the round-off is ~ 1e-16 / h = 1e-11 relative; the truncation error is
    h^2 f''' / 6 f', and along tau f is a sum of 1 / (lambda + tau) modes, so f''' / f' is at
    most 6 / tau^2 = 1.2e3 at tau = 0.07: 2e-8 relative at worst.  The bar of 1e-7 sits above
    that and still sees any wrong sign, factor or missing term."""
    X, Y, gbar, knn = case
    _, st = O.forward(X, Y, TAU, eps, K, knn=knn)
    pg = param_grads(st, gbar)
    h = 1e-5
    fdY = np.zeros_like(Y)
    for j in range(BASE):
        for c in range(C):
            Yp, Ym = Y.copy(), Y.copy()
            Yp[j, c] += h
            Ym[j, c] -= h
            fdY[j, c] = (_loss(X, Yp, TAU, eps, gbar, knn) - _loss(X, Ym, TAU, eps, gbar, knn)) / (2 * h)
    eY = O.rel_err(pg.grad_Y, fdY)
    fd_tau = (_loss(X, Y, TAU + h, eps, gbar, knn) - _loss(X, Y, TAU - h, eps, gbar, knn)) / (2 * h)
    e_tau = abs(pg.grad_tau - fd_tau) / abs(fd_tau)
    print(f"eps={eps}: grad_Y rel err {eY:.2e}; grad_tau {pg.grad_tau:.10f} vs {fd_tau:.10f}")
    assert eY < 1e-7 and e_tau < 1e-7
    assert pg.tau_terms >= abs(pg.grad_tau)
    if eps == "auto":
        assert pg.grad_eps is None and pg.eps_terms is None   # no epsilon input
    else:
        fd_eps = (_loss(X, Y, TAU, eps + h, gbar, knn) - _loss(X, Y, TAU, eps - h, gbar, knn)) / (2 * h)
        print(f"grad_eps {pg.grad_eps:.10f} vs {fd_eps:.10f}")
        assert abs(pg.grad_eps - fd_eps) / abs(fd_eps) < 1e-7
        assert pg.eps_terms >= abs(pg.grad_eps)


def test_header_and_exports_declare_the_param_grad_calls():
    src = open(os.path.join(ROOT, "include", "gll.h")).read()
    for name in ("gll_param_grad_scratch_bytes", "gll_param_grad_batched"):
        assert re.search(r"^\w[\w\s\*]*?\b" + name + r"\s*\(", src, flags=re.M), name
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name)
    for name, val in (("GLL_PG_Y", _lib.PG_Y), ("GLL_PG_TAU", _lib.PG_TAU),
                      ("GLL_PG_EPS", _lib.PG_EPS), ("GLL_K_PARAM", _lib.K_PARAM),
                      ("GLL_K_COUNT", _lib.K_COUNT)):
        assert int(re.search(r"#define\s+" + name + r"\s+(\d+)", src).group(1)) == val
    assert _lib.kernel_name(_lib.K_PARAM) == "param_grad_kernel"
    assert _lib.lib().gll_prof_enable(_lib.K_PARAM, 0) == 0


def test_param_grad_rejects_bad_arguments_without_touching_the_gpu():
    """Every case returns before anything is launched, so the pointers are never followed:
    0x1000 only stands for 'not NULL'."""
    lib = _lib.lib()
    call = lib.gll_param_grad_batched
    p = G.make_problem(100, 16, 50, 10, 5, 0.07, 1.0)
    pa = G.make_problem(100, 16, 50, 10, 5, 0.07, "auto")
    nn = 0x1000
    every = _lib.PG_Y | _lib.PG_TAU | _lib.PG_EPS
    assert call(None, 1, nn, every, nn, nn, nn, nn, None) == -1             # no problem
    assert call(ct.byref(p), 1, None, every, nn, nn, nn, nn, None) == -1    # no workspace
    assert call(ct.byref(p), 1, nn, _lib.PG_Y, None, None, None, None, None) == -1
    assert call(ct.byref(p), 1, nn, _lib.PG_TAU, None, None, None, nn, None) == -1
    assert call(ct.byref(p), 1, nn, _lib.PG_EPS, None, None, None, nn, None) == -1
    assert call(ct.byref(p), 1, nn, _lib.PG_TAU, None, nn, None, None, None) == -1   # no scratch
    assert call(ct.byref(p), 0, nn, every, nn, nn, nn, nn, None) == -1      # B out of range
    assert call(ct.byref(p), 65536, nn, every, nn, nn, nn, nn, None) == -1
    assert call(ct.byref(p), 1, nn, 8, nn, nn, nn, nn, None) == -1          # unknown bit
    assert call(ct.byref(p), 1, nn, every | 16, nn, nn, nn, nn, None) == -1
    assert call(ct.byref(pa), 1, nn, _lib.PG_EPS, None, None, nn, nn, None) == -1    # 'auto'
    # no labeled rows: the label gradient is empty -- OK, nothing written, nothing launched
    p0 = G.make_problem(100, 16, 0, 10, 5, 0.07, 1.0)
    assert call(ct.byref(p0), 1, nn, _lib.PG_Y, None, None, None, None, None) == 0
    # scratch: two float64 partials per row and graph
    sb = lib.gll_param_grad_scratch_bytes
    assert sb(ct.byref(p), 1) >= 2 * 100 * 8
    assert sb(ct.byref(p), 3) == 3 * sb(ct.byref(p), 1)
    assert sb(ct.byref(p), 0) == 0 and sb(None, 1) == 0
