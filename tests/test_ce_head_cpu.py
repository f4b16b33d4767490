"""CPU checks of the cross-entropy head: the float64 yardstick itself (tests/ce_head_ref.py
against central finite differences of its own loss), the conditioning of the inputs the GPU
tests use (on the float64 oracle), the C ABI declarations and its argument validation (no GPU
call is made)."""
import ctypes as ct
import functools
import os
import re

import numpy as np
import pytest

from graphlearninglayer_amd import GLL as G
from graphlearninglayer_amd import _lib
from oracle import gll_oracle as O
from tests import ce_head_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _oracle_U(tag, eps, tau):
    X, Y, _ = R.inputs(tag)
    U, _ = O.forward(X, Y, tau, eps, R.CASES[tag].k)
    U.setflags(write=False)
    return U


def test_reference_gradient_matches_finite_differences():
    """gbar = dloss/dU by central differences on T1's oracle U.  With h = 1e-6 and p >= 0.019
    the truncation error h^2 / (3 p^2) is below 1e-9 relative and the round-off
    2^-53 * loss / h ~ 1e-10 absolute against entries >= 1 / m = 0.016: the bar of 1e-6 relative
    sits far above both and still sees a wrong sign, factor or divisor."""
    U = _oracle_U("T1", 1.0, 0.07)
    _, _, t = R.inputs("T1")
    ref = R.ce_head(U, t)
    h = 1e-6
    fd = np.zeros_like(ref.gbar)
    for i in range(U.shape[0]):
        for c in range(U.shape[1]):
            Up, Um = U.copy(), U.copy()
            Up[i, c] += h
            Um[i, c] -= h
            fd[i, c] = (R.ce_head(Up, t).loss - R.ce_head(Um, t).loss) / (2 * h)
    hot = np.zeros(U.shape, dtype=bool)
    hot[np.arange(len(t)), t] = True
    err = float(np.max(np.abs(ref.gbar[hot] - fd[hot]) / np.abs(fd[hot])))
    print(f"max relative error at the target entries {err:.2e}")
    assert err < 1e-6
    assert (ref.gbar[~hot] == 0).all() and (fd[~hot] == 0).all()
    assert abs(ref.loss - np.mean(ref.row_loss)) <= 1e-15 * abs(ref.loss)


def test_reference_masks_targets_outside_the_classes():
    U = _oracle_U("T1", 1.0, 0.07)
    _, _, t = R.inputs("T1")
    full = R.ce_head(U, t)
    tm = t.copy()
    tm[::4] = -1
    tm[1:9:4] = U.shape[1]
    out = np.nonzero((tm < 0) | (tm >= U.shape[1]))[0]
    ref = R.ce_head(U, tm)
    assert (ref.row_loss[out] == 0).all() and (ref.gbar[out] == 0).all()
    keep = np.setdiff1d(np.arange(len(t)), out)
    np.testing.assert_array_equal(ref.row_loss[keep], full.row_loss[keep])
    np.testing.assert_array_equal(ref.gbar[keep], full.gbar[keep])     # the divisor is still m
    assert ref.loss == np.sum(full.row_loss[keep]) / len(t)
    np.testing.assert_array_equal(ref.pred_label, full.pred_label)
    assert ref.correct == int(np.sum(full.pred_label[keep] == t[keep]))


@pytest.mark.parametrize("tag,eps,tau", [s for s in R.SETTINGS if s[0] != "T6"])
def test_inputs_are_well_conditioned_on_the_oracle(tag, eps, tau):
    """T1-T5: every target probability >= 1e-3 and no argmax near-tie (top-2 gap >= 1e-4), so
    fp32 solves cannot flip a label or blow a row loss up."""
    U = _oracle_U(tag, eps, tau)
    _, _, t = R.inputs(tag)
    pt = U[np.arange(len(t)), t]
    gap = R.top2_gap(U)
    print(f"{tag} eps={eps} tau={tau}: min p_t {pt.min():.3g}, min top-2 gap {gap:.3g}")
    assert pt.min() >= 1e-3
    assert gap >= 1e-4


def test_header_and_exports_declare_the_ce_head():
    src = open(os.path.join(ROOT, "include", "gll.h")).read()
    for name in ("gll_ce_head_scratch_bytes", "gll_ce_head_batched"):
        assert re.search(r"^\w[\w\s\*]*?\b" + name + r"\s*\(", src, flags=re.M), name
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name)
    for name, val in (("GLL_K_LOSS", _lib.K_LOSS), ("GLL_K_COUNT", _lib.K_COUNT)):
        assert int(re.search(r"#define\s+" + name + r"\s+(\d+)", src).group(1)) == val
    assert _lib.K_LOSS == 8 and _lib.K_COUNT == 9
    assert _lib.kernel_name(_lib.K_LOSS) == "ce_head_kernel"
    assert _lib.lib().gll_prof_enable(_lib.K_LOSS, 0) == 0
    assert "losses.py:128-136" in src and "FullySup.py:156-171" in src


def test_ce_head_rejects_bad_arguments_without_touching_the_gpu():
    """Every case returns before anything is launched, so the pointers are never followed:
    0x1000 only stands for 'not NULL'."""
    lib = _lib.lib()
    call = lib.gll_ce_head_batched
    p = G.make_problem(100, 16, 50, 10, 5, 0.07, 1.0)
    nn = 0x1000
    assert call(None, 1, nn, nn, nn, nn, nn, nn, nn, nn, None) == -1              # no problem
    assert call(ct.byref(p), 1, None, nn, nn, nn, nn, nn, nn, nn, None) == -1     # no workspace
    assert call(ct.byref(p), 1, nn, None, nn, nn, nn, nn, nn, nn, None) == -1     # no targets
    assert call(ct.byref(p), 1, nn, nn, None, nn, nn, nn, nn, nn, None) == -1     # no loss
    assert call(ct.byref(p), 0, nn, nn, nn, nn, nn, nn, nn, nn, None) == -1       # B out of range
    assert call(ct.byref(p), 65536, nn, nn, nn, nn, nn, nn, nn, nn, None) == -1
    bad = G.make_problem(100, 16, 50, 10, 5, 0.07, 1.0)
    bad.K = 1
    assert call(ct.byref(bad), 1, nn, nn, nn, nn, nn, nn, nn, nn, None) == -1     # bad problem
    # scratch: none while a graph's rows fit one workgroup (covers m <= 2048), required past it
    sb = lib.gll_ce_head_scratch_bytes
    assert sb(ct.byref(p), 1) == 0 and sb(ct.byref(p), 7) == 0
    assert sb(ct.byref(G.make_problem(2048 + 50, 16, 50, 10, 5, 0.07, 1.0)), 3) == 0
    big = G.make_problem(5000, 16, 100, 10, 5, 0.07, 1.0)
    assert sb(ct.byref(big), 1) >= 4900 * 12
    assert sb(ct.byref(big), 3) == 3 * sb(ct.byref(big), 1)
    assert sb(ct.byref(big), 0) == 0 and sb(None, 1) == 0
    assert call(ct.byref(big), 1, nn, nn, nn, nn, nn, nn, nn, None, None) == -1   # scratch missing


def test_python_surface():
    import torch
    from graphlearninglayer_amd import LaplaceLearningSparseHard, custom_ce_loss
    assert LaplaceLearningSparseHard.ce_loss is G._ext().ce_loss   # the native function, no wrapper
    assert callable(LaplaceLearningSparseHard.ce_loss_python)
    U = torch.from_numpy(np.array(_oracle_U("T1", 1.0, 0.07)))
    _, _, t = R.inputs("T1")
    ref = R.ce_head(U.numpy(), t)
    got = float(custom_ce_loss(U, torch.from_numpy(np.array(t))))
    assert abs(got - ref.loss) <= 1e-14 * abs(ref.loss)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="GPU"):
            LaplaceLearningSparseHard.ce_loss(torch.zeros(10, 4), torch.zeros(5, 2),
                                              torch.zeros(5, dtype=torch.int64), 0.0, 1.0)
