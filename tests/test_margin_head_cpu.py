"""CPU checks of the Carlini-Wagner margin head: the C ABI declarations and argument validation
(no GPU call is made), the float64 yardstick itself (tests/margin_ref.py against torch.autograd
of the reference's own expression, adversarial.py:688-725, and on hand-made rows), and the
conditioning of the inputs the GPU tests compare labels on (on the float64 oracle)."""
import ctypes as ct
import functools
import os
import re

import numpy as np
import pytest
import torch

from graphlearninglayer_amd import GLL as G
from graphlearninglayer_amd import _lib
from oracle import gll_oracle as O
from tests import ce_head_ref as R
from tests import margin_ref as M
from tests.margin_ref import LAYER_CASES, WELL_SEPARATED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_exports_declare_the_margin_head():
    src = open(os.path.join(ROOT, "include", "gll.h")).read()
    for name in ("gll_margin_head_scratch_bytes", "gll_margin_head_batched"):
        assert re.search(r"^\w[\w\s\*]*?\b" + name + r"\s*\(", src, flags=re.M), name
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name)
    for name, val in (("GLL_K_LOSS", _lib.K_LOSS), ("GLL_K_COUNT", _lib.K_COUNT)):
        assert int(re.search(r"#define\s+" + name + r"\s+(\d+)", src).group(1)) == val
    assert _lib.K_LOSS == 8 and _lib.K_COUNT == 9
    assert _lib.kernel_name(_lib.K_LOSS) == "ce_head_kernel"
    assert "adversarial.py:688-751" in src


def test_margin_head_rejects_bad_arguments_without_touching_the_gpu():
    """Every case returns before anything is launched, so the pointers are never followed:
    0x1000 only stands for 'not NULL'."""
    lib = _lib.lib()
    call = lib.gll_margin_head_batched
    p = G.make_problem(100, 16, 50, 10, 5, 0.07, 1.0)
    nn = 0x1000
    assert call(None, 1, nn, nn, nn, nn, nn, nn, nn, nn, nn, None) == -1           # no problem
    assert call(ct.byref(p), 1, None, nn, nn, nn, nn, nn, nn, nn, nn, None) == -1  # no workspace
    assert call(ct.byref(p), 1, nn, nn, None, nn, nn, nn, nn, nn, nn, None) == -1  # no loss
    assert call(ct.byref(p), 0, nn, nn, nn, nn, nn, nn, nn, nn, nn, None) == -1    # B out of range
    assert call(ct.byref(p), 65536, nn, nn, nn, nn, nn, nn, nn, nn, nn, None) == -1
    bad = G.make_problem(100, 16, 50, 10, 5, 0.07, 1.0)
    bad.K = 1
    assert call(ct.byref(bad), 1, nn, nn, nn, nn, nn, nn, nn, nn, nn, None) == -1  # bad problem
    wide = G.make_problem(100, 16, 50, 10, 5, 0.07, 1.0)
    wide.C = 257
    assert call(ct.byref(wide), 1, nn, nn, nn, nn, nn, nn, nn, nn, nn, None) != 0  # C <= 256
    sb = lib.gll_margin_head_scratch_bytes
    assert sb(ct.byref(p), 1) == 0 and sb(ct.byref(p), 7) == 0
    assert sb(ct.byref(G.make_problem(4096 + 50, 16, 50, 10, 5, 0.07, 1.0)), 3) == 0
    big = G.make_problem(5000, 16, 100, 10, 5, 0.07, 1.0)
    assert sb(ct.byref(big), 1) >= 4900 * 12
    assert sb(ct.byref(big), 3) == 3 * sb(ct.byref(big), 1)
    assert sb(ct.byref(big), 0) == 0 and sb(None, 1) == 0
    assert call(ct.byref(big), 1, nn, nn, nn, nn, nn, nn, nn, nn, None, None) == -1  # no scratch


def test_python_surface():
    from graphlearninglayer_amd import LaplaceLearningSparseHard, cw_margin
    assert LaplaceLearningSparseHard.margin_loss is G._ext().margin_loss   # native, no wrapper
    assert callable(LaplaceLearningSparseHard.margin_loss_python)
    assert cw_margin is G.cw_margin
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="GPU"):
            LaplaceLearningSparseHard.margin_loss(torch.zeros(10, 4), torch.zeros(5, 2), None,
                                                  0.0, 1.0)
    with pytest.raises(TypeError):
        LaplaceLearningSparseHard.margin_loss(torch.zeros(10, 4), torch.zeros(5, 2),
                                              torch.zeros(5), 0.0, 1.0)   # float `other`
    with pytest.raises(TypeError):
        LaplaceLearningSparseHard.margin_loss(torch.zeros(10, 4), torch.zeros(5, 2))


# ------------------------------------------------------------------------------------------
# the yardstick against the reference's own expression
# ------------------------------------------------------------------------------------------
def _reference_cw(U, other=None):
    """adversarial.py:688-692 (the -1e6 edit) and loss2 of :725 with c = 1, divided by m, in
    float64 torch on the CPU; returns (init_pred, next_pred, loss, dloss/dU for next_pred or
    `other`)."""
    out = torch.from_numpy(np.array(U, dtype=np.float64))
    idx = torch.arange(out.shape[0])
    edit = out.clone()
    init_pred = edit.max(1, keepdim=False)[1]
    edit[idx, init_pred] = -1000000
    next_pred = edit.max(1, keepdim=False)[1]
    o = next_pred if other is None else torch.from_numpy(np.asarray(other))
    out.requires_grad_(True)
    loss = torch.clamp(torch.max(out, 1)[0] - out[idx, o], min=0).sum() / out.shape[0]
    loss.backward()
    return init_pred.numpy(), next_pred.numpy(), float(loss.detach()), out.grad.numpy()


@pytest.mark.parametrize("m,C,seed", [(1, 2, 0), (7, 3, 1), (64, 10, 2), (33, 17, 3), (5, 200, 4)])
def test_reference_matches_torch_on_tie_free_rows(m, C, seed):
    """Random tie-free rows (values above -1e6, so the edit finds the runner-up).  Every term of
    the loss is the same float64 difference in both; the sums differ in order only, which the
    summation bound (4 m + 8) 2^-53 mean|row_margin| covers (test_gpu_ce_head.py's form).  The
    gradient entries are 1/m in float64 there and float32(1/m) here: 2^-24 relative."""
    rng = np.random.default_rng(seed)
    U = rng.standard_normal((m, C)).astype(np.float32)
    U[::3] *= -1                      # negatives at the top as well
    assert len(np.unique(U)) == U.size
    a, s, _, _ = _reference_cw(U)
    other = rng.integers(0, C, size=m)
    other[::2] = s[::2]               # the attack's choice on half the rows, anything elsewhere
    if m > 2:
        other[1] = a[1]               # an already-flipped row
    _, _, loss, grad = _reference_cw(U, other)
    ref = M.margin_head(U, other)
    np.testing.assert_array_equal(ref.labels, a)
    np.testing.assert_array_equal(ref.second, s)
    assert abs(ref.loss - loss) <= (4 * m + 8) * 2.0 ** -53 * np.mean(np.abs(ref.row_margin))
    assert ref.moved == int((a == other).sum())
    np.testing.assert_array_equal(np.sign(ref.gbar), np.sign(grad))
    hot = grad != 0
    assert np.all(np.abs(ref.gbar[hot] - grad[hot]) <= 2.0 ** -24 * np.abs(grad[hot]))
    # other = None is the pure top-2 query
    q = M.margin_head(U)
    np.testing.assert_array_equal(q.labels, a)
    np.testing.assert_array_equal(q.second, s)
    assert q.loss == 0.0 and q.moved == 0 and not q.gbar.any() and not q.row_margin.any()


# ------------------------------------------------------------------------------------------
# the yardstick on hand-made rows
# ------------------------------------------------------------------------------------------
def test_reference_on_hand_made_rows():
    f = np.float32
    g = f(1.0 / 8)
    U = np.array([[0.2, 0.5, 0.5, 0.1],      # 0: tie at first place: a = 1, s = 2
                  [0.7, 0.1, 0.1, 0.05],     # 1: tie at second place: s = 1
                  [0.1, 0.6, 0.2, 0.1],      # 2: a == other
                  [0.3, 0.4, 0.2, 0.1],      # 3: other = -1
                  [0.3, 0.4, 0.2, 0.1],      # 4: other = C
                  [np.nan, 0.4, 0.5, 0.1],   # 5: a NaN entry, other on it: the margin is NaN
                  [np.nan, 0.4, 0.5, 0.1],   # 6: a NaN entry, other elsewhere
                  [-3.0, -1.0, -2.0, -4.0]],  # 7: negatives
                 dtype=f)
    other = np.array([2, 2, 1, -1, 4, 0, 1, 3])
    r = M.margin_head(U, other)
    np.testing.assert_array_equal(r.labels, [1, 0, 1, 1, 1, 2, 2, 1])
    np.testing.assert_array_equal(r.second, [2, 1, 2, 0, 0, 1, 1, 2])
    want = np.array([0.0, np.float64(f(0.7)) - np.float64(f(0.1)), 0.0, 0.0, 0.0, np.nan,
                     np.float64(f(0.5)) - np.float64(f(0.4)), 3.0])
    np.testing.assert_array_equal(r.row_margin, want)
    assert np.isnan(r.loss)
    assert r.moved == 1                                    # row 2 alone: row 0 has a = 1, other = 2
    G_ = np.zeros((8, 4), dtype=f)
    G_[0, 1], G_[0, 2] = g, -g                             # a tie still pulls the two apart
    G_[1, 0], G_[1, 2] = g, -g
    G_[5, 2], G_[5, 0] = g, -g                             # NaN margin: the gradient passes
    G_[6, 2], G_[6, 1] = g, -g
    G_[7, 1], G_[7, 3] = g, -g
    np.testing.assert_array_equal(r.gbar, G_)
    assert r.gbar.dtype == np.float32
    # without the NaN rows the loss is the mean over all m rows, masked ones included
    keep = [0, 1, 2, 3, 4, 7]
    r6 = M.margin_head(U[keep], other[keep])
    assert r6.loss == np.sum(r6.row_margin) / 6 and r6.loss > 0.5
    # C = 1: s = 0, and other = 0 is a == other
    r1 = M.margin_head(np.array([[0.3], [np.nan]], dtype=f), np.array([0, 5]))
    np.testing.assert_array_equal(r1.labels, [0, 0])
    np.testing.assert_array_equal(r1.second, [0, 0])
    assert r1.moved == 1 and r1.loss == 0.0 and not r1.gbar.any()
    # a row of NaN and a row of -inf: lowest indices
    r2 = M.margin_head(np.array([[np.nan] * 3, [-np.inf] * 3, [np.nan, -np.inf, np.nan]], dtype=f))
    np.testing.assert_array_equal(r2.labels, [0, 0, 1])
    np.testing.assert_array_equal(r2.second, [1, 1, 0])
    # the same first label as the cross-entropy head's yardstick
    np.testing.assert_array_equal(r.labels[[0, 1, 2, 3, 4, 7]],
                                  R.ce_head(U[[0, 1, 2, 3, 4, 7]], other[[0, 1, 2, 3, 4, 7]]).pred_label)


# ------------------------------------------------------------------------------------------
# conditioning of the layer-level GPU cases
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_U(tag, eps, tau):
    X, Y, _ = R.inputs(tag)
    U, _ = O.forward(X, Y, tau, eps, R.CASES[tag].k)
    return U


@pytest.mark.parametrize("tag,eps,tau", LAYER_CASES)
def test_layer_cases_have_no_tie_on_the_oracle(tag, eps, tau):
    """The GPU test compares labels and second with torch's on the GPU's own U, where only an
    exact tie at the compared rank can make the two differ (torch promises no tie rule).  Here,
    on the float64 oracle: no case has an exact tie at first or second place, and the cases in
    WELL_SEPARATED keep both gaps above the 1e-4 parity tolerance, so the fp32 route cannot tie
    there and the GPU test leaves no row of them out.  The other cases have a few rows inside
    1e-4 (printed); there the GPU test may leave exactly tied rows out, at most 1% of m."""
    U = _oracle_U(tag, eps, tau)
    g12, g23 = M.top3_gaps(U)
    s = np.sort(U, axis=1)
    near = (s[:, -1] - s[:, -2] <= 1e-4) | (s[:, -2] - s[:, -3] <= 1e-4)
    print(f"{tag} eps={eps} tau={tau}: min top-1/2 gap {g12:.3g}, min top-2/3 gap {g23:.3g}, "
          f"{int(near.sum())} of {len(U)} rows within 1e-4")
    assert g12 > 0 and g23 > 0
    if (tag, eps, tau) in WELL_SEPARATED:
        assert g12 > 1e-4 and g23 > 1e-4
