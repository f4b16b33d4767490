"""CPU checks of the score/objective head and DeviceScoreStore: the float64 yardstick itself
(tests/objective_ref.py against central finite differences of its own loss, its masking and
zero-weight rules), the store against the plain-Python selection rule, the C ABI declarations
and their argument validation (no GPU call is made)."""
import ctypes as ct
import functools
import os
import re

import numpy as np
import pytest
import torch

from graphlearninglayer_amd import GLL as G
from graphlearninglayer_amd import _lib
from graphlearninglayer_amd.base_data import DeviceBaseLoader, DeviceScoreStore
from oracle import gll_oracle as O
from tests import ce_head_ref as R
from tests import objective_ref as OB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _oracle_U(tag, eps, tau):
    X, Y, _ = R.inputs(tag)
    U, _ = O.forward(X, Y, tau, eps, R.CASES[tag].k)
    U.setflags(write=False)
    return U


# ------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", OB.WEIGHTS, ids=str)
def test_reference_gradient_matches_finite_differences(weights):
    """gbar = dloss/dU by central differences on T1's oracle U (every entry >= 1.4e-4, every
    target entry >= 0.019).  With h = 1e-7 the truncation error is h^2 / 6 times the third
    derivative: (1/m) h^2 / (6 u^2) <= 8.5e-8 / m for the entropy term, less for the others.
    The round-off of the difference of two O(1) float64 losses over 2 h is about
    sqrt(m) 2^-53 / (2 h) = 4e-9 against entries of order 1 / m = 1.6e-2.  The bar of
    1e-5 max(|fd|, 1 / m) sits above both and still sees a wrong sign, factor or divisor."""
    U = _oracle_U("T1", 1.0, 0.07)
    _, _, t = R.inputs("T1")
    m, C = U.shape
    assert U.min() >= 1.4e-4
    ref = OB.objective(U, t, weights)
    h = 1e-7
    fd = np.zeros_like(ref.gbar)
    for i in range(m):
        for c in range(C):
            Up, Um = U.copy(), U.copy()
            Up[i, c] += h
            Um[i, c] -= h
            fd[i, c] = (OB.objective(Up, t, weights).loss - OB.objective(Um, t, weights).loss) / (2 * h)
    err = np.abs(ref.gbar - fd) / np.maximum(np.abs(fd), 1.0 / m)
    print(f"weights {weights}: max scaled error {err.max():.2e}; max |gbar| {np.abs(ref.gbar).max():.3g}")
    assert err.max() < 1e-5
    assert np.abs(ref.gbar).max() > 0


def test_reference_equals_the_ce_reference_at_unit_ce_weight():
    U = _oracle_U("T1", 1.0, 0.07)
    _, _, t = R.inputs("T1")
    a, b = OB.objective(U, t), R.ce_head(U, t)
    assert a.loss == b.loss and a.correct == b.correct
    np.testing.assert_array_equal(a.row_ce, b.row_loss)
    np.testing.assert_array_equal(a.gbar, b.gbar)
    np.testing.assert_array_equal(a.pred_label, b.pred_label)
    np.testing.assert_array_equal(a.row_l2, 1.0 - np.sum(U * U, axis=1))


def test_reference_masking_and_zero_weight_rules():
    U = np.array(_oracle_U("T1", 1.0, 0.07))
    _, _, t = R.inputs("T1")
    m, C = U.shape
    w = (1.0, 0.3, 0.1)
    full = OB.objective(U, t, w)
    tm = t.copy()
    tm[::4] = -1
    tm[1:9:4] = C
    out = (tm < 0) | (tm >= C)
    ref = OB.objective(U, tm, w)
    # masking: the ce term, row_ce and correct alone
    assert (ref.row_ce[out] == 0).all()
    np.testing.assert_array_equal(ref.row_ce[~out], full.row_ce[~out])
    np.testing.assert_array_equal(ref.row_entropy, full.row_entropy)
    np.testing.assert_array_equal(ref.row_l2, full.row_l2)
    np.testing.assert_array_equal(ref.pred_label, full.pred_label)
    assert ref.correct == int(np.sum(full.pred_label[~out] == t[~out]))
    np.testing.assert_array_equal(ref.gbar[~out], full.gbar[~out])     # the divisor is still m
    reg = OB.objective(U, None, (0.0, 0.3, 0.1))     # the regularisers alone
    np.testing.assert_array_equal(ref.gbar[out], reg.gbar[out])
    assert (reg.row_ce == 0).all() and reg.correct == 0
    # the same float64 terms summed in another order: m u times their mean magnitude
    assert abs(ref.loss - (np.sum(full.row_ce[~out]) + 0.3 * np.sum(full.row_entropy)
                           - 0.1 * np.sum(full.sq)) / m) <= m * 2.0 ** -53 * np.mean(full.row_abs)
    # targets None == every target out of range
    none = OB.objective(U, None, w)
    allm = OB.objective(U, np.full(m, -1), w)
    assert none.loss == allm.loss
    np.testing.assert_array_equal(none.gbar, allm.gbar)
    # a zero weight leaves its term out even where it is NaN
    bad = U.copy()
    bad[3, 1] = -1e-3          # log(negative) in the entropy term
    bad[5, t[5]] = -1e-3       # ... and in a ce term
    with_ent = OB.objective(bad, t, (1.0, 0.3, 0.1))
    assert np.isnan(with_ent.loss) and np.isnan(with_ent.row_entropy[3])
    assert np.isnan(with_ent.gbar[3, 1])
    t5 = t.copy()
    t5[5] = -1                 # masked: its ce term is not evaluated either
    no_ent = OB.objective(bad, t5, (1.0, 0.0, 0.1))
    assert np.isfinite(no_ent.loss) and np.isfinite(no_ent.gbar).all()
    only_l2 = OB.objective(bad, t, (0.0, 0.0, 1.0))
    assert np.isfinite(only_l2.loss) and np.isfinite(only_l2.gbar).all()
    assert np.isnan(only_l2.row_ce[5]) and np.isnan(only_l2.row_entropy[3])   # outputs keep them
    assert only_l2.loss == -np.sum(np.sum(bad * bad, axis=1)) / m
    np.testing.assert_array_equal(only_l2.gbar, -2.0 * bad / m)
    zero = OB.objective(bad, t, (0.0, 0.0, 0.0))
    assert zero.loss == 0.0 and (zero.gbar == 0).all()


# ------------------------------------------------------------------------------------------
# DeviceScoreStore on the CPU
# ------------------------------------------------------------------------------------------
def _store_data():
    rng = np.random.default_rng(7)
    sizes = [61, 3, 40, 17, 52, 1, 26]                      # 7 classes of uneven size, N = 200
    names = [4, 9, 0, 7, 2, 5, 3]                            # class values, not in sorted order
    labels = np.repeat(names, sizes)
    rng.shuffle(labels)
    n = len(labels)
    assert n == 200
    scores = np.round(rng.uniform(-1, 3, n) * 8) / 8         # eighths: ties are common
    touched = rng.permutation(n)[:150]                       # 50 untouched zeros stay
    scores_full = np.zeros(n, dtype=np.float32)
    scores_full[touched] = scores[touched].astype(np.float32)
    scores_full[touched[0]] = np.nan
    scores_full[touched[1]] = -np.inf
    return labels.astype(np.int64), touched, scores_full


def test_score_store_matches_the_plain_python_rule():
    labels, touched, scores = _store_data()
    st = DeviceScoreStore(torch.from_numpy(labels), device="cpu", seed=0)
    assert st.scores.dtype == torch.float32 and st.scores.shape == (200,) and len(st) == 200
    assert (st.scores == 0).all()
    first_seen = list(dict.fromkeys(labels.tolist()))
    assert st.classes.tolist() == first_seen
    st.update_score(torch.from_numpy(touched), torch.from_numpy(scores[touched]))
    np.testing.assert_array_equal(st.scores.numpy(), scores)
    host = st.scores.tolist()
    assert len(set(host)) < 60                               # ties are common
    for uniform in (False, True):
        for num in (0, 1, 7, 50, 63, 140, 200, 260):
            got = st.select_indices(num, class_uniform_sample=uniform, mode="score")
            want = OB.select_by_score(host, labels, num, uniform)
            assert got.dtype == torch.int64
            assert got.tolist() == want, (uniform, num)
    # NaN ranks after -inf, both after every number
    order = st.select_indices(200, mode="score").tolist()
    assert order[-1] == int(touched[0]) and order[-2] == int(touched[1])
    with pytest.raises(ValueError):
        st.select_indices(10, mode="best")


def test_score_store_random_mode():
    labels, _, _ = _store_data()
    a = DeviceScoreStore(torch.from_numpy(labels), device="cpu", seed=3)
    b = DeviceScoreStore(torch.from_numpy(labels), device="cpu", seed=3)
    got = a.select_indices(50, mode="random")
    assert got.dtype == torch.int64 and len(set(got.tolist())) == 50
    assert 0 <= int(got.min()) and int(got.max()) < 200
    assert got.tolist() == b.select_indices(50, mode="random").tolist()
    again = a.select_indices(50, mode="random")
    assert again.tolist() != got.tolist()                    # the generator moved on
    per = a.select_indices(70, class_uniform_sample=True, mode="random")
    b.select_indices(50, mode="random")
    assert per.tolist() == b.select_indices(70, class_uniform_sample=True, mode="random").tolist()
    assert len(set(per.tolist())) == len(per)
    lab = labels[per.numpy()]
    sizes = {int(c): int((labels == c).sum()) for c in np.unique(labels)}
    for c, size in sizes.items():
        assert int((lab == c).sum()) == min(70 // 7, size)
    # classes come in first-appearance order
    assert list(dict.fromkeys(lab.tolist())) == list(dict.fromkeys(labels.tolist()))
    with pytest.raises(ValueError):
        a.select_indices(201, mode="random")


def test_update_score_is_vectorised(monkeypatch):
    labels, touched, scores = _store_data()
    st = DeviceScoreStore(torch.from_numpy(labels), device="cpu")
    calls = []
    real = torch.Tensor.index_put_

    def spy(self, *a, **kw):
        calls.append(self.shape)
        return real(self, *a, **kw)

    monkeypatch.setattr(torch.Tensor, "index_put_", spy)
    st.update_score(torch.from_numpy(touched), torch.from_numpy(scores[touched]))
    assert calls == [st.scores.shape]                        # one index_put_ for 150 samples
    np.testing.assert_array_equal(st.scores.numpy(), scores)
    # a float64 batch of scores (the head's row outputs) is stored as float32
    st.update_score(touched[:3].tolist(), torch.tensor([0.1, 0.2, 0.3], dtype=torch.float64))
    assert st.scores[torch.from_numpy(touched[:3])].tolist() == [np.float32(0.1), np.float32(0.2), np.float32(0.3)]


def test_selection_hands_over_to_the_base_loader():
    labels, touched, scores = _store_data()
    data = torch.arange(200, dtype=torch.float32).reshape(200, 1) * 2
    st = DeviceScoreStore(torch.from_numpy(labels), device="cpu")
    st.update_score(torch.from_numpy(touched), torch.from_numpy(scores[touched]))
    idx = st.select_indices(70, class_uniform_sample=True, mode="score")
    loader = DeviceBaseLoader(data[:5], torch.from_numpy(labels[:5]), device="cpu", shuffle=False)
    loader.update(data[idx], st.labels[idx])
    x, y = next(iter(loader))
    assert x.flatten().tolist() == (idx * 2).tolist() and y.tolist() == labels[idx.numpy()].tolist()


# ------------------------------------------------------------------------------------------
# the C ABI
# ------------------------------------------------------------------------------------------
def test_header_and_exports_declare_the_objective_head():
    src = open(os.path.join(ROOT, "include", "gll.h")).read()
    for name in ("gll_objective_head_scratch_bytes", "gll_objective_head_batched"):
        assert re.search(r"^\w[\w\s\*]*?\b" + name + r"\s*\(", src, flags=re.M), name
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name)
    for name, val in (("GLL_SCORE_NONE", _lib.SCORE_NONE), ("GLL_SCORE_ENTROPY", _lib.SCORE_ENTROPY),
                      ("GLL_SCORE_L2", _lib.SCORE_L2), ("GLL_K_LOSS", _lib.K_LOSS)):
        assert int(re.search(r"#define\s+" + name + r"\s+(\d+)", src).group(1)) == val
    assert "losses.py:100-101" in src and ":111-112" in src and "FullySup.py:165-173" in src


def test_objective_head_rejects_bad_arguments_without_touching_the_gpu():
    """Every case returns before anything is launched, so the pointers are never followed:
    0x1000 only stands for 'not NULL'."""
    lib = _lib.lib()
    fn = lib.gll_objective_head_batched
    p = G.make_problem(100, 16, 50, 10, 5, 0.07, 1.0)
    nn = 0x1000

    def call(prob=p, B=1, ws=nn, targets=nn, loss=nn, kind=0, score_out=None, score_len=0,
             indices=None, scratch=None):
        return fn(None if prob is None else ct.byref(prob), B, ws, targets, 1.0, 0.0, 0.0, loss,
                  nn, nn, nn, nn, nn, nn, kind, score_out, score_len, indices, scratch, None)

    assert call(prob=None) == -1
    assert call(ws=None) == -1
    assert call(loss=None) == -1
    assert call(B=0) == -1 and call(B=65536) == -1
    bad = G.make_problem(100, 16, 50, 10, 5, 0.07, 1.0)
    bad.K = 1
    assert call(prob=bad) == -1
    assert call(kind=3, score_out=nn, score_len=10, indices=nn) == -1
    assert call(kind=-1, score_out=nn, score_len=10, indices=nn) == -1
    assert call(kind=1, score_out=None, score_len=10, indices=nn) == -1
    assert call(kind=2, score_out=nn, score_len=10, indices=None) == -1
    assert call(kind=1, score_out=nn, score_len=-1, indices=nn) == -1
    sb = lib.gll_objective_head_scratch_bytes
    assert sb(ct.byref(p), 1) == 0 and sb(ct.byref(p), 7) == 0
    assert sb(ct.byref(G.make_problem(4096 + 50, 16, 50, 10, 5, 0.07, 1.0)), 3) == 0
    big = G.make_problem(5000, 16, 100, 10, 5, 0.07, 1.0)
    assert sb(ct.byref(big), 1) == lib.gll_ce_head_scratch_bytes(ct.byref(big), 1) >= 4900 * 12
    assert sb(ct.byref(big), 3) == 3 * sb(ct.byref(big), 1)
    assert sb(ct.byref(big), 0) == 0 and sb(None, 1) == 0
    assert call(prob=big, scratch=None) == -1                # scratch missing past the switch


def test_python_surface():
    from graphlearninglayer_amd import LaplaceLearningSparseHard as L
    assert L.objective is G._ext().objective     # the native function, no wrapper
    assert callable(L.objective_python)
    X, Y, t = (torch.zeros(10, 4), torch.zeros(5, 2), torch.zeros(5, dtype=torch.int64))
    # argument errors come before any device work
    with pytest.raises(ValueError):
        L.objective(X, Y, t, 0.0, 1.0, score="l2", score_out=torch.zeros(20))       # no indices
    with pytest.raises(ValueError):
        L.objective(X, Y, t, 0.0, 1.0, score="l2", indices=t)                       # no score_out
    with pytest.raises(ValueError):
        L.objective(X, Y, t, 0.0, 1.0, score="l2", score_out=torch.zeros(20), indices=t)  # CPU store
    with pytest.raises(ValueError):
        L.objective(X, Y, t, 0.0, 1.0, score="margin")
    with pytest.raises(ValueError):
        L.objective(X, Y, t, 0.0, 1.0, weights=(1.0, 0.0))
    with pytest.raises(TypeError):
        L.objective(X, Y, t.float(), 0.0, 1.0)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="GPU"):
            L.objective(X, Y, t, 0.0, 1.0)
