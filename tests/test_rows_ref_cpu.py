"""tests/rows_ref.py on the CPU: the float64 row-build reference pinned to the oracle, its bounds
checked against float32 arithmetic, its check() against injected errors, its restated route
against libgll.so's kernels, and the regimes its cases claim against float64 exact kNN lists of
their features.

Worst err / bound of the float32 evaluation (numpy's float32 exp, each row summed sequentially in
a random order -- harsher on long rows than the kernel's lane-strided sums), as run:
    eight golden fixtures       w 0.28-0.75   deg 0.11-0.53   diag 0.15-0.53   rhs 0.09-0.36
    the 51 cases of the GPU test   w <= 0.79   deg <= 0.90 (a 236-entry hub row)   diag <= 0.89
                                   rhs <= 0.59   eps <= 0.50 of an ulp
and rows_ref equals the oracle's graph_from_knn / W_ul Y to 1e-14 relative on all eight.
"""
import os
import re

import numpy as np
import pytest

from oracle import gll_oracle as O
from tests import rows_ref as R
from tests.golden_io import Case as Golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIXTURES = ("plumbing_eps1p0_tau0p07_f32", "plumbing_epsauto_tau0p07_f32", "ns_epsauto_tau0p07_f32",
            "ns_eps1p0_tau0p07_f32_C17", "ns_eps1p0_tau0p07_f32_k64", "ns_epsauto_tau0p07_f32_k100",
            "fullysup_eps1p0_tau0p07_f32", "stress_epsauto_tau0p07_f32")
_cache = {}


def _fixture(name):
    """(knn_idx, knn_d2 fp32, Y, eps, K, base) of a golden fixture: its kNN lists with the exact
    squared distances of the listed pairs, rounded to fp32 as the select stores them."""
    if name not in _cache:
        c = Golden(name)
        X = c.X.astype(np.float64)
        idx = c.knn
        d2 = np.empty(idx.shape, dtype=np.float32)
        for r0 in range(0, X.shape[0], 256):
            d2[r0:r0 + 256] = ((X[r0:r0 + 256, None, :] - X[idx[r0:r0 + 256]]) ** 2).sum(axis=2)
        _cache[name] = (idx, d2, c.Y, c.eps, idx.shape[1], c.Y.shape[0])
    return _cache[name]


def _fixture_stage(name, eps32=True):
    """eps32: the auto eps as the workspace holds it (fp32); else its float64 value, as the oracle
    forms it."""
    idx, d2, Y, eps, K, base = _fixture(name)
    n = idx.shape[0]
    auto = isinstance(eps, str)
    ep = np.sqrt(d2[:, K - 1].astype(np.float64))
    if eps32:
        ep = ep.astype(np.float32)
    return R.rows_stage(idx, d2, ep, Y, R.TAU, base, K, R.layout(n, base, K),
                        None if auto else np.float32(eps)), (idx, d2, Y, eps, base)


@pytest.mark.parametrize("name", FIXTURES)
def test_stage_reference_equals_the_oracle(name):
    """Pattern exact; W, deg and rhs (= W_ul Y = -Lul Y, what oracle.forward solves for) to float64
    rounding."""
    st, (idx, d2, Y, eps, base) = _fixture_stage(name, eps32=False)
    g = O.graph_from_knn(idx, np.sqrt(d2.astype(np.float64)), eps)
    assert np.array_equal(g.rows, st.row) and np.array_equal(g.cols, st.col)
    assert np.array_equal(g.dist ** 2 == 0, np.zeros(g.rows.size, bool))
    np.testing.assert_allclose(st.d2.astype(np.float64), g.dist ** 2, rtol=4e-16)
    np.testing.assert_allclose(st.eps_in, g.eps, rtol=1e-15)
    np.testing.assert_allclose(st.W, g.W, rtol=1e-14, atol=0)
    W = g.csr(g.W)
    deg = np.asarray(W.sum(axis=1)).ravel()
    np.testing.assert_allclose(st.deg, deg, rtol=1e-14)
    rhs = W[base:, :base] @ Y.astype(np.float64)
    np.testing.assert_allclose(st.rhs, rhs, rtol=1e-14, atol=1e-14 * np.abs(rhs).max())
    np.testing.assert_allclose(st.diag, deg[base:] + np.float64(np.float32(R.TAU)), rtol=1e-14)
    assert np.array_equal(st.ucnt + st.nlab[base:], st.row_len[base:])


def _bound_use(st, seeds=2):
    worst = {}
    for seed in range(seeds):
        got = R.check(st, R.emulate_f32(st, np.random.default_rng(seed)))
        for k, (cnt, r) in got.items():
            worst[k] = max(worst.get(k, 0.0), r)
    return worst


@pytest.mark.parametrize("name", FIXTURES)
def test_bounds_hold_for_float32_arithmetic_on_the_fixtures(name):
    st, _ = _fixture_stage(name)
    worst = _bound_use(st)
    print(f"{name}: float32 evaluation, worst err/bound " +
          ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert 0 < worst["w"] <= 1 and 0 < worst["deg"] <= 1 and 0 < worst["rhs"] <= 1


_stage = {}


def _case_stage(name):
    if name not in _stage:
        _stage[name] = R.cpu_stage(R.CASES[name])
    return _stage[name]


@pytest.mark.parametrize("name", list(R.CASES))
def test_bounds_hold_for_float32_arithmetic_on_every_case(name):
    """Every case of the GPU test is CPU-evaluable (float64 exact kNN lists of its features)."""
    worst = _bound_use(_case_stage(name), seeds=1)
    print(f"{name}: float32 evaluation, worst err/bound " +
          ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1


# ------------------------------------------------------------------------------------------
# check() rejects what it must
# ------------------------------------------------------------------------------------------
def _good():
    """A stage with a mutual pair whose two directions differ by one ulp, and its float32 image."""
    idx, d2, Y, eps, K, base = _fixture("plumbing_eps1p0_tau0p07_f32")
    d2 = d2.copy()
    i = 70
    j = next(int(j) for j in idx[i, 1:] if i in idx[j, 1:])           # a mutual pair
    t = int(np.flatnonzero(idx[i] == j)[0])
    d2[i, t] = np.nextafter(d2[i, t], np.float32(np.inf))
    n = idx.shape[0]
    lay = R.layout(n, base, K)
    st = R.rows_stage(idx, d2, None, Y, R.TAU, base, K, lay, np.float32(eps))
    assert st.mutual_diff == 1
    return st, R.emulate_f32(st), (i, j), (idx, d2, Y, eps, K, base, lay)


def _entry(st, out, i, j):
    """Storage index of entry (i, j)."""
    q = int(np.flatnonzero((st.row == i) & (st.col == j))[0])
    return int(out.row_start[i]) + q - int(st.row_ptr[i])


def test_check_accepts_the_float32_image():
    st, out, _, _ = _good()
    R.check(st, out)


def test_check_rejects_a_swapped_column_pair():
    st, out, (i, j), _ = _good()
    s = int(out.row_start[i])
    for arr in (out.col, out.w, out.d2):
        arr[s], arr[s + 1] = arr[s + 1].copy(), arr[s].copy()
    with pytest.raises(AssertionError, match="col differs"):
        R.check(st, out)


def test_check_rejects_a_weight_off_by_1e_6_relative():
    st, out, (i, j), _ = _good()
    for a, b in ((i, j), (j, i)):                  # both directions: it is not the symmetry check
        out.w[_entry(st, out, a, b)] *= np.float32(1 + 1e-6)
    with pytest.raises(AssertionError, match="w err/bound"):
        R.check(st, out)
    st, out, (i, j), _ = _good()
    out.w[_entry(st, out, i, j)] *= np.float32(1 + 1e-6)
    with pytest.raises(AssertionError, match="w is not symmetric"):
        R.check(st, out)


def test_check_rejects_the_minimum_of_the_two_directions():
    st, out, (i, j), (idx, d2, *_rest) = _good()
    lo = np.nextafter(out.d2[_entry(st, out, i, j)], np.float32(0))
    assert lo == d2[j, int(np.flatnonzero(idx[j] == i)[0])]           # the other direction
    for a, b in ((i, j), (j, i)):
        out.d2[_entry(st, out, a, b)] = lo
    with pytest.raises(AssertionError, match="d2 differs on 2 entries"):
        R.check(st, out)


def test_check_rejects_a_nonzero_ell_pad_slot():
    st, out, _, _ = _good()
    pad = np.argwhere(st.ell_src < 0)
    assert pad.size
    s, u = (int(x) for x in pad[0])
    m = st.lay.m
    out.ell[((s // 2) * m + u) * 4 + (s % 2) * 2 + 1] = np.float32(1e-30).view(np.int32)
    with pytest.raises(AssertionError, match="ELL pad slot"):
        R.check(st, out)


def test_check_rejects_a_nonzero_rhs_element_that_must_be_zero():
    st, out, _, _ = _good()
    zero = np.argwhere(st.rhs_b == 0)
    assert zero.size                               # one-hot labels: most classes of most rows
    u, c = (int(x) for x in zero[0])
    out.rhs[u, c] = np.float32(1e-30)
    with pytest.raises(AssertionError, match="rhs: 1 elements that must be exactly 0"):
        R.check(st, out)


def test_check_rejects_overlapping_rows_an_unwritten_slot_and_a_wrong_status_word():
    st, out, (i, j), _ = _good()
    out.row_start[i + 1] = out.row_start[i]
    with pytest.raises(AssertionError, match="slot row"):
        R.check(st, out)
    st, out, _, _ = _good()
    out.deg[5] = np.nan                            # what a 0xFF-filled workspace holds
    with pytest.raises(AssertionError, match="non-finite"):
        R.check(st, out)
    st, out, _, _ = _good()
    out.tiny_eps = 1
    with pytest.raises(AssertionError, match="TINY_EPS"):
        R.check(st, out)


# ------------------------------------------------------------------------------------------
# route() and CASES against the library; the regimes the cases claim
# ------------------------------------------------------------------------------------------
def _library_instantiations():
    """{(TY, PRE, FLAT, FH)} of every row_build_kernel device stub in libgll.so, decoded from the
    mangled names (f / d / l label type, Lb<v>E booleans PRE, FLAT, R, Li<v>E the list parts)."""
    data = open(os.path.join(ROOT, "graphlearninglayer_amd", "libgll.so"), "rb").read()
    out = set()
    for ty, pre, flat, r, fh in set(re.findall(
            rb"_ZN3gll\d+__device_stub__row_build_kernelI([fdl])Lb(\d)ELb(\d)ELb(\d)ELi(\d+)EEEv", data)):
        assert r == b"0"
        out.add((ty.decode(), int(pre), int(flat), int(fh)))
    return out


def test_cases_reach_every_row_build_instantiation():
    have = _library_instantiations()
    want = {c.route() for c in R.ALL_CASES}
    assert sorted(want - have) == [], "routes to kernels the library does not hold"
    assert sorted(have - want) == [], "instantiations no case reaches"
    assert len(have) == 21


def test_route_restates_launch_finalize():
    assert R.route(10, 1, "f32") == ("f", 1, 0, 1)
    assert R.route(10, 1, "f32", 2) == ("f", 0, 0, 1)
    assert R.route(10, 3, "f64") == ("d", 0, 1, 1)
    assert R.route(10, 3, "i64", 1) == ("l", 1, 0, 1)
    assert R.route(65, 1, "f32")[3] == 1 and R.route(66, 1, "f32")[3] == 2
    assert R.route(129, 2, "f32")[3] == 2 and R.route(130, 2, "f32") == ("f", 0, 1, 4)
    assert R.route(66, 1, "f32", 2) == ("f", 1, 0, 2)      # the knob is read at FH = 1 only
    assert R.route(66, 3, "f32", 1) == ("f", 0, 1, 2)
    assert [R.layout(m + 20, 20, 10).SE for m in (500, 512, 513, 2048, 2049, 4096, 4097)] == \
        [24, 24, 16, 16, 4, 4, 0]
    assert R.layout(150, 25, 25).VRM == 16 and R.layout(1000, 500, 10).VRM == 0
    assert R.layout(1000, 500, 10, R.FLAG_CG_VR).VRM == 7 and R.layout(2068, 20, 10).VRM == 7 and R.layout(300, 60, 130).VRM == 63
    assert R.layout(12, 4, 25).K == 12


def test_every_regime_is_reached():
    """Counted on float64 exact kNN lists of each case's features: every tag of REQUIRED by some
    case, and by each case the tags it is there for."""
    seen = set()
    for c in R.ALL_CASES:
        tags = R.regimes(_case_stage(c.name), c)
        assert set(c.expect) <= tags, (c.name, sorted(set(c.expect) - tags))
        seen |= tags
    assert sorted(R.REQUIRED - seen) == []
    st = _case_stage("stage_global_slot")
    lb = (st.nf + st.rc)[60]
    assert R.K_STAGE < lb <= st.lay.Wcap and 206 <= st.rc[60] <= 212
    st = _case_stage("stage_bump_lds_noovf")
    assert st.lay.Wcap - st.nf[20] < st.rc[20] <= st.lay.RCAP
    st = _case_stage("dups_auto")
    assert (st.row_len == 0).sum() >= 12 and not st.deg[st.row_len == 0].any()
    assert (st.W[(st.eps_in[st.row] == 0) | (st.eps_in[st.col] == 0)] == 0).all()
