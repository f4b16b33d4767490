"""tests/grad_ref.py on the CPU: the float64 stage reference pinned to the oracle, its derived
bound checked against float32 arithmetic, its restated route against libgll.so's kernels.

Worst err / bound of the float32 evaluation (random edge order per row), as run:
    plumbing fixed 0.050   plumbing auto 0.070   C = 3 auto 0.073   C = 17 fixed 0.079
    C = 10, K = 42, hub row of 199 edges, auto 0.004
so the bound holds with 13-230 x slack on the CPU (and grad_ref equals oracle.backward to
2.6e-16 ... 5.5e-16 on the five shapes); what the kernels use of it is recorded in
tests/test_gpu_grad_stage.py.
"""
import os
import re

import numpy as np
import pytest

from oracle import gll_oracle as O
from tests import grad_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _shape(name):
    """(X float32, Y, eps, K, gbar) of a CPU shape."""
    from graphlearninglayer_amd.synth import CONFIGS, one_hot, seeded_gbar, synth
    c = CONFIGS["plumbing"]
    if name in ("plumbing_fixed", "plumbing_auto"):
        X, lab = synth(c["base"], c["batch"], c["d"], r=c["r"], seed=0)
        return X, one_hot(lab[:64]), (1.0 if name.endswith("fixed") else "auto"), c["k"], \
            seeded_gbar(64, 10)
    if name == "C3_auto":
        X, lab = synth(50, 81, 20, C=3, seed=3)
        return X, one_hot(lab[:50], 3), "auto", 7, seeded_gbar(81, 3, 5)
    if name == "C17_fixed":
        X, lab = synth(50, 81, 20, C=17, seed=17)
        return X, one_hot(lab[:50], 17), 1.0, 7, seeded_gbar(81, 17, 6)
    assert name == "hub_K42_auto"
    rng = np.random.default_rng(9)
    X = rng.standard_normal((200, 32)).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    X[0] = 0.0
    return X, one_hot(np.arange(60) % 10), "auto", 42, seeded_gbar(140, 10, 7)


SHAPES = ("plumbing_fixed", "plumbing_auto", "C3_auto", "C17_fixed", "hub_K42_auto")
_cache = {}


def _oracle_arrays(name):
    """The oracle's own float64 arrays of a shape in the layout grad_ref takes, and its grad_X."""
    if name not in _cache:
        X, Y, eps, K, gb = _shape(name)
        _, st = O.forward(X, Y, R.TAU, eps, K)
        g = st.graph
        _, _, wU = O.edge_coefficients(st, gb)
        rl = np.bincount(g.rows, minlength=g.n)
        arrs = dict(row_start=np.cumsum(rl) - rl, row_len=rl, col=g.cols, w=g.W, d2=g.dist ** 2,
                    eps=g.eps, knn_idx=g.kth, P=np.concatenate([st.Y, st.U]),
                    Wadj=np.concatenate([np.zeros_like(st.Y), wU]), X=st.X, auto=g.auto,
                    eps_fixed=None if g.auto else float(eps))
        _cache[name] = (arrs, O.backward(st, gb))
    return _cache[name]


@pytest.mark.parametrize("name", SHAPES)
def test_stage_reference_equals_the_oracle(name):
    arrs, want = _oracle_arrays(name)
    st = R.grad_stage(**arrs)
    err = O.rel_err(st.grad, want)
    print(f"{name}: grad_ref vs oracle.backward rel err {err:.2e}, longest row {arrs['row_len'].max()}")
    assert err <= 1e-12
    if name.startswith("hub"):
        assert arrs["row_len"].max() == 199
    # the bound is not vacuous: far below the suite's 1e-4 of max|grad| on ordinary rows
    ordinary = st.Lmax <= 4 * arrs["row_len"].mean()
    assert (st.bound[ordinary] <= 2e-5 * np.abs(want).max()).all()


@pytest.mark.parametrize("name", SHAPES)
def test_bound_holds_for_float32_arithmetic_in_any_edge_order(name):
    arrs, _ = _oracle_arrays(name)
    a32 = {k: (np.asarray(v, dtype=np.float32) if isinstance(v, np.ndarray) and v.dtype == np.float64
               else v) for k, v in arrs.items()}
    if a32["eps_fixed"] is not None:
        a32["eps_fixed"] = np.float32(a32["eps_fixed"])
    st = R.grad_stage(**a32)               # float64 closed form of the fp32 inputs
    worst = 0.0
    for seed in range(3):
        got = R.grad_stage_f32(**a32, rng=np.random.default_rng(seed))
        ratio, rel = R.check(got, st)
        worst = max(worst, ratio)
    print(f"{name}: float32 evaluation, worst err/bound {worst:.4f}, err/max|grad| {rel:.2e}")
    assert 0 < worst <= 1.0


def test_check_rejects_what_it_must():
    arrs, _ = _oracle_arrays("plumbing_fixed")
    st = R.grad_stage(**arrs)
    good = st.grad.astype(np.float32)
    R.check(good, st)
    bad = good.copy()
    bad[17, 3] = np.nan                    # an unwritten element of a NaN-filled output
    with pytest.raises(AssertionError, match="non-finite"):
        R.check(bad, st)
    i, k = np.unravel_index(np.argmax(st.bound), st.bound.shape)
    bad = good.copy()
    bad[i, k] += np.float32(4 * st.bound[i, k] + 1e-30)
    with pytest.raises(AssertionError, match="err/bound"):
        R.check(bad, st)
    # a small element next to max|grad|: a relative error of 1e-5 of the LARGEST element passes
    # the max-norm bar and fails here
    j, q = np.unravel_index(np.argmin(np.where(st.bound > 0, st.bound, np.inf)), st.bound.shape)
    bad = good.copy()
    bad[j, q] += np.float32(1e-5 * np.abs(st.grad).max())
    assert O.rel_err(bad, st.grad) <= 1e-4
    with pytest.raises(AssertionError, match="err/bound"):
        R.check(bad, st)


def test_empty_rows_have_zero_bound_and_must_be_exactly_zero():
    arrs, _ = _oracle_arrays("plumbing_fixed")
    a = dict(arrs)
    rl = a["row_len"].copy()
    rl[5] = 0                              # row 5 loses its edges (as a duplicate's row does)
    a["row_len"] = rl
    st = R.grad_stage(**a)
    assert not st.bound[5].any() and not st.grad[5].any()
    out = st.grad.astype(np.float32)
    R.check(out, st)
    out[5, 0] = 1e-30
    with pytest.raises(AssertionError, match="bound is 0"):
        R.check(out, st)


# ------------------------------------------------------------------------------------------
# route() and CASES against the library
# ------------------------------------------------------------------------------------------
FAMILIES = ("edge_coef_kernel", "grad_spmm_kernel", "grad_chunk_kernel", "cg_grad_fused_kernel")


def _library_instantiations():
    """{(kernel, template arguments)} of every gradient-kernel device stub in libgll.so, decoded
    from the mangled names: Li<v>E / Lin<v>E integers, Lb<v>E booleans, f / d types."""
    data = open(os.path.join(ROOT, "graphlearninglayer_amd", "libgll.so"), "rb").read()
    out = set()
    for name, args in set(re.findall(
            rb"_ZN3gll\d+__device_stub__(" + b"|".join(f.encode() for f in FAMILIES) +
            rb")I((?:L[ib]n?\d+E|[fd])+)EEv", data)):
        toks = re.findall(rb"L[ib](n?)(\d+)E|([fd])", args)
        out.add((name.decode(), tuple(t[2].decode() if t[2] else (-int(t[1]) if t[0] else int(t[1]))
                                      for t in toks)))
    return out


def test_cases_reach_every_gradient_kernel_instantiation():
    """Every edge_coef / grad_spmm / grad_chunk / cg_grad_fused instantiation the library holds is
    the route of some case of the GPU test, and no case routes to a kernel that does not exist.
    No exemptions: an instantiation no shape can reach is dead code and fails here."""
    have = _library_instantiations()
    assert {k for k, _ in have} == set(FAMILIES)
    want = set().union(*[c.kernels() for c in R.ALL_CASES])
    assert sorted(want - have, key=str) == [], "routes to kernels the library does not hold"
    assert sorted(have - want, key=str) == [], "instantiations no case reaches"
    per = {f: sum(1 for k, _ in have if k == f) for f in FAMILIES}
    assert per == {"edge_coef_kernel": 24, "grad_spmm_kernel": 48, "grad_chunk_kernel": 6,
                   "cg_grad_fused_kernel": 24}, per


def test_route_restates_the_gates():
    U, CH, RO = R.FLAG_BWD_UNFUSED, R.FLAG_GRAD_CHUNK, R.FLAG_GRAD_ROWS
    # the north-star shape: fused, one launch
    r = R.route(1000, 512, 500, 10, 10, 1, False, True)
    assert r.counts == (0, 0, 1, 0) and r.kernels == {("cg_grad_fused_kernel", (512, 24, "d", 2))}
    # every gate of launch_cg_grad_fused sends it to two launches
    two = (0, 1, 0, 1)
    assert R.route(1000, 512, 500, 10, 10, 1, False, True, U).counts == two
    assert R.route(1000, 512, 500, 10, 10, 1, False, True, R.FLAG_CG_GRID).counts == two
    assert R.route(1000, 512, 500, 10, 10, 1, False, False).counts == two       # X off 16 B
    assert R.route(1000, 510, 500, 10, 10, 1, False, True).counts == two        # d % 4
    assert R.route(1000, 512, 500, 9, 10, 1, False, True).counts == two         # C != 10
    assert R.route(1013, 512, 500, 10, 10, 1, False, True).counts == two        # m = 513
    assert R.route(1000, 1028, 500, 10, 10, 1, False, True).counts == two       # d > 1024
    assert R.route(1500, 128, 250, 10, 25, 1, False, True).counts == two        # balanced CG (RV)
    assert R.route(1500, 1024, 1000, 10, 10, 1, False, True).counts == (1, 1, 0, 1)   # > 4 MB
    assert R.route(1000, 512, 500, 10, 10, 2, False, True).counts == two        # a batch
    assert R.route(1000, 512, 500, 10, 10, 1, True, True).counts == (1, 1, 0, 1)      # auto eps
    assert R.route(1000, 512, 1000, 10, 10, 1, False, True).counts == (0, 1, 0, 0)    # m = 0
    # chunks: forced, a batch of narrow graphs, X past 4 MB; never without 16-B rows or d < 128
    assert R.route(1000, 512, 500, 10, 10, 1, False, True, CH).family == "chunk"
    assert R.route(1000, 128, 500, 10, 10, 3, False, True).family == "chunk"
    assert R.route(1000, 128, 500, 10, 10, 3, False, True, RO).family == "spmm"
    assert R.route(1000, 256, 500, 10, 10, 3, False, True).family == "spmm"
    assert R.route(8192, 1024, 4096, 10, 30, 1, True, True).kernels == {
        ("edge_coef_kernel", (-10, 16)), ("grad_chunk_kernel", (1, 32))}
    assert R.route(1000, 124, 500, 10, 10, 1, False, True, CH).family == "spmm"
    assert R.route(1000, 512, 500, 10, 10, 1, False, False, CH).family == "spmm"
    assert R.route(1000, 132, 500, 10, 10, 1, False, True, CH).nch == 3
    # the edge pass: exact even forms, bounds, the loop; lanes by K (clamped to n)
    assert [R.edge_form(C, 10)[0] for C in (1, 2, 3, 4, 5, 8, 9, 15, 16, 17)] == \
        [4, -2, 4, -4, 8, -8, 16, 16, -16, 0]
    assert R.edge_form(10, 40)[1] == 16 and R.edge_form(10, 41)[1] == 32
    assert R.route(30, 12, 10, 10, 64, 1, True, True).kernels >= {("edge_coef_kernel", (-10, 16))}


def test_fused_cases_sweep_every_workgroup_residue():
    """The residues the fused kernel's workgroup rank depends on are all present."""
    for nt in (64, 128, 256, 512):
        nw = nt // 64
        ns = R.fused_ns(nt)
        assert sorted(((n + nw - 1) // nw) % 8 for n in ns) == list(range(8))
        assert all(n % 64 for n in ns) and (nw == 1 or all(n % nw for n in ns))
        for n in ns:
            for m in R.FUSED_M[nt]:
                c = R.CASES[f"fused_NT{nt}_m{m}_n{n}"]
                assert c.route().family == "fused" and c.route().kernels == {
                    ("cg_grad_fused_kernel", (nt, 24, "f", 1))}
                assert 10 + (n + nw - 1) // nw <= 256
    for c in R.ALL_CASES:          # every case's family is the one its name and record claim
        fam = c.route().family
        assert fam == c.group or (c.group == "edge" and c.route().counts[0] == 1), c.name
