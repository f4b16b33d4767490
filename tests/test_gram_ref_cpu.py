"""tests/gram_ref.py on the CPU: the model against the contract the select relies on, the derived
bound against float32 arithmetic, check() against a list of injected errors, the tight bound's
teeth on the coherent inputs, and the restated route against libgll.so (gll_gram_route and the
device stubs).  No GPU.

As run (worst over every case and graph):
    the model uses at most 0.1223 of the contract 2^-13 (|a_i| + |a_j|)^2 -- on the coherent
    inputs, whose dropped lo lo terms all add; 0.0573 at most on every other input family;
    float32 evaluation in shuffled order: worst err/bound 0.2914 on fp32 storage (0.978 on fp16
    storage, where an honest round to nearest may use all of the 2^-11 |v| the bound grants it);
    the dropped lo hi / hi lo product leaves the tight bound on 100 % of the off-diagonal pairs of
    every family's coherent case (the smallest excess is 81.8 x the bound).
"""
import ctypes as ct
import itertools
import os
import re

import numpy as np
import pytest

from tests import gram_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = tuple(range(6))
_models = {}


def _graphs(case, limit=3):
    """The graphs of a case the CPU tests evaluate: one of each input family it holds."""
    return list(range(min(case.B, max(len(case.feats), 1), limit)))


def _model(case, g):
    key = (case.name.split("+")[0], g)
    if key not in _models:
        X = R.features(case, g)
        _models[key] = (X, R.Model(case, X))
    return _models[key]


def _small(case):
    return case.n * case.n * case.d <= 2.5e7


@pytest.mark.parametrize("name", list(R.CASES))
def test_model_stays_within_the_contract(name):
    """The intended arithmetic itself keeps |D2 - d2_true| <= kGramErr (|a_i| + |a_j|)^2 on every
    case's inputs, and an honest rounding of it passes check()."""
    case = R.CASES[name]
    worst = 0.0
    for g in _graphs(case, 8):
        X, m = _model(case, g)
        c = m.contract()
        err = np.abs(m.D2 - m.truth)
        assert (err <= c).all()
        nz = c > 0
        if nz.any():
            worst = max(worst, float((err[nz] / c[nz]).max()))
        got = R.check(case, [X], [R.emulate(case, X)], graphs=[g], models=[m])
        assert got["D2"][0] == m.rt.planes * case.buffer_rows().size * case.n
        # one honest rounding: half an ulp of fp32 (fp16 storage may use all of its 2^-11)
        if not m.rt.H:
            assert got["D2"][1] <= 0.5 and got["contract"][1] <= 0.5
    print(f"{name}: model uses {worst:.4f} of the contract")
    assert worst <= 0.5, "the derivation at select.hip kGramErr does not hold: stop and report"


@pytest.mark.parametrize("name", [c.name for c in R.CASES.values() if _small(c)])
def test_bound_holds_for_float32_arithmetic_in_shuffled_order(name):
    case = R.CASES[name]
    worst = 0.0
    for g in _graphs(case, 2):
        X, m = _model(case, g)
        out = R.emulate(case, X, f32=True, rng=np.random.default_rng(g))
        got = R.check(case, [X], [out], graphs=[g], models=[m])
        worst = max(worst, got["D2"][1], got["norm"][1])
    print(f"{name}: float32 evaluation, worst err/bound {worst:.4f}")
    assert worst <= 1.0
    if "allsame" not in case.feats[:2] or len(case.feats) > 1:
        assert worst > 0


def _applies(mut, case):
    rt = case.route()
    if mut == "plane1_diag":
        return rt.planes == 2
    if mut in ("scale_from_max", "fp16_trunc"):
        return bool(rt.H)
    return True


@pytest.mark.parametrize("fam", FAMILIES, ids=R.FAMILY_NAMES)
@pytest.mark.parametrize("mut", [m for m in R.MUTATIONS if m != "no_centre"])
def test_check_rejects_injected_errors_on_the_coherent_case(mut, fam):
    case = R.CASES[R.COHERENT[fam]]
    assert R.feat_kind(case, 0) == "coherent" and case.route().family == fam
    if not _applies(mut, case):
        # no second plane / no fp16 storage on this family: the error cannot be made there
        assert (mut == "plane1_diag" and fam != R.BF3S) or fam not in (R.PK, R.PK2)
        return
    X, m = _model(case, 0)
    with pytest.raises(AssertionError, match=case.name):
        R.check(case, [X], [R.emulate(case, X, mut=mut)], models=[m])


@pytest.mark.parametrize("fam", FAMILIES, ids=R.FAMILY_NAMES)
def test_check_rejects_a_skipped_centring_on_the_offset_case(fam):
    case = R.CASES[R.OFFSET[fam]]
    g = case.feats.index("offset")
    assert case.route().family == fam
    X, m = _model(case, g)
    R.check(case, [X], [R.emulate(case, X)], graphs=[g], models=[m])
    with pytest.raises(AssertionError, match=case.name):
        R.check(case, [X], [R.emulate(case, X, mut="no_centre")], graphs=[g], models=[m])


def test_every_fp16_family_sees_the_fp16_mutations():
    for fam in (R.PK, R.PK2):
        assert R.CASES[R.COHERENT[fam]].route().H == 1


@pytest.mark.parametrize("fam", FAMILIES, ids=R.FAMILY_NAMES)
def test_tight_bound_has_teeth_on_the_coherent_case(fam):
    """A kernel that dropped a whole lo hi (or hi lo) product would leave the bound on at least
    half of the off-diagonal pairs: a condition on the inputs, not on the bound."""
    case = R.CASES[R.COHERENT[fam]]
    X, m = _model(case, 0)
    n = case.n
    off = ~np.eye(n, dtype=bool)
    off[0, :] = off[:, 0] = False          # row 0 is the centre: a_0 = 0, nothing to drop
    bnd = sum(m.bound())
    for drop in ("lohi", "hilo"):
        G, _ = R._sym3(m.hi, m.lo, slice(0, case.d), (drop,))
        err = np.abs((m.N[:, None] + m.N[None, :] - 2 * G) - m.D2)
        frac = float((err > bnd)[off].mean())
        print(f"{case.name}: drop {drop}: {100 * frac:.1f} % of pairs outside the bound, "
              f"smallest err/bound {float((err[off] / bnd[off]).min()):.2f}")
        assert frac >= 0.5


# ------------------------------------------------------------------------------------------
# route() and CASES against the library
# ------------------------------------------------------------------------------------------
def _lib():
    from graphlearninglayer_amd import _lib
    return _lib


def _library_route(n, d, B, K, flags, aligned, cus):
    L = _lib()
    p = L.Problem(n=n, d=d, base=0, C=1, K=K, max_iter=0, tau=0.0, eps=1.0, rtol=0.0, flags=flags,
                  status_sink=None)
    out = (ct.c_int32 * L.GRAM_ROUTE_WORDS)()
    rc = L.lib().gll_gram_route(ct.byref(p), B, int(aligned), cus, out)
    return rc, tuple(out)


def test_route_restates_gll_gram_route():
    L = _lib()
    shapes = [(3, 2), (64, 128), (65, 129), (300, 64), (300, 100), (300, 200), (257, 600),
              (512, 192), (513, 192), (1000, 300), (1024, 512), (1025, 512), (1200, 100),
              (2900, 192), (2900, 128), (4000, 16), (12288, 132), (12289, 132), (70, 4096)]
    seen = set()
    try:
        for tile, tail in itertools.product((0, 128, 256), (0, 1, 2)):
            L.set_knob(L.KNOB_GRAM_TILE, tile)
            L.set_knob(L.KNOB_GRAM_TAIL, tail)
            for (n, d), B, K, flags, al, cus in itertools.product(
                    shapes, (1, 2, 43, 52, 86, 90), (10, 60),
                    (0, R.FLAG_GRAM_INLINE, R.FLAG_KNN_PANEL, R.FLAG_D2_F32), (0, 1), (256, 304)):
                if n > 3000 and B > 2:
                    continue
                rc, got = _library_route(n, d, B, K, flags, al, cus)
                if R.panel_rows(n, flags) < n and B > 1:
                    assert rc == -2        # row panels: single graphs only
                    continue
                assert rc == 0
                want = R.route_of(n, d, B, K, flags, tile, tail, al, cus)
                assert got == tuple(want), ((n, d, B, K, flags, tile, tail, al, cus), got, want)
                seen.add(got)
    finally:
        L.set_knob(L.KNOB_GRAM_TILE, 0)
        L.set_knob(L.KNOB_GRAM_TAIL, 0)
    assert {r[0] for r in seen} == set(FAMILIES)
    assert {r[7] for r in seen} == {0, 4, 16} and {r[8] for r in seen} >= {0, 2, 3}


def _library_instantiations():
    """{(kernel, template arguments)} of every Gram device stub in libgll.so."""
    data = open(os.path.join(ROOT, "graphlearninglayer_amd", "libgll.so"), "rb").read()
    out = set()
    for name, args in set(re.findall(
            rb"_ZN3gll\d+__device_stub__(gram_\w+?_kernel)I((?:L[ib]\d+E)+)EEv", data)):
        out.add((name.decode(), tuple(int(v) for v in re.findall(rb"L[ib](\d+)E", args))))
    return out


def test_cases_reach_every_gram_instantiation():
    """Every Gram instantiation the library holds is launched by some case at 256 CUs, no case
    routes to a kernel that does not exist, and every case's route is what gll_gram_route returns
    and the family its record claims."""
    L = _lib()
    have = _library_instantiations()
    want = set()
    try:
        for c in R.all_routed_cases():
            L.set_knob(L.KNOB_GRAM_TILE, c.tile)
            L.set_knob(L.KNOB_GRAM_TAIL, c.tail)
            rt = c.route(256)
            rc, got = _library_route(c.n, c.d, c.B, c.K, c.flags, not c.misalign, 256)
            assert rc == 0 and got == tuple(rt), (c.name, got, rt)
            assert rt.family == c.fam, (c.name, rt)
            want |= R.kernels(rt)
    finally:
        L.set_knob(L.KNOB_GRAM_TILE, 0)
        L.set_knob(L.KNOB_GRAM_TAIL, 0)
    assert sorted(want - have) == [], "routes to kernels the library does not hold"
    assert sorted(have - want) == [], "instantiations no case reaches"
    assert len(have) == 16
    per = {}
    for k, _ in have:
        per[k] = per.get(k, 0) + 1
    assert per == {"gram_bf3_kernel": 2, "gram_bf3h_kernel": 2, "gram_bf3s_kernel": 2,
                   "gram_bf3w_kernel": 2, "gram_split_kernel": 2, "gram_pk_kernel": 4,
                   "gram_pk2_kernel": 2}, per


def test_case_table_claims():
    """The claims the GPU test leans on: the tails, the panels' buffer rows, the input families."""
    c = R.CASES["pk2_tail0_B90_512x192"].route()
    assert (c.tail, c.sub) == (14, 16)
    assert R.CASES["pk2_tail1_B90_512x192"].route().tail == 0
    c = R.CASES["pk2_tail2_B90_512x192"].route()
    assert (c.tail, c.sub) == (14, 4)
    c = R.CASES["pk2_B52_513x192_t256"].route()
    assert (c.tail, c.sub) == (56, 4)
    assert R.CASES["pk2_B52_512x192"].route() == R.Route(R.PK2, 1, 1, 1, 1, 1, 0, 0, 0)
    assert R.CASES["pk_B43_300x100_K60"].route().H == 0          # the wide select keeps fp32 rows
    assert R.CASES["pk_2900x192"].route().H == 0
    rows = R.CASES["bf3w_panel_1200x100"].buffer_rows()
    assert rows.size == 1024 and (rows[:176] == np.arange(1024, 1200)).all()
    assert (rows[176:] == np.arange(176, 1024)).all()
    rows = R.CASES["bf3w_panel_2100x64"].buffer_rows()
    assert (rows[:52] == np.arange(2048, 2100)).all() and (rows[52:] == np.arange(1076, 2048)).all()
    assert R.CASES["bf3w_panel_2100x64"].route().panels == 3
    for fam in FAMILIES:          # every family sees every input family
        kinds = set()
        for case in R.CASES.values():
            if case.fam == fam:
                kinds |= {R.feat_kind(case, g) for g in range(case.B)}
        need = {"normal", "coherent", "far", "offset", "dups"}
        assert need <= kinds, (R.FAMILY_NAMES[fam], sorted(need - kinds))
        if fam in (R.PK, R.PK2):
            assert {"scale_up", "scale_dn", "allsame"} <= kinds
    X = R.features(R.CASES["bf3h_B3_130x64"], 2)
    assert (X == X[0]).all()
    # the reference's bf16 rounding is torch's (ties to even, both signs, subnormal results)
    import torch
    a = np.concatenate([R.features(R.CASES["bf3_300x200"]).ravel(),
                        np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 0.0, -0.0,
                                  1e-39, 3e38, float(R.COHERENT_C)], dtype=np.float32)])
    t = torch.from_numpy(a).to(torch.bfloat16)
    assert np.array_equal(R.bf16(a)[1], t.view(torch.int16).numpy().view(np.uint16))
    assert np.array_equal(R.bf16(a)[0], t.to(torch.float32).numpy())
    assert R.d2_scale(0.0) == 1.0 and R.d2_scale(1.0) == 2.0 ** 11 and R.d2_scale(0.99) == 2.0 ** 12
