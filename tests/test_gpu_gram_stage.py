"""Every Gram kernel instantiation on the MI355X (-m gpu) against the float64 stage reference of
tests/gram_ref.py: the D2 matrix, the pre-split planes, the norms, the fp16 scale word and the
locality order, element by element.

Everything goes through the C ABI (gll_graph for single graphs, gll_forward_batched for batches)
into a workspace filled with 0xFF bytes beforehand, so an fp32 or fp16 element nobody wrote reads
as NaN; the arrays are found with gll_workspace_knn_view and the route with gll_gram_route (the
launchers launch from the same record, knn_route.h gram_route).  Nothing after the Gram writes
what is read here: both select kernels take D2 and the scale word as const float*, order.hip
takes D2 const, and xhi / xlo / xnrm / d2s appear in no launcher but gram.hip's and in no kernel
signature outside it; pid and perm are written by order.hip alone and read const by the select and
the chunked gradient.

Per case of gram_ref.CASES (pinned against libgll.so's 16 stubs by tests/test_gram_ref_cpu.py):
the route, that every element of D2[0:n, 0:n] of every graph is written (for row panels: the last
panel's rows and the rows of the one before that it left standing), the tight bound against the
model, the select's contract against the true float64 distance, bitwise symmetry (per plane, and
plane 1 of the split-phase kernel's diagonal tiles exactly 0), D2[i][0] as |a_i|^2, the planes
bitwise and the norms within their bound, and for fp16 storage the scale word bitwise, the halves
bitwise float16(v s) of the GLL_FLAG_D2_F32 run's v (every half, subnormal ones included: it held
on the MI355X, so nothing is narrowed) and |t / s - v| <= 2^-11 |v| + 2^-25 / s on every element.  Then the bitwise
equalities the code comments claim: graph g of a batch against another batch position or the
single call on the same route, the three tail settings, 128- against 256-tiles.

Measured on the MI355X (profiles/gm01_gpu_gram_stage.txt: per case and the teardown table;
profiles/gm01_gpu_tests.txt: the whole suite, 836 tests), elements checked and worst err/bound:
  family      D2 (tight bound)       norm               contract             fp16 contract
  bf3            384,749  0.1698      1,587  0.1700        384,749  0.1226
  bf3h           702,759  0.2335      1,499  0.2337        702,759  0.1227
  bf3s         4,180,876  0.2428      2,412  0.1264      2,090,438  0.1226
  bf3w        28,348,000  0.2375     32,872  0.2377     28,348,000  0.1227
  pk          26,730,107  0.2281    131,102  0.2697     26,730,107  0.1228
  pk/fp16     10,580,107  0.9939     73,702  0.9939     10,580,107  0.7963   10,580,107  0.9995
  pk2         65,464,980  0.2192    276,984  0.2593     65,464,980  0.1227
  pk2/fp16    65,464,980  0.9921    276,984  0.9921     65,464,980  0.7949   65,464,980  0.9995
(/fp16: D2 stored as halves; a round to nearest may use all of the 2^-11 |v| that the bound and
the widened contract grant the storage, and does.)  The pre-split planes are bitwise the model's
on all 117 M bf16 elements.  1,069 graphs in 56 tests; the file runs in 10 s, features and the
numpy model included.  Every bitwise claim of gram.hip's comments holds: D2 symmetric, zeros in
plane 1 of split diagonal tiles, the three tail settings, 128- against 256-tiles on fp16 and fp32
storage, a graph wherever it sits in a batch, the halves float16(v s) of the fp32 run.  No element
outside its bound: no defect found in gram.hip.  No tolerance is tuned to these figures: KAPPA_M is
an assumption stated in gram_ref.py, the rest is counted from the code.
"""
import ctypes as ct
import dataclasses
import time

import numpy as np
import pytest
import torch

from graphlearninglayer_amd import _lib as L
from tests import abi as A
from tests import gram_ref as R

pytestmark = pytest.mark.gpu

_stats = {}      # family (/fp16: D2 stored as halves) -> quantity -> [elements, worst err/bound]
_record = {"graphs": 0, "t0": None}
_sessions = {}
_model_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    A.need_gpu()
    _record["t0"] = time.perf_counter()
    yield
    _sessions.clear()
    _model_cache.clear()
    print(f"\ngram stage: {_record['graphs']} graphs, {time.perf_counter() - _record['t0']:.1f} s")
    for fam in sorted(_stats):
        for q in ("D2", "plane", "norm", "fp16", "contract"):
            cnt, worst = _stats[fam].get(q, (0, 0.0))
            if cnt:
                print(f"gram stage {fam:8s} {q:8s}: {cnt:10d} elements, worst err/bound {worst:.4f}")


def _cus():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus == 256, (f"the case table's routes are derived for 256 CUs; this device has {cus} "
                        "(gram_tile256 and the tail rule read the CU count)")
    return cus


BASE, CLASSES, TAU = 8, 2, 0.1     # batches go through gll_forward_batched: a few labeled rows


class Session:
    """One case on the device (tests/abi.py Run): its B graphs (or the graphs `graphs`, a batch of
    that many), B workspace blocks of 0xFF bytes, one graph build with the case's flags and
    knobs."""

    def __init__(self, case, graphs=None, order=False):
        self.case = case
        self.graphs = list(range(case.B)) if graphs is None else list(graphs)
        B = self.B = len(self.graphs)
        n = case.n
        self.Xh = [R.features(case, g) for g in self.graphs]
        single = case.B == 1
        if single:
            assert B == 1
            X, Y = self.Xh[0], None
        else:
            X, Y = np.stack(self.Xh), np.zeros((B, BASE, CLASSES), dtype=np.float32)
            Y[:, np.arange(BASE), np.arange(BASE) % CLASSES] = 1.0
        run = A.Run(X, Y, case.K, TAU, 1.0, case.flags, C=1 if single else None,
                    aligned=not case.misalign, ws_fill=0xFF)
        out = (ct.c_int32 * L.GRAM_ROUTE_WORDS)()
        with A.knobs({L.KNOB_GRAM_TILE: case.tile, L.KNOB_GRAM_TAIL: case.tail}):
            L.check(L.lib().gll_gram_route(ct.byref(run.problem()), B, int(not case.misalign),
                                           _cus(), out), "gll_gram_route")
            self.route = R.Route(*out)
            if single:
                run.graph()
            else:
                run.forward()
        v = run.knn_view()
        rt = self.route
        assert (v.planes, v.d2_half, v.rows, v.ldD, v.dp) == \
            (rt.planes, rt.H, case.buffer_rows().size, (n + 3) & ~3, case.dp)
        esz = 2 if rt.H else 4
        nb = ((rt.planes - 1) * v.plane_stride + v.rows * v.ldD) * esz
        raw = run.blocks(v.D2, nb).view(np.float16 if rt.H else np.float32)
        self.D2 = np.stack([raw[:, q * v.plane_stride: q * v.plane_stride + v.rows * v.ldD]
                            .reshape(B, v.rows, v.ldD)[:, :, :n] for q in range(rt.planes)], axis=1)
        self.outs = []
        if rt.presplit:
            xhi = run.blocks(v.xhi, n * v.dp * 2).view(np.uint16).reshape(B, n, v.dp)
            xlo = run.blocks(v.xlo, n * v.dp * 2).view(np.uint16).reshape(B, n, v.dp)
            xnrm = run.blocks(v.xnrm, n * 4).view(np.float32)
        scale = run.blocks(v.d2_scale, 4).view(np.float32)[:, 0] if rt.H else None
        for q in range(B):
            o = {"D2": self.D2[q], "scale": None if scale is None else scale[q]}
            if rt.presplit:
                o.update(xhi=xhi[q], xlo=xlo[q], xnrm=xnrm[q])
            self.outs.append(o)
        if order:
            assert v.order == 1
            self.pid = run.blocks(v.pid, n * 4).view(np.int32)[0]
            self.perm = run.blocks(v.perm, n * 4).view(np.int32)[0]


def _session(case):
    if case.name not in _sessions:
        _sessions[case.name] = Session(case)
    return _sessions[case.name]


def _models(ses, qs):
    """The models of graphs ses.graphs[q], shared by the cases that run the same inputs on the same
    family (an fp16 case and its fp32 twin, the three tail settings)."""
    c, out = ses.case, []
    for q in qs:
        g = ses.graphs[q]
        key = (c.seed, c.n, c.d, c.feats, g, c.fam, c.misalign, c.flags & R.FLAG_KNN_PANEL)
        if key not in _model_cache:
            _model_cache[key] = R.Model(c, ses.Xh[q])
        out.append(_model_cache[key])
    return out


def _hold(case, like=None):
    """The case's graphs under gram_ref.check.  like: a case already held whose D2 this one's must
    equal bit for bit (the same inputs on another tail setting); then only the first graphs and
    the last ten -- the ones the tail tiles lie in -- are checked again element by element."""
    ses = _session(case)
    want = case.route(256)
    assert ses.route == want, f"{case.name}: gll_gram_route {ses.route}, the case claims {want}"
    assert want.family == case.fam
    qs = list(range(ses.B))
    if like is not None:
        ref = _session(like)
        assert all(np.array_equal(x, y) for x, y in zip(ses.Xh, ref.Xh))
        assert np.array_equal(A.bits(ses.D2), A.bits(ref.D2)), f"{case.name} differs from {like.name}"
        qs = qs[:3] + qs[-10:]
    outs = [ses.outs[q] for q in qs]
    if want.H:       # the halves against the fp32 run of the same inputs
        twin = _session(R.f32_twin(case))
        assert twin.route == want._replace(H=0)
        outs = [dict(o, D2_f32=twin.outs[q]["D2"]) for o, q in zip(outs, qs)]
    got = R.check(case, [ses.Xh[q] for q in qs], outs, graphs=[ses.graphs[q] for q in qs],
                  models=_models(ses, qs))
    fam = _stats.setdefault(R.FAMILY_NAMES[case.fam] + ("/fp16" if want.H else ""), {})
    for k, (cnt, worst) in got.items():
        s = fam.setdefault(k, [0, 0.0])
        s[0] += cnt
        s[1] = max(s[1], worst)
    _record["graphs"] += len(qs)
    print(f"{case.name} {sorted(R.kernels(want))}: " +
          ", ".join(f"{k} {c} el. {w:.4f}" for k, (c, w) in got.items() if c))
    return ses, got, len(qs)


def _like(case):
    """Tail settings 1 and 2 run tail setting 0's inputs."""
    if case.name.startswith(("pk2_tail1", "pk2_tail2")):
        return dataclasses.replace(case, name="pk2_tail0" + case.name[9:], tail=0)
    return None


@pytest.mark.parametrize("name", list(R.CASES))
def test_every_case_against_the_stage_reference(name):
    case = R.CASES[name]
    ses, got, ng = _hold(case, _like(case))
    rows = case.buffer_rows()
    assert got["D2"][0] == ng * ses.route.planes * rows.size * case.n
    if ses.route.panels:
        # coverage is over both the last panel's rows and the earlier panel's rows below them
        last = case.n - ((case.n - 1) // rows.size) * rows.size
        assert 0 < last < rows.size and (rows[:last] >= case.n - last).all()
        assert (rows[last:] < case.n - last).all() and np.unique(rows).size == rows.size
    if ses.route.presplit:
        assert got["plane"][0] == ng * 2 * case.n * case.dp
    if ses.route.H:
        assert got["fp16"][0] == ng * rows.size * case.n
    for g in ses.graphs:     # a graph that is all one row: a = 0, D2 exactly 0, s = 1
        if R.feat_kind(case, g) == "allsame":
            q = ses.graphs.index(g)
            assert not ses.D2[q].astype(np.float32).any()
            if ses.route.H:
                assert ses.outs[q]["scale"] == 1.0


@pytest.mark.parametrize("name", [c.name for c in R.all_routed_cases() if c.name.endswith("+f32")])
def test_fp32_twin_of_every_fp16_case(name):
    """The GLL_FLAG_D2_F32 run an fp16 case is compared with is held to the reference itself
    (these are the gram_pk<false, TS> and gram_pk2<false> kernels)."""
    case = R.f32_twin(R.CASES[name[:-4]])
    like = _like(case)
    _hold(case, like)


@pytest.mark.parametrize("name", ["bf3h_B3_130x64", "bf3_B2_300x300", "bf3w_B86_300x64",
                                  "pk_B43_300x100", "pk2_B52_512x192"])
def test_graph_of_a_batch_is_the_graph_alone(name):
    """Graph g's D2 (and fp16 scale word) does not depend on where in a batch it sits: against the
    single call where that takes the same kernel (gram_bf3h), else against the batch in reverse
    order (the same route by construction: it depends on B, not on the order)."""
    case = R.CASES[name]
    ses = _session(case)
    if name.startswith("bf3h"):
        for g in ses.graphs:     # the same features: graph g of the batch, alone
            solo = Session(dataclasses.replace(case, B=1), graphs=[g])
            assert np.array_equal(solo.Xh[0], ses.Xh[g]) and solo.route == ses.route
            assert np.array_equal(A.bits(solo.D2[0]), A.bits(ses.D2[g]))
        return
    rev = Session(case, graphs=ses.graphs[::-1])
    assert rev.route == ses.route
    assert np.array_equal(A.bits(rev.D2[::-1]), A.bits(ses.D2))
    if ses.route.H:
        assert [o["scale"] for o in rev.outs[::-1]] == [o["scale"] for o in ses.outs]


def test_tail_settings_give_bitwise_equal_d2():
    """The 14 tail tiles as 64-subtiles, inside the 256-tile launch, and as 128-subtiles."""
    a, b, c = (_session(R.CASES[f"pk2_tail{k}_B90_512x192"]) for k in (0, 1, 2))
    assert (a.route.tail, a.route.sub, b.route.tail, c.route.tail, c.route.sub) == (14, 16, 0, 14, 4)
    assert all(np.array_equal(x, y) for x, y in zip(a.Xh, b.Xh))
    for other in (b, c):
        assert np.array_equal(A.bits(a.D2), A.bits(other.D2))
        assert [o["scale"] for o in a.outs] == [o["scale"] for o in other.outs]
    # and on fp32 storage (gram_pk<false, 64> and gram_pk<false, 128> against gram_pk2<false>)
    fa, fb, fc = (_session(R.f32_twin(R.CASES[f"pk2_tail{k}_B90_512x192"])) for k in (0, 1, 2))
    for other in (fb, fc):
        assert np.array_equal(A.bits(fa.D2), A.bits(other.D2))


@pytest.mark.parametrize("flags", [0, R.FLAG_D2_F32], ids=["fp16", "fp32"])
def test_128_tiles_and_256_tiles_give_bitwise_equal_d2(flags):
    """gram_pk<H, 128> and gram_pk2<H> on the same planes: the same k order per element and the
    same epilogue, so the same bits."""
    c256 = dataclasses.replace(R.CASES["pk2_B43_300x100_t256"], flags=flags,
                               name=f"pk2_B43_300x100_t256/{flags}")
    c128 = dataclasses.replace(c256, tile=128, fam=R.PK, name=f"pk2_B43_300x100_t128/{flags}")
    a, b = _session(c256), _session(c128)
    assert (a.route.family, b.route.family) == (R.PK2, R.PK) and a.route.H == b.route.H
    assert np.array_equal(A.bits(a.D2), A.bits(b.D2))
    for k in ("xhi", "xlo", "xnrm"):
        assert all(np.array_equal(A.bits(x[k]) if k == "xnrm" else x[k],
                                  A.bits(y[k]) if k == "xnrm" else y[k])
                   for x, y in zip(a.outs, b.outs))


def test_locality_order():
    """1100 x 1024, one graph: perm is a permutation of the rows grouped by pivot in order.hip's
    order (pivots ascending, 64-row blocks ascending within a pivot, lanes ascending within a
    block), and pid[i] is the pivot nearest to row i under the stored D2 -- ties to the lower
    pivot -- with the row's rank among its block's rows of that pivot."""
    case = R.ORDER_CASE
    ses = Session(case, order=True)
    assert ses.route == case.route(256) and ses.route.family == R.BF3
    R.check(case, ses.Xh, ses.outs)
    n = case.n
    D2 = ses.D2[0, 0]
    piv_rows = np.array([R.pivot_row(j, n) for j in range(64)])
    want = np.argmin(D2[piv_rows, :], axis=0)          # first minimum: the lower pivot
    piv, rank = ses.pid & 0xFF, ses.pid >> 8
    assert np.array_equal(piv, want)
    assert np.unique(piv).size > 8                     # the grouping is not trivial
    for b0 in range(0, n, 64):
        blk = piv[b0: b0 + 64]
        r = np.array([(blk[:q] == blk[q]).sum() for q in range(blk.size)])
        assert np.array_equal(rank[b0: b0 + 64], r)
    assert np.array_equal(np.sort(ses.perm), np.arange(n))
    assert np.array_equal(ses.perm, np.argsort(piv, kind="stable"))
