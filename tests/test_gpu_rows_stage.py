"""Every row_build_kernel instantiation and every staging / right-hand-side / ELL / virtual-row
regime on the MI355X (-m gpu) against the float64 stage reference of tests/rows_ref.py: exact
where the reference is exact, element by element under its derived bound elsewhere.

Everything goes through the C ABI (gll_forward / gll_forward_batched, gll_graph for base = 0) into
a workspace filled with 0xFF bytes beforehand: a slot nobody wrote reads as NaN or -1.  Per case
of rows_ref.CASES (pinned against libgll.so's 21 stubs and against the regimes each case claims
by tests/test_rows_ref_cpu.py, on float64 exact kNN lists of the same features):
  1. GLL_K_FINALIZE is bracketed and counts exactly one launch per forward, batched or not;
     GLL_KNOB_ROW_PRE is set for the call and restored in a finally;
  2. the reference is evaluated on the GPU's own knn_idx / knn_d2 / eps (gll_workspace_view) and
     the labels as passed, and rows_ref.check holds row_start / row_len / col / d2 / w / deg
     (gll_workspace_view) and ucnt / diag / rhs / P / ELL / virtual rows
     (gll_workspace_solve_view) of every graph to it.
The solves only read rhs, diag, ucnt, ell and vr (const in every kernel signature of solve.hip and
gridcg.hip, and launch_cg_luu takes the right-hand sides as const void*), so after gll_forward they
stand as the row build left them; P's labeled rows and wadj's are never written again by a forward.

The overflow case runs at K = 25, not the K = 10 first proposed for it: of 700 random unit rows in
16 dimensions about 13 lie closer to a row than the origin does, so at K = 10 the hub is in few
lists (rows_ref._regime_cases).

Measured on the MI355X (profiles/rs01_gpu_rows_stage.txt is the run's own output, per case and the
teardown table; profiles/rs01_gpu_tests.txt the whole suite, 780 tests):
  quantity   elements checked   worst err/bound
  w               948,358           0.7022
  deg              20,722           0.2402
  diag             17,012           0.8899      (its own rounding: half an ulp of deg + tau)
  rhs             371,168           0.5165
  eps              12,400           0.5000      (of one ulp: the square root is correctly rounded)
74 graphs in 52 tests; the file runs in 3.8 s, features and the numpy reference included.  One
bracketed launch per forward in every case, every exact quantity equal, every element within its
bound: no defect found in rows.hip.  Union-max: of 251,946 mutual pairs 142 had two different
directed knn_d2 (hub and near-tie cases, where the select re-ranks a row in float64), so the
maximum was exercised on the MI355X as well as in the CPU reference.  No tolerance is tuned to
these figures: KAPPA_E is an assumption stated in rows_ref.py, the rest is counted from the code.
"""
import time

import numpy as np
import pytest
import torch

from graphlearninglayer_amd import GLL
from graphlearninglayer_amd import _lib as L
from tests import abi as A
from tests import rows_ref as R

pytestmark = pytest.mark.gpu

_stats = {}        # quantity -> [elements, worst err/bound]
_record = {"mutual": 0, "mutual_diff": 0, "graphs": 0, "t0": None}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    A.need_gpu()
    _record["t0"] = time.perf_counter()
    yield
    print(f"\nrows stage: {_record['graphs']} graphs, {time.perf_counter() - _record['t0']:.1f} s")
    for q in ("w", "deg", "diag", "rhs", "eps"):
        cnt, worst = _stats.get(q, (0, 0.0))
        print(f"rows stage {q:5s}: {cnt:9d} elements, worst err/bound {worst:.4f}")
    print(f"rows stage union-max: {_record['mutual']} mutual pairs, {_record['mutual_diff']} with "
          "two different directed knn_d2")


class Session:
    """One case on the device (tests/abi.py Run): the features and labels of its B graphs, B
    workspace blocks of 0xFF bytes, one forward with GLL_K_FINALIZE bracketed."""

    def __init__(self, case, B=None, graphs=None):
        self.case = c = case
        self.B = B = c.B if B is None else B
        self.graphs = list(range(B)) if graphs is None else graphs     # feature seeds
        self.lay = c.layout()
        Xh = np.stack([R.features(c, g) for g in self.graphs])
        self.Yh = [R.labels(c, g) for g in self.graphs]
        one = B == 1
        Y = (self.Yh[0] if one else np.stack(self.Yh)) if c.base else None
        self.run = A.Run(Xh[0] if one else Xh, Y, c.K, R.TAU, c.eps, c.flags, C=c.C, ws_fill=0xFF,
                         y_dtype=c.y_dtype)
        with A.knobs({L.KNOB_ROW_PRE: c.knob_pre}), A.launches(L.K_FINALIZE) as ran:
            if c.graph_api:
                assert B == 1 and c.base == 0
                self.run.graph()
            else:
                self.run.forward()
        self.launches = ran[0]
        self.host = self.run.host_copy()

    def graph(self, q):
        """(Stage on the GPU's own lists, Out) of graph number q of the batch."""
        c, lay, run = self.case, self.lay, self.run
        v, sv = run.view(q), run.solve_view(q)
        assert (sv.SE, sv.VRM, sv.Wcap, sv.RCAP) == (lay.SE, lay.VRM, lay.Wcap, lay.RCAP)
        i32, f32 = np.int32, np.float32
        n, m, C, K = c.n, c.m, c.C, lay.K
        a = lambda ptr, count, dt: run.array(ptr, count, dt, q, snapshot=self.host)
        idx = a(v.knn_idx, n * K, i32).reshape(n, K)
        d2 = a(v.knn_d2, n * K, f32).reshape(n, K)
        eps = a(v.eps, n, f32)
        assert (idx[:, 0] == np.arange(n)).all() and not d2[:, 0].any()
        Y = self.Yh[q] if c.base else np.zeros((0, C), dtype=f32)
        st = R.rows_stage(idx, d2, eps, Y, R.TAU, c.base, K, lay,
                          None if c.auto else np.float32(c.eps))
        P = a(sv.P, n * C, f32).reshape(n, C)
        wadj = a(v.wadj - 4 * c.base * C, c.base * C, f32).reshape(c.base, C)
        out = R.Out(a(v.row_start, n, i32), a(v.row_len, n, i32), a(v.col, lay.Etot, i32),
                    a(v.w, lay.Etot, f32), a(v.d2, lay.Etot, f32), a(v.deg, n, f32),
                    a(sv.ucnt, m, i32), a(sv.diag, m, f32), a(sv.rhs, m * C, f32).reshape(m, C),
                    P[: c.base], wadj, a(sv.ell, lay.SE * m * 2, i32),
                    a(sv.vr, m * lay.VRM * R.VR_SLOT, np.uint8), eps,
                    int(a(v.status, L.ST_NWORDS, i32)[L.ST_TINY_EPS]))
        return st, out


def _hold(ses):
    """Every graph of a session under rows_ref.check; the stages."""
    assert ses.launches == 1, f"{ses.launches} bracketed row_build launches in one forward"
    stages, worst_of = [], {}
    for q in range(ses.B):
        st, out = ses.graph(q)
        got = R.check(st, out)
        for k, (cnt, worst) in got.items():
            s = _stats.setdefault(k, [0, 0.0])
            s[0] += cnt
            s[1] = max(s[1], worst)
            worst_of[k] = max(worst_of.get(k, 0.0), worst)
        _record["mutual"] += st.mutual
        _record["mutual_diff"] += st.mutual_diff
        _record["graphs"] += 1
        stages.append((st, out))
    c = ses.case
    route = R.route(ses.lay.K, ses.B, c.y_dtype, c.knob_pre)
    print(f"{c.name} row_build_kernel<{','.join(map(str, route))}>: longest row "
          f"{max(int(st.row_len.max()) for st, _ in stages)}, worst err/bound " +
          ", ".join(f"{k} {v:.3f}" for k, v in worst_of.items()) +
          f", mutual pairs with two d2: {sum(st.mutual_diff for st, _ in stages)}")
    return stages


def _tags(stages, case):
    return set().union(*[R.regimes(st, case) for st, _ in stages])


@pytest.mark.parametrize("name", [c.name for c in R.ALL_CASES if c.name.startswith(("inst_", "kclamp"))])
def test_every_instantiation(name):
    """Label type f32 / f64 / i64 x (K = 10: B = 1, B = 1 prefetch off, B = 3, B = 3 prefetch on;
    K = 66: B = 1, 2; K = 130: B = 1, 2): all 21 instantiations, n = 130 / 150 / 300 with a ragged
    last block, soft and negative labels, C through every class-per-lane form; K = 257; K >= n."""
    case = R.CASES[name]
    stages = _hold(Session(case))
    tags = _tags(stages, case)
    assert set(case.expect) <= tags, sorted(set(case.expect) - tags)
    if name.startswith("kclamp"):
        assert all((st.row_len == case.n - 1).all() for st, _ in stages)


@pytest.mark.parametrize("name", [c.name for c in R.ALL_CASES
                                  if c.name.startswith(("stage_", "rhs_", "ell_", "vr_"))])
def test_every_regime(name):
    """Staging (slot / bump x LDS / global x overflow, the reverse loop's second pass, an overflow
    list past 512 entries holding two rows' entries), right-hand-side forms (prefetched short and
    hub rows, 1-4 classes per lane, 0 / 1 / 15 / 16 / 17 / 33 labeled neighbours, all / none
    labeled, base = 0 and n - 1), ELL widths 24 / 16 / 4 / 0 and the virtual rows.  The tags a case
    is there for are asserted on the GPU's own lists, not only on the CPU's."""
    case = R.CASES[name]
    stages = _hold(Session(case))
    tags = _tags(stages, case)
    assert set(case.expect) <= tags, sorted(set(case.expect) - tags)


@pytest.mark.parametrize("name", ["dups_fixed", "dups_auto", "lattice_ties"])
def test_dropped_edges_and_near_ties(name):
    """Duplicate clusters larger and smaller than K: rows without an entry have deg exactly 0,
    diag exactly tau and rhs exactly 0 out of a 0xFF-filled workspace; with auto eps the rows whose
    eps is 0 have w = 0 as the float64 formula gives, and the status word is set.  The lattice
    set is there for the union-max count (near-ties: the select re-ranks rows in float64)."""
    case = R.CASES[name]
    (st, out), = _hold(Session(case))
    tags = _tags([(st, out)], case)
    assert set(case.expect) <= tags, sorted(set(case.expect) - tags)
    if name.startswith("dups"):
        empty = st.row_len == 0
        assert empty.sum() >= 12
        assert not out.deg[empty].any() and not out.rhs[empty[case.base:]].any()
        assert (out.diag[empty[case.base:]] == np.float32(R.TAU)).all()
    if name == "dups_auto":
        z = (out.eps[st.row] == 0) | (out.eps[st.col] == 0)
        e = np.repeat(out.row_start.astype(np.int64) - st.row_ptr[:-1], st.row_len) + \
            np.arange(st.col.size)
        assert z.any() and not out.w[e][z].any()
        assert out.tiny_eps == 1


def _compact(st, out):
    e = np.repeat(out.row_start.astype(np.int64) - st.row_ptr[:-1], st.row_len) + \
        np.arange(st.col.size)
    return [out.row_len, out.col[e], out.w[e].view(np.uint32), out.d2[e].view(np.uint32),
            out.deg.view(np.uint32), out.ucnt, out.diag.view(np.uint32),
            out.rhs.view(np.uint32), out.ell, out.vr, out.eps.view(np.uint32)]


def test_non_finite_row_in_a_batch_leaves_the_other_graphs_alone():
    """One row of NaN features in graph 1 of three: graphs 0 and 2 are bitwise what single calls
    give (the storage compared row by row: bump rows are handed out in arrival order), and graph
    1 itself is held to the reference of its own lists."""
    case = R.CASES["nonfinite_in_batch"]
    batch = _hold(Session(case))
    assert not np.isfinite(R.features(case, 1)).all()
    for g in (0, 2):
        (st, out), = _hold(Session(case, B=1, graphs=[g]))
        for a, b in zip(_compact(*batch[g]), _compact(st, out)):
            assert np.array_equal(a, b)


def test_device_graph_compacts_the_padded_rows_of_the_view():
    """GLL.device_graph's row_ptr / col / w / d2 are the padded rows of the workspace view, bitwise,
    on a hub case (bump rows included)."""
    hub = R.CASES["stage_bump_lds_ovf"]
    case = R.Case("device_graph_hub", hub.n, 0, C=1, K=hub.K, hubs=hub.hubs, feat="hub",
                  graph_api=True, seed=hub.seed)
    (st, out), = _hold(Session(case))
    assert "bump+lds+ovf" in R.regimes(st, case)
    g = GLL.device_graph(torch.from_numpy(R.features(case)), case.K, 1.0)
    rl, col, w, d2 = _compact(st, out)[:4]
    assert np.array_equal(g["row_ptr"].cpu().numpy(), np.r_[0, np.cumsum(rl)])
    assert np.array_equal(g["col"].cpu().numpy(), col)
    assert np.array_equal(g["w"].cpu().numpy().view(np.uint32), w)
    assert np.array_equal(g["d2"].cpu().numpy().view(np.uint32), d2)
    assert np.array_equal(g["deg"].cpu().numpy(), out.deg)
