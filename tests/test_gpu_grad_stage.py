"""Every feature-gradient kernel on the MI355X (-m gpu) against the float64 stage reference of
tests/grad_ref.py, element by element under its derived bound.

Everything goes through the C ABI (flags, an X pointer off 16-B alignment and the batched entry
points are not reachable from `apply`).  Per case of grad_ref.CASES (the smallest shapes that reach
each of the 102 edge_coef / grad_spmm / grad_chunk / cg_grad_fused instantiations -- pinned against
libgll.so's stubs by tests/test_grad_ref_cpu.py -- plus the residues the fused kernel's workgroup
rank depends on, hubs, duplicate clusters and K >= n), and per backward on the case's workspace:
  1. grad_X is filled with NaN before the call: a row no wave wrote fails isfinite;
  2. the launches of the edge pass, the gradient, the fused backward and the CG are bracketed and
     their counts equal grad_ref.route()'s -- the intended kernel ran (for the fused backward,
     whose co-residency gate route() cannot restate, GLL_K_BWD == 1 is the proof);
  3. the float64 closed form is evaluated on the arrays the kernels read (gll_workspace_view after
     the backward: the GPU's own fp32 graph, U32 and wadj), and EVERY element of every row of
     every graph satisfies |gpu - ref| <= bound, with exact zeros where the bound is 0.
Features: synth, tau 0.07, gbar seeded_gbar; the fused cases run three backwards on one workspace
(gbar fp32, fp64, fp32).

Measured on the MI355X (profiles/gs01_gpu_tests.txt holds every figure of the run; wall time is
the tests' own, features and the numpy reference included):
  family                              cases   worst err/bound   worst err/max|grad|   wall time
  edge pass (edge_coef_kernel)          81        0.0798             4.27e-07            0.2 s
  grad_spmm_kernel                     114        0.1087             3.87e-07            0.7 s
  grad_chunk_kernel                     30        0.1025             4.14e-07            0.1 s
  fused backward (cg_grad_fused)        75        0.0843             3.44e-07            0.9 s
The hub row of 149 edges: 0.017 of its bound in the fused kernel, 0.008 through the 32-lane edge
pass.  Every launch count equalled route()'s, every fused case ran the fused kernel, and no
element was left NaN: no defect found.  The whole file runs in 5 s.
"""
import time

import numpy as np
import pytest

from graphlearninglayer_amd import _lib as L
from tests import abi as A
from tests import grad_ref as R
from tests.launch_counts import counted

pytestmark = pytest.mark.gpu

_worst = {}     # family -> [cases, worst err/bound, worst err/max|grad|, seconds]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    A.need_gpu()
    yield
    for fam, (cnt, rb, rg, sec) in sorted(_worst.items()):
        print(f"\ngrad stage {fam}: {cnt} cases, worst err/bound {rb:.4f}, worst err/max|grad| "
              f"{rg:.2e}, {sec:.1f} s")


class Session:
    """One case on the device (tests/abi.py Run): the features of its B graphs (optionally 4
    bytes off 16-B alignment), B workspace blocks, one forward; then backwards into NaN-filled
    outputs."""

    def __init__(self, case):
        self.case = c = case
        xy = [R.features(c, g) for g in range(c.B)]
        self.Xh = np.stack([x for x, _ in xy])
        self.Yh = np.stack([y for _, y in xy])
        self.gb = np.stack([R.gbar(c, g) for g in range(c.B)])
        one = c.B == 1
        self.run = A.Run(self.Xh[0] if one else self.Xh, self.Yh[0] if one else self.Yh, c.K, R.TAU,
                         c.eps, c.flags, aligned=c.aligned)
        self.U = self.run.forward().reshape(c.B, c.m, c.C)

    def backward(self, g_dtype):
        """(grad_X B x n x d from a NaN-filled buffer, the launches bracketed)."""
        c = self.case
        with counted() as got:
            gx = self.run.backward(self.gb, L.GLL_DT_F32 if g_dtype == "f32" else L.GLL_DT_F64)
        return gx.reshape(c.B, c.n, c.d), got

    def stage(self, g):
        """The float64 closed form on graph g's workspace arrays as the backward left them."""
        c, run = self.case, self.run
        v = run.view(g)
        K = min(c.K, c.n)
        i32, f32 = np.int32, np.float32
        a = lambda ptr, count, dt: run.array(ptr, count, dt, g)
        rs, rl = a(v.row_start, c.n, i32), a(v.row_len, c.n, i32)
        E = int((rs.astype(np.int64) + rl).max())
        U32 = a(v.U32, c.m * c.C, f32).reshape(c.m, c.C)
        wadj = a(v.wadj, c.m * c.C, f32).reshape(c.m, c.C)
        assert np.isfinite(U32).all() and np.isfinite(wadj).all()
        st = a(v.status, L.ST_NWORDS, i32)
        assert st[L.ST_SOLVE_FAILED] == 0 and st[L.ST_BWD_NONCONV] == 0
        return R.grad_stage(
            rs, rl, a(v.col, E, i32), a(v.w, E, f32), a(v.d2, E, f32), a(v.eps, c.n, f32),
            a(v.knn_idx, c.n * K, i32).reshape(c.n, K),
            np.concatenate([self.Yh[g], U32]), np.concatenate([np.zeros_like(self.Yh[g]), wadj]),
            self.Xh[g], c.auto, None if c.auto else np.float32(c.eps)), rl


def _run(case):
    """Every backward of a case under the three rules of the docstring: (worst err/bound, worst
    err/max|grad|, longest row)."""
    t0 = time.perf_counter()
    ses = Session(case)
    worst_b = worst_g = 0.0
    longest = 0
    for q, g_dtype in enumerate(case.g_dtypes):
        gx, got = ses.backward(g_dtype)
        want = case.route(g_dtype)
        assert got.counts == want.counts, (case.name, q, got, want)
        for g in range(case.B):
            st, rl = ses.stage(g)
            longest = max(longest, int(rl.max()))
            rb, rg = R.check(gx[g], st)
            worst_b, worst_g = max(worst_b, rb), max(worst_g, rg)
            assert np.abs(st.grad).max() > 0          # a case that computes nothing proves nothing
    sec = time.perf_counter() - t0
    w = _worst.setdefault(case.group, [0, 0.0, 0.0, 0.0])
    w[0] += 1
    w[1], w[2], w[3] = max(w[1], worst_b), max(w[2], worst_g), w[3] + sec
    ran = ", ".join(sorted(k + "<" + ",".join(map(str, a)) + ">" for k, a in case.kernels()))
    print(f"{case.name} ({ran}): launches {case.route().counts}, longest row {longest}, "
          f"worst err/bound {worst_b:.4f}, err/max|grad| {worst_g:.2e}, {sec * 1e3:.0f} ms")
    return worst_b, worst_g, longest, ses


def _names(group):
    return [c.name for c in R.ALL_CASES if c.group == group and not c.name.startswith(
        ("hub_", "dups_", "kclamp_"))]


@pytest.mark.parametrize("name", _names("edge"))
def test_edge_pass_every_class_form_and_lane_count(name):
    """edge_coef_kernel: auto eps at C = 1..18 and 33 (every exact form, every bound form with C
    strictly below the bound, the generic loop) x 16 / 32 lanes per row x one graph / three; the
    fixed-eps pass of the chunked gradient.  n = 130: a ragged last block of 16 or 8 rows."""
    case = R.CASES[name]
    assert case.route().counts[0] == 1
    _run(case)


@pytest.mark.parametrize("name", _names("spmm"))
def test_grad_spmm_every_form(name):
    """grad_spmm_kernel: AUTO x ND x VEC x WIDE x CV, all 48 forms, at n = 70 (not a multiple of
    the 4 rows of a block); VEC off by an odd d and by an X pointer 4 bytes off alignment."""
    case = R.CASES[name]
    assert case.route().family == "spmm"
    _run(case)


@pytest.mark.parametrize("name", _names("chunk"))
def test_grad_chunk_every_form(name):
    """grad_chunk_kernel: COEF 1 / 2 x LPR 16 / 32 / 64, whole and ragged last chunks, forced at
    B = 1 and automatic at B = 2."""
    case = R.CASES[name]
    assert case.route().family == "chunk"
    _run(case)


@pytest.mark.parametrize("name", _names("fused"))
def test_fused_backward_gradient_role(name):
    """cg_grad_fused_kernel: every NT x ND x gbar type; per NT both ends of its m range and eight
    n that take the gradient-workgroup count through every residue mod 8 (the XCD-major rank) with
    ragged last chunks of the class sort and a ragged last workgroup; a hub row (the e0 != beg
    path); one non-empty class.  Three backwards on the workspace: the counters re-arm."""
    case = R.CASES[name]
    _, _, longest, ses = _run(case)
    for g_dtype in case.g_dtypes:
        assert case.route(g_dtype).counts == (0, 0, 1, 0)
    if case.feat == "hub":
        assert longest > 128
    if case.feat == "one_class":
        P = np.concatenate([ses.Yh[0], ses.U[0]])
        assert (P.argmax(axis=1) == 0).all()


@pytest.mark.parametrize("name", [c.name for c in R.ALL_CASES
                                  if c.name.startswith(("hub_", "dups_", "kclamp_"))])
def test_hubs_duplicates_and_clamped_k_in_every_family(name):
    """Rows longer than two 64-edge steps (a hub), rows with no edge (duplicates beyond K:
    exactly 0 out of a NaN-filled buffer) and the complete graph (K >= n) through the edge pass,
    grad_spmm, grad_chunk and the fused backward."""
    case = R.CASES[name]
    assert case.route().family == case.group or case.group == "edge"
    _, _, longest, ses = _run(case)
    if case.feat == "hub":
        assert longest > 128
    if case.feat == "dups":
        st, rl = ses.stage(0)
        assert (rl == 0).sum() >= 3 and not st.bound[rl == 0].any()
    if name.startswith("kclamp"):
        assert longest == case.n - 1
