"""Float64 reference of the graph row build STAGE alone (rows.hip row_build_kernel), with exact
and derived elementwise conditions -- a test helper, not a test (numpy only; never imported by
the product).

The yardstick of tests/test_gpu_rows_stage.py (pinned on the CPU by tests/test_rows_ref_cpu.py).
The inputs are exactly what the kernel reads: the workspace's knn_idx / knn_d2 (fp32 squared
distances as the select wrote them), eps (per row, or the fixed eps as fp32), Y in its own dtype,
tau, base, K.  With list(i) = knn_idx[i, 1:K]:

    row(i)   = {j in list(i): d2 > 0, j != i}  U  {l: i in list(l) with d2 > 0}, columns ascending
    d2_ij    = the fp32 maximum of the two directions (one direction: that one)
    W_ij     = exp(-a_ij),  a_ij = 4 d2_ij / (eps_i eps_j)           float64 of the fp32 inputs
    deg_i    = sum_j W_ij           diag_u = deg_{base+u} + tau
    rhs[u,c] = sum_{j < base} W_ij float32(Y[j, c])                  i = base + u
    ucnt_u   = #{j in row(i): j >= base}: the row's sorted suffix;   nlab = row_len - ucnt
    P[j]     = float32(Y[j]) on the labeled rows

EXACT (bitwise against the workspace): row_len, col, d2, ucnt; the ELL and virtual-row columns;
the ELL and virtual-row weights against the CSR w of the same edge; P on labeled rows; the labeled
rows of wadj (0); the symmetry of the graph (pattern, d2 and w of (i, j) and (j, i)); the storage
rule (rows disjoint inside Etot, a slot row at i Wcap, the others in the bump region behind
n Wcap).  An eps_i eps_j of 0 ('auto' eps of a row whose K nearest coincide with it) makes a = inf
and W = 0 in float64 as in fp32: w is then exactly 0.

BOUNDED, u = 2^-24, every element (check() asserts; where a bound is 0 the value is exactly 0):
    w     |w - W| <= W u (KAPPA_A a + KAPPA_E) + TINY
          KAPPA_A = 2: the argument -4 d2 / fl(eps_i eps_j) takes two roundings, the product and
          the division (-4 d2 is exact), each a relative u of a, i.e. an absolute 2 u a in the
          exponent, i.e. a relative 2 u a of W to first order.  One rounding for the division
          needs it correctly rounded: hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt
          decides that, and build.py's FLAGS (-O3, no fast-math, no
          -fno-hip-fp32-correctly-rounded-divide-sqrt) leave the default on.
          KAPPA_E = 4: the device expf taken as accurate to 2 ulp, and an ulp is at most 2 u of
          the value.  This is an ASSUMPTION: neither the HIP headers nor any document installed
          with the toolchain state expf's accuracy (AMD's published HIP math tables say 1 ulp).
          It is not taken from what a GPU returned.
          TINY = the smallest normal fp32: results below it may be flushed to 0 or rounded as
          subnormals.
    deg   sum of the row's w bounds + u (ceil(L / 64) + 7) sum W: the lane-strided partial sums
          (ceil(L / 64) additions per lane) and the six steps of the wave reduction (+1 spare)
    diag  the deg bound + u |diag| (one rounding); exactly tau on a row without entries
    rhs   sum_j |Y_jc| bound(W_ij) + u (nlab + 1) sum_j W_ij |Y_jc|: a product and at most nlab
          additions per term, whatever the order; exactly 0.0 where no labeled neighbour of the
          row has a nonzero label in class c
    eps   (auto) within 1 ulp of the float64 sqrt of knn_d2[i, K-1], K clamped to n;
          GLL_ST_TINY_EPS is set exactly when some eps is below 1e-10

Thresholds restated here (next to each: the code it restates):
    Wcap = 5 (K-1) + 8, RCAP = 8 (K-1) + 8, Etot = n Wcap + 2 n (K-1)   gll_internal.h Layout
    slot / bump:     nf + rc <= Wcap / >     rows.hip row_build_kernel `lbound > a.Wcap`
    LDS / global:    nf + rc <= 256 / >      rows.hip kStage, `lbound <= kStage`
    overflow:        rc > RCAP               rows.hip build_row `rc > a.RCAP` (select.hip pushes
                                             reverse entry number RCAP.. onto the overflow list)
    second reverse pass: min(rc, RCAP) > 64  rows.hip build_row `r0 += kWave`
    second overflow scan: more than 512 overflow entries   rows.hip build_row OB * kWave
    prefetched labels: PRE kernel, LDS row, C <= 16; <= 64 entries / hub   rows.hip ypre
    classes per lane: ceil(C / 64) of 4 accumulators                       rows.hip kMaxCPerLane
    SE = 24 / 16 / 4 / 0 by m                gll_internal.h ell_slots
    VRM = min(63, ceil(Wcap / 8)) when the balanced CG runs, else 0   gll_internal.h vr_max_per_row
with nf the valid forward entries of a row and rc its reverse entries (= the valid directed
entries naming it).  `route` restates launch_finalize's choice of instantiation; CASES holds the
shapes of the GPU test, and tests/test_rows_ref_cpu.py checks on float64 exact kNN lists of the
same features that they reach every instantiation libgll.so holds and every regime of REQUIRED.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from tests import cg_ref

U = 2.0 ** -24                              # unit roundoff of fp32
TINY = float(np.finfo(np.float32).tiny)     # smallest normal fp32
KAPPA_A = 2.0
KAPPA_E = 4.0
K_STAGE, WAVE, VS, VR_SLOT, OVF_STEP = 256, 64, 8, 48, 512
FLAG_CG_ELL, FLAG_CG_VR = 512, 1024
D = 16                                      # feature dimension of every case
TAU = 0.07


def ell_slots(m):
    return 24 if m <= 512 else 16 if m <= 2048 else 4 if m <= 4096 else 0


@dataclass(frozen=True)
class Layout:
    n: int
    base: int
    m: int
    K: int
    Wcap: int
    RCAP: int
    Etot: int
    SE: int
    VRM: int


def layout(n, base, K, flags=0, knob_rv=0):
    K = min(K, n)
    m = n - base
    wcap = 5 * (K - 1) + 8
    rv = cg_ref.vr_threads(n, m, K, flags, knob_rv)
    return Layout(n, base, m, K, wcap, 8 * (K - 1) + 8, n * wcap + 2 * n * (K - 1), ell_slots(m),
                  min(63, (wcap + VS - 1) // VS) if rv else 0)


def _seg_sum(T, seg, nseg):
    """Sum the rows of T per segment id (seg ascending): nseg x T.shape[1:]."""
    out = np.zeros((nseg,) + T.shape[1:], dtype=T.dtype)
    if T.shape[0]:
        cnt = np.bincount(seg, minlength=nseg)
        live = cnt > 0
        out[live] = np.add.reduceat(T, (np.cumsum(cnt) - cnt)[live], axis=0)
    return out


def y_f32(Y):
    """float32(Y) as the kernel's static_cast takes it (round to nearest from float64 / int64)."""
    return np.asarray(Y).astype(np.float32)


@dataclass
class Stage:
    lay: Layout
    C: int
    row_len: np.ndarray     # n
    row_ptr: np.ndarray     # n + 1 (compact)
    row: np.ndarray         # E (compact CSR, row-major, columns ascending)
    col: np.ndarray         # E
    d2: np.ndarray          # E float32
    a: np.ndarray           # E float64
    W: np.ndarray           # E float64
    wb: np.ndarray          # E bound of w
    deg: np.ndarray
    deg_b: np.ndarray
    diag: np.ndarray        # m
    diag_b: np.ndarray
    rhs: np.ndarray         # m x C
    rhs_b: np.ndarray
    nlab: np.ndarray        # n labeled entries per row
    ucnt: np.ndarray        # m
    P_lab: np.ndarray       # base x C float32
    nf: np.ndarray          # n valid forward entries
    rc: np.ndarray          # n reverse entries
    ell_src: np.ndarray     # SE x m: compact edge of the slot, -1 = pad
    vr_src: np.ndarray      # m x VRM x 8: compact edge, -1 = zero pad, -2 = slot not written
    mutual: int             # mutual pairs
    mutual_diff: int        # ... whose two directed d2 differ
    eps_in: np.ndarray      # n float64 eps the weights were formed with
    auto: bool
    eps_ref: np.ndarray     # n float64 sqrt(knn_d2[:, K-1])
    tau: float


def rows_stage(knn_idx, knn_d2, eps, Y, tau, base, K, lay: Layout, eps_fixed=None):
    """The reference above.  knn_idx / knn_d2: n x K as in the workspace; eps: n values as they
    stand in the workspace (auto; taken to float64 exactly), or eps_fixed for every row; Y: base x C
    in its own dtype."""
    f = np.float64
    knn_idx = np.asarray(knn_idx)
    knn_d2 = np.asarray(knn_d2, dtype=np.float32)
    n = knn_idx.shape[0]
    assert knn_idx.shape == (n, K) and knn_d2.shape == (n, K) and K == lay.K and n == lay.n
    i = np.repeat(np.arange(n, dtype=np.int64), K - 1)
    j = knn_idx[:, 1:].astype(np.int64).ravel()
    dd = knn_d2[:, 1:].ravel()
    valid = (dd > 0) & (j != i) & (j >= 0) & (j < n)          # rows.hip fval; NaN is not > 0
    i, j, dd = i[valid], j[valid], dd[valid]
    nf = np.bincount(i, minlength=n)
    rc = np.bincount(j, minlength=n)
    key = np.concatenate([i * n + j, j * n + i])
    dv = np.concatenate([dd, dd])
    order = np.argsort(key, kind="stable")
    ks, dv = key[order], dv[order]
    first = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]]) if ks.size else np.zeros(0, np.int64)
    if ks.size:
        d2 = np.maximum.reduceat(dv, first).astype(np.float32)
        dmin = np.minimum.reduceat(dv, first)
        mult = np.diff(np.r_[first, ks.size])
    else:
        d2, dmin, mult = np.zeros(0, np.float32), np.zeros(0, np.float32), np.zeros(0, np.int64)
    assert (mult <= 2).all()                                   # a list names a column once
    row, col = ks[first] // n, ks[first] % n
    row_len = np.bincount(row, minlength=n)
    row_ptr = np.r_[0, np.cumsum(row_len)]
    auto = eps_fixed is None
    ep = np.asarray(eps, dtype=f) if auto else np.full(n, f(np.float32(eps_fixed)))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        a = 4.0 * d2.astype(f) / (ep[row] * ep[col])
        W = np.exp(-a)
        wb = np.where(W > 0, W * U * (KAPPA_A * np.where(np.isfinite(a), a, 0.0) + KAPPA_E), 0.0)
    wb = np.where(np.isfinite(a), wb + TINY, 0.0)              # eps_i eps_j = 0: exactly 0
    deg = _seg_sum(W, row, n)
    deg_b = _seg_sum(wb, row, n) + U * ((row_len + WAVE - 1) // WAVE + 7) * deg
    tau64 = f(np.float32(tau))
    diag = deg[base:] + tau64
    diag_b = np.where(row_len[base:] > 0, deg_b[base:] + U * np.abs(diag), 0.0)
    Y32 = y_f32(Y)
    C = Y32.shape[1]
    Y64 = Y32.astype(f)
    lab = col < base
    nlab = np.bincount(row[lab], minlength=n)
    lm = lab & (row >= base)
    m = n - base
    Ya = np.abs(Y64[col[lm]])
    rhs = _seg_sum(W[lm, None] * Y64[col[lm]], row[lm] - base, m)
    rhs_b = (_seg_sum(Ya * wb[lm, None], row[lm] - base, m)
             + U * (nlab[base:] + 1)[:, None] * _seg_sum(W[lm, None] * Ya, row[lm] - base, m))
    rhs_b[_seg_sum((Ya > 0).astype(f), row[lm] - base, m) == 0] = 0.0
    ucnt = (row_len - nlab)[base:]
    # expected ELL slice and virtual rows, as the compact edge each slot copies
    ub = (row_ptr[:-1] + nlab)[base:]                          # first U-block edge of each U row
    s = np.arange(lay.SE, dtype=np.int64)[:, None]
    ell_src = np.where(s < ucnt[None, :], ub[None, :] + s, -1)
    q = np.arange(lay.VRM * VS, dtype=np.int64)[None, :]
    nv = np.minimum((ucnt + VS - 1) // VS, lay.VRM)[:, None]
    vr_src = np.where(q < nv * VS, np.where(q < ucnt[:, None], ub[:, None] + q, -1), -2)
    vr_src = vr_src.reshape(m, lay.VRM, VS)
    kth2 = knn_d2[:, K - 1].astype(f)
    return Stage(lay, C, row_len, row_ptr, row, col, d2, a, W, wb, deg, deg_b, diag, diag_b, rhs,
                 rhs_b, nlab, ucnt, Y32, nf, rc, ell_src, vr_src, int((mult == 2).sum()) // 2,
                 int(((mult == 2) & (dmin != d2)).sum()) // 2, ep, auto, np.sqrt(kth2), float(tau64))


# ------------------------------------------------------------------------------------------
# What a workspace holds after the row build, and its check
# ------------------------------------------------------------------------------------------
@dataclass
class Out:
    row_start: np.ndarray   # n int32
    row_len: np.ndarray     # n int32
    col: np.ndarray         # Etot int32 (padded storage)
    w: np.ndarray           # Etot float32
    d2: np.ndarray          # Etot float32
    deg: np.ndarray         # n float32
    ucnt: np.ndarray        # m int32
    diag: np.ndarray        # m float32
    rhs: np.ndarray         # m x C float32
    P_lab: np.ndarray       # base x C float32
    wadj_lab: np.ndarray    # base x C float32, or None
    ell: np.ndarray         # SE * m * 2 int32, raw
    vr: np.ndarray          # m * VRM * 48 uint8, raw
    eps: np.ndarray         # n float32
    tiny_eps: int = None    # GLL_ST_TINY_EPS word, or None


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _ratio(err, bound, what, got, ref):
    """Worst err / bound; asserts err <= bound everywhere and exact zeros where the bound is 0."""
    got = np.asarray(got)
    assert np.isfinite(got).all(), f"{what}: {int((~np.isfinite(got)).sum())} non-finite elements"
    zero = bound == 0
    assert not (got[zero] != ref[zero]).any(), \
        f"{what}: {int((got[zero] != ref[zero]).sum())} elements that must be exactly " \
        f"{'0' if not ref[zero].any() else 'the reference'} are not"
    r = np.where(zero, 0.0, err / np.where(zero, 1.0, bound))
    worst = float(r.max(initial=0.0))
    if worst > 1.0:
        k = np.unravel_index(int(np.argmax(r)), r.shape)
        raise AssertionError(f"{what} err/bound {worst:.3f} at {tuple(int(x) for x in k)}: got "
                             f"{got[k]!r}, float64 {ref[k]!r}, bound {bound[k]:.3e}, "
                             f"{int((r > 1).sum())} elements past the bound")
    return worst


def check(st: Stage, o: Out, poison=True):
    """Hold a workspace to the stage reference.  Returns {quantity: (elements, worst err/bound)}
    for w, deg, diag, rhs, eps.  `poison`: the workspace was filled with 0xFF bytes beforehand,
    so a virtual-row slot the kernel must not write still holds them."""
    lay = st.lay
    n, base, m, C = lay.n, lay.base, lay.m, st.C
    f = np.float64
    rl = np.asarray(o.row_len, dtype=np.int64)
    rs = np.asarray(o.row_start, dtype=np.int64)
    bad = np.flatnonzero(rl != st.row_len)
    assert bad.size == 0, f"row_len differs on {bad.size} rows, first {bad[0]}: " \
                          f"{rl[bad[0]]} != {st.row_len[bad[0]]}"
    # storage: a slot row at i Wcap, the others in the bump region; disjoint, inside Etot
    slot = st.nf + st.rc <= lay.Wcap
    assert (rs[slot] == np.arange(n)[slot] * lay.Wcap).all(), "a slot row does not start at i Wcap"
    assert (rs[~slot] >= n * lay.Wcap).all(), "a bump row starts inside the slots"
    assert (rs >= 0).all() and (rs + rl <= lay.Etot).all(), "a row leaves the Etot entries"
    live = np.flatnonzero(rl > 0)
    by = live[np.argsort(rs[live], kind="stable")]
    assert (rs[by][1:] >= (rs + rl)[by][:-1]).all(), "rows overlap in storage"
    e = np.repeat(rs - st.row_ptr[:-1], rl) + np.arange(int(rl.sum()), dtype=np.int64)
    col, d2, w = np.asarray(o.col)[e], np.asarray(o.d2)[e], np.asarray(o.w)[e]
    bad = np.flatnonzero(col != st.col)
    assert bad.size == 0, f"col differs on {bad.size} entries, first in row {st.row[bad[0]]}: " \
                          f"{col[bad[0]]} != {st.col[bad[0]]}"
    bad = np.flatnonzero(_bits(d2) != _bits(st.d2))
    assert bad.size == 0, f"d2 differs on {bad.size} entries, first ({st.row[bad[0]]}, " \
                          f"{st.col[bad[0]]}): {d2[bad[0]]!r} != {st.d2[bad[0]]!r}"
    # symmetry: the pattern and d2 equal a symmetric reference; w of (i, j) and (j, i) bitwise
    t = np.searchsorted(st.row * n + st.col, st.col * n + st.row)
    assert (_bits(d2)[t] == _bits(d2)).all() and (col[t] == st.row).all(), "d2 is not symmetric"
    bad = np.flatnonzero(_bits(w)[t] != _bits(w))
    assert bad.size == 0, f"w is not symmetric on {bad.size} entries, first ({st.row[bad[0]]}, " \
                          f"{st.col[bad[0]]})"
    stats = {}
    stats["w"] = (w.size, _ratio(np.abs(w.astype(f) - st.W), st.wb, "w", w, st.W))
    deg = np.asarray(o.deg)
    stats["deg"] = (n, _ratio(np.abs(deg.astype(f) - st.deg), st.deg_b, "deg", deg, st.deg))
    diag = np.asarray(o.diag)
    stats["diag"] = (m, _ratio(np.abs(diag.astype(f) - st.diag), st.diag_b, "diag", diag,
                               np.where(st.diag_b == 0, f(np.float32(st.tau)), st.diag)))
    rhs = np.asarray(o.rhs).reshape(m, C)
    stats["rhs"] = (m * C, _ratio(np.abs(rhs.astype(f) - st.rhs), st.rhs_b, "rhs", rhs, st.rhs))
    bad = np.flatnonzero(np.asarray(o.ucnt) != st.ucnt)
    assert bad.size == 0, f"ucnt differs on {bad.size} rows, first u = {bad[0]}"
    assert (_bits(np.asarray(o.P_lab).reshape(base, C)) == _bits(st.P_lab)).all(), \
        "P differs from float32(Y) on a labeled row"
    if o.wadj_lab is not None:
        assert not _bits(o.wadj_lab).any(), "a labeled row of wadj is not 0"
    # ELL slice: column-major, two slots per 16-B record
    if lay.SE and m:
        rec = np.asarray(o.ell, dtype=np.int32).reshape(lay.SE // 2, m, 2, 2)
        got = rec.transpose(0, 2, 1, 3).reshape(lay.SE, m, 2)      # slot s = 2 (s / 2) + s % 2
        pad = st.ell_src < 0
        assert not got[pad].any(), f"ELL pad slot not (0, 0.0): {int(got[pad].any(axis=1).sum())} slots"
        src = st.ell_src[~pad]
        assert (got[~pad][:, 0] == st.col[src] - base).all(), "ELL column differs"
        assert (got[~pad][:, 1].view(np.uint32) == _bits(w)[src]).all(), \
            "ELL weight differs from the CSR w of its edge"
    # virtual rows: 8 u16 offsets then 8 fp32 weights per 48-B slot
    if lay.VRM and m:
        raw = np.asarray(o.vr, dtype=np.uint8).reshape(m, lay.VRM, VR_SLOT)
        off = np.ascontiguousarray(raw[:, :, :2 * VS]).view(np.uint16).reshape(m, lay.VRM, VS)
        wt = np.ascontiguousarray(raw[:, :, 2 * VS:]).view(np.uint32).reshape(m, lay.VRM, VS)
        edge, padq, none = st.vr_src >= 0, st.vr_src == -1, st.vr_src == -2
        src = st.vr_src[edge]
        assert (4 * (st.col[src] - base) < 65536).all()
        assert (off[edge] == 4 * (st.col[src] - base)).all(), "virtual-row column offset differs"
        assert (wt[edge] == _bits(w)[src]).all(), \
            "virtual-row weight differs from the CSR w of its edge"
        assert not off[padq].any() and not wt[padq].any(), "virtual-row pad entry not (0, 0.0)"
        if poison:
            assert (off[none] == 0xFFFF).all() and (wt[none] == 0xFFFFFFFF).all(), \
                "a virtual-row slot past the row's count was written"
    # eps
    eps = np.asarray(o.eps, dtype=np.float32)
    if st.auto:
        ulp = np.spacing(np.maximum(st.eps_ref.astype(np.float32), np.float32(TINY))).astype(f)
        stats["eps"] = (n, _ratio(np.abs(eps.astype(f) - st.eps_ref), ulp, "eps", eps, st.eps_ref))
    else:
        assert (_bits(eps) == _bits(st.eps_in.astype(np.float32))).all(), "eps is not the fixed eps"
        stats["eps"] = (0, 0.0)
    if o.tiny_eps is not None:
        want = bool((~(eps >= np.float32(1e-10))).any())
        assert bool(o.tiny_eps) == want, f"GLL_ST_TINY_EPS {o.tiny_eps}, some eps < 1e-10: {want}"
    return stats


def emulate_f32(st: Stage, rng=None):
    """The same formulas in numpy float32 -- numpy's float32 exp, one rounding per operation, each
    row's sums in a random order -- laid out as a workspace holds them (0xFF-filled storage, bump
    rows in row order): an Out.  What the bounds must admit on the CPU, and the raw material of
    the failure-injection tests."""
    f32 = np.float32
    rng = np.random.default_rng(0) if rng is None else rng
    lay = st.lay
    n, base, m, C = lay.n, lay.base, lay.m, st.C
    ep = st.eps_in.astype(f32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        w = np.exp((f32(-4.0) * st.d2) / (ep[st.row] * ep[st.col]))
    assert w.dtype == f32
    deg = np.zeros(n, dtype=f32)
    rhs = np.zeros((m, C), dtype=f32)
    for i in range(n):
        q = st.row_ptr[i] + rng.permutation(int(st.row_len[i]))
        if q.size:
            deg[i] = np.cumsum(w[q], dtype=f32)[-1]
        if i >= base:
            ql = q[st.col[q] < base]
            if ql.size:
                rhs[i - base] = np.cumsum(w[ql, None] * st.P_lab[st.col[ql]], axis=0, dtype=f32)[-1]
    lb = st.nf + st.rc
    bump = lb > lay.Wcap
    rs = np.arange(n, dtype=np.int64) * lay.Wcap
    rs[bump] = n * lay.Wcap + (np.cumsum(np.where(bump, lb, 0)) - lb)[bump]
    col = np.full(lay.Etot, -1, dtype=np.int32)
    ws = np.full(lay.Etot, np.nan, dtype=f32)
    d2s = np.full(lay.Etot, np.nan, dtype=f32)
    e = np.repeat(rs - st.row_ptr[:-1], st.row_len) + np.arange(st.col.size, dtype=np.int64)
    col[e], ws[e], d2s[e] = st.col, w, st.d2
    wbits = w.view(np.uint32)
    pad = st.ell_src < 0
    src = np.where(pad, 0, st.ell_src)
    slots = np.zeros((lay.SE, m, 2), dtype=np.int32)
    if st.col.size:
        slots[..., 0] = np.where(pad, 0, st.col[src] - base)
        slots[..., 1] = np.where(pad, 0, wbits[src]).astype(np.uint32).view(np.int32)
    ell = slots.reshape(lay.SE // 2, 2, m, 2).transpose(0, 2, 1, 3).ravel()
    vr = np.full((m, lay.VRM, VR_SLOT), 0xFF, dtype=np.uint8)
    if lay.VRM and st.col.size:
        edge, none = st.vr_src >= 0, st.vr_src == -2
        src = np.where(edge, st.vr_src, 0)
        off = np.where(edge, 4 * (st.col[src] - base), 0).astype(np.uint16)
        wt = np.where(edge, wbits[src], 0).astype(np.uint32)
        off[none], wt[none] = 0xFFFF, 0xFFFFFFFF
        vr[:, :, :2 * VS] = off.view(np.uint8).reshape(m, lay.VRM, 2 * VS)
        vr[:, :, 2 * VS:] = wt.view(np.uint8).reshape(m, lay.VRM, 4 * VS)
    eps = st.eps_ref.astype(f32) if st.auto else ep
    return Out(rs.astype(np.int32), st.row_len.astype(np.int32), col, ws, d2s, deg,
               st.ucnt.astype(np.int32), deg[base:] + f32(st.tau), rhs, st.P_lab.copy(),
               np.zeros((base, C), dtype=f32), ell, vr.ravel(), eps,
               int((~(eps >= f32(1e-10))).any()))


# ------------------------------------------------------------------------------------------
# Which instantiation a launch runs: rows.hip launch_finalize, restated.
# ------------------------------------------------------------------------------------------
TY = {"f32": "f", "f64": "d", "i64": "l"}       # as the mangled stub names spell the label type


def route(K, B, y_dtype, knob_pre=0):
    """(TY, PRE, FLAT, FH) of row_build_kernel for a launch over B graphs; K already clamped."""
    fh = 4 if K - 1 > 2 * WAVE else 2 if K - 1 > WAVE else 1
    if fh > 1:
        pre = B == 1                                    # GLL_ROWS_FH: the knob is not consulted
    else:
        pre = knob_pre == 1 or (knob_pre == 0 and B == 1)
    flat = not pre and B > 1
    return TY[y_dtype], int(pre), int(flat), fh


# ------------------------------------------------------------------------------------------
# Per-row regimes, from the counts the kernel branches on
# ------------------------------------------------------------------------------------------
REQUIRED = frozenset({
    "slot+lds", "slot+global", "bump+lds+ovf", "bump+lds+noovf", "bump+global+ovf",
    "bump+global+noovf", "ovf>512", "ovf_other_rows", "rev_pass2",
    "pre_short", "pre_hub", "pre_hub_nlab>32", "acc1", "acc2", "acc3", "acc4",
    "nlab0", "nlab1", "nlab15", "nlab16", "nlab17", "nlab33", "ucnt0", "empty_row", "eps0",
    "ell24", "ell16", "ell4", "ell0", "ell_longer", "ell_shorter",
    "vr", "vr_pad", "vr_off_max", "vrm63", "vr_clamp", "complete", "fh2", "fh4",
})


def regimes(st: Stage, case):
    """The tags of REQUIRED (and a few more) that some row of this graph reaches."""
    lay = st.lay
    lb = st.nf + st.rc
    slot, lds, ovf = lb <= lay.Wcap, lb <= K_STAGE, st.rc > lay.RCAP
    out = set()
    for name, mask in (("slot+lds", slot & lds), ("slot+global", slot & ~lds),
                       ("bump+lds+ovf", ~slot & lds & ovf), ("bump+lds+noovf", ~slot & lds & ~ovf),
                       ("bump+global+ovf", ~slot & ~lds & ovf),
                       ("bump+global+noovf", ~slot & ~lds & ~ovf)):
        if mask.any():
            out.add(name)
    novf = int(np.maximum(st.rc - lay.RCAP, 0).sum())
    if novf > OVF_STEP:
        out.add("ovf>512")
    if ovf.sum() >= 2:
        out.add("ovf_other_rows")
    if (np.minimum(st.rc, lay.RCAP) > WAVE).any():
        out.add("rev_pass2")
    ty, pre, flat, fh = route(lay.K, case.B, case.y_dtype, case.knob_pre)
    out.add(f"fh{fh}")
    un = np.arange(lay.n) >= lay.base
    L = st.row_len
    if lay.m and lay.base:
        if pre and st.C <= 16:
            if (un & lds & (L <= WAVE) & (st.nlab > 0)).any():
                out.add("pre_short")
            if (un & lds & (L > WAVE) & (st.nlab > 0)).any():
                out.add("pre_hub")
            if (un & lds & (L > WAVE) & (st.nlab > 32)).any():
                out.add("pre_hub_nlab>32")
            if (un & ~lds & (st.nlab > 0)).any():
                out.add("acc1")
        elif (un & (st.nlab > 0)).any():
            out.add(f"acc{(st.C + WAVE - 1) // WAVE}")
        for v in (0, 1, 15, 16, 17, 33):
            if (un & (L > 0) & (st.nlab == v)).any():
                out.add(f"nlab{v}")
        if (st.ucnt[L[lay.base:] > 0] == 0).any():
            out.add("ucnt0")
    if (L == 0).any():
        out.add("empty_row")
    if st.auto and (st.eps_in == 0).any() and (st.eps_in[st.row] * st.eps_in[st.col] == 0).any():
        out.add("eps0")
    if lay.m:
        out.add(f"ell{lay.SE}")
        if lay.SE and (st.ucnt > lay.SE).any():
            out.add("ell_longer")
        if lay.SE and ((st.ucnt < lay.SE) & (st.ucnt > 0)).any():
            out.add("ell_shorter")
    if lay.VRM:
        out.add("vr")
        if (st.ucnt % VS != 0).any():
            out.add("vr_pad")
        edge = st.vr_src >= 0
        if edge.any() and (st.col[st.vr_src[edge]] - lay.base).max() == 2047:
            out.add("vr_off_max")
        if lay.VRM == 63:
            out.add("vrm63")
        if ((st.ucnt + VS - 1) // VS > lay.VRM).any():
            out.add("vr_clamp")
    if (L == lay.n - 1).all():
        out.add("complete")
    return out


# ------------------------------------------------------------------------------------------
# The shapes of the GPU test
# ------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    n: int
    base: int
    C: int = 3
    K: int = 10
    eps: object = 1.0            # a float, or 'auto'
    B: int = 1
    y_dtype: str = "f32"
    knob_pre: int = 0            # GLL_KNOB_ROW_PRE
    flags: int = 0
    feat: str = "gauss"          # gauss | hub | dups | lattice | nonfinite
    hubs: tuple = ()             # hub rows (feat hub): the first at the origin, the next beside it
    far: int = 0                 # trailing rows moved to a far cluster (they list only each other)
    graph_api: bool = False      # base = 0 through gll_graph
    expect: tuple = ()           # tags of REQUIRED this case is there for
    seed: int = 0

    @property
    def m(self):
        return self.n - self.base

    @property
    def auto(self):
        return isinstance(self.eps, str)

    def layout(self):
        return layout(self.n, self.base, self.K, self.flags)

    def route(self):
        return route(min(self.K, self.n), self.B, self.y_dtype, self.knob_pre)


def _inst_cases():
    """Every instantiation: label type x the eight settings of (K, B, knob) below.  n = 130 leaves
    a ragged last block of four rows; C walks through the class-per-lane forms."""
    out = []
    settings = (("K10_B1", 130, 10, 1, 0, 16), ("K10_B1_pre_off", 130, 10, 1, 2, 17),
                ("K10_B3", 130, 10, 3, 0, 65), ("K10_B3_pre_on", 130, 10, 3, 1, 1),
                ("K66_B1", 150, 66, 1, 0, 129), ("K66_B2", 150, 66, 2, 0, 64),
                ("K130_B1", 300, 130, 1, 0, 256), ("K130_B2", 300, 130, 2, 0, 10))
    for t, y in enumerate(("f32", "f64", "i64")):
        for s, (tag, n, K, B, knob, C) in enumerate(settings):
            out.append(Case(f"inst_{y}_{tag}", n, 60, C=C, K=K, eps=("auto" if (s + t) % 2 else 1.0),
                            B=B, y_dtype=y, knob_pre=knob, seed=10 * t + s))
    out.append(Case("inst_K257", 300, 60, C=3, K=257, eps="auto", seed=41, expect=("fh4",)))
    out.append(Case("kclamp_complete", 12, 4, C=3, K=25, eps="auto", seed=42, expect=("complete",)))
    return out


def _regime_cases():
    V = FLAG_CG_VR
    return [
        # staging: unit-sphere rows plus hubs at the origin; `far` rows never list a hub
        Case("stage_bump_lds_ovf", 150, 50, C=10, K=6, hubs=(50, 3), feat="hub", seed=1,
             expect=("bump+lds+ovf", "ovf_other_rows", "pre_hub", "pre_hub_nlab>32")),
        Case("stage_bump_lds_noovf", 150, 20, C=10, K=6, hubs=(20,), far=109, feat="hub", seed=2,
             expect=("bump+lds+noovf",)),
        # (K = 25, not 10: of 700 random unit rows in 16 dimensions about 13 lie closer to a row
        # than the origin does, so the hub is in nearly every list only when K - 1 is well past 13)
        Case("stage_global_bump_ovf", 700, 100, C=10, K=25, hubs=(100, 5), feat="hub", seed=3,
             eps="auto", expect=("bump+global+ovf", "ovf>512", "ovf_other_rows", "rev_pass2")),
        Case("stage_global_bump_noovf", 277, 60, C=10, K=30, hubs=(60,), far=40, feat="hub",
             seed=4, expect=("bump+global+noovf", "rev_pass2")),
        Case("stage_global_slot", 270, 60, C=10, K=52, hubs=(60,), far=60, feat="hub", seed=5,
             eps="auto", expect=("slot+global", "rev_pass2")),
        # right-hand side: labeled-neighbour counts 0, 1, 15, 16, 17, 33 (complete graphs: every
        # unlabeled row has exactly `base` of them), all / none labeled, base = 0 and n - 1
        *[Case(f"rhs_complete_base{b}", n, b, C=5, K=64, y_dtype=y, seed=50 + b,
               expect=(f"nlab{b}", "complete", "pre_short"))
          for b, n, y in ((1, 24, "f32"), (15, 24, "f64"), (16, 24, "i64"), (17, 24, "f32"),
                          (33, 40, "f64"))],
        Case("rhs_all_or_none_labeled", 130, 100, C=7, K=10, far=29, seed=6, eps="auto",
             expect=("ucnt0", "nlab0")),
        Case("rhs_base0_graph", 130, 0, C=1, K=10, graph_api=True, seed=7, eps="auto"),
        Case("rhs_base_n_minus_1", 130, 129, C=3, K=10, seed=8),
        # ELL widths 24 / 16 / 4 / 0; a hub in the U block of the first: a suffix longer than SE
        Case("ell_m500", 520, 20, K=10, hubs=(20,), feat="hub", seed=9,
             expect=("ell24", "ell_longer", "ell_shorter")),
        Case("ell_m513", 533, 20, K=10, seed=10, eps="auto", expect=("ell16", "ell_shorter")),
        Case("ell_m2049", 2069, 20, K=10, seed=11, expect=("ell4", "ell_longer")),
        Case("ell_m4097", 4117, 20, K=10, seed=12, eps="auto", expect=("ell0",)),
        # virtual rows: automatic (25 + 125 at K = 25), forced at m = 2048 (offset 4 * 2047), the
        # 63-slot clamp (K = 130), a hub in the U block longer than 8 VRM
        Case("vr_fullysup_like", 150, 25, C=10, K=25, seed=13, expect=("vr", "vr_pad")),
        Case("vr_m2048", 2068, 20, K=10, flags=V, seed=14, eps="auto", expect=("vr", "vr_off_max")),
        Case("vr_K130_clamp", 300, 60, C=10, K=130, seed=15, expect=("vr", "vrm63", "fh4")),
        Case("vr_hub_past_vrm", 150, 20, C=10, K=10, hubs=(20,), feat="hub", flags=V, seed=16,
             expect=("vr", "vr_clamp")),
        # dropped edges: duplicate clusters larger and smaller than K, fixed and auto eps
        Case("dups_fixed", 130, 40, C=10, K=10, feat="dups", seed=17, expect=("empty_row",)),
        Case("dups_auto", 130, 40, C=10, K=10, feat="dups", eps="auto", seed=17,
             expect=("empty_row", "eps0")),
        Case("nonfinite_in_batch", 130, 40, C=10, K=10, B=3, feat="nonfinite", seed=18),
        # near-ties: the select's float64 refinement is likely, the two directions may differ
        Case("lattice_ties", 200, 40, C=10, K=10, feat="lattice", eps="auto", seed=19),
    ]


ALL_CASES = (*_inst_cases(), *_regime_cases())
CASES = {c.name: c for c in ALL_CASES}
assert len(CASES) == len(ALL_CASES)


def features(case: Case, g: int = 0):
    """X (n x 16 float32) of graph g of a case."""
    n = case.n
    rng = np.random.default_rng(1000 * case.seed + g)
    X = rng.standard_normal((n, D)).astype(np.float32)
    if case.feat == "hub":
        X /= np.linalg.norm(X, axis=1, keepdims=True)      # pairwise distances ~ sqrt(2)
        for q, h in enumerate(case.hubs):
            X[h] = 0.0                                     # distance ~1 to every unit row
            X[h, 1] = 0.05 * q
    elif case.feat == "lattice":
        # lattice points a hair off the lattice: squared distances tie to ~1e-6 relative, where
        # the select re-ranks a row in float64 (and then stores the rounded float64 d2)
        X = (rng.integers(0, 3, size=(n, D)) + 1e-6 * rng.standard_normal((n, D))).astype(np.float32)
    if case.far:
        X[n - case.far:, 0] += 10.0
    if case.feat == "dups":
        X[41:53] = X[40]            # 13 copies > K among ordinary rows: eps_i = 0 ('auto'),
        X[5:7] = X[4]               # their edges come from the rows that list them; 3 copies < K
        X[118:130] = X[117] + 10.0  # 12 copies far from everything: rows without an entry
    elif case.feat == "nonfinite" and g == 1:
        X[7] = np.nan
    return X


def labels(case: Case, g: int = 0):
    """Y (base x C) of graph g in the case's dtype: soft rows (Dirichlet) with a few negative
    entries for f32 / f64, values from {-2, 0, 1, 3} for i64."""
    rng = np.random.default_rng(77 + 1000 * case.seed + g)
    if case.y_dtype == "i64":
        return rng.choice(np.array([-2, 0, 0, 1, 3], dtype=np.int64), size=(case.base, case.C))
    Y = rng.dirichlet(np.full(case.C, 0.5), size=case.base) if case.C > 1 else \
        rng.random((case.base, 1))
    Y[rng.random(Y.shape) < 0.05] *= -1.0
    Y[rng.random(Y.shape) < 0.2] = 0.0
    return Y.astype(np.float32 if case.y_dtype == "f32" else np.float64)


def exact_knn(X, K):
    """(knn_idx n x K int32, knn_d2 n x K float32) as the select defines them, in float64: self
    first, then ascending exact squared distance (ties by index), d2 the correctly rounded
    difference form; a row with a non-finite feature -- and every entry naming one -- falls back
    to (self, 0)."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    K = min(K, n)
    idx = np.empty((n, K), dtype=np.int32)
    d2 = np.empty((n, K), dtype=np.float32)
    fin = np.isfinite(X).all(axis=1)
    for r0 in range(0, n, 128):
        blk = X[r0:r0 + 128]
        dd = ((blk[:, None, :] - X[None, :, :]) ** 2).sum(axis=2)
        dd[~np.isfinite(dd)] = np.inf
        dd[np.arange(blk.shape[0]), np.arange(r0, r0 + blk.shape[0])] = -1.0
        o = np.argsort(dd, axis=1, kind="stable")[:, :K]
        idx[r0:r0 + 128] = o
        d2[r0:r0 + 128] = np.take_along_axis(dd, o, axis=1)
    d2[:, 0] = 0.0
    dead = ~np.isfinite(d2) | ~fin[:, None]
    idx[dead] = np.broadcast_to(np.arange(n, dtype=np.int32)[:, None], idx.shape)[dead]
    d2[dead] = 0.0
    return idx, d2


def cpu_stage(case: Case, g: int = 0):
    """The stage reference of a case on float64 exact kNN lists of its features (no GPU)."""
    lay = case.layout()
    idx, d2 = exact_knn(features(case, g), lay.K)
    eps = np.sqrt(d2[:, lay.K - 1].astype(np.float64)).astype(np.float32)
    Y = labels(case, g) if case.base else np.zeros((0, case.C), dtype=np.float32)
    return rows_stage(idx, d2, eps, Y, TAU, case.base, lay.K, lay,
                      None if case.auto else np.float32(case.eps))
