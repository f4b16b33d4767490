"""Float64 closed form of the feature-gradient STAGE alone, with a derived elementwise error
bound -- a test helper, not a test (numpy only; never imported by the product).

The yardstick of tests/test_gpu_grad_stage.py (pinned on the CPU by tests/test_grad_ref_cpu.py).
The end-to-end bar (||a - b||_inf / ||b||_inf <= 1e-4 against the oracle) is dominated by the two
CG solves and by the largest element; here the solves are taken as given.  The inputs are the
arrays the gradient kernels themselves read, as they stand in fp32 in the workspace after a
backward (gll_workspace_view): row_start / row_len / col / w / d2 / eps / knn_idx, P = [Y; U32],
Wadj = [0; wadj], and X.  With (r, c) the directed edges e of the padded CSR:

    G_e    = sum_k (Wadj[r,k] - Wadj[c,k]) (P[c,k] - P[r,k])      Gabs_e = sum_k |..| |..|
    V_e    = -8 w_e / (eps_r eps_c)                                Sabs_e = Gabs_e |V_e|
    coef_e = S_e = G_e V_e                                         (fixed eps)
    b_i    = sum_{e in row i} S_e d2_e / (2 eps_i^2)               Babs_i: the same with Sabs
    coef_e = S_e - b_r [c = kth(r)] - b_c [kth(c) = r]             (auto eps; kth = knn_idx[:, K-1])
    cabs_e = Sabs_e + Babs_r [c = kth(r)] + Babs_c [kth(c) = r]
    grad[i,k]  = sum_{e in row i} coef_e (X[i,k] - X[c,k])
    A[i,k]     = sum_{e in row i} cabs_e |X[i,k] - X[c,k]|
    bound[i,k] = 2 u (C + 12 + Lmax_i) A[i,k],      u = 2^-24,
    Lmax_i     = max(L_i, max_{j in N(i)} L_j),     L = row_len

The pass condition is |gpu - grad| <= bound on EVERY element; where bound == 0 the GPU value must
be exactly 0 (check()).

Derivation of the bound (first order in u; every kernel form evaluates these expressions, in fp32,
with one rounding per operation; the forms differ only in the order of the sums, which the count
does not depend on).  Each term coef_e dx_e of grad[i,k] carries, relative to cabs_e |dx_e|:
    1        dx = fl(x_i - x_c)
    2        the two differences fl(w_r - w_c), fl(p_c - p_r) inside a term of G
    C        the fma chain of G (one rounding per class)
    3        V = -8 w / fl(eps_r eps_c): the product, the division (8 w is exact); S = fl(G V)
    L_j      [auto] the fma accumulation of b_j = sum S d2 over row j of length L_j, j = r or c
             (partial sums per lane and a shuffle tree: adding an empty partial is exact, so no
             path through the tree rounds more than L_j times)
    3        [auto] b's scale: fl(eps eps), 2 x (exact), the division   (2 counted would do)
    2        [auto] the two subtractions S - b_r - b_c
    L_i      the fma accumulation of row i's sum over its L_i edges
so at most N1 = C + 11 + L_i + Lmax_i roundings, |error| <= N1 u A[i,k] to first order.  The bound
takes 2 (C + 12 + Lmax_i) >= N1 + (C + 13): the factor 2 turns the sum L_i + Lmax_i of the two
accumulations into one maximum and leaves (C + 13) u A for the second-order terms, which are at
most N1^2 u^2 A / (1 - N1 u) -- covered while N1^2 u <= C + 13, i.e. rows shorter than ~7,000
edges (the longest row of any test here has 199).  Fixed eps has no b terms; the same bound is
used (it is only looser there).  Underflow is not modelled: the tests' weights stay above 1e-7.
The constant is derived, not measured; tests/test_grad_ref_cpu.py evaluates the same formulas in
numpy float32 with the edges of each row in a random order and records how much of the bound that
uses (0.004-0.08: 13 x slack or more, while the bound still sits below 2e-5 of max|grad| on
ordinary rows, against the suite's 1e-4).

`route` restates the host-side choice of the backward (api.hip backward_impl, fused_bwd.hip
launch_cg_grad_fused, grad.hip launch_backward_grad / grad_use_chunks / grad_nd / grad_chunked) in
the style of cg_ref.route: which kernel instantiations run and how many launches of each
(GLL_K_EDGE, GLL_K_GRAD, GLL_K_BWD, GLL_K_CG) a backward makes.  The one gate it cannot restate is
run_fused's co-residency test (resident blocks x CUs >= workgroups), which asks the device:
`route` takes the fused branch as reached, and the GPU test's GLL_K_BWD == 1 is the check that
it was.  CASES holds the shapes of the GPU test; tests/test_grad_ref_cpu.py checks that they reach
every gradient-kernel instantiation libgll.so holds.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from tests import cg_ref

U = 2.0 ** -24       # unit roundoff of fp32


# ------------------------------------------------------------------------------------------
# The closed form
# ------------------------------------------------------------------------------------------
def edge_list(row_start, row_len):
    """(r, e): row of every stored edge in row order, and its position in col / w / d2."""
    rl = np.asarray(row_len, dtype=np.int64)
    rs = np.asarray(row_start, dtype=np.int64)
    r = np.repeat(np.arange(rl.shape[0], dtype=np.int64), rl)
    first = np.cumsum(rl) - rl
    e = np.repeat(rs - first, rl) + np.arange(int(rl.sum()), dtype=np.int64)
    return r, e


def _row_sums(T, row_len):
    """Sum the rows of T (E x d, edges in row order) per graph row: n x d."""
    rl = np.asarray(row_len, dtype=np.int64)
    out = np.zeros((rl.shape[0],) + T.shape[1:], dtype=T.dtype)
    live = rl > 0
    if T.shape[0]:
        out[live] = np.add.reduceat(T, (np.cumsum(rl) - rl)[live], axis=0)
    return out


@dataclass
class Stage:
    grad: np.ndarray     # n x d float64
    bound: np.ndarray    # n x d float64
    A: np.ndarray        # n x d: sum |coef| |dx|
    coef: np.ndarray     # per edge, row order
    b: np.ndarray        # per row (auto), else None
    Lmax: np.ndarray     # n


def grad_stage(row_start, row_len, col, w, d2, eps, knn_idx, P, Wadj, X, auto, eps_fixed=None):
    """The closed form above in float64.  `knn_idx`: n x K lists, or the n kth neighbours;
    `eps`: per-row values (auto) -- with fixed eps `eps_fixed` is used for every row."""
    f = np.float64
    r, e = edge_list(row_start, row_len)
    c = np.asarray(col)[e].astype(np.int64)
    we = np.asarray(w)[e].astype(f)
    P, Wadj, X = (np.asarray(a, dtype=f) for a in (P, Wadj, X))
    n, C = P.shape
    assert Wadj.shape == (n, C) and X.shape[0] == n
    assert c.size == 0 or (c.min() >= 0 and c.max() < n)
    ep = np.asarray(eps, dtype=f) if auto else np.full(n, f(eps_fixed))
    dw, dp = Wadj[r] - Wadj[c], P[c] - P[r]
    G = np.sum(dw * dp, axis=1)
    Gabs = np.sum(np.abs(dw) * np.abs(dp), axis=1)
    V = -8.0 * we / (ep[r] * ep[c])
    S, Sabs = G * V, Gabs * np.abs(V)
    coef, cabs, b = S.copy(), Sabs.copy(), None
    if auto:
        kth = np.asarray(knn_idx, dtype=np.int64)
        kth = kth[:, -1] if kth.ndim == 2 else kth
        d2e = np.asarray(d2)[e].astype(f)
        scale = 2.0 * ep * ep
        b = np.bincount(r, weights=S * d2e, minlength=n) / scale
        Babs = np.bincount(r, weights=Sabs * d2e, minlength=n) / scale
        hr, hc = c == kth[r], kth[c] == r
        coef -= np.where(hr, b[r], 0.0) + np.where(hc, b[c], 0.0)
        cabs += np.where(hr, Babs[r], 0.0) + np.where(hc, Babs[c], 0.0)
    dx = X[r] - X[c]
    grad = _row_sums(coef[:, None] * dx, row_len)
    A = _row_sums(cabs[:, None] * np.abs(dx), row_len)
    L = np.asarray(row_len, dtype=np.int64)
    Lmax = L.copy()
    np.maximum.at(Lmax, r, L[c])
    bound = 2.0 * U * (C + 12 + Lmax)[:, None] * A
    return Stage(grad, bound, A, coef, b, Lmax)


def grad_stage_f32(row_start, row_len, col, w, d2, eps, knn_idx, P, Wadj, X, auto, eps_fixed=None,
                   rng=None):
    """The same formulas in float32, one rounding per operation (fmas as the kernels issue them:
    the exact float64 product of two fp32 numbers plus the addend, rounded to fp32), the edges of
    every row summed in a random order: n x d float32."""
    f, f64 = np.float32, np.float64
    rng = np.random.default_rng(0) if rng is None else rng

    def fma(a, b, c):
        return (np.asarray(a, dtype=f64) * np.asarray(b, dtype=f64) + np.asarray(c, dtype=f64)).astype(f)

    r, e = edge_list(row_start, row_len)
    c = np.asarray(col)[e].astype(np.int64)
    we = np.asarray(w)[e].astype(f)
    P, Wadj, X = (np.asarray(a, dtype=f) for a in (P, Wadj, X))
    n, C = P.shape
    ep = np.asarray(eps, dtype=f) if auto else np.full(n, f(eps_fixed), dtype=f)
    dw, dp = Wadj[r] - Wadj[c], P[c] - P[r]
    g = np.zeros(r.shape[0], dtype=f)
    for k in range(C):
        g = fma(dw[:, k], dp[:, k], g)
    S = g * (f(-8.0) * we / (ep[r] * ep[c]))
    rl = np.asarray(row_len, dtype=np.int64)
    first = np.cumsum(rl) - rl
    orders = [first[i] + rng.permutation(int(rl[i])) for i in range(n)]
    coef = S.copy()
    if auto:
        kth = np.asarray(knn_idx, dtype=np.int64)
        kth = kth[:, -1] if kth.ndim == 2 else kth
        d2e = np.asarray(d2)[e].astype(f)
        b = np.zeros(n, dtype=f)
        for i in range(n):
            bp = f(0.0)
            for q in orders[i]:
                bp = fma(S[q], d2e[q], bp)
            b[i] = bp / (f(2.0) * ep[i] * ep[i])
        hr, hc = c == kth[r], kth[c] == r
        coef = np.where(hr, coef - b[r], coef).astype(f)
        coef = np.where(hc, coef - b[c], coef).astype(f)
    out = np.zeros(X.shape, dtype=f)
    for i in range(n):
        acc = np.zeros(X.shape[1], dtype=f)
        for q in orders[i]:
            acc = fma(coef[q], X[i] - X[c[q]], acc)
        out[i] = acc
    return out


def check(gx, st: Stage):
    """(worst err / bound, worst err / max|grad|) of a GPU result against a Stage; asserts that
    every element is finite and within its bound, and exactly 0 where the bound is 0."""
    gx = np.asarray(gx)
    assert gx.shape == st.grad.shape, (gx.shape, st.grad.shape)
    assert np.isfinite(gx).all(), f"{int((~np.isfinite(gx)).sum())} non-finite elements"
    err = np.abs(gx.astype(np.float64) - st.grad)
    zero = st.bound == 0
    assert not gx[zero].any(), "non-zero output where the bound is 0"
    ratio = np.where(zero, 0.0, err / np.where(zero, 1.0, st.bound))
    worst = float(ratio.max(initial=0.0))
    if worst > 1.0:
        i, k = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        raise AssertionError(f"err/bound {worst:.3f} at [{i},{k}]: gpu {gx[i, k]!r}, float64 "
                             f"{st.grad[i, k]!r}, bound {st.bound[i, k]:.3e}, "
                             f"{int((ratio > 1).sum())} elements past the bound")
    gmax = float(np.abs(st.grad).max(initial=0.0))
    return worst, float(err.max(initial=0.0) / gmax) if gmax > 0 else 0.0


# ------------------------------------------------------------------------------------------
# Which kernels a backward runs: the host-side choice of the library, restated.
# ------------------------------------------------------------------------------------------
FLAG_CG_GRID, FLAG_GRAD_ROWS, FLAG_GRAD_CHUNK, FLAG_BWD_UNFUSED = 1, 2048, 4096, 16384
FOUR_MB = 4 << 20


@dataclass(frozen=True)
class Route:
    counts: tuple          # launches of (GLL_K_EDGE, GLL_K_GRAD, GLL_K_BWD, GLL_K_CG)
    kernels: frozenset     # {(kernel, template arguments)} as libgll.so's stubs name them
    family: str            # 'fused' | 'chunk' | 'spmm'
    nch: int = 0           # grad_chunk: feature chunks


def edge_form(C, K):
    """launch_backward_grad's edge pass: (CV, LPR) of edge_coef_kernel."""
    if C % 2 == 0 and 2 <= C <= 16:
        cv = -C
    else:
        cv = 4 if C <= 4 else 8 if C <= 8 else 16 if C <= 16 else 0
    return cv, (16 if K <= 40 else 32)


def route(n, d, base, C, K, B, auto, x_aligned, flags=0, g_dtype="f64"):
    """The kernels of one gll_backward(_batched) call and their launch counts."""
    K = min(K, n)
    m = n - base
    vec = bool(x_aligned) and d % 4 == 0
    nd = (d + 255) // 256
    assert 1 <= nd <= 16
    fused = (B == 1 and not auto and C == 10 and vec and 1 <= m <= 512
             and cg_ref.vr_threads(n, m, K, flags) == 0           # L.RV != 0
             and (24 if m <= 512 else 16) == 24                   # ell_emit(L, 1) != 24
             and d <= 1024
             and not flags & (FLAG_BWD_UNFUSED | FLAG_CG_GRID | FLAG_GRAD_CHUNK)
             and n * d * 4 <= FOUR_MB)
    if fused:
        nt = 64 if m <= 64 else 128 if m <= 128 else 256 if m <= 256 else 512
        ndf = 1 if nd <= 1 else 2 if nd <= 2 else 4
        tb = {"f32": "f", "f64": "d"}[g_dtype]
        return Route((0, 0, 1, 0), frozenset({("cg_grad_fused_kernel", (nt, 24, tb, ndf))}), "fused")
    chunk = (vec and d >= 128 and not flags & FLAG_GRAD_ROWS
             and bool(flags & FLAG_GRAD_CHUNK or (B > 1 and d < 256) or n * d * 4 > FOUR_MB))
    ks = set()
    edge = auto or chunk
    if edge:
        ks.add(("edge_coef_kernel", edge_form(C, K)))
    nch = 0
    if chunk:
        lpr = 16
        while lpr < 64 and 4 * lpr * 8 < d:
            lpr *= 2
        nch = (d + 4 * lpr - 1) // (4 * lpr)
        ks.add(("grad_chunk_kernel", (1 if auto else 2, lpr)))
    else:
        ndk = next(v for v in (1, 2, 4, 8, 16) if nd <= v)
        cv = -10 if (not auto and C == 10) else 0
        ks.add(("grad_spmm_kernel", (int(auto), ndk, int(vec), int(B == 1 and ndk <= 4), cv)))
    return Route((int(edge), 1, 0, int(m > 0)), frozenset(ks), "chunk" if chunk else "spmm", nch)


# ------------------------------------------------------------------------------------------
# The shapes of the GPU test: the smallest that reach every instantiation, every residue the
# fused kernel's workgroup rank depends on, and the hub / duplicate / clamped-K rows.
# ------------------------------------------------------------------------------------------
TAU = 0.07


@dataclass(frozen=True)
class Case:
    name: str
    group: str             # the record's family: edge | spmm | chunk | fused
    base: int
    m: int
    d: int
    C: int = 10
    K: int = 5
    eps: object = 1.0      # a float, or 'auto'
    B: int = 1
    flags: int = 0
    aligned: bool = True   # False: X starts 4 bytes past a 16-B boundary
    g_dtypes: tuple = ("f64",)     # one backward per entry, all on one workspace
    feat: str = "synth"    # synth | hub | dups | one_class
    seed: int = 0

    @property
    def n(self):
        return self.base + self.m

    @property
    def auto(self):
        return isinstance(self.eps, str)

    def route(self, g_dtype=None):
        return route(self.n, self.d, self.base, self.C, self.K, self.B, self.auto, self.aligned,
                     self.flags, g_dtype or self.g_dtypes[0])

    def kernels(self):
        return frozenset().union(*[self.route(g).kernels for g in self.g_dtypes])


def _edge_cases():
    out = []
    for C in (*range(1, 19), 33):          # every exact form, every bound with C below it, the loop
        for K in (6, 42):                  # 16 and 32 lanes per row
            for B in (1, 3):
                out.append(Case(f"edge_auto_C{C}_K{K}_B{B}", "edge", 40, 90, 12, C=C, K=K,
                                eps="auto", B=B, seed=C))
    for C in (5, 10):                      # the fixed-eps edge pass of the chunked gradient
        out.append(Case(f"edge_fixed_C{C}", "edge", 40, 90, 132, C=C, K=6, flags=FLAG_GRAD_CHUNK,
                        seed=40 + C))
    return out


SPMM_D = {1: (1, 3, 37, 252, 256), 2: (257, 260, 512), 4: (516, 1023, 1024), 8: (1028, 2048),
          16: (2052, 4093, 4096)}
SPMM_COEF = {"auto": ("auto", 10), "fixed10": (1.0, 10), "fixed7": (1.0, 7)}


def _spmm_case(coef, d, B, aligned):
    eps, C = SPMM_COEF[coef]
    flags = FLAG_BWD_UNFUSED if coef == "fixed10" else 0
    if B > 1 and aligned and d % 4 == 0 and 128 <= d < 256:
        flags |= FLAG_GRAD_ROWS            # a batch of narrow graphs would take the chunks
    tag = f"spmm_{coef}_d{d}_B{B}" + ("" if aligned else "_off4")
    return Case(tag, "spmm", 24, 46, d, C=C, K=5, eps=eps, B=B, flags=flags, aligned=aligned,
                seed=d % 97)


def _spmm_cases():
    out = []
    for coef in SPMM_COEF:
        for nd, ds in SPMM_D.items():
            for d in ds:
                for B in ((1, 2) if nd <= 4 else (1,)):      # WIDE on / off; ND 8, 16 have one form
                    out.append(_spmm_case(coef, d, B, True))
                    if d % 256 == 0:                         # VEC off by the pointer, not by d
                        out.append(_spmm_case(coef, d, B, False))
        out.append(_spmm_case(coef, 2048, 2, True))          # graph strides at ND 8
    return out


def _chunk_cases():
    out = []
    for eps in (1.0, "auto"):
        for d in (128, 132, 512, 520, 1024, 1028):           # LPR 16 16 16 32 32 64; 132, 520 and
            for base, m in ((24, 46), (40, 91)):             # 1028 leave a ragged last chunk
                out.append(Case(f"chunk_{'auto' if eps == 'auto' else 'fixed'}_d{d}_n{base + m}",
                                "chunk", base, m, d, K=5, eps=eps, flags=FLAG_GRAD_CHUNK,
                                seed=d % 89))
        out.append(Case(f"chunk_{'auto' if eps == 'auto' else 'fixed'}_d132_B2_automatic", "chunk",
                        24, 46, 132, K=5, eps=eps, B=2, seed=7))
    return out


FUSED_M = {64: (1, 64), 128: (65, 128), 256: (129, 256), 512: (257, 512)}
FUSED_G0 = {64: 97, 128: 96, 256: 120, 512: 160}    # first of eight gradient-workgroup counts
FUSED_3 = ("f32", "f64", "f32")                     # three backwards on one workspace


def fused_ns(nt):
    """Eight n whose gradient-workgroup count ceil(n / NW), NW = NT / 64, takes every residue
    mod 8, with n % 64 != 0 and, for NW > 1, every non-zero n % NW in turn; 10 + count <= 256."""
    nw = nt // 64
    out = []
    for q in range(8):
        g = FUSED_G0[nt] + q
        n = nw * g - (q % (nw - 1) + 1 if nw > 1 else 0)
        assert (n + nw - 1) // nw == g and n % 64 != 0 and 10 + g <= 256 and (nw == 1 or n % nw)
        out.append(n)
    return out


def _fused_cases():
    out = []
    for nt, ms in FUSED_M.items():
        for m in ms:
            for n in fused_ns(nt):
                out.append(Case(f"fused_NT{nt}_m{m}_n{n}", "fused", n - m, m, 8, K=6,
                                g_dtypes=FUSED_3, seed=n))
        n = fused_ns(nt)[3]
        out.append(Case(f"fused_NT{nt}_ND2", "fused", n - ms[1], ms[1], 260, K=6, g_dtypes=FUSED_3,
                        seed=nt))
        n = min(n, 1021)                   # n d 4 <= 4 MB at d = 1024
        out.append(Case(f"fused_NT{nt}_ND4", "fused", n - ms[1], ms[1], 1024, K=6,
                        g_dtypes=FUSED_3, seed=nt + 1))
    out.append(Case("fused_hub", "fused", 50, 100, 64, K=6, g_dtypes=FUSED_3, feat="hub", seed=1))
    out.append(Case("fused_one_class", "fused", 60, 75, 8, K=6, g_dtypes=FUSED_3,
                    feat="one_class", seed=2))
    return out


def _edge_row_cases():
    """Hubs (row 0 is everybody's neighbour: > 128 edges), clusters of exact duplicates (their
    zero-distance pairs are dropped: empty rows) and K >= n (clamped: the complete graph), in
    every family.  The duplicates keep to fixed eps, except a cluster smaller than K (auto eps of
    a row whose K nearest coincide with it would be 0)."""
    U, CH = FLAG_BWD_UNFUSED, FLAG_GRAD_CHUNK
    hub = dict(base=50, m=100, K=6, feat="hub", seed=1)
    dup = dict(base=40, m=91, K=6, feat="dups", seed=3)
    return [
        Case("hub_spmm_fixed", "spmm", d=64, flags=U, **hub),
        Case("hub_spmm_auto", "spmm", d=64, eps="auto", **hub),         # edge pass, 16 lanes
        Case("hub_spmm_auto_d37", "spmm", d=37, eps="auto", **hub),
        Case("hub_chunk_fixed", "chunk", d=128, flags=CH, **hub),
        Case("hub_chunk_auto", "chunk", d=128, eps="auto", flags=CH, **hub),
        Case("hub_edge_32_lanes", "edge", d=64, eps="auto", C=7, **{**hub, "K": 42}),
        Case("dups_spmm_fixed", "spmm", d=40, flags=U, **dup),
        Case("dups_chunk_fixed", "chunk", d=128, flags=CH, **dup),
        Case("dups_fused", "fused", d=40, g_dtypes=FUSED_3, **dup),
        Case("dups_small_cluster_auto", "edge", d=40, eps="auto", **{**dup, "feat": "dups3"}),
        Case("kclamp_auto", "edge", 10, 40, 12, K=64, eps="auto", seed=5),
        Case("kclamp_spmm_fixed", "spmm", 10, 40, 12, K=64, flags=U, seed=5),
        Case("kclamp_chunk_auto", "chunk", 10, 40, 128, K=64, eps="auto", flags=CH, seed=5),
        Case("kclamp_fixed_unflagged", "spmm", 10, 40, 12, K=64, g_dtypes=("f32", "f64"), seed=5),
    ]


ALL_CASES = (*_edge_cases(), *_spmm_cases(), *_chunk_cases(), *_fused_cases(), *_edge_row_cases())
CASES = {c.name: c for c in ALL_CASES}
assert len(CASES) == len(ALL_CASES)


def features(case: Case, g: int = 0):
    """(X n x d float32, Y base x C float32 one-hot) of graph g of a case."""
    from graphlearninglayer_amd.synth import one_hot, synth
    n, seed = case.n, 1000 * case.seed + g
    if case.feat == "hub":
        rng = np.random.default_rng(seed)
        X = rng.standard_normal((n, case.d)).astype(np.float32)
        X /= np.linalg.norm(X, axis=1, keepdims=True)   # pairwise distances ~ sqrt(2)
        X[0] = 0.0                                      # distance 1 to every row: in every list
        lab = np.arange(n) % case.C
    elif case.d == 1:
        # unit rows of one feature are +-1: every pair at distance 0 (dropped) or 2, no graph.
        # Plain Gaussians instead, as test_odd_shapes takes them.
        X = np.random.default_rng(seed).standard_normal((n, 1)).astype(np.float32)
        lab = np.arange(n) % case.C
    else:
        X, lab = synth(case.base, case.m, case.d, C=case.C, latent=min(16, case.d), seed=seed)
    if case.feat == "dups":
        X[60:80] = X[59]        # 21 copies > K: rows with no edge of their own
        X[5:8] = X[4]           # duplicates among the labelled rows
    elif case.feat == "dups3":
        X[60:62] = X[59]        # 3 copies < K
        X[5:7] = X[4]
    if case.feat == "one_class":
        lab = np.zeros(n, dtype=np.int64)
    return X, one_hot(lab[: case.base], case.C)


def gbar(case: Case, g: int = 0):
    from graphlearninglayer_amd.synth import seeded_gbar
    return seeded_gbar(case.m, case.C, 77 + 1000 * case.seed + g)
