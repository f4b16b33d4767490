"""Float64 stage reference of the Gram (graphlearninglayer_amd/csrc/gram.hip): what every Gram
kernel is meant to compute, an elementwise bound on how far fp32 hardware may stray from it, the
contract the select builds its certificate on, the host's route restated, and the case table of
the GPU test (tests/test_gpu_gram_stage.py; tests/test_gram_ref_cpu.py runs this module on the CPU).
numpy throughout (the bf16 casts are integer arithmetic on the bits, held to torch's cast by the
CPU test).

Model (evaluated on the X the kernel reads, graph by graph):
    a = fl32(x - x_0), hi = bf16_rne(a), lo = bf16_rne(fl32(a - hi)), zero past d
    G_ij = sum_k (lo_ik hi_jk + hi_ik lo_jk + hi_ik hi_jk),  N_i = sum_k a_ik^2      in float64
    D2_model = N_i + N_j - 2 G_ij
The split-phase kernel (gram_bf3s) writes the same per feature phase of 256, one plane each, except
that a diagonal 64-tile puts both phases into plane 0 and zeros into plane 1.

bound(): |kernel - model| per element, counted from the code of each kernel family.  With
u = 2^-24 (fp32, round to nearest) and S_ij = sum_k (|lo hi| + |hi lo| + |hi hi|):
  * products of two bf16 values are exact in fp32 (8 x 8 significand bits);
  * ASSUMPTION (no installed document gives the rounding inside v_mfma_f32_32x32x16_bf16): one
    MFMA returns acc + sum_{k<16} a_k b_k with an error of at most
    KAPPA_M u (|acc| + sum |a_k b_k|), KAPPA_M = 32: at most 16 additions, each allowed a whole ulp (2 u relative: truncation rather
    than round-to-nearest), in any order.  A chain of T MFMAs into one accumulator is then within
    gamma(KAPPA_M T) S of the exact sum;
  * T, the chain per wave: 12 per 256-feature phase for gram_bf3 (a wave multiplies a quarter of
    each phase: 4 k-steps x 3), 12 for gram_bf3h, 24 for gram_bf3s (a diagonal tile runs both
    phases), 24 per 128-feature phase for gram_bf3w, 3 dp / 16 for gram_pk / gram_pk2;
  * the fixed-order sum of the KQ feature-group partials (4, 2, 4; none on the 128-/256-tiles):
    gamma(KQ - 1) S;
  * a norm is a sum of d squares through an addition tree of depth D (3 within a lane's four
    features, one per phase or loop trip into the running sum, then the DPP levels of the wave or
    half-wave sum; gram_bf3s adds its two phase norms on diagonal tiles): gamma(D + 1) N_i, fused
    multiply-adds only make it smaller;
  * the combine fl(fl(n_i + n_j) - 2 v): u (n_i + n_j) + u |result| <= 2 u (N_i + N_j + 2 S),
    evaluated on the perturbed operands (the factor 1 + 2^-10 below covers every second-order term).
Nothing here is tuned to a measurement.

contract(): what select.hip assumes (kGramErr, select.hip above knn_rescan):
    |D2 - d2_true| <= 2^-13 (|a_i| + |a_j|)^2,  d2_true = sum_k (x_ik - x_jk)^2 in float64,
and for fp16 storage t = fp16(v s): |t / s - v| <= 2^-11 |v| + 2^-25 / s with s = d2_scale(max N).
d2_true is evaluated as N_i + N_j - 2 <a_i, a_j> on float64 centred rows (relative error 1e-15 of
N, eleven orders below the contract).
"""
from __future__ import annotations

import contextlib
import dataclasses
from typing import NamedTuple

import numpy as np

U = 2.0 ** -24
KAPPA_M = 32.0                 # see ASSUMPTION above
K_GRAM_ERR = 2.0 ** -13        # select.hip kGramErr
RHO16, SIG16 = 2.0 ** -11, 2.0 ** -25   # fp16 contract: |t/s - v| <= RHO16 |v| + SIG16 / s
SLOP = 1.0 + 2.0 ** -10        # second-order terms of the first-order bound

FLAG_GRAM_INLINE, FLAG_KNN_PANEL, FLAG_D2_F32 = 8192, 65536, 131072
K_MAX_KM1 = 56                 # gll_internal.h kMaxKm1
BF3, BF3H, BF3S, BF3W, PK, PK2 = range(6)
FAMILY_NAMES = ("bf3", "bf3h", "bf3s", "bf3w", "pk", "pk2")
TILE = (64, 64, 64, 128, 128, 256)      # tile side of each family's main kernel
KQ = (4, 2, 4, 1, 1, 1)                 # feature-group partials summed per element


def blas_threads(n=4):
    """A few BLAS threads for the many small float64 products of the model: a pool as wide as the
    machine spends its time waking up (optional: without threadpoolctl nothing is limited)."""
    try:
        import threadpoolctl
    except ImportError:
        return contextlib.nullcontext()
    return threadpoolctl.threadpool_limits(n, user_api="blas")


def gamma(k):
    return k * U / (1.0 - k * U)


# ------------------------------------------------------------------------------------------
# route(): the host's choice restated (gll_internal.h, knn_route.h gram_route)
# ------------------------------------------------------------------------------------------
class Route(NamedTuple):
    family: int
    vec: int
    planes: int
    presplit: int
    H: int
    t256: int
    tail: int
    sub: int
    panels: int


def gram_splits(n, d):
    return 2 if ((n + 63) // 64 <= 16 and 256 < d <= 512) else 1


def panel_rows(n, flags):
    row_bytes = ((n + 3) & ~3) * 4
    pr = n
    if flags & FLAG_KNN_PANEL:
        pr = 1024
    elif n * row_bytes > (32 << 30):
        pr = (8 << 30) // row_bytes
    if pr >= n:
        return n
    pr = max((pr // 128) * 128, 128)
    return pr if pr < n else n


def d2_scale(M):
    """gram.hip d2_scale, bit for bit: 2^(14 - e) with fl32(4 M) = f 2^e, f in [0.5, 1)."""
    t = np.float32(4.0) * np.float32(M)
    if not (t > np.float32(1e-30)) or not (t < np.float32(1e38)):
        return np.float32(1.0)
    e = int(np.frexp(t)[1])
    return np.float32(np.ldexp(1.0, min(max(14 - e, -120), 120)))


def route_of(n, d, B, K, flags, tile, tail_knob, aligned, cus):
    K = min(K, n)
    vec = int(bool(aligned) and d % 4 == 0)
    PR = panel_rows(n, flags)
    KS = 1 if PR < n else gram_splits(n, d)
    planes = 2 if (KS == 2 and B == 1) else 1
    dp = (d + 63) & ~63
    if PR < n:
        return Route(BF3W, vec, planes, 0, 0, 0, 0, 0, (n + PR - 1) // PR)
    if planes == 2:
        return Route(BF3S, vec, 2, 0, 0, 0, 0, 0, 0)
    T, T2 = (n + 127) // 128, (n + 255) // 256
    presplit = (B * T * (T + 1) // 2 >= 256 and not (flags & FLAG_GRAM_INLINE) and
                (B > 1 or (d > 128 and n <= 12288)))
    if presplit:
        H = int(not (flags & FLAG_D2_F32) and B > 1 and K - 1 <= K_MAX_KM1)
        if tile > 0:
            t256 = tile == 256 and dp % 32 == 0
        elif dp % 32 or dp <= 128:
            t256 = False
        else:
            t1, t2 = B * T * (T + 1) // 2, B * T2 * (T2 + 1) // 2
            r1, r2 = (t1 + cus - 1) // cus, (t2 + cus - 1) // cus
            t256 = r2 * 2 * (dp // 32) * 32 < r1 * (dp // 64) * 64
        nt2 = B * T2 * (T2 + 1) // 2
        tail = nt2 % cus if (t256 and nt2 > cus) else 0
        sub = 16 if (tail_knob != 2 and tail * 16 <= 2 * cus) else 4
        if (sub == 4 and tail * 4 > cus) or tail_knob == 1:
            tail = 0
        return Route(PK2 if t256 else PK, vec, 1, 1, H, int(t256), tail, sub if tail else 0, 0)
    if B * T * (T + 1) // 2 >= 512:
        return Route(BF3W, vec, 1, 0, 0, 0, 0, 0, 0)
    return Route(BF3H if d <= 128 else BF3, vec, 1, 0, 0, 0, 0, 0, 0)


def kernels(rt):
    """{(kernel, template arguments)} a route launches."""
    if not rt.presplit:
        return {("gram_%s_kernel" % FAMILY_NAMES[rt.family], (rt.vec,))}
    ks = {("gram_split_kernel", (rt.vec,))}
    if rt.t256:
        ks.add(("gram_pk2_kernel", (rt.H,)))
        if rt.tail:
            ks.add(("gram_pk_kernel", (rt.H, 64 if rt.sub == 16 else 128)))
    else:
        ks.add(("gram_pk_kernel", (rt.H, 128)))
    return ks


# ------------------------------------------------------------------------------------------
# Cases
# ------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    fam: int                    # the family the case is there for (checked against the route)
    n: int
    d: int
    B: int = 1
    K: int = 10
    flags: int = 0
    tile: int = 0               # GLL_KNOB_GRAM_TILE
    tail: int = 0               # GLL_KNOB_GRAM_TAIL
    misalign: bool = False      # X 4 bytes off a 16-B boundary (VEC 0)
    feats: tuple = ("normal",)  # graph g takes feats[g % len(feats)]
    seed: int = 0

    def route(self, cus=256):
        return route_of(self.n, self.d, self.B, self.K, self.flags, self.tile, self.tail,
                        not self.misalign, cus)

    @property
    def dp(self):
        return (self.d + 63) & ~63

    def buffer_rows(self):
        """Graph row held by each row of the D2 buffer after the build.  Whole matrix: 0..n-1.
        Row panels: the last panel's rows, then what the panel before it left below them."""
        PR = panel_rows(self.n, self.flags)
        if PR >= self.n:
            return np.arange(self.n)
        r0 = ((self.n - 1) // PR) * PR
        rows = np.arange(PR) + (r0 - PR)
        rows[: self.n - r0] = np.arange(r0, self.n)
        return rows


def _mk():
    N, C, F, O, D = "normal", "coherent", "far", "offset", "dups"
    UP, DN, SAME = "scale_up", "scale_dn", "allsame"
    cs = [
        # gram_bf3h (d <= 128)
        Case("bf3h_3x2", BF3H, 3, 2),
        Case("bf3h_64x128", BF3H, 64, 128, feats=(F,)),
        Case("bf3h_65x100", BF3H, 65, 100, feats=(C,)),
        Case("bf3h_777x37", BF3H, 777, 37, feats=(D,)),
        Case("bf3h_200x128_off4", BF3H, 200, 128, misalign=True, feats=(O,)),
        Case("bf3h_B3_130x64", BF3H, 130, 64, B=3, feats=(N, C, SAME)),
        # gram_bf3
        Case("bf3_300x200", BF3, 300, 200, feats=(D,)),
        Case("bf3_130x132", BF3, 130, 132, feats=(C,)),
        Case("bf3_257x600", BF3, 257, 600, feats=(O,)),
        Case("bf3_100x1025", BF3, 100, 1025, feats=(F,)),
        Case("bf3_70x4096", BF3, 70, 4096),
        Case("bf3_B2_300x300", BF3, 300, 300, B=2, feats=(N, C)),
        Case("bf3_130x133_off4", BF3, 130, 133, misalign=True),
        # gram_bf3s (B = 1, n <= 1024, 256 < d <= 512)
        Case("bf3s_64x260", BF3S, 64, 260),
        Case("bf3s_65x257", BF3S, 65, 257, feats=(C,)),
        Case("bf3s_129x512", BF3S, 129, 512, feats=(F,)),
        Case("bf3s_1000x300", BF3S, 1000, 300, feats=(D,)),
        Case("bf3s_1024x512", BF3S, 1024, 512, feats=(O,)),
        Case("bf3s_130x258_off4", BF3S, 130, 258, misalign=True),
        # gram_bf3w
        Case("bf3w_4000x16", BF3W, 4000, 16, feats=(D,)),
        Case("bf3w_B86_300x64", BF3W, 300, 64, B=86, flags=FLAG_GRAM_INLINE,
             feats=(N, F, O, SAME)),
        Case("bf3w_panel_1200x100", BF3W, 1200, 100, flags=FLAG_KNN_PANEL, feats=(C,)),
        Case("bf3w_panel_2100x64", BF3W, 2100, 64, flags=FLAG_KNN_PANEL),
        Case("bf3w_panel_1200x37", BF3W, 1200, 37, flags=FLAG_KNN_PANEL, feats=(O,)),
        # gram_split + gram_pk<H, 128>
        Case("pk_B43_300x100", PK, 300, 100, B=43, feats=(C, N, F, O, D, UP, DN, SAME)),
        Case("pk_B43_300x100_f32", PK, 300, 100, B=43, flags=FLAG_D2_F32,
             feats=(C, N, F, O, D, UP, DN, SAME)),
        Case("pk_B43_300x37", PK, 300, 37, B=43, feats=(N, C, UP, DN)),
        Case("pk_B43_257x64", PK, 257, 64, B=43, feats=(N, F, SAME)),
        Case("pk_B43_300x100_K60", PK, 300, 100, B=43, K=60),
        Case("pk_2900x192", PK, 2900, 192, feats=(D,)),
        # gram_split + gram_pk2<H>
        Case("pk2_B52_512x192", PK2, 512, 192, B=52, feats=(N, F, O, UP, DN, SAME)),
        Case("pk2_B43_300x64_t256", PK2, 300, 64, B=43, tile=256),
        Case("pk2_B43_300x100_t256", PK2, 300, 100, B=43, tile=256, feats=(C, N, D)),
        # (B = 52 of 513 x 192 and B = 90 of 512 x 192 take 128-tiles on their own at 256 CUs --
        # gram_tile256 asks for strictly fewer stage bytes and both tie at 768 -- so the knob
        # picks the 256-tiles; 513 then has a tail of 56 tiles as 128-subtiles)
        Case("pk2_B52_513x192_t256", PK2, 513, 192, B=52, tile=256),
        # tails: 270 256-tiles, 14 of them in the last round
        Case("pk2_tail0_B90_512x192", PK2, 512, 192, B=90, tile=256, tail=0,
             feats=(N, UP, DN), seed=77),
        Case("pk2_tail1_B90_512x192", PK2, 512, 192, B=90, tile=256, tail=1,
             feats=(N, UP, DN), seed=77),
        Case("pk2_tail2_B90_512x192", PK2, 512, 192, B=90, tile=256, tail=2,
             feats=(N, UP, DN), seed=77),
    ]
    out = {}
    for q, c in enumerate(cs):
        out[c.name] = dataclasses.replace(c, seed=c.seed or 100 + q)
    return out


CASES = _mk()
# the locality order's shape (test_gpu_gram_stage): past the order's n >= 1024 and 4 MB gates
ORDER_CASE = Case("order_1100x1024", BF3, 1100, 1024, seed=99)
# the family's coherent case: the input on which the tight bound has teeth
COHERENT = {BF3: "bf3_130x132", BF3H: "bf3h_65x100", BF3S: "bf3s_65x257",
            BF3W: "bf3w_panel_1200x100", PK: "pk_B43_300x100", PK2: "pk2_B43_300x100_t256"}
OFFSET = {BF3: "bf3_257x600", BF3H: "bf3h_200x128_off4", BF3S: "bf3s_1024x512",
          BF3W: "bf3w_panel_1200x37", PK: "pk_B43_300x100", PK2: "pk2_B52_512x192"}


def f32_twin(case):
    """The same inputs with GLL_FLAG_D2_F32 (the run an fp16 case's halves are compared with)."""
    return dataclasses.replace(case, name=case.name + "+f32", flags=case.flags | FLAG_D2_F32)


def all_routed_cases():
    """Every case, and the fp32 twin of every fp16 one (the GPU test runs both)."""
    cs = list(CASES.values())
    return cs + [f32_twin(c) for c in cs if c.route().H]


# bf16 residues of one sign and near-maximal size: c = 1 + 2^-9 (1 + 126/128) + 2^-17 - 2^-23, so
# hi = 1 (residue +0.996 of the half ulp 2^-8) and lo = 2^-9 (1 + 126/128) (residue 2^-17 - 2^-23
# of the half ulp 2^-17); 2 c has the same residues doubled.  Every dropped term then adds.
COHERENT_C = np.float32(1.0 + 2.0 ** -9 * (1 + 126 / 128) + 2.0 ** -17 - 2.0 ** -23)


def feat_kind(case, g):
    return case.feats[g % len(case.feats)]


def features(case, g=0):
    """Graph g of a case: n x d float32."""
    n, d = case.n, case.d
    kind = feat_kind(case, g)
    rng = np.random.default_rng([case.seed, g])
    X = rng.standard_normal((n, d)).astype(np.float32)
    if kind == "coherent":
        X = np.where(rng.random((n, d)) < 0.5, COHERENT_C, np.float32(2) * COHERENT_C)
        X = X.astype(np.float32)
        X[0] = 0
    elif kind == "far":
        X *= np.float32(0.01)
        v = rng.standard_normal(d)
        X[0] = (10.0 * v / np.linalg.norm(v)).astype(np.float32)
    elif kind == "offset":
        v = rng.standard_normal(d)
        X += (1000.0 * v / np.linalg.norm(v)).astype(np.float32)
    elif kind == "scale_up":
        X *= np.float32(1e3)
    elif kind == "scale_dn":
        X *= np.float32(1e-3)
    elif kind == "dups":
        k = min(200, n // 2)
        X[5: 5 + k] = X[5]
    elif kind == "allsame":
        X[:] = X[1]
    else:
        assert kind == "normal", kind
    return np.ascontiguousarray(X)


# ------------------------------------------------------------------------------------------
# Model
# ------------------------------------------------------------------------------------------
def bf16(a):
    """bf16_rne of a finite float32 array: (values as float32, bit patterns as uint16).  Integer
    arithmetic on the bits (round to nearest, ties to even); tests/test_gram_ref_cpu.py holds it to
    torch's cast."""
    b = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    hb = ((b + (((b >> 16) & 1) + np.uint32(0x7FFF))) >> 16).astype(np.uint16)
    return (hb.astype(np.uint32) << 16).view(np.float32), hb


def split(X, centre=True):
    """a, hi, lo (float32 values) and the bit patterns of hi, lo."""
    a = (X - X[0]).astype(np.float32) if centre else X.astype(np.float32)
    hi, hb = bf16(a)
    lo, lb = bf16((a - hi).astype(np.float32))
    return a, hi, lo, hb, lb


def _sym3(hi, lo, sl, drop=()):
    """(G, S) over the feature slice sl in float64; drop: terms left out ('lohi', 'hilo')."""
    h, l = hi[:, sl].astype(np.float64), lo[:, sl].astype(np.float64)
    hT = np.ascontiguousarray(h.T)      # (a product with its own transpose takes a slower path)
    lh = l @ hT
    G = h @ hT
    if "lohi" not in drop:
        G = G + lh
    if "hilo" not in drop:
        G = G + lh.T
    ah, al = np.abs(h), np.abs(l)
    ahT = np.abs(hT)
    alh = al @ ahT
    return G, ah @ ahT + alh + alh.T


class Model:
    """One graph's model: planes[p] = D2_model of plane p, with the S and N each was built from."""

    def __init__(self, case, X):
        with blas_threads():
            self._build(case, X)

    def _build(self, case, X):
        self.case, self.rt = case, case.route()
        n, d = X.shape
        self.a, self.hi, self.lo, self.hb, self.lb = split(X)
        a64 = self.a.astype(np.float64)
        self.N = (a64 * a64).sum(1)
        G, self.S = _sym3(self.hi, self.lo, slice(0, d))
        self.D2 = self.N[:, None] + self.N[None, :] - 2 * G
        # the true squared distances, float64, on exactly centred rows
        c = X.astype(np.float64) - X[0].astype(np.float64)
        cn = (c * c).sum(1)
        cc = c @ np.ascontiguousarray(c.T)
        self.truth = np.maximum(cn[:, None] + cn[None, :] - 2 * cc, 0.0)
        np.fill_diagonal(self.truth, 0.0)
        self.diag_tiles = (np.arange(n)[:, None] // 64) == (np.arange(n)[None, :] // 64)
        if self.rt.planes == 2:
            self.pN, self.pS, pD = [], [], []
            for sl in (slice(0, 256), slice(256, d)):
                Np = (a64[:, sl] ** 2).sum(1)
                Gp, Sp = _sym3(self.hi, self.lo, sl)
                self.pN.append(Np)
                self.pS.append(Sp)
                pD.append(Np[:, None] + Np[None, :] - 2 * Gp)
            dg = self.diag_tiles
            self.planes = [np.where(dg, self.D2, pD[0]), np.where(dg, 0.0, pD[1])]
        else:
            self.planes = [self.D2]

    # -- bounds ---------------------------------------------------------------------------
    def chain(self):
        """(T, D): MFMAs chained into one accumulator per wave; depth of the norm's sum."""
        d, dp, f = self.case.d, self.case.dp, self.rt.family
        if f == BF3:
            nph = (d + 255) // 256
            return 12 * nph, 3 + nph + 6
        if f == BF3H:
            return 12, 3 + 5
        if f == BF3S:
            return 24, 3 + 6 + 1
        if f == BF3W:
            nph = (d + 127) // 128
            return 24 * nph, 3 + 5 + nph
        return 3 * dp // 16, 3 + (dp + 255) // 256 + 6

    def norm_bound(self, N=None):
        return gamma(self.chain()[1] + 1) * (self.N if N is None else N) * SLOP

    def _bound(self, S, N):
        T = self.chain()[0]
        eg = (gamma(KAPPA_M * T) + gamma(KQ[self.rt.family] - 1)) * S
        en = self.norm_bound(N)
        comb = 2 * U * (N[:, None] + N[None, :] + 2 * S)
        return (2 * eg + en[:, None] + en[None, :] + comb) * SLOP

    def bound(self):
        """Per plane: elementwise bound on |kernel - model| (fp32 storage)."""
        full = self._bound(self.S, self.N)
        if self.rt.planes == 1:
            return [full]
        dg = self.diag_tiles
        return [np.where(dg, full, self._bound(self.pS[0], self.pN[0])),
                np.where(dg, 0.0, self._bound(self.pS[1], self.pN[1]))]

    def contract(self):
        r = np.sqrt(self.N)
        return K_GRAM_ERR * (r[:, None] + r[None, :]) ** 2


# ------------------------------------------------------------------------------------------
# emulate(): the arrays a kernel would leave, from the model (float64 rounded once, or float32
# arithmetic with a shuffled summation order), optionally with one injected error
# ------------------------------------------------------------------------------------------
MUTATIONS = ("drop_lohi", "drop_hilo", "drop_tail16", "drop_tail64", "drop_tail256", "no_centre",
             "bf16_norms", "transpose_tile", "stale_tile", "plane1_diag", "scale_from_max",
             "fp16_trunc")


def _groups(case, rt):
    """Feature groups (index arrays) whose products one wave chains, per plane; the kernel sums a
    plane's groups in this order."""
    d, f = case.d, rt.family
    k = np.arange(d)
    if f == BF3:
        return [[k[(k % 256) // 64 == q] for q in range(4)]]
    if f == BF3H:
        return [[k[k // 64 == q] for q in range(2)]]
    if f == BF3S:
        return [[k[(k < 256) & ((k % 256) // 64 == q)] for q in range(4)],
                [k[(k >= 256) & ((k % 256) // 64 == q)] for q in range(4)]]
    return [[k]]


def _chain_f32(hi, lo, ks, rng):
    """float32 accumulator over the features ks in k-steps of 16: lo hi, hi lo, hi hi, each step's
    16 products added one by one in a shuffled order."""
    n = hi.shape[0]
    acc = np.zeros((n, n), dtype=np.float32)
    for s0 in range(0, len(ks), 16):
        kk = ks[s0: s0 + 16]
        for A, Bm in ((lo, hi), (hi, lo), (hi, hi)):
            for k in rng.permutation(kk):
                acc = acc + np.outer(A[:, k], Bm[:, k])     # bf16 x bf16: exact in float32
    return acc


def _tree_sum_f32(sq):
    """Pairwise float32 sum along axis 1 (depth log2 of the padded width)."""
    w = 1 << max(int(sq.shape[1] - 1).bit_length(), 0)
    t = np.zeros((sq.shape[0], w), dtype=np.float32)
    t[:, : sq.shape[1]] = sq
    while t.shape[1] > 1:
        t = t[:, ::2] + t[:, 1::2]
    return t[:, 0]


def emulate(case, X, mut=None, f32=False, rng=None):
    """One graph's arrays as check() takes them."""
    rt = case.route()
    n, d = X.shape
    ts = TILE[rt.family]
    a, hi, lo, hb, lb = split(X, centre=mut != "no_centre")
    if mut in ("drop_tail16", "drop_tail64", "drop_tail256"):
        cut = (d // int(mut[9:])) * int(mut[9:])
        a, hi, lo = a.copy(), hi.copy(), lo.copy()
        a[:, cut:] = 0
        hi[:, cut:] = 0
        lo[:, cut:] = 0
    drop = {"drop_lohi": ("lohi",), "drop_hilo": ("hilo",)}.get(mut, ())
    sls = [slice(0, 256), slice(256, d)] if rt.planes == 2 else [slice(0, d)]
    planes = []
    if f32:
        sq = (a * a).astype(np.float32)
        for p, groups in enumerate(_groups(case, rt)):
            g = np.zeros((n, n), dtype=np.float32)
            for ks in groups:
                g = g + _chain_f32(hi, lo, ks, rng)
            N = _tree_sum_f32(sq[:, sls[p]])
            pl = (N[:, None] + N[None, :]) - np.float32(2) * g
            planes.append(np.triu(pl) + np.triu(pl, 1).T)      # upper triangle, mirrored
        Nall = _tree_sum_f32(sq)
    else:
        a64 = a.astype(np.float64)
        for sl in sls:
            N = (a64[:, sl] ** 2).sum(1)
            if mut == "bf16_norms":
                N = bf16(N.astype(np.float32))[0].astype(np.float64)
            G, _ = _sym3(hi, lo, sl, drop)
            planes.append((N[:, None] + N[None, :] - 2 * G).astype(np.float32))
        Nall = (a64 ** 2).sum(1)
        if mut == "bf16_norms":
            Nall = bf16(Nall.astype(np.float32))[0]
        Nall = Nall.astype(np.float32)
    if rt.planes == 2:
        dg = (np.arange(n)[:, None] // 64) == (np.arange(n)[None, :] // 64)
        planes = [np.where(dg, planes[0] + planes[1], planes[0]).astype(np.float32),
                  np.where(dg, np.float32(0), planes[1]).astype(np.float32)]
        if mut == "plane1_diag":
            planes[1][0, min(1, n - 1)] = np.float32(2.0 ** -20)
            planes[1][min(1, n - 1), 0] = np.float32(2.0 ** -20)
    D2 = np.stack(planes)
    t = max(min(ts, n // 2), 1)
    if mut == "transpose_tile":     # the last rows' tile against the first columns, mirrored
        D2[:, n - t: n, 0: t] = D2[:, 0: t, n - t: n]          # without the transpose
    if mut == "stale_tile":         # 0xFF bytes: what an unwritten tile reads as
        D2[-1, n - t: n, 0: t] = np.float32(np.nan)
    out = {"D2": D2[:, case.buffer_rows(), :], "scale": None}
    if rt.presplit:
        dp = case.dp
        out["xhi"] = np.zeros((n, dp), dtype=np.uint16)
        out["xlo"] = np.zeros((n, dp), dtype=np.uint16)
        out["xhi"][:, :d], out["xlo"][:, :d] = bf16(hi)[1], bf16(lo)[1]
        out["xnrm"] = Nall
    if rt.H:
        M = np.float32(Nall.max())
        s = d2_scale(M / np.float32(4) if mut == "scale_from_max" else M)
        v = out["D2"]
        out["D2_f32"] = v
        vs = v * s
        h = vs.astype(np.float16)
        if mut == "fp16_trunc":
            up = np.abs(h.astype(np.float32)) > np.abs(vs)
            h = np.where(up, np.nextafter(h, np.float16(0)), h).astype(np.float16)
        out["D2"] = h
        out["scale"] = s
    return out


# ------------------------------------------------------------------------------------------
# check()
# ------------------------------------------------------------------------------------------
def _where(case, rt, g, p, r, j, rows):
    ts = TILE[rt.family]
    i = int(rows[r])
    bi, bj = i // ts, j // ts
    if rt.panels:
        ori = "panel"
    else:
        ori = "diagonal" if bi == bj else ("direct" if bi < bj else "mirrored")
    return (f"graph {g} ({feat_kind(case, g)}), plane {p}, element ({i}, {j}), "
            f"{ts}-tile ({min(bi, bj)}, {max(bi, bj)}) {ori}")


def _first(mask):
    return tuple(int(v) for v in np.argwhere(mask)[0])


def check(case, Xs, outs, graphs=None, models=None):
    """Hold the arrays of graphs `graphs` (default 0 .. len(outs) - 1; Xs[q], outs[q] belong to
    graph graphs[q]) to the model.  Returns {quantity: (elements, worst err / bound)} for D2,
    plane, norm, fp16 and contract; raises AssertionError naming the first offending (graph,
    element, tile, orientation)."""
    rt = case.route()
    n, rows = case.n, case.buffer_rows()
    graphs = list(range(len(outs))) if graphs is None else graphs
    stats = {k: [0, 0.0] for k in ("D2", "plane", "norm", "fp16", "contract")}

    def hold(key, err, bnd, what):
        bad = ~(err <= bnd)
        if bad.any():
            at = _first(bad)
            raise AssertionError(f"{case.name}: {key} {what(at)}: err {err[at]:.3e}, "
                                 f"bound {bnd[at]:.3e}, err/bound {err[at] / bnd[at] if bnd[at] else np.inf:.3f}"
                                 + ("" if bnd[at] else " (bound is 0: must be exact)"))
        nz = bnd > 0
        stats[key][0] += int(err.size)
        if nz.any():
            stats[key][1] = max(stats[key][1], float((err[nz] / bnd[nz]).max()))

    for q, g in enumerate(graphs):
        X, o = Xs[q], outs[q]
        m = models[q] if models is not None else Model(case, X)
        raw = o["D2"]
        assert raw.shape == (rt.planes, rows.size, n), (raw.shape, rt.planes, rows.size, n)
        assert (raw.dtype == np.float16) == bool(rt.H), raw.dtype
        loc = lambda at: _where(case, rt, g, at[0], at[1], at[2], rows)
        fin = np.isfinite(raw)
        assert fin.all(), f"{case.name}: D2 non-finite (unwritten?) at {loc(_first(~fin))}"
        mdl = np.stack([pl[rows] for pl in m.planes])
        bnd = np.stack([b[rows] for b in m.bound()])
        v = raw.astype(np.float64)
        extra = 0.0
        if rt.H:
            s = np.float32(o["scale"])
            want = d2_scale(np.float32(np.max(o["xnrm"])))
            assert s.view(np.uint32) == want.view(np.uint32), \
                f"{case.name}: graph {g}: scale word {s!r}, d2_scale(max xnrm) = {want!r}"
            v = v / float(s)
            extra = RHO16 * (np.abs(mdl) + bnd) + SIG16 / float(s)
            if o.get("D2_f32") is not None:
                v32 = o["D2_f32"].astype(np.float32)
                hold("fp16", np.abs(v - v32.astype(np.float64)),
                     RHO16 * np.abs(v32.astype(np.float64)) + SIG16 / float(s), loc)
                h = (v32 * s).astype(np.float16)
                ne = h.view(np.uint16) != raw.view(np.uint16)      # subnormal halves included
                assert not ne.any(), (f"{case.name}: stored half is not float16(v s) at "
                                      f"{loc(_first(ne))}: {raw[_first(ne)]!r} vs {h[_first(ne)]!r}")
        hold("D2", np.abs(v - mdl), bnd + extra, loc)
        tot = v.sum(0)
        cw = m.contract()[rows]
        if rt.H:
            cw = cw + RHO16 * (m.truth[rows] + cw) + SIG16 / float(s)
        hold("contract", np.abs(tot - m.truth[rows])[None], cw[None], loc)
        # |a_i|^2 as the select reads it: D2[i][0] (a_0 = 0), planes summed in order
        col0 = raw[:, :, 0].astype(np.float32).sum(0, dtype=np.float32).astype(np.float64)
        if rt.H:
            col0 = col0 / float(s)
        assert (col0 >= 0).all(), f"{case.name}: graph {g}: D2[i][0] < 0 at row {rows[_first(col0 < 0)[0]]}"
        nb = m.norm_bound()[rows] * rt.planes + (1 + rt.planes) * U * m.N[rows]
        if rt.H:
            nb = nb + RHO16 * (m.N[rows] + nb) + SIG16 / float(s)
        hold("norm", np.abs(col0 - m.N[rows]), nb, lambda at: f"graph {g} D2[{rows[at[0]]}][0]")
        if not rt.panels:
            for p in range(rt.planes):
                ne = raw[p].view(np.uint16 if rt.H else np.uint32) != \
                    raw[p].T.view(np.uint16 if rt.H else np.uint32)
                assert not ne.any(), f"{case.name}: D2 not bitwise symmetric at {loc((p,) + _first(ne))}"
            if rt.planes == 2:
                nz = (raw[1].view(np.uint32) != 0) & m.diag_tiles
                assert not nz.any(), (f"{case.name}: plane 1 of a diagonal tile is not zero at "
                                      f"{loc((1,) + _first(nz))}")
        if rt.presplit:
            dp = case.dp
            for key, bits in (("xhi", m.hb), ("xlo", m.lb)):
                wantb = np.zeros((n, dp), dtype=np.uint16)
                wantb[:, : case.d] = bits
                ne = o[key].reshape(n, dp) != wantb
                assert not ne.any(), (f"{case.name}: graph {g}: {key} differs from the model's plane "
                                      f"at (row, feature) {_first(ne)}")
                stats["plane"][0] += int(ne.size)
            hold("norm", np.abs(o["xnrm"].astype(np.float64) - m.N), m.norm_bound(),
                 lambda at: f"graph {g} xnrm[{at[0]}]")
            if not rt.H:   # n_i + n_0 - 2 * 0 is n_i exactly
                ne = raw[0][:, 0].view(np.uint32) != o["xnrm"].view(np.uint32)[rows]
                assert not ne.any(), \
                    f"{case.name}: graph {g}: D2[i][0] is not bitwise xnrm[i] at {_first(ne)}"
    return {k: tuple(v) for k, v in stats.items()}


def pivot_row(j, n):
    """order.hip pivot_row."""
    return ((j * 2654435761 + 12345) & 0xFFFFFFFF) % n
