"""The layer's front end on the GPU (features.hip): the two stage kernels against
the float64 stage reference and its derived bounds (tests/unit_ref.py), their order independence,
the layer with normalize=True / fp16 / bf16 features against the stages it is made of (bitwise),
which route a call takes (gll_features_calls), the whole chain against float64, and the host
contract of the new argument."""

import numpy as np
import pytest
import torch

from graphlearninglayer_amd.synth import CONFIGS, one_hot, seeded_gbar, synth
from oracle import gll_oracle as O
from tests import abi as A
from tests import unit_ref as R

pytestmark = pytest.mark.gpu
TOL = 1e-4                      # the project's parity bar (tests/test_gpu_parity.py)
DT = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
SENT = -7.25                    # guard value, exact in every dtype


def _G():
    from graphlearninglayer_amd import GLL
    return GLL


def _L():
    from graphlearninglayer_amd import _lib
    return _lib


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    A.need_gpu()


def _calls():
    return _L().lib().gll_features_calls()


def _guarded(rows, d, dtype):
    """rows x d in the middle of a sentinel-filled (rows + 2) x d tensor."""
    big = torch.full((rows + 2, d), SENT, dtype=dtype, device="cuda")
    return big, big[1:-1]


def _guards_intact(big):
    return bool((big[0] == SENT).all()) and bool((big[-1] == SENT).all())


def _forward_raw(Z, normalize, with_rnorm=True):
    """gll_features_forward into guarded outputs; returns (X, rnorm, their guarded parents)."""
    L = _L()
    rows, d = Z.shape
    Xbig, X = _guarded(rows, d, torch.float32)
    rbig = torch.full((rows + 2,), SENT, dtype=torch.float32, device="cuda")
    rn = rbig[1:-1]
    code = {torch.float32: L.XT_F32, torch.float16: L.XT_F16, torch.bfloat16: L.XT_BF16}[Z.dtype]
    rc = L.lib().gll_features_forward(rows, d, Z.data_ptr(), code,
                                      L.UF_NORMALIZE if normalize else 0, X.data_ptr(),
                                      rn.data_ptr() if with_rnorm else None, A.stream())
    assert rc == 0
    torch.cuda.synchronize()
    return X, rn, Xbig, rbig


def _backward_raw(gX, X, rn, dtype, normalize):
    L = _L()
    rows, d = gX.shape
    gbig, gZ = _guarded(rows, d, dtype)
    code = {torch.float32: L.XT_F32, torch.float16: L.XT_F16, torch.bfloat16: L.XT_BF16}[dtype]
    rc = L.lib().gll_features_backward(rows, d, gX.data_ptr(),
                                       X.data_ptr() if normalize else None,
                                       rn.data_ptr() if normalize else None,
                                       L.UF_NORMALIZE if normalize else 0, gZ.data_ptr(), code,
                                       A.stream())
    assert rc == 0
    torch.cuda.synchronize()
    return gZ, gbig


def _stage_rows(rows, d, name):
    z = R.rows_input(rows, d, seed=1000 * d + rows, dtype=name)
    return torch.from_numpy(z).to(DT[name]).cuda()


_STAGE = {}


def _stage(rows, d, name):
    """The forward stage's result at one shape and dtype, computed once for the tests below."""
    key = (rows, d, name)
    if key not in _STAGE:
        Z = _stage_rows(rows, d, name)
        _STAGE[key] = (Z,) + _forward_raw(Z, True)
    return _STAGE[key]


# ------------------------------------------------------------------------------------------
# 1. forward stage
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(DT))
@pytest.mark.parametrize("rows,d", R.SHAPES)
def test_forward_stage_within_the_derived_bound(rows, d, name):
    Z, X, rn, Xbig, rbig = _stage(rows, d, name)
    z64 = Z.double().cpu().numpy()
    x, r = R.forward_ref(z64)
    Xh, rh = X.cpu().numpy().astype(np.float64), rn.cpu().numpy().astype(np.float64)
    err, bound = np.abs(Xh - x), R.forward_bound(x, d)
    worst = float((err / np.where(bound > 0, bound, 1.0)).max())
    print(f"forward {name} {rows}x{d}: {worst:.3f} of the bound")
    assert np.isfinite(Xh).all() and (err <= bound).all()
    assert (np.abs(rh - r) <= (d + 8) * R.U * r).all()
    assert _guards_intact(Xbig) and _guards_intact(rbig)
    f1e12 = float(np.float32(1e12))
    if rows > 1:     # zero row
        assert (Xh[0] == 0).all() and rh[0] == f1e12
    if rows > 2:     # one-hot row: exact
        assert np.array_equal(Xh[1], z64[1]) and rh[1] == 1.0
    if rows > 3 and name == "float32":   # 1e-20: clamped, X = 1e-8
        assert rh[2] == f1e12 and abs(Xh[2, 0] - 1e-8) <= 1e-8 * 1e-6 and (Xh[2, 1:] == 0).all()
    if rows > 4 and name == "float16":   # the largest fp16 row
        assert (z64[3] == 65504.0).all() and abs(rh[3] * 65504.0 * np.sqrt(d) - 1) <= (d + 8) * R.U


@pytest.mark.parametrize("name", list(DT))
@pytest.mark.parametrize("rows,d", R.SHAPES)
def test_forward_pass_through_is_the_exact_widening(rows, d, name):
    dt = DT[name]
    Z = _stage_rows(rows, d, name)
    fi = torch.finfo(dt)
    flat = Z.view(-1)
    special = torch.tensor([float("inf"), float("-inf"), float("nan"), fi.tiny / 4, -fi.tiny / 8,
                            fi.max, -0.0, fi.tiny * fi.eps], dtype=torch.float64).to(dt).cuda()
    k = min(flat.numel(), special.numel())
    flat[-k:] = special[:k]                      # incl. subnormals of the type, +-inf, NaN
    for with_rnorm in (True, False):
        X, rn, Xbig, rbig = _forward_raw(Z, False, with_rnorm)
        want = Z.float()
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(X), nan)
        assert A.same_bits(torch.where(nan, 0.0, X), torch.where(nan, 0.0, want))
        assert bool((rbig == SENT).all())        # rnorm is not touched
        assert _guards_intact(Xbig)


# ------------------------------------------------------------------------------------------
# 2. backward stage
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(DT))
@pytest.mark.parametrize("rows,d", R.SHAPES)
def test_backward_stage_within_the_derived_bound(rows, d, name):
    dt = DT[name]
    Z, X, rn, _, _ = _stage(rows, d, name)
    g = torch.from_numpy(np.random.Generator(np.random.PCG64(77 * d + rows))
                         .standard_normal((rows, d)).astype(np.float32)).cuda()
    gZ, gbig = _backward_raw(g, X.contiguous(), rn.contiguous(), dt, True)
    assert _guards_intact(gbig)
    g64, x64, r32 = g.double().cpu().numpy(), X.double().cpu().numpy(), rn.cpu().numpy()
    ref = R.backward_ref(g64, x64, r32)
    bound = R.backward_bound(g64, x64, r32, name)
    cl = R.clamped(r32)
    if rows > 1:
        assert cl[0]                                           # the zero row
    got = gZ.double().cpu().numpy()
    live = ~cl
    err = np.abs(got[live] - ref[live])
    worst = float((err / np.where(bound[live] > 0, bound[live], 1.0)).max()) if live.any() else 0.0
    print(f"backward {name} {rows}x{d}: {worst:.3f} of the bound")
    assert np.isfinite(got[live]).all() and (err <= bound[live]).all()
    # a clamped row is one fp32 multiplication r g, rounded once (fp16: 1e12 g overflows to inf)
    if cl.any():
        c = torch.from_numpy(cl).cuda()
        assert A.same_bits(gZ[c], (rn[c, None] * g[c]).to(dt))


@pytest.mark.parametrize("name", list(DT))
@pytest.mark.parametrize("rows,d", R.SHAPES)
def test_backward_pass_through_is_the_cast(rows, d, name):
    dt = DT[name]
    rng = np.random.Generator(np.random.PCG64(5 * d + rows))
    g = (rng.standard_normal((rows, d)) * 10.0 ** rng.uniform(-9, 6, size=(rows, d)))
    g = torch.from_numpy(g.astype(np.float32)).cuda()    # past fp16's range both ways
    gZ, gbig = _backward_raw(g, None, None, dt, False)
    assert A.same_bits(gZ, g.to(dt)) and _guards_intact(gbig)


# ------------------------------------------------------------------------------------------
# 3. order independence
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(DT))
@pytest.mark.parametrize("rows,d", [(257, 8), (37, 7), (9, 129), (6, 1028)])
def test_rows_do_not_depend_on_their_place(rows, d, name):
    G, dt = _G(), DT[name]
    Z = _stage_rows(rows, d, name)
    g = torch.randn(rows, d, device="cuda", generator=torch.Generator("cuda").manual_seed(d))
    perm = torch.randperm(rows, device="cuda", generator=torch.Generator("cuda").manual_seed(rows))
    X, rn = G.unit_features(Z)
    gZ = G.unit_features_backward(g, X, rn, dt)
    Xp, rnp = G.unit_features(Z[perm].contiguous())
    gZp = G.unit_features_backward(g[perm].contiguous(), Xp, rnp, dt)
    assert A.same_bits(Xp, X[perm]) and A.same_bits(rnp, rn[perm]) and A.same_bits(gZp, gZ[perm])


@pytest.mark.parametrize("name", list(DT))
@pytest.mark.parametrize("B,n,d", [(3, 5, 7), (3, 4, 64), (2, 3, 1001)])
def test_a_batch_is_its_separate_calls(B, n, d, name):
    """Odd n x d with a half type: graph b's rows start misaligned inside the batch (the scalar
    form) and aligned on their own... the sums take the same order either way."""
    G, dt = _G(), DT[name]
    Z = _stage_rows(B * n, d, name).view(B, n, d)
    g = torch.randn(B, n, d, device="cuda", generator=torch.Generator("cuda").manual_seed(n))
    X, rn = G.unit_features(Z)
    gZ = G.unit_features_backward(g, X, rn, dt)
    assert X.shape == (B, n, d) and rn.shape == (B, n) and gZ.shape == (B, n, d)
    for b in range(B):
        Xb, rb = G.unit_features(Z[b].clone())
        assert A.same_bits(Xb, X[b]) and A.same_bits(rb, rn[b])
        assert A.same_bits(G.unit_features_backward(g[b].clone(), Xb, rb, dt), gZ[b])


def test_more_rows_than_one_launch_holds():
    """2^24 + 5 rows of d = 1: two launches of each kernel (4 rows a workgroup, 2^22 workgroups a
    launch), row indices past the first launch's end."""
    G = _G()
    rows = (1 << 24) + 5
    Z = torch.randn(rows, 1, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    Z[Z == 0] = 1.0
    c0 = _calls()
    X, rn = G.unit_features(Z)
    assert _calls() - c0 == 2
    assert bool(((X - torch.sign(Z)).abs() <= 9 * R.U).all())
    assert bool(((rn[:, None] * Z.abs() - 1).abs() <= 9 * R.U).all())
    g = torch.randn(rows, 1, device="cuda", generator=torch.Generator("cuda").manual_seed(2))
    gZ = G.unit_features_backward(g, None, None, torch.bfloat16, normalize=False)
    assert _calls() - c0 == 4
    assert A.same_bits(gZ, g.to(torch.bfloat16))


# ------------------------------------------------------------------------------------------
# 4. the layer is the stages
# ------------------------------------------------------------------------------------------
PLUMB = CONFIGS["plumbing"]
LAYER_SHAPES = {"plumbing": (PLUMB["base"], PLUMB["batch"], PLUMB["d"], PLUMB["k"], PLUMB["r"]),
                "d37": (30, 67, 37, 6, 0.75)}


def _raw_features(shape, B, name, seed=0):
    """Un-normalised features: synth's unit rows times a per-row scale, in dtype `name`."""
    base, batch, d, k, r = LAYER_SHAPES[shape]
    zs, Ys, ts = [], [], []
    for b in range(B):
        X, labels = synth(base, batch, d, r=r, seed=seed + b)
        rng = np.random.Generator(np.random.PCG64(50 + seed + b))
        zs.append(X * rng.uniform(0.25, 4.0, size=(X.shape[0], 1)).astype(np.float32))
        Ys.append(one_hot(labels[:base]))
        ts.append(labels[base:])
    z = torch.from_numpy(np.stack(zs)).to(DT[name]).cuda()
    Y = torch.from_numpy(np.stack(Ys)).cuda()
    t = torch.from_numpy(np.stack(ts)).cuda()
    gbar = torch.from_numpy(np.stack([seeded_gbar(batch, 10, seed=7 + b) for b in range(B)])).cuda()
    if B == 1:
        z, Y, t, gbar = z[0], Y[0], t[0], gbar[0]
    return z.contiguous(), Y.contiguous(), t.contiguous(), gbar.contiguous(), k


def _leaves(Y):
    return (Y.clone().requires_grad_(True),
            torch.tensor(0.05, dtype=torch.float64, device="cuda", requires_grad=True))


@pytest.mark.parametrize("name", list(DT))
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("eps", [1.0, "auto"])
@pytest.mark.parametrize("shape", list(LAYER_SHAPES))
def test_layer_with_normalize_is_bitwise_its_stages(shape, eps, B, name):
    G = _G()
    F = G.LaplaceLearningSparseHard
    z, Y, t, gbar, k = _raw_features(shape, B, name)
    Xh, rn = G.unit_features(z)
    # apply
    zA, (YA, tauA) = z.clone().requires_grad_(True), _leaves(Y)
    UA = F.apply(zA, YA, tauA, eps, k, normalize=True)
    UA.backward(gbar)
    XB, (YB, tauB) = Xh.clone().requires_grad_(True), _leaves(Y)
    UB = F.apply(XB, YB, tauB, eps, k)
    UB.backward(gbar)
    assert A.same_bits(UA.detach(), UB.detach())
    assert zA.grad.dtype == z.dtype
    assert A.same_bits(zA.grad, G.unit_features_backward(XB.grad, Xh, rn, z.dtype))
    assert A.same_bits(YA.grad, YB.grad) and A.same_bits(tauA.grad, tauB.grad)
    # ce_loss (normalize given positionally)
    zC, (YC, tauC) = z.clone().requires_grad_(True), _leaves(Y)
    outC = F.ce_loss(zC, YC, t, tauC, eps, k, True)
    outC[0].sum().backward()
    XD, (YD, tauD) = Xh.clone().requires_grad_(True), _leaves(Y)
    outD = F.ce_loss(XD, YD, t, tauD, eps, k)
    outD[0].sum().backward()
    for a, b in zip(outC, outD):
        assert A.same_bits(a.detach(), b.detach())
    assert A.same_bits(outC[1], UA.detach())
    assert A.same_bits(zC.grad, G.unit_features_backward(XD.grad, Xh, rn, z.dtype))
    assert A.same_bits(YC.grad, YD.grad) and A.same_bits(tauC.grad, tauD.grad)


# ------------------------------------------------------------------------------------------
# 5. routes
# ------------------------------------------------------------------------------------------
def _fwd_bwd(z, Y, gbar, k, normalize, eps=1.0):
    F = _G().LaplaceLearningSparseHard
    zl = z.clone().requires_grad_(True)
    c0 = _calls()
    U = F.apply(zl, Y, 0.05, eps, k, normalize)
    c1 = _calls()
    U.backward(gbar)
    c2 = _calls()
    return U.detach(), zl.grad, c1 - c0, c2 - c1


@pytest.mark.parametrize("B", [1, 3])
def test_fp32_without_normalize_takes_the_old_route(B):
    z, Y, t, gbar, k = _raw_features("plumbing", B, "float32")
    U1, g1, f1, b1 = _fwd_bwd(z, Y, gbar, k, False)
    U2, g2, f2, b2 = _fwd_bwd(z, Y, gbar, k, False)
    assert (f1, b1, f2, b2) == (0, 0, 0, 0)
    assert A.same_bits(U1, U2) and A.same_bits(g1, g2)
    F = _G().LaplaceLearningSparseHard
    zl = z.clone().requires_grad_(True)
    c0 = _calls()
    F.ce_loss(zl, Y, t, 0.05, 1.0, k)[0].sum().backward()
    assert _calls() == c0


@pytest.mark.parametrize("name", ["float16", "bfloat16"])
@pytest.mark.parametrize("B", [1, 3])
def test_half_features_without_normalize_convert_once_each_way(B, name):
    z, Y, t, gbar, k = _raw_features("plumbing", B, name)
    U, g, f, b = _fwd_bwd(z, Y, gbar, k, False)
    assert (f, b) == (1, 1)
    U32, g32, f32, b32 = _fwd_bwd(z.float(), Y, gbar, k, False)
    assert (f32, b32) == (0, 0)
    assert A.same_bits(U, U32) and g.dtype == z.dtype and A.same_bits(g, g32.to(z.dtype))


@pytest.mark.parametrize("name", list(DT))
@pytest.mark.parametrize("B", [1, 3])
def test_normalize_is_one_launch_each_way(B, name):
    z, Y, t, gbar, k = _raw_features("plumbing", B, name)
    _, g, f, b = _fwd_bwd(z, Y, gbar, k, True)
    assert (f, b) == (1, 1) and g.dtype == z.dtype and g.shape == z.shape
    F = _G().LaplaceLearningSparseHard
    c0 = _calls()
    F.apply(z, Y, 0.05, 1.0, k, True)                 # nothing requires grad: forward only
    assert _calls() - c0 == 1


# ------------------------------------------------------------------------------------------
# 6. end to end against float64
# ------------------------------------------------------------------------------------------
def _float64_chain(z, Y, gbar, k, eps, tau=0.05):
    """U and dloss/dz in float64: normalise z.double() on the CPU, the oracle for U and grad_X
    (on the GPU's kNN lists, checked exact against the float64 search), torch's float64 autograd
    through the normalisation."""
    G = _G()
    z64 = z.detach().double().cpu().requires_grad_(True)
    x64 = torch.nn.functional.normalize(z64, dim=1)
    xn = x64.detach().numpy()
    ind = G.device_graph(G.unit_features(z)[0], k, eps)["knn_idx"].cpu().numpy().astype(np.int64)
    assert O.knn_set_mismatch(xn, ind, k) == []
    Uo, st = O.forward(xn, Y.cpu().numpy(), tau, eps, k, knn=(ind, None))
    x64.backward(torch.from_numpy(O.backward(st, gbar.cpu().numpy())))
    return Uo, z64.grad.numpy()


_CHAIN = {}


def _chain(name, eps):
    if (name, eps) not in _CHAIN:
        z, Y, t, gbar, k = _raw_features("plumbing", 1, name)
        _CHAIN[(name, eps)] = (z, Y, gbar, k) + _float64_chain(z, Y, gbar, k, eps)
    return _CHAIN[(name, eps)]


@pytest.mark.parametrize("name", list(DT))
@pytest.mark.parametrize("eps", [1.0, "auto"])
def test_end_to_end_against_float64(eps, name):
    z, Y, gbar, k, Uo, gzo = _chain(name, eps)
    zl = z.clone().requires_grad_(True)
    U = _G().LaplaceLearningSparseHard.apply(zl, Y, 0.05, eps, k, normalize=True)
    U.backward(gbar)
    eU = O.rel_err(U.detach().cpu().numpy(), Uo)
    eg = O.rel_err(zl.grad.double().cpu().numpy(), gzo)
    print(f"end to end {name} eps={eps}: U {eU:.2e}, grad_z {eg:.2e}")
    assert eU < TOL
    assert eg < TOL + R.ROUNDING[name][0]


# ------------------------------------------------------------------------------------------
# 7. host contract
# ------------------------------------------------------------------------------------------
def test_cpu_bf16_input_comes_back_to_the_cpu():
    z, Y, t, gbar, k = _raw_features("plumbing", 1, "bfloat16")
    F = _G().LaplaceLearningSparseHard
    zd = z.clone().requires_grad_(True)
    Ud = F.apply(zd, Y, 0.05, 1.0, k, normalize=True)
    Ud.backward(gbar)
    zc = z.cpu().requires_grad_(True)
    Uc = F.apply(zc, Y.cpu(), 0.05, 1.0, k, normalize=True)
    assert Uc.device.type == "cpu" and Uc.dtype == torch.float64
    Uc.backward(gbar.cpu())
    assert zc.grad.device.type == "cpu" and zc.grad.dtype == torch.bfloat16
    assert A.same_bits(Uc, Ud.detach().cpu()) and A.same_bits(zc.grad, zd.grad.cpu())


@pytest.mark.parametrize("name", ["float32", "float16"])
def test_noncontiguous_input(name):
    z, Y, t, gbar, k = _raw_features("plumbing", 1, name)
    F = _G().LaplaceLearningSparseHard
    zt = z.t().contiguous().t()                       # same values, column-major storage
    assert not zt.is_contiguous()
    za, zb = z.clone().requires_grad_(True), zt.detach().requires_grad_(True)
    Ua, Ub = F.apply(za, Y, 0.05, 1.0, k, True), F.apply(zb, Y, 0.05, 1.0, k, True)
    Ua.backward(gbar)
    Ub.backward(gbar)
    assert A.same_bits(Ua.detach(), Ub.detach()) and A.same_bits(za.grad, zb.grad)


def test_float64_input_gets_a_float64_gradient():
    z, Y, gbar, k, Uo, gzo = _chain("float32", 1.0)
    c0 = _calls()
    zl = z.double().requires_grad_(True)
    U = _G().LaplaceLearningSparseHard.apply(zl, Y, 0.05, 1.0, k, normalize=True)
    U.backward(gbar)
    assert _calls() - c0 == 2 and zl.grad.dtype == torch.float64
    assert O.rel_err(U.detach().cpu().numpy(), Uo) < TOL
    assert O.rel_err(zl.grad.cpu().numpy(), gzo) < TOL


def test_normalize_must_be_a_bool():
    z, Y, t, gbar, k = _raw_features("plumbing", 1, "float32")
    F = _G().LaplaceLearningSparseHard
    for bad in (1, 0, None, "True", torch.tensor(True)):
        with pytest.raises(TypeError):
            F.apply(z, Y, 0.05, 1.0, k, bad)
        with pytest.raises(TypeError):
            F.ce_loss(z, Y, t, 0.05, 1.0, k, normalize=bad)
    with pytest.raises(TypeError):
        F.apply(z, Y, 0.05, 1.0, k, True, True)       # one argument too many


@pytest.mark.parametrize("name", ["float32", "bfloat16"])
def test_repeated_backward(name):
    z, Y, t, gbar, k = _raw_features("plumbing", 1, name)
    F = _G().LaplaceLearningSparseHard
    zl = z.clone().requires_grad_(True)
    U = F.apply(zl, Y, 0.05, 1.0, k, normalize=True)
    U.backward(gbar)
    with pytest.raises(RuntimeError, match="second time|already been freed"):
        U.backward(gbar)
    zr = z.clone().requires_grad_(True)
    U = F.apply(zr, Y, 0.05, 1.0, k, normalize=True)
    U.backward(gbar, retain_graph=True)
    g1 = zr.grad.clone()
    zr.grad = None
    U.backward(gbar)
    assert A.same_bits(g1, zr.grad) and A.same_bits(g1, zl.grad)
