"""CPU pins of the front-end stage reference (tests/unit_ref.py) and of the C ABI's argument checks
(gll_features_forward / gll_features_backward / gll_features_calls) -- no GPU call anywhere."""
import ctypes as ct

import numpy as np
import pytest
import torch

from graphlearninglayer_amd import _lib
from tests import unit_ref as R

EMU_D = (1, 2, 3, 7, 64, 100, 512, 1028, 4096)


def _special_rows(d):
    z = np.random.Generator(np.random.PCG64(d)).standard_normal((6, d))
    z[1] = 0.0                       # zero row: clamped
    z[2] = 0.0
    z[2, 0] = 1e-13                  # norm 1e-13: clamped
    z[3] = 0.0
    z[3, d - 1] = 1.0                # one-hot
    z[4] *= 1e3
    return z


@pytest.mark.parametrize("d", [1, 3, 64, 129])
def test_reference_is_torch_normalize_and_its_autograd(d):
    z = _special_rows(d)
    g = np.random.Generator(np.random.PCG64(100 + d)).standard_normal(z.shape)
    zt = torch.from_numpy(z).requires_grad_(True)
    xt = torch.nn.functional.normalize(zt, dim=1)
    xt.backward(torch.from_numpy(g))
    x, r = R.forward_ref(z)
    assert np.abs(x - xt.detach().numpy()).max() <= 1e-12
    assert r[1] == 1e12 and abs(r[2] - 1e12) <= 1e-12 * 1e12 and abs(r[3] - 1.0) <= 1e-15
    assert R.clamped(r).tolist() == [False, True, True, False, False, False]
    gz = R.backward_ref(g, x, r)
    ref = zt.grad.numpy()
    assert np.abs(gz - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
    # the clamped rule, spelled out: no projection, the gradient scaled by 1e12
    assert np.array_equal(gz[1], 1e12 * g[1])


@pytest.mark.parametrize("d", EMU_D)
def test_bounds_hold_for_an_fp32_emulation_with_sequential_sums(d):
    """The bounds are derived (unit_ref docstring); this pins them: numpy float32 with one rounding
    per operation and the worst summation order stays inside, using at most a quarter."""
    rows = 64 if d <= 512 else 8
    z = R.rows_input(rows, d, seed=7 * d)
    x32, r32 = R.emulate_forward_f32(z)
    x, r = R.forward_ref(z)
    live = ~R.clamped(r32)           # underflow-free rows (the clamped ones may underflow in s)
    fb = R.forward_bound(x, d)
    err = np.abs(x32.astype(np.float64) - x)
    assert (err <= fb).all()
    assert (np.abs(r32.astype(np.float64) - r) <= (d + 8) * R.U * r).all()
    ratio_f = (err[live] / np.where(fb[live] > 0, fb[live], 1.0)).max()
    g = np.random.Generator(np.random.PCG64(9 * d + 1)).standard_normal((rows, d)).astype(np.float32)
    out32 = R.emulate_backward_f32(g, x32, r32)
    ref = R.backward_ref(g, x32, r32)
    bb = R.backward_bound(g, x32, r32)
    errb = np.abs(out32.astype(np.float64) - ref)
    assert (errb <= bb).all()
    ratio_b = (errb / np.where(bb > 0, bb, 1.0)).max()
    print(f"d={d}: forward uses {ratio_f:.3f} of its bound, backward {ratio_b:.3f}")
    assert ratio_f <= 0.25 and ratio_b <= 0.25
    # clamped rows: one multiplication, exact in the emulation as in the kernel
    c = R.clamped(r32)
    assert np.array_equal(out32[c], (r32[c, None] * g[c]).astype(np.float32))


def test_output_rounding_terms_are_the_formats_half_spacing():
    for name, dt, mant, emin in (("bfloat16", torch.bfloat16, 8, -126), ("float16", torch.float16, 11, -14)):
        rel, floor = R.ROUNDING[name]
        assert rel == 2.0 ** -mant
        fi = torch.finfo(dt)
        assert rel == fi.eps / 2 and fi.tiny == 2.0 ** emin
        assert floor == fi.tiny * fi.eps / 2      # half the subnormal spacing
        v = torch.linspace(-3.0, 3.0, 4001, dtype=torch.float64)
        v = torch.cat([v, v * 2.0 ** (emin - 3)])   # normal and subnormal results
        err = (v.to(dt).double() - v).abs()
        assert bool((err <= torch.maximum(rel * v.abs(), torch.tensor(floor, dtype=torch.float64))).all())


def test_shapes_reach_every_instantiation_and_both_load_forms():
    """unit_rows_kernel / unit_grad_kernel<T, STEPS, VEC>: STEPS is the power of two with
    64 E STEPS >= d (E = 4 fp32, 8 half types), VEC needs d % E == 0."""
    for E, most in ((4, 16), (8, 8)):
        seen = set()
        for _, d in R.SHAPES:
            steps = 1
            while steps * 64 * E < d:
                steps *= 2
            seen.add((steps, d % E == 0))
        assert {s for s, _ in seen} == {1 << q for q in range(most.bit_length())}
        assert {v for _, v in seen} == {True, False}


# ------------------------------------------------------------------------------------------
# The C ABI without a GPU: every argument check comes before any HIP call
# ------------------------------------------------------------------------------------------
def _fwd(rows, d, Z=1 << 20, dt=0, flags=0, X=1 << 20, rn=1 << 20):
    return _lib.lib().gll_features_forward(rows, d, Z, dt, flags, X, rn, None)


def _bwd(rows, d, gX=1 << 20, X=1 << 20, rn=1 << 20, flags=0, gZ=1 << 20, dt=0):
    return _lib.lib().gll_features_backward(rows, d, gX, X, rn, flags, gZ, dt, None)


def test_feature_entry_points_reject_bad_arguments_without_a_gpu():
    before = _lib.lib().gll_features_calls()
    for call in (_fwd, _bwd):
        assert call(-1, 8) == -1                    # rows < 0
        assert call(4, 0) == -1 and call(4, -3) == -1    # d < 1
        assert call(4, 4097) == -1                  # d > 4096
        assert call(4, 8, dt=3) == -1 and call(4, 8, dt=-1) == -1   # unknown dtype
        assert call(4, 8, flags=2) == -1 and call(4, 8, flags=3) == -1   # unknown flag bit
        # the checks hold for rows == 0 as well: nothing is launched either way
        assert call(0, 0) == -1 and call(0, 8, dt=7) == -1 and call(0, 8, flags=4) == -1
    # NULL required pointers with rows > 0
    assert _fwd(4, 8, Z=None) == -1 and _fwd(4, 8, X=None) == -1
    assert _fwd(4, 8, flags=_lib.UF_NORMALIZE, rn=None) == -1
    assert _bwd(4, 8, gX=None) == -1 and _bwd(4, 8, gZ=None) == -1
    assert _bwd(4, 8, flags=_lib.UF_NORMALIZE, X=None) == -1
    assert _bwd(4, 8, flags=_lib.UF_NORMALIZE, rn=None) == -1
    assert _lib.lib().gll_features_calls() == before


def test_zero_rows_is_ok_launches_nothing_and_does_not_count():
    before = _lib.lib().gll_features_calls()
    for dt in (_lib.XT_F32, _lib.XT_F16, _lib.XT_BF16):
        for flags in (0, _lib.UF_NORMALIZE):
            assert _fwd(0, 1, Z=None, dt=dt, flags=flags, X=None, rn=None) == 0
            assert _bwd(0, 4096, gX=None, X=None, rn=None, flags=flags, gZ=None, dt=dt) == 0
    assert _lib.lib().gll_features_calls() == before


def test_constants_match_the_header():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "gll.h")).read()
    val = {k: int(v) for k, v in re.findall(r"#define (GLL_(?:XT|UF)_\w+) (\d+)", src)}
    assert val == {"GLL_XT_F32": _lib.XT_F32, "GLL_XT_F16": _lib.XT_F16,
                   "GLL_XT_BF16": _lib.XT_BF16, "GLL_UF_NORMALIZE": _lib.UF_NORMALIZE}
    assert ct.sizeof(ct.c_int64) == 8 and _lib.lib().gll_features_calls.restype is ct.c_int64


def test_wrappers_reject_what_the_abi_would():
    from graphlearninglayer_amd import GLL as G
    with pytest.raises(TypeError):
        G.unit_features(torch.zeros(4, 8), normalize=1)
    with pytest.raises(TypeError):
        G.unit_features(torch.zeros(4, 8, dtype=torch.float64))
    with pytest.raises(ValueError):
        G.unit_features(torch.zeros(4, 4097))
    with pytest.raises(ValueError):
        G.unit_features(torch.zeros(8))
    with pytest.raises(TypeError):
        G.LaplaceLearningSparseHard.apply(torch.zeros(10, 4), torch.zeros(5, 2), 0.0, 1.0, 5, 1)
    with pytest.raises(TypeError):
        G.LaplaceLearningSparseHard.ce_loss(torch.zeros(10, 4), torch.zeros(5, 2),
                                            torch.zeros(5, dtype=torch.long), normalize="yes")
