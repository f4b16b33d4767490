"""CPU checks of the fused SupCon / SimCLR loss: the float64 stage reference (tests/supcon_ref.py)
against the fixtures the reference's losses.py generated (tests/golden/make_supcon_golden.py)
and against finite differences, and the host side of the C ABI (no GPU call is made: every
rejected argument is rejected before any launch)."""
import ctypes as ct
import glob
import os
import re

import numpy as np
import pytest
import torch

import supcon_ref as S
from graphlearninglayer_amd import _lib, losses

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "supcon", "supcon_*.npz")))
NAMES = [os.path.basename(p)[len("supcon_"):-len(".npz")] for p in FIXTURES]


def load(path):
    z = np.load(path)
    return dict(f=z["features"], y=z["labels"] if "labels" in z else None, T=float(z["T"]),
                Tb=float(z["Tb"]), mode=str(z["mode"]), loss=float(z["loss64"]), grad=z["grad64"],
                e_loss=float(z["ref32_loss_err"]), e_grad=float(z["ref32_grad_relerr"]))


def test_fixture_set_covers_the_issue():
    fx = [load(p) for p in FIXTURES]
    assert len(fx) >= 8
    assert {c["mode"] for c in fx} == {"all", "one"}
    assert {c["f"].shape[1] for c in fx} == {1, 2, 3}
    assert any(c["y"] is None for c in fx) and any(c["y"] is not None for c in fx)
    assert {(c["T"], c["Tb"]) for c in fx} == {(0.07, 0.07), (0.5, 0.07)}
    assert sum(np.isnan(c["loss"]) for c in fx) == 1
    for p in FIXTURES:
        assert os.path.getsize(p) < 300 * 1024


@pytest.mark.parametrize("path", FIXTURES, ids=NAMES)
def test_reference_matches_fixture(path):
    c = load(path)
    r = S.supcon(c["f"], c["y"], c["T"], c["Tb"], c["mode"])
    if np.isnan(c["loss"]):
        assert np.isnan(r.loss) and np.isnan(r.gZ).all() and np.isnan(c["grad"]).all()
        return
    assert abs(r.loss - c["loss"]) <= 1e-12 * abs(c["loss"])
    assert np.linalg.norm(r.gZ - c["grad"]) <= 1e-12 * np.linalg.norm(c["grad"])
    # row_loss in the reference's order averages to the loss; stats are self-consistent
    assert abs(r.row_loss.mean() - r.loss) <= 1e-12 * abs(r.loss)
    assert np.allclose(np.exp(-r.stats[:, 1]), r.stats[:, 3], rtol=1e-12)


@pytest.mark.parametrize("path", FIXTURES, ids=NAMES)
def test_torch_yardstick_matches_fixture(path):
    c = load(path)
    x = torch.from_numpy(c["f"]).double().requires_grad_(True)
    y = None if c["y"] is None else torch.from_numpy(c["y"])
    loss = losses.supcon_loss_torch(x, y, temperature=c["T"], base_temperature=c["Tb"],
                                    contrast_mode=c["mode"])
    loss.backward()
    if np.isnan(c["loss"]):
        assert torch.isnan(loss) and torch.isnan(x.grad).all()
        return
    assert abs(loss.item() - c["loss"]) <= 1e-12 * abs(c["loss"])
    assert np.linalg.norm(x.grad.numpy() - c["grad"]) <= 1e-12 * np.linalg.norm(c["grad"])


def test_torch_yardstick_mask_is_the_label_mask():
    rng = np.random.default_rng(5)
    f = torch.from_numpy(rng.standard_normal((9, 2, 7)))
    y = torch.from_numpy(rng.integers(0, 3, 9))
    mask = (y[:, None] == y[None, :]).double()
    a = losses.supcon_loss_torch(f, y)
    b = losses.supcon_loss_torch(f, mask=mask)
    assert abs(a.item() - b.item()) <= 1e-12 * abs(a.item())
    with pytest.raises(ValueError):
        losses.supcon_loss_torch(f, y, mask=mask)


@pytest.mark.parametrize("mode,labelled,V", [("all", True, 2), ("one", True, 3), ("all", False, 2),
                                             ("one", False, 2), ("all", True, 1)])
def test_reference_gradient_against_finite_differences(mode, labelled, V):
    rng = np.random.default_rng(11)
    bsz, d = 8, 5
    f = rng.standard_normal((bsz, V, d))
    f /= np.linalg.norm(f, axis=-1, keepdims=True)
    y = (np.arange(bsz) % 3) if labelled else None
    T, Tb = 0.3, 0.07
    r = S.supcon(f, y, T, Tb, mode, gl=1.0)
    idx = rng.choice(f.size, 12, replace=False)
    fd = S.finite_difference(f, y, T, Tb, mode, idx)
    g = r.gZ.reshape(-1)[idx]
    assert np.abs(fd - g).max() <= 1e-7 * max(1.0, np.abs(g).max())
    # and gl scales it
    assert np.allclose(S.supcon(f, y, T, Tb, mode, gl=-2.5).gZ, -2.5 * r.gZ, rtol=1e-14, atol=0)


def test_nan_propagation_of_a_singleton_label():
    c = load([p for p in FIXTURES if p.endswith("supcon_c0_v1.npz")][0])
    r = S.supcon(c["f"], c["y"], c["T"], c["Tb"], c["mode"])
    lone = np.flatnonzero(r.stats[:, 2] == 0)
    assert len(lone) == 1
    assert np.isnan(r.loss) and np.isnan(r.gZ).all()
    rl = r.row_loss
    assert np.isnan(rl[lone]).all() and np.isfinite(np.delete(rl, lone)).all()


def test_bound_is_small_and_covers_a_float32_evaluation():
    """The bound is an honest fp32 bound: the closed form evaluated in float32 numpy (another
    summation order, the same number format) lies inside it, and it stays far below the loss."""
    c = load([p for p in FIXTURES if p.endswith("supcon_all_lab_v2.npz")][0])
    r = S.supcon(c["f"], c["y"], c["T"], c["Tb"], c["mode"])
    b = S.bound(c["f"], c["y"], c["T"], c["Tb"], c["mode"])
    assert b.loss < 1e-3 * abs(r.loss) and (b.row_loss < 1e-2).all()
    assert c["e_loss"] <= b.loss
    f = c["f"]
    Z = f.reshape(-1, f.shape[-1])
    L = (Z @ Z.T) / np.float32(c["T"])
    assert (np.abs(L.astype(np.float64) - (Z.astype(np.float64) @ Z.astype(np.float64).T) / c["T"]).max(1)
            <= b.stats[:, 0]).all()


# ---- host side of the C ABI ----------------------------------------------------------------
NEW = ("gll_supcon_scratch_bytes", "gll_supcon_forward", "gll_supcon_backward", "gll_supcon_launches")


def test_header_and_lib_agree_on_the_new_entry_points():
    src = open(os.path.join(ROOT, "include", "gll.h")).read()
    lib = _lib.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.EXPORTS
        assert hasattr(lib, name)
    assert int(re.search(r"#define GLL_SC_ALL (\d+)", src).group(1)) == _lib.SC_ALL
    assert int(re.search(r"#define GLL_SC_ONE (\d+)", src).group(1)) == _lib.SC_ONE
    assert "losses.py:11-98" in src
    # the argument lists of the header, one ctypes type each
    fwd = re.search(r"int gll_supcon_forward\((.*?)\);", src, re.S).group(1)
    bwd = re.search(r"int gll_supcon_backward\((.*?)\);", src, re.S).group(1)
    assert len(fwd.split(",")) == len(lib.gll_supcon_forward.argtypes) == 13
    assert len(bwd.split(",")) == len(lib.gll_supcon_backward.argtypes) == 13
    # the tile constants mirrored for the tests
    hdr = open(os.path.join(ROOT, "graphlearninglayer_amd", "csrc", "gll_internal.h")).read()
    for cname, val in (("kScTile", _lib.SC_TILE), ("kScKc", _lib.SC_KC), ("kScTargetWg", _lib.SC_TARGET_WG),
                       ("kScTargetWgFwd", _lib.SC_TARGET_WG_FWD),
                       ("kScPartBytes", _lib.SC_PART_BYTES)):
        assert int(re.search(r"constexpr int %s = (\d+);" % cname, hdr).group(1)) == val
    assert _lib.SC_ROWS == _lib.SC_TILE * int(re.search(r"constexpr int kScWaves = (\d+);", hdr).group(1))


def _bufs():
    keep = [(ct.c_double * 64)() for _ in range(8)]
    return keep, [ct.addressof(k) for k in keep]


def test_bad_arguments_are_rejected_before_any_launch():
    lib = _lib.lib()
    keep, (Z, y, loss, rl, st, sc, gl, gZ) = _bufs()
    INV, UNS = -1, -2
    before = lib.gll_supcon_launches()

    def fwd(rows=8, V=2, d=4, Z=Z, y=y, mode=0, T=0.07, Tb=0.07, loss=loss, rl=rl, st=st, sc=sc):
        return lib.gll_supcon_forward(rows, V, d, Z, y, mode, T, Tb, loss, rl, st, sc, None)

    def bwd(rows=8, V=2, d=4, Z=Z, y=y, mode=0, T=0.07, Tb=0.07, st=st, gl=gl, gZ=gZ, sc=sc):
        return lib.gll_supcon_backward(rows, V, d, Z, y, mode, T, Tb, st, gl, gZ, sc, None)

    for f in (fwd, bwd):
        assert f(Z=None) == INV and f(st=None) == INV and f(sc=None) == INV
        assert f(mode=2) == INV and f(mode=-1) == INV
        for bad in (0.0, -0.07, float("inf"), float("nan")):
            assert f(T=bad) == INV and f(Tb=bad) == INV
        assert f(rows=9, V=2) == INV and f(V=0) == INV and f(rows=1, V=1) == INV and f(d=0) == INV
        assert f(rows=65536 + 2) == UNS and f(d=4097) == UNS
        assert f(Z=Z + 2) == INV and f(sc=sc + 4) == INV
    assert fwd(loss=None) == INV and bwd(gl=None) == INV and bwd(gZ=None) == INV
    assert lib.gll_supcon_launches() == before
    assert lib.gll_supcon_scratch_bytes(1, 4) == 0 and lib.gll_supcon_scratch_bytes(8, 0) == 0
    assert lib.gll_supcon_scratch_bytes(65537, 4) == 0 and lib.gll_supcon_scratch_bytes(8, 4097) == 0


def test_scratch_is_never_rows_by_rows_and_linear_in_rows_per_chunk():
    lib = _lib.lib()
    for d in (1, 33, 128, 130, 512, 4096):
        for R in (2, 6, 74, 150, 512, 1024, 1300, 2500, 4096, 30000, 65536):
            ntiles, rowblocks, chunks, tpc, fchunks, ftpc = _lib.supcon_plan(R, d)
            nb = lib.gll_supcon_scratch_bytes(R, d)
            # linear in R per chunk; one backward chunk keeps no gZ partials
            assert nb == R * (fchunks * _lib.SC_PART_BYTES + (chunks * 4 * d if chunks > 1 else 0)), (R, d)
            assert 1 <= chunks <= ntiles and (chunks - 1) * tpc < ntiles <= chunks * tpc
            assert chunks <= fchunks <= ntiles and (fchunks - 1) * ftpc < ntiles <= fchunks * ftpc
            if R >= 1024:
                assert nb < 4 * R * R, (R, d)
    # the flagship shape: most CUs get a workgroup, the scratch stays well under R x R floats
    ntiles, rowblocks, chunks, tpc, fchunks, ftpc = _lib.supcon_plan(2500, 128)
    assert rowblocks * chunks >= 256 and rowblocks * fchunks >= 512
    assert chunks * 2500 * 4 * 128 <= 2 * 2500 * 2500 < lib.gll_supcon_scratch_bytes(2500, 128) + 2 * 2500 * 2500
    ntiles, rowblocks, chunks, tpc, fchunks, ftpc = _lib.supcon_plan(512, 128)
    assert rowblocks * chunks >= 64 and rowblocks * fchunks >= 128


def test_python_argument_handling_mirrors_the_reference():
    f = torch.zeros(4, 2, 3)
    crit = losses.SupConLoss()
    with pytest.raises(ValueError):
        crit(torch.zeros(4, 6))
    with pytest.raises(ValueError):
        crit(f, torch.zeros(5, dtype=torch.int64))
    with pytest.raises(ValueError):
        crit(f, torch.zeros(4, dtype=torch.int64), torch.eye(4))
    with pytest.raises(NotImplementedError, match="supcon_loss_torch"):
        crit(f, mask=torch.eye(4))
    with pytest.raises(ValueError):
        losses.supcon_loss(f, contrast_mode="some")
    with pytest.raises(TypeError):
        losses.supcon_loss(f, normalize=1)
    import graphlearninglayer_amd as pkg
    assert pkg.SupConLoss is losses.SupConLoss and pkg.supcon_loss is losses.supcon_loss
