"""The fused SupCon / SimCLR loss on the GPU (supcon.hip): both kernels against
the float64 stage reference within its derived fp32 bound (tests/supcon_ref.py), against the
fixtures of the reference's losses.py within 8x the reference's own float32 error, against the
plain-torch yardstick, bitwise repeatability, the Python front ends, the launch budget and the
memory contract (never an R x R array).  Shapes come from the kernel's tile constants."""
import functools
import glob
import json
import os

import numpy as np
import pytest
import torch

from tests import abi as A
from tests import supcon_ref as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "supcon", "supcon_*.npz")))
FIXNAMES = [os.path.basename(p)[len("supcon_"):-len(".npz")] for p in FIXTURES]
PARITY = {}


def _L():
    from graphlearninglayer_amd import _lib
    return _lib


def _M():
    from graphlearninglayer_amd import losses
    return losses


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    A.need_gpu()
    yield
    try:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "sn01_parity.json"), "w") as fh:
            json.dump(PARITY, fh, indent=1, sort_keys=True)
    except OSError:
        pass


from graphlearninglayer_amd._lib import SC_KC, SC_ROWS, SC_TILE, supcon_plan  # noqa: E402

# R = 150: three row blocks of SC_ROWS, five column tiles of SC_TILE in five chunks, a multiple of
# neither; R = 1500: backward chunks of three tiles, forward chunks of two (the in-chunk running
# maximum and the longer chain); R = 6: less than one tile, one chunk (the backward writes gZ itself).  d around SC_KC: one feature
# stage, two (130), three with 16-B loads (300); 1, 5, 33, 130: scalar loads and zero fill.
MULTI = 75            # bsz at V = 2
assert MULTI * 2 > 2 * SC_ROWS and (MULTI * 2) % SC_TILE and supcon_plan(MULTI * 2, 128)[2] >= 2
assert supcon_plan(1500, 33)[3] >= 2 and supcon_plan(1500, 33)[5] >= 2 and supcon_plan(6, 5)[2] == 1
assert SC_KC == 128
# name: bsz, V, d, mode, labels ('y' classes, None SimCLR, 'wild' negative and huge int64), T, Tb
CASES = {
    "d1": (MULTI, 2, 1, "all", "y", 0.07, 0.07),
    "d5": (MULTI, 2, 5, "all", "y", 0.07, 0.07),
    "d33": (MULTI, 2, 33, "all", "y", 0.07, 0.07),
    "d128": (MULTI, 2, 128, "all", "y", 0.07, 0.07),
    "d130": (MULTI, 2, 130, "all", "y", 0.07, 0.07),
    "d300_one": (MULTI, 2, 300, "one", "y", 0.5, 0.07),
    "v3_one": (50, 3, 33, "one", "y", 0.07, 0.07),
    "v3_all_simclr": (50, 3, 128, "all", None, 0.5, 0.07),
    "v1_all": (2 * MULTI, 1, 128, "all", "y", 0.07, 0.07),
    "v1_one": (2 * MULTI, 1, 5, "one", "y", 0.07, 0.07),
    "tiny_simclr": (3, 2, 5, "all", None, 0.07, 0.07),
    "tiny_one": (3, 2, 128, "one", "y", 0.07, 0.07),
    "simclr_all": (MULTI, 2, 128, "all", None, 0.07, 0.07),
    "simclr_one": (MULTI, 2, 33, "one", None, 0.07, 0.07),
    "wild_labels": (MULTI, 2, 33, "all", "wild", 0.07, 0.07),
    "chunks_of_3": (750, 2, 33, "all", "y", 0.07, 0.07),
}
GL = -1.75   # incoming gradient of the loss (exact in fp32)


def _inputs(bsz, V, d, labels, seed):
    rng = np.random.default_rng(seed)
    f = rng.standard_normal((bsz, V, d))
    y = None
    if labels is not None:
        y = (np.arange(bsz) % 7).astype(np.int64)
        rng.shuffle(y)
        f += 1.5 * rng.standard_normal((7, 1, d))[y]
        if labels == "wild":
            y = np.array([-2 ** 63, -1, 2 ** 63 - 1, 0, 2 ** 40 + 1, -2 ** 40, 7], dtype=np.int64)[y]
    f = (f / np.maximum(np.linalg.norm(f, axis=-1, keepdims=True), 1e-12)).astype(np.float32)
    return f, y


@functools.lru_cache(maxsize=None)
def _case(name):
    """Inputs, float64 reference and bound of a case: computed once, shared, never modified."""
    bsz, V, d, mode, labels, T, Tb = CASES[name]
    f, y = _inputs(bsz, V, d, labels, 4200 + sorted(CASES).index(name))
    return (f, y, T, Tb, mode) + _ref_and_bound(f, y, T, Tb, mode)


def _ref_and_bound(f, y, T, Tb, mode):
    R, d = f.shape[0] * f.shape[1], f.shape[2]
    _, _, _, tpc, fchunks, ftpc = supcon_plan(R, d)
    ref = S.supcon(f, y, T, Tb, mode, gl=GL)
    bnd = S.bound(f, y, T, Tb, mode, gl=GL, chain=SC_TILE * tpc + 2, nresc=ftpc + 1 + fchunks)
    return ref, bnd


def _raw(f, y, T, Tb, mode, gl=GL):
    """The two C entry points on device arrays: loss (float64), row_loss, stats, gZ."""
    _lib = _L()
    lib = _lib.lib()
    dev = torch.device("cuda", 0)
    Z = f if torch.is_tensor(f) else torch.from_numpy(f).to(dev)
    bsz, V, d = Z.shape
    R = bsz * V
    lab = None if y is None else torch.from_numpy(y).to(dev)
    code = {"all": _lib.SC_ALL, "one": _lib.SC_ONE}[mode]
    A = R if mode == "all" else bsz
    loss = torch.full((), -7.0, dtype=torch.float64, device=dev)
    rl = torch.full((A,), -7.0, dtype=torch.float32, device=dev)
    st = torch.full((R, 4), -7.0, dtype=torch.float32, device=dev)
    gZ = torch.full((bsz, V, d), -7.0, dtype=torch.float32, device=dev)
    glt = torch.full((), gl, dtype=torch.float64, device=dev)
    nb = lib.gll_supcon_scratch_bytes(R, d)
    assert nb > 0
    scratch = torch.empty(nb, dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    lp = None if lab is None else lab.data_ptr()
    _lib.check(lib.gll_supcon_forward(R, V, d, Z.data_ptr(), lp, code, T, Tb, loss.data_ptr(),
                                      rl.data_ptr(), st.data_ptr(), scratch.data_ptr(), s), "forward")
    _lib.check(lib.gll_supcon_backward(R, V, d, Z.data_ptr(), lp, code, T, Tb, st.data_ptr(),
                                       glt.data_ptr(), gZ.data_ptr(), scratch.data_ptr(), s), "backward")
    torch.cuda.synchronize()
    return loss.item(), rl.cpu().numpy().astype(np.float64), st.cpu().numpy().astype(np.float64), \
        gZ.cpu().numpy().astype(np.float64)


def _within(got, ref, bnd, what):
    got, ref, bnd = np.asarray(got), np.asarray(ref), np.asarray(bnd)
    assert np.isfinite(got).all(), what
    over = np.abs(got - ref) - bnd
    assert (over <= 0).all(), (what, float(over.max()), float(np.abs(got - ref).max()), float(bnd.max()))
    return float((np.abs(got - ref) / np.maximum(bnd, 1e-300)).max())


def _check_against(name, f, y, T, Tb, mode, ref, bnd):
    loss, rl, st, gZ = _raw(f, y, T, Tb, mode)
    out = {
        "loss_abs_err": abs(loss - ref.loss), "loss_bound": bnd.loss,
        "row_loss_err_over_bound": _within(rl, ref.row_loss, bnd.row_loss, "row_loss"),
        "stats_err_over_bound": _within(st, ref.stats, np.maximum(bnd.stats, 0.0), "stats"),
        "gZ_err_over_bound": _within(gZ, ref.gZ, bnd.gZ, "gZ"),
        "gZ_rel_fro": float(np.linalg.norm(gZ - ref.gZ) / np.linalg.norm(ref.gZ)),
    }
    assert (st[:, 2] == ref.stats[:, 2]).all()   # the positive count is exact
    assert abs(loss - ref.loss) <= bnd.loss, out
    print(name, out)
    PARITY[name] = out
    return loss, gZ


@pytest.mark.parametrize("name", sorted(CASES))
def test_kernels_against_float64_reference(name):
    f, y, T, Tb, mode, ref, bnd = _case(name)
    _check_against(name, f, y, T, Tb, mode, ref, bnd)


@pytest.mark.parametrize("path", FIXTURES, ids=FIXNAMES)
def test_fixtures_of_the_reference(path):
    z = np.load(path)
    f, y = z["features"], (z["labels"] if "labels" in z else None)
    T, Tb, mode = float(z["T"]), float(z["Tb"]), str(z["mode"])
    if np.isnan(float(z["loss64"])):
        loss, rl, st, gZ = _raw(f, y, T, Tb, mode, gl=1.0)
        assert np.isnan(loss) and np.isnan(gZ).all()
        return
    ref, bnd = _ref_and_bound(f, y, T, Tb, mode)
    loss, gZ = _check_against("fixture_" + os.path.basename(path)[7:-4], f, y, T, Tb, mode, ref, bnd)
    # the reference's own autograd gradient (for grad_loss = 1) and its own float32 error
    g64 = GL * z["grad64"]
    rel = float(np.linalg.norm(gZ - g64) / np.linalg.norm(g64))
    own = float(z["ref32_grad_relerr"])
    print("fixture", os.path.basename(path), "gZ rel err", rel, "reference fp32", own,
          "loss err", abs(loss - float(z["loss64"])), "reference fp32", float(z["ref32_loss_err"]))
    PARITY["fixture_" + os.path.basename(path)[7:-4]].update(gZ_rel_vs_reference=rel, reference_fp32_rel=own)
    assert rel <= 8 * own
    assert abs(loss - float(z["loss64"])) <= bnd.loss


@pytest.mark.parametrize("name", ["d33", "d130", "v3_one", "simclr_all", "tiny_one", "v1_all"])
def test_python_front_end_against_torch_yardstick_and_reference(name):
    """supcon_loss and its autograd against supcon_loss_torch in float64 on the device (a wrong
    closed form would show here, not a wrong kernel), the same bounds; two calls bitwise equal;
    the module equals the function."""
    M = _M()
    f, y, T, Tb, mode, ref, bnd = _case(name)
    dev = torch.device("cuda", 0)
    yt = None if y is None else torch.from_numpy(y).to(dev)

    def ours(fn):
        x = torch.from_numpy(f).to(dev).requires_grad_(True)
        loss = fn(x)
        (loss * GL).backward()
        return loss.detach(), x.grad

    l1, g1 = ours(lambda x: M.supcon_loss(x, yt, T, Tb, mode))
    l2, g2 = ours(lambda x: M.supcon_loss(x, yt, T, Tb, mode))
    l3, g3 = ours(lambda x: M.SupConLoss(T, mode, Tb)(x, yt))
    assert l1.dtype == torch.float32 and l1.dim() == 0 and l1.device.type == "cuda"
    assert torch.equal(l1, l2) and torch.equal(g1, g2) and torch.equal(l1, l3) and torch.equal(g1, g3)
    x64 = torch.from_numpy(f).to(dev).double().requires_grad_(True)
    lt = M.supcon_loss_torch(x64, yt, temperature=T, base_temperature=Tb, contrast_mode=mode)
    (lt * GL).backward()
    assert abs(l1.item() - lt.item()) <= bnd.loss
    assert abs(l1.item() - ref.loss) <= bnd.loss
    _within(g1.cpu().numpy().astype(np.float64), x64.grad.cpu().numpy(), bnd.gZ, "gZ vs torch float64")
    _within(g1.cpu().numpy().astype(np.float64), ref.gZ, bnd.gZ, "gZ vs reference")
    # return_rows: the anchors' losses in the reference's order, not differentiable
    lr, rows = M.supcon_loss(torch.from_numpy(f).to(dev).requires_grad_(True), yt, T, Tb, mode,
                             return_rows=True)
    assert not rows.requires_grad and torch.equal(lr, l1)
    _within(rows.cpu().numpy().astype(np.float64), ref.row_loss, bnd.row_loss, "row_loss")


def test_default_module_and_higher_rank_features():
    M = _M()
    dev = torch.device("cuda", 0)
    f, y, *_ = _case("d128")
    yt = torch.from_numpy(y).to(dev)
    x = torch.from_numpy(f).to(dev)
    a = M.SupConLoss()(x, yt)
    b = M.supcon_loss(x, yt)
    c = M.SupConLoss()(x.view(x.shape[0], 2, 8, 16), yt)     # flattened to [bsz, V, -1]
    assert torch.equal(a, b) and torch.equal(a, c)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_normalize_is_the_front_end_around_the_loss(dtype):
    from graphlearninglayer_amd import GLL
    M, lib = _M(), _L().lib()
    dev = torch.device("cuda", 0)
    f, y, T, Tb, mode, *_ = _case("d130")
    yt = torch.from_numpy(y).to(dev)
    raw = (torch.from_numpy(f).to(dev) * 3.5).to(dtype)
    x = raw.clone().requires_grad_(True)
    n0, u0 = lib.gll_supcon_launches(), lib.gll_features_calls()
    loss = M.supcon_loss(x, yt, T, Tb, mode, normalize=True)
    n1, u1 = lib.gll_supcon_launches(), lib.gll_features_calls()
    (loss * GL).backward()
    n2, u2 = lib.gll_supcon_launches(), lib.gll_features_calls()
    assert n1 - n0 <= 2 and u1 - u0 == 1 and n2 - n1 <= 2 and u2 - u1 == 1
    assert x.grad.dtype == dtype and x.grad.shape == x.shape
    Xh, rnorm = GLL.unit_features(raw)
    xs = Xh.clone().requires_grad_(True)
    stage = M.supcon_loss(xs, yt, T, Tb, mode)
    (stage * GL).backward()
    assert torch.equal(loss, stage)
    assert torch.equal(x.grad, GLL.unit_features_backward(xs.grad, Xh, rnorm, dtype))
    if dtype != torch.float32:    # half precision without normalize: the same front end, no norm
        x2 = Xh.to(dtype).requires_grad_(True)
        l2 = M.supcon_loss(x2, yt, T, Tb, mode)
        (l2 * GL).backward()
        x3 = x2.detach().float().requires_grad_(True)
        l3 = M.supcon_loss(x3, yt, T, Tb, mode)
        (l3 * GL).backward()
        assert x2.grad.dtype == dtype and torch.equal(l2, l3) and torch.equal(x2.grad, x3.grad.to(dtype))


def test_launch_budget_without_normalize():
    M, lib = _M(), _L().lib()
    dev = torch.device("cuda", 0)
    for name in ("d128", "tiny_one"):
        f, y, T, Tb, mode, *_ = _case(name)
        x = torch.from_numpy(f).to(dev).requires_grad_(True)
        n0, u0 = lib.gll_supcon_launches(), lib.gll_features_calls()
        loss = M.supcon_loss(x, torch.from_numpy(y).to(dev), T, Tb, mode)
        n1 = lib.gll_supcon_launches()
        loss.backward()
        n2, u2 = lib.gll_supcon_launches(), lib.gll_features_calls()
        assert 1 <= n1 - n0 <= 2 and 1 <= n2 - n1 <= 2 and u2 == u0


def test_misaligned_view_gives_the_aligned_result_bitwise():
    M = _M()
    dev = torch.device("cuda", 0)
    f, y, T, Tb, mode, *_ = _case("d128")
    yt = torch.from_numpy(y).to(dev)
    a = torch.from_numpy(f).to(dev).requires_grad_(True)
    buf = torch.zeros(f.size + 1, dtype=torch.float32, device=dev)
    buf[1:] = a.detach().reshape(-1)
    v = buf[1:].view(f.shape).requires_grad_(True)       # 4 B past a 16-B boundary: scalar loads
    assert a.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 4 and v.is_contiguous()
    la = M.supcon_loss(a, yt, T, Tb, mode)
    la.backward()
    lv = M.supcon_loss(v, yt, T, Tb, mode)
    lv.backward()
    assert torch.equal(la, lv) and torch.equal(a.grad, v.grad)


def test_singleton_label_gives_nan_loss_and_all_nan_gradient():
    M = _M()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(3)
    f = rng.standard_normal((8, 1, 5)).astype(np.float32)
    f /= np.linalg.norm(f, axis=-1, keepdims=True)
    y = torch.tensor([0, 0, 1, 1, 1, 2, 0, 1], device=dev)     # label 2 is alone: c_r = 0
    x = torch.from_numpy(f).to(dev).requires_grad_(True)
    loss = M.supcon_loss(x, y)
    loss.backward()
    assert torch.isnan(loss) and torch.isnan(x.grad).all()


def test_argument_errors_on_the_device():
    M = _M()
    dev = torch.device("cuda", 0)
    f = torch.zeros(4, 2, 3, device=dev)
    y = torch.zeros(4, dtype=torch.int64, device=dev)
    with pytest.raises(NotImplementedError, match="supcon_loss_torch"):
        M.SupConLoss()(f, mask=torch.eye(4, device=dev))
    with pytest.raises(ValueError):
        M.SupConLoss()(f.view(4, 6))
    with pytest.raises(ValueError):
        M.SupConLoss()(f, y[:3])
    with pytest.raises(ValueError):
        M.SupConLoss()(f, y, torch.eye(4, device=dev))
    with pytest.raises(ValueError):
        M.SupConLoss(contrast_mode="two")(f, y)
    with pytest.raises(TypeError):
        M.supcon_loss(f.double(), y)


def test_no_rows_by_rows_allocation_at_the_reference_batch():
    """A step at the reference's batch (1,250 samples x 2 views, d = 128) allocates less than one
    R x R float array above its inputs; the plain-torch form needs several."""
    M = _M()
    dev = torch.device("cuda", 0)
    bsz, V, d = 1250, 2, 128
    R = bsz * V
    g = torch.Generator(device="cpu").manual_seed(9)
    x = torch.nn.functional.normalize(torch.randn(bsz, V, d, generator=g), dim=-1).to(dev).requires_grad_(True)
    y = (torch.arange(bsz) % 10).to(dev)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    loss = M.supcon_loss(x, y)
    loss.backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - base
    print("peak bytes above the inputs", peak, "R x R floats", 4 * R * R)
    PARITY["memory_R2500_d128"] = {"peak_bytes_above_inputs": int(peak), "rows_by_rows_bytes": 4 * R * R}
    assert peak < 4 * R * R
    assert torch.isfinite(loss) and torch.isfinite(x.grad).all()
