"""Where the fused backward's last gradient waves spend their time (diagnostic, GPU box).

Loads the timestamp build (tools/libgll_trace.so.trace, a copy of _obj/libgll_trace.so made by
`python -m graphlearninglayer_amd.build --trace`; TRACE_LIB names another), runs NS forward +
backward through the C ABI and reads, per gradient wave of cg_grad_fused_kernel, the
s_memrealtime (100 MHz) stamps of: release seen, w loaded (+ first coefficients), products done,
stored; plus the row, its length and the wave's CU / XCC.  A row may run as several waves (parts
of its feature range, fused_bwd.hip): a row's times are those of its last part to store.  Prints the
distribution of each phase after the release, the slowest rows, the maximum stored time by row
length, and the adjoint solves' last exit (which the gradient waves' polling must not move).

TRACE_SPLIT = 0 / 1 / 2 sets GLL_KNOB_GRAD_SPLIT (automatic / on / off) where the library has it.
A library from before the row parts stamps one wave per row, indexed by row: read the same way.

Limits of the timestamp build: 4,096 stamp entries (one per wave that holds an item) and 12 bits
of row index, so n <= 2,048 here (every bench config with a fused backward is below it); the
"first release" and block checkpoints are those of the first gradient workgroup's wave 0.
"""
import ctypes as ct
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from graphlearninglayer_amd import GLL  # noqa: E402
from graphlearninglayer_amd.synth import CONFIGS, one_hot, seeded_gbar, synth  # noqa: E402

_tl = os.environ.get("TRACE_LIB", os.path.join(ROOT, "tools", "libgll_trace.so.trace"))
lib = ct.CDLL(_tl if os.path.exists(_tl) else
              os.path.join(ROOT, "graphlearninglayer_amd", "_obj", "libgll_trace.so"))
lib.gll_workspace_bytes.restype = ct.c_size_t
lib.gll_trace_read_fz.argtypes = [ct.POINTER(ct.c_ulonglong)]
lib.gll_trace_read.argtypes = [ct.c_int, ct.POINTER(ct.c_ulonglong)]
KNOB_GRAD_SPLIT = 6
if "TRACE_SPLIT" in os.environ:
    if lib.gll_set_knob(KNOB_GRAD_SPLIT, int(os.environ["TRACE_SPLIT"])) != 0:
        print("this library has no GLL_KNOB_GRAD_SPLIT: TRACE_SPLIT ignored")
c = CONFIGS[os.environ.get("TRACE_CFG", "ns")]
n, base, d, k = c["base"] + c["batch"], c["base"], c["d"], c["k"]
assert n <= 2048, f"n = {n}: the timestamp build holds 4,096 wave stamps and 12-bit row indices"
dev = torch.device("cuda", 0)
X_np, lab = synth(base, n - base, d, r=c["r"], seed=0)
X = torch.from_numpy(X_np).to(dev)
Y = torch.from_numpy(one_hot(lab[:base])).to(dev)
g = torch.from_numpy(seeded_gbar(n - base, 10)).to(dev)
prob = GLL.make_problem(n, d, base, 10, k, 0.07, 1.0)
ws = torch.empty(lib.gll_workspace_bytes(ct.byref(prob)), dtype=torch.uint8, device=dev)
U = torch.empty(n - base, 10, dtype=torch.float64, device=dev)
gx = torch.empty(n, d, dtype=torch.float32, device=dev)
s = ct.c_void_p(torch.cuda.current_stream().cuda_stream)
vp = ct.c_void_p
EB = 16 if d <= 512 else 8   # neighbour rows a whole-row wave holds (fused_bwd.hip)
BINS = [(0, 16), (17, 32), (33, 64), (65, 1 << 30)]


def fwd():
    assert lib.gll_forward(ct.byref(prob), vp(X.data_ptr()), vp(Y.data_ptr()), 0,
                           vp(ws.data_ptr()), vp(U.data_ptr()), s) == 0


def bwd():
    assert lib.gll_backward(ct.byref(prob), vp(X.data_ptr()), vp(Y.data_ptr()), 0,
                            vp(ws.data_ptr()), vp(g.data_ptr()), 1, vp(gx.data_ptr()), s) == 0


def read_rows():
    """Per row: (release, w, products, stored) of its last part to store, length, cu, xcc, parts."""
    buf = (ct.c_ulonglong * (5 * 4096))()
    lib.gll_trace_read_fz(buf)
    a = np.array(buf[:], dtype=np.uint64).reshape(5, 4096)
    info = a[4]
    if np.any(info >> np.uint64(63)):   # one entry per wave (item), the row in the info word
        it = np.nonzero(info >> np.uint64(63))[0]
        row = ((info[it] >> np.uint64(48)) & np.uint64(0xFFF)).astype(np.int64)
    else:                               # one wave per row, indexed by row
        it = np.arange(n)
        row = np.arange(n)
    t = a[:4, it].astype(np.int64)
    inf = info[it].astype(np.uint64)
    parts = np.bincount(row, minlength=n)
    assert parts.min() >= 1, "a row without a stamp"
    last = np.full(n, -1)
    for j in np.argsort(t[3], kind="stable"):   # ascending stored time: the last part wins
        last[row[j]] = j
    t = t[:, last]
    inf = inf[last]
    L = (inf & np.uint64(0xFFFF)).astype(np.int64)
    cu = ((inf >> np.uint64(16)) & np.uint64(0xFFFF)).astype(np.int64)
    xcc = ((inf >> np.uint64(40)) & np.uint64(0xFF)).astype(np.int64)
    return t, L, cu, xcc, parts


for _ in range(20):
    fwd()
    bwd()
torch.cuda.synchronize()
tails = []
for rep in range(5):
    fwd()
    torch.cuda.synchronize()
    lib.gll_trace_reset(2)
    bwd()
    torch.cuda.synchronize()
    (rel, wld, fma, sto), L, cu, xcc, parts = read_rows()
    t0 = rel.min()
    ph = {"release seen": rel - t0, "w loaded": wld - t0, "products done": fma - t0,
          "stored": sto - t0}
    print(f"--- rep {rep}: us after the first wave saw the release (n = {n} rows, "
          f"{int(parts.sum())} waves)")
    for nm, v in ph.items():
        q = np.percentile(v, [0, 50, 90, 99, 100]) * 0.01
        print(f"  {nm:14s} min {q[0]:5.2f} p50 {q[1]:5.2f} p90 {q[2]:5.2f} p99 {q[3]:5.2f} max {q[4]:5.2f}")
    dw = (wld - rel) * 0.01
    df = (fma - wld) * 0.01
    ds = (sto - fma) * 0.01
    print(f"  per row: release->w {np.median(dw):.2f} (max {dw.max():.2f}), w->products "
          f"{np.median(df):.2f} (max {df.max():.2f}), products->stored {np.median(ds):.2f} "
          f"(max {ds.max():.2f})")
    slow = np.argsort(sto)[-8:]
    print("  slowest rows (row, len, parts, xcc, cu, release, w, products, stored):")
    for i in slow[::-1]:
        print(f"    {i:5d} {L[i]:3d} {parts[i]:1d} {xcc[i]:2d} {cu[i]:5x} {0.01 * (rel[i] - t0):6.2f} "
              f"{0.01 * (wld[i] - t0):6.2f} {0.01 * (fma[i] - t0):6.2f} {0.01 * (sto[i] - t0):6.2f}")
    by_x = [0.01 * np.median(sto[xcc == x] - t0) for x in range(8) if np.any(xcc == x)]
    print("  median stored time by XCC: " + " ".join(f"{v:.2f}" for v in by_x))
    cor = np.corrcoef(L, sto)[0, 1]
    print(f"  corr(row length, stored time) {cor:.2f}; rows > 16 edges: {int((L > 16).sum())}")
    mx = []
    for lo, hi in BINS:
        sel = (L >= lo) & (L <= hi)
        mx.append(0.01 * (sto[sel] - t0).max() if sel.any() else float("nan"))
        nm = f"<= {hi}" if lo == 0 else (f"> {lo - 1}" if hi > 1 << 20 else f"{lo}-{hi}")
        print(f"  max stored, rows of {nm:6s} edges: {mx[-1]:5.2f}  ({int(sel.sum())} rows)")
    late = int((np.minimum(L, 64) > EB * parts).sum())
    print(f"  rows in parts: {int((parts > 1).sum())} (2 parts {int((parts == 2).sum())}, 4 parts "
          f"{int((parts == 4).sum())}); rows that fetch x_j after the release: {late}")
    tail = 0.01 * (sto - t0).max() - mx[0]
    tails.append(tail)
    print(f"  tail (max stored over all rows - max stored over rows of <= 16 edges): {tail:.2f}")
    buf = (ct.c_ulonglong * 64)()
    lib.gll_trace_read(6, buf)   # trace unit 6: fused_bwd.hip
    fz = np.array(buf[:], dtype=np.uint64).astype(np.int64)
    if fz[16] and 0 < fz[32] < 2 ** 62:
        print(f"  us from the first CG entry: last CG exit +{0.01 * (fz[33] - fz[32]):.2f}, first "
              f"release seen +{0.01 * (t0 - fz[32]):.2f}, last grad exit +{0.01 * (fz[19] - fz[32]):.2f}")
print(f"tail over the {len(tails)} repetitions: " + " ".join(f"{v:.2f}" for v in tails) +
      f"  (mean {np.mean(tails):.2f})")
