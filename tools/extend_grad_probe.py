"""A/B of the differentiable out-of-sample extension (GPU only: fails without a device).

    grad   A : GLL.extend_torch on the lists of GLL.knn_query + backward  (plain PyTorch, float32)
           B : GLL.extend + backward                  (query.hip + extend_grad.hip)
           at the evaluation shape Q = 10,000, N = 50,250, d = 128, k = 50 and at the minibatch
           shape Q = 1,250, N = 250, d = 128, k = 25, each with only Xq requiring grad (one backward
           launch) and with Xq, Xdb, P and epsilon requiring grad (six).  A is handed its lists: the
           kNN search is outside its time and inside B's.
    step   A : ce_loss + backward at the FullySup shape (250 labeled + 1,250 rows, d 128, k 25): a
               graph build, two solves and the fused backward per step
           B : the memory-bank step: the 1,250 rows as queries against the 250 labeled rows and
               their one-hot predictions (detached), knn_query + extend + custom_ce_loss + backward
               to the queries: no graph build and no solve.

Every route is warmed up, then timed in alternating windows of at least --window seconds (a host
clock around a device synchronise), --rounds rounds in one process; the report gives each route's
median and spread (min .. max) over its windows.

    python tools/extend_grad_probe.py [--rounds 5] [--window 0.5] [--what grad step] [--out FILE]

Kernel lists (a separate run, the tracer slows the host):

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- \
        python tools/extend_grad_probe.py --trace all --calls 5

runs `--calls` extend + backward calls at the evaluation shape (after 2 warm-up calls, counted
too) with Xq alone (`xq`) or every input (`all`) requiring grad; `--summarize OUT LABEL=CSV ...
--build ID` turns the kernel_stats.csv files of such runs into the launch summary (no GPU needed).
"""
import argparse
import csv
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from graphlearninglayer_amd import GLL, _lib  # noqa: E402
from graphlearninglayer_amd.synth import CONFIGS, one_hot, synth  # noqa: E402

SHAPES = {"eval": (10_000, 50_250, 128, 50), "minibatch": (1_250, 250, 128, 25)}
EPS, TAU, C = 1.0, 0.07, 10
WARM = 2


def window(step, seconds):
    """Milliseconds per call over a window of at least `seconds`, ended by a synchronise."""
    torch.cuda.synchronize()
    n = 0
    t0 = time.perf_counter()
    while True:
        step()
        n += 1
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return dt / n * 1e3


def alternate(steps, rounds, seconds, emit, tag):
    for _ in range(WARM):
        for s in steps.values():
            s()
    torch.cuda.synchronize()
    t = {k: [] for k in steps}
    for r in range(rounds):
        for k, s in steps.items():
            t[k].append(window(s, seconds))
        emit(f"{tag} round {r}: " + "  ".join(f"{k} {t[k][-1]:9.3f}" for k in steps) + "  ms/call")
    for k, v in t.items():
        emit(f"{tag} {k} median {statistics.median(v):.3f} ms (min {min(v):.3f} .. max {max(v):.3f})")
    return {k: statistics.median(v) for k, v in t.items()}


def tensors(name, everything):
    """Xq, Xdb, P, epsilon of a shape on the device; Xq (or all of them) requiring grad."""
    Q, N, d, k = SHAPES[name]
    X, labels = synth(N, Q, d, C=C, r=1.0, seed=3)
    dev = torch.device("cuda", 0)
    Xdb = torch.from_numpy(X[:N]).to(dev).requires_grad_(everything)
    Xq = torch.from_numpy(X[N:]).to(dev).requires_grad_(True)
    P = torch.from_numpy(one_hot(labels[:N], C)).to(dev)
    P = (0.9 * P + 0.01).requires_grad_(everything)
    eps = torch.tensor(EPS, device=dev, requires_grad=True) if everything else EPS
    gU = torch.from_numpy(np.random.default_rng(1).standard_normal((Q, C))).to(dev)
    return Xq, Xdb, P, eps, gU, k


def clear(*ts):
    for t in ts:
        if torch.is_tensor(t):
            t.grad = None


def grad_ab(name, everything, rounds, seconds, emit):
    Xq, Xdb, P, eps, gU, k = tensors(name, everything)
    idx = GLL.knn_query(Xq, Xdb, k - 1)[0]
    g32 = gU.float()
    tag = f"[grad {name} {'all' if everything else 'Xq'}]"

    def a():
        clear(Xq, Xdb, P, eps)
        (GLL.extend_torch(Xq, Xdb, P, idx, eps) * g32).sum().backward()

    def b():
        clear(Xq, Xdb, P, eps)
        (GLL.extend(Xq, Xdb, P, k=k, epsilon=eps)[0] * gU).sum().backward()

    n0 = _lib.lib().gll_extend_grad_launches()
    b()
    n1 = _lib.lib().gll_extend_grad_launches()
    gb = Xq.grad.clone()
    a()
    rel = float((Xq.grad - gb).abs().max() / gb.abs().max())
    Q, N, d, _ = SHAPES[name]
    emit(f"{tag} Q {Q}, N {N}, d {d}, k {k}; backward launches {n1 - n0}; max |gXq(A) - gXq(B)| / "
         f"max |gXq(B)| = {rel:.2e}")
    med = alternate({"A(extend_torch+bwd)": a, "B(extend+bwd)": b}, rounds, seconds, emit, tag)
    emit(f"{tag} A / B = {med['A(extend_torch+bwd)'] / med['B(extend+bwd)']:.2f}x")


def step_ab(rounds, seconds, emit):
    c = CONFIGS["fullysup"]
    X, lab = synth(c["base"], c["batch"], c["d"], r=c["r"], seed=0)
    dev = torch.device("cuda", 0)
    x = torch.from_numpy(X).to(dev).requires_grad_(True)
    Y = torch.from_numpy(one_hot(lab[: c["base"]])).to(dev)
    t = torch.from_numpy(lab[c["base"]:]).to(dev)
    L = GLL.LaplaceLearningSparseHard
    bank, xq = x[: c["base"]].detach().clone(), x[c["base"]:].detach().clone().requires_grad_(True)
    tag = "[step fullysup]"

    def a():
        x.grad = None
        L.ce_loss(x, Y, t, TAU, EPS, c["k"])[0].backward()

    def b():
        xq.grad = None
        GLL.custom_ce_loss(GLL.extend(xq, bank, Y, k=c["k"], epsilon=EPS)[0], t).backward()

    emit(f"{tag} base {c['base']}, batch {c['batch']}, d {c['d']}, k {c['k']}")
    med = alternate({"A(ce_loss+bwd)": a, "B(memory bank)": b}, rounds, seconds, emit, tag)
    emit(f"{tag} A / B = {med['A(ce_loss+bwd)'] / med['B(memory bank)']:.2f}x")


def trace(route, calls):
    Xq, Xdb, P, eps, gU, k = tensors("eval", route == "all")
    for _ in range(WARM + calls):
        clear(Xq, Xdb, P, eps)
        (GLL.extend(Xq, Xdb, P, k=k, epsilon=eps)[0] * gU).sum().backward()
    torch.cuda.synchronize()
    print(f"traced {WARM + calls} extend + backward calls ({route}); build {_lib.build_id()}")


def summarize(out, pairs, calls, build):
    total = WARM + calls
    lines = [f"Kernels of one extend + backward call at Q 10,000, N 50,250, d 128, k 50: rocprofv3 "
             f"--kernel-trace --stats over {total} calls", f"({WARM} warm-up + {calls}) of "
             f"tools/extend_grad_probe.py --trace per run (build {build}).", ""]
    for pair in pairs:
        label, path = pair.split("=", 1)
        with open(path, newline="") as fh:
            rows = [(r["Name"], int(r["Calls"]), float(r["TotalDurationNs"]), float(r["AverageNs"]))
                    for r in csv.DictReader(fh)]
        n = sum(r[1] for r in rows) / total
        ms = sum(r[2] for r in rows) / total / 1e6
        lines.append(f"{label}: {n:.1f} kernel launches per call, {ms:.3f} ms of kernel time per call")
        for name, cnt, _, avg in rows:
            name = name[5:] if name.startswith("void ") else name
            lines.append(f"    {cnt:4d} calls  {avg / 1e3:9.2f} us avg  {name[:100]}")
        lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("\n".join(lines))
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--what", nargs="+", default=["grad", "step"], choices=["grad", "step"])
    ap.add_argument("--trace", choices=("xq", "all"), help="run one route only (under rocprofv3)")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", help="also write the report to this file")
    ap.add_argument("--summarize", nargs="+", metavar=("OUT", "LABEL=CSV"))
    ap.add_argument("--build", default="?")
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize[0], a.summarize[1:], a.calls, a.build)
        return
    if not torch.cuda.is_available():
        sys.exit("extend_grad_probe: needs a GPU (no CPU fallback, nothing measured)")
    if a.trace:
        trace(a.trace, a.calls)
        return
    if a.rounds < 5 or a.window < 0.5:
        sys.exit("extend_grad_probe: at least 5 rounds of windows of at least 0.5 s")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:   # kept current: a run cut short still leaves what it measured
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    emit(f"extend_grad_probe: build {_lib.build_id()}, torch {torch.__version__}, "
         f"{torch.cuda.get_device_name(0)}; {a.rounds} rounds, windows >= {a.window} s")
    if "grad" in a.what:
        for name in SHAPES:
            for everything in (False, True):
                grad_ab(name, everything, a.rounds, a.window, emit)
    if "step" in a.what:
        step_ab(a.rounds, a.window, emit)


if __name__ == "__main__":
    main()
