"""A/B of the layer on caller-supplied neighbour lists against the search (GPU only: fails without
a device).

    step     A : apply + backward with the exact search           (gram + select + row build + ...)
             B : apply(neighbors=) + backward on the same lists   (reset + ingest + row build + ...,
                 ingest.hip)
             at NS (500 + 500 rows, d 512, k 10) and FullySup (250 + 1,250 rows, d 128, k 25), one
             graph and a batch of 64, epsilon 1.0 and tau 0.07.  B is handed the lists A's search
             finds (GLL.device_graph(X)["knn_idx"]): the same graph, the search outside its time.
    laplace  A : utils.laplace at 60,250 x 128, k = 50 (the evaluation graph)
             B : utils.laplace(neighbors=) on the lists of A's graph
             with gll_workspace_bytes of both problems beside the times.

Every route is warmed up, then timed in alternating windows of at least --window seconds (a host
clock around a device synchronise), --rounds rounds in one process; the report gives each route's
median and spread (min .. max) over its windows.

    python tools/lists_probe.py [--rounds 5] [--window 0.5] [--what step laplace] [--out FILE]

Kernel lists (a separate run, the tracer slows the host):

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- \
        python tools/lists_probe.py --trace ns --calls 5

runs `--calls` steps of route B at that shape (after 2 warm-up steps, counted too);
`--summarize OUT CSV` turns the kernel_stats.csv of such a run into the launch summary (no GPU
needed).
"""
import argparse
import csv
import ctypes as ct
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from graphlearninglayer_amd import GLL, _lib, utils  # noqa: E402
from graphlearninglayer_amd.synth import CONFIGS, one_hot, seeded_gbar, synth  # noqa: E402

EPS, TAU, C = 1.0, 0.07, 10
WARM = 2
EVAL = dict(base=250, rows=60_000, d=128, k=50)


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
            return 1e3 * dt / n


def alternate(routes, rounds, seconds):
    """name -> list of ms per call, the routes' windows alternating."""
    for f in routes.values():
        for _ in range(WARM):
            f()
    out = {k: [] for k in routes}
    for _ in range(rounds):
        for k, f in routes.items():
            out[k].append(window(f, seconds))
    return out


def fmt(v, unit="us", scale=1e3):
    return (f"{statistics.median(v) * scale:10.1f} {unit}  ({min(v) * scale:.1f} .. "
            f"{max(v) * scale:.1f})")


def layer_inputs(config, B):
    c = CONFIGS[config]
    Xs, Ys, Ns = [], [], []
    for g in range(B):
        X, lab = synth(c["base"], c["batch"], c["d"], r=c["r"], seed=g)
        Xs.append(X)
        Ys.append(one_hot(lab[: c["base"]]))
    X = torch.from_numpy(np.stack(Xs)).cuda()
    Y = torch.from_numpy(np.stack(Ys)).cuda()
    for g in range(B):
        Ns.append(GLL.device_graph(X[g], c["k"], EPS)["knn_idx"].clone())
    N = torch.stack(Ns)
    gbar = torch.from_numpy(np.stack([seeded_gbar(c["batch"], C, seed=7 + g) for g in range(B)])).cuda()
    if B == 1:
        X, Y, N, gbar = X[0], Y[0], N[0], gbar[0]
    return X.contiguous(), Y.contiguous(), N.contiguous(), gbar.contiguous(), c["k"]


def step_routes(config, B):
    X, Y, N, gbar, k = layer_inputs(config, B)
    apply = GLL.LaplaceLearningSparseHard.apply

    def run(nb):
        Xt = X.detach().requires_grad_(True)
        U = apply(Xt, Y, TAU, EPS, k, neighbors=nb)
        U.backward(gbar)
        return Xt.grad

    return {"search": lambda: run(None), "lists": lambda: run(N)}


def probe_step(args, say):
    say("apply + backward, epsilon 1.0, tau 0.07: the search against neighbors= (the same lists)")
    for config in ("ns", "fullysup"):
        for B in (1, 64):
            res = alternate(step_routes(config, B), args.rounds, args.window)
            c = CONFIGS[config]
            say(f"{config} (n {c['base'] + c['batch']}, d {c['d']}, k {c['k']}), B = {B}")
            for name, v in res.items():
                say(f"    {name:7s} {fmt(v)} per step")
            say(f"    lists / search = {statistics.median(res['lists']) / statistics.median(res['search']):.3f}")


def probe_laplace(args, say):
    e = EVAL
    X, lab = synth(e["base"], e["rows"], e["d"], seed=0)
    n = X.shape[0]
    Xd = torch.from_numpy(X).cuda()
    N = GLL.device_graph(Xd, e["k"], "auto")["knn_idx"].clone()
    torch.cuda.synchronize()
    nb = {}
    for name, flags in (("search", 0), ("lists", _lib.FLAG_KNN_GIVEN)):
        p = GLL.make_problem(n, e["d"], 0, 1, e["k"], 0.0, "auto", flags=flags)
        nb[name] = _lib.lib().gll_workspace_bytes(ct.byref(p))
    routes = {"search": lambda: utils.laplace(Xd, lab[: e["base"]], knn_num=e["k"]),
              "lists": lambda: utils.laplace(Xd, lab[: e["base"]], knn_num=e["k"], neighbors=N)}
    res = alternate(routes, max(2, args.rounds // 2), args.window)
    say(f"utils.laplace at {n} x {e['d']}, k = {e['k']}, epsilon 'auto' (graph build, CSR assembly "
        "in torch, refined solve)")
    for name, v in res.items():
        say(f"    {name:7s} {fmt(v, 'ms', 1.0)} per call, graph workspace {nb[name] / 1e6:10.1f} MB")
    graph = {"search": lambda: GLL.device_graph(Xd, e["k"], "auto"),
             "lists": lambda: GLL.device_graph(Xd, e["k"], "auto", neighbors=N)}
    res = alternate(graph, max(2, args.rounds // 2), args.window)
    say("  the graph build alone (GLL.device_graph: kernels + the compact CSR in torch)")
    for name, v in res.items():
        say(f"    {name:7s} {fmt(v, 'ms', 1.0)} per call")


def trace(args):
    f = step_routes(args.trace, 1)["lists"]
    for _ in range(WARM + args.calls):
        f()
    torch.cuda.synchronize()


def summarize(out, path):
    rows = list(csv.DictReader(open(path)))
    with open(out, "w") as fh:
        fh.write("rocprofv3 --kernel-trace --stats of tools/lists_probe.py --trace (apply(neighbors=) + "
                 "backward): kernel, calls, average ns, share of GPU time\n")
        for r in rows:
            fh.write(f"{r['Name'][:110]:110s} {r['Calls']:>6s} {float(r['AverageNs']):12.1f} "
                     f"{float(r['Percentage']):6.2f}%\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--what", nargs="+", default=["step", "laplace"], choices=["step", "laplace"])
    ap.add_argument("--out")
    ap.add_argument("--trace", choices=["ns", "fullysup"])
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--summarize", nargs=2, metavar=("OUT", "CSV"))
    a = ap.parse_args()
    if a.summarize:
        summarize(*a.summarize)
        return
    if a.trace:
        trace(a)
        return
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"tools/lists_probe.py --rounds {a.rounds} --window {a.window}: median (min .. max) over "
        f"alternating windows, build {_lib.build_id()}, {torch.cuda.get_device_name(0)}")
    if "step" in a.what:
        probe_step(a, say)
    if "laplace" in a.what:
        probe_laplace(a, say)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
