"""The out-of-sample extension on caller-supplied lists and pools against the searching route and
the plain-torch yardstick (GPU only: fails without a device).

    search  GLL.extend: the exact search (three launches a panel) + the extension
    list    GLL.extend(neighbors=idx), idx the search's k - 1 columns: re-rank (list mode) + extension
    pool    GLL.extend(neighbors=pool), pool the search's min(4 (k - 1), 256) columns -- the widest
            one search returns; the 512-column cap of the re-rank is not reached: re-rank (pool mode)
            + extension
    torch   GLL.extend_torch handed idx (plain PyTorch, float32)

at the minibatch shape Q = 1,250, N = 250, d = 128, k = 25 and the evaluation shape Q = 10,000,
N = 50,250, d = 128, k = 50, each forward alone, + backward to Xq, + backward to every input (Xq,
Xdb, P, epsilon).  Every route is warmed up, then timed in alternating windows of at least --window
seconds (a host clock around a device synchronise), --rounds rounds in one process; the report
gives each route's median and spread (min .. max) over its windows, the bytes of database rows the
re-rank gathers (Q c d 4) and the rate that makes of its share of the time.

    python tools/extend_lists_probe.py [--rounds 5] [--window 0.5] [--out FILE]

Kernel durations (a separate run, the tracer slows the host):

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- \
        python tools/extend_lists_probe.py --trace list --calls 5

runs `--calls` extend + backward (to Xq) calls of one route at the evaluation shape after 2 warm-up
calls, counted too; `--summarize OUT LABEL=CSV ... --build ID` turns the kernel_stats.csv files of
such runs into the launch summary (no GPU needed).
"""
import argparse
import csv
import os
import sys

import torch

from extend_grad_probe import ROOT, SHAPES, WARM, alternate, clear, tensors  # noqa: F401  (tools/ is sys.path[0])

from graphlearninglayer_amd import GLL, _lib  # noqa: E402

ROUTES = ("search", "list", "pool", "torch")
MODES = ("fwd", "bwd_xq", "bwd_all")


def pool_width(k):
    return min(4 * (k - 1), _lib.QUERY_MAX_K)


SEARCH_KERNELS = ("query_norm_kernel", "query_gram_kernel", "query_select_kernel")


def routes(name, mode, check=True):
    """{route: step} of a shape and mode, and the shape's (Q, N, d, k, c)."""
    everything = mode == "bwd_all"
    Xq, Xdb, P, eps, gU, k = tensors(name, everything)
    if mode == "fwd":
        Xq = Xq.detach()
    with torch.no_grad():
        idx = GLL.knn_query(Xq, Xdb, k - 1)[0]
        pool = GLL.knn_query(Xq, Xdb, pool_width(k))[0]
    g32 = gU.float()

    def run(fn, g):
        def step():
            clear(Xq, Xdb, P, eps)
            out = fn()
            if mode != "fwd":
                (out * g).sum().backward()
        return step

    steps = {
        "search": run(lambda: GLL.extend(Xq, Xdb, P, k=k, epsilon=eps)[0], gU),
        "list": run(lambda: GLL.extend(Xq, Xdb, P, k=k, epsilon=eps, neighbors=idx)[0], gU),
        "pool": run(lambda: GLL.extend(Xq, Xdb, P, k=k, epsilon=eps, neighbors=pool)[0], gU),
        "torch": run(lambda: GLL.extend_torch(Xq, Xdb, P, idx, eps), g32),
    }
    # the three routes of the package agree bitwise (the pool holds the lists); torch within float32
    with torch.no_grad():
        ref = GLL.extend(Xq, Xdb, P, k=k, epsilon=eps)[0] if check else None
        for nb in (idx, pool) if check else ():
            assert torch.equal(GLL.extend(Xq, Xdb, P, k=k, epsilon=eps, neighbors=nb)[0], ref)
    Q, N, d, _ = SHAPES[name]
    return steps, (Q, N, d, k, pool.shape[1])


def rerank_alone(name, rounds, seconds, emit):
    """The re-rank launch by itself, list and pool mode: time, bytes gathered, rate."""
    Xq, Xdb, _, _, _, k = tensors(name, False)
    Xq = Xq.detach()
    idx = GLL.knn_query(Xq, Xdb, k - 1)[0].int()
    pool = GLL.knn_query(Xq, Xdb, pool_width(k))[0].int()
    Q, N, d, _ = SHAPES[name]
    tag = f"[rerank {name}]"
    steps = {"list": lambda: GLL.knn_query(Xq, Xdb, k - 1, candidates=idx, keep_order=True),
             "pool": lambda: GLL.knn_query(Xq, Xdb, k - 1, candidates=pool)}
    med = alternate(steps, rounds, seconds, emit, tag)
    for key, c in (("list", idx.shape[1]), ("pool", pool.shape[1])):
        mb = Q * c * d * 4 / 1e6
        emit(f"{tag} {key}: c {c}, gathers Q c d 4 = {mb:.1f} MB of database rows (the database is "
             f"{N * d * 4 / 1e6:.1f} MB), {mb / med[key]:.1f} GB/s over the call (host time included)")


def trace(route, calls):
    steps, _ = routes("eval", "bwd_xq", check=False)
    for _ in range(WARM + calls):
        steps[route]()
    torch.cuda.synchronize()
    print(f"traced {WARM + calls} {route} + backward calls; build {_lib.build_id()}")


def summarize(out, pairs, calls, build):
    total = WARM + calls
    lines = [f"Kernels of one extension + backward (to Xq) call at Q 10,000, N 50,250, d 128, k 50 by "
             f"route: rocprofv3 --kernel-trace --stats", f"over {total} calls ({WARM} warm-up + {calls}) "
             f"of tools/extend_lists_probe.py --trace per run (build {build}).", ""]
    for pair in pairs:
        label, path = pair.split("=", 1)
        with open(path, newline="") as fh:
            rows = [(r["Name"], int(r["Calls"]), float(r["TotalDurationNs"]), float(r["AverageNs"]))
                    for r in csv.DictReader(fh)]
        # the two searches that make the lists and the pool run once, before the calls
        setup = [r for r in rows if label != "search" and any(s in r[0] for s in SEARCH_KERNELS)]
        rows = [r for r in rows if r not in setup]
        n = sum(r[1] for r in rows) / total
        ms = sum(r[2] for r in rows) / total / 1e6
        lines.append(f"{label}: {n:.1f} kernel launches per call, {ms:.3f} ms of kernel time per call"
                     " (tensor set-up included)")
        for name, cnt, _, avg in rows:
            name = name[5:] if name.startswith("void ") else name
            lines.append(f"    {cnt:4d} calls  {avg / 1e3:9.2f} us avg  {name[:100]}")
        if label == "search":
            lines.append("    (the two set-up searches that make the lists and the pool are among the "
                         "query_* launches)")
        if setup:
            lines.append(f"    (set-up, not counted: {sum(r[1] for r in setup)} launches of the two "
                         f"searches that make the lists and the pool)")
        lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("\n".join(lines))
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--trace", choices=ROUTES, help="run one route only (under rocprofv3)")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", help="also write the report to this file")
    ap.add_argument("--summarize", nargs="+", metavar=("OUT", "LABEL=CSV"))
    ap.add_argument("--build", default="?")
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize[0], a.summarize[1:], a.calls, a.build)
        return
    if not torch.cuda.is_available():
        sys.exit("extend_lists_probe: needs a GPU (no CPU fallback, nothing measured)")
    if a.trace:
        trace(a.trace, a.calls)
        return
    if a.rounds < 5 or a.window < 0.5:
        sys.exit("extend_lists_probe: at least 5 rounds of windows of at least 0.5 s")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:   # kept current: a run cut short still leaves what it measured
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    emit(f"extend_lists_probe: build {_lib.build_id()}, torch {torch.__version__}, "
         f"{torch.cuda.get_device_name(0)}; {a.rounds} rounds, windows >= {a.window} s")
    for name in a.shapes:
        rerank_alone(name, a.rounds, a.window, emit)
        for mode in MODES:
            steps, (Q, N, d, k, c) = routes(name, mode)
            tag = f"[{name} {mode}]"
            emit(f"{tag} Q {Q}, N {N}, d {d}, k {k}, pool c {c}")
            med = alternate(steps, a.rounds, a.window, emit, tag)
            for r in ("list", "pool"):
                emit(f"{tag} search / {r} = {med['search'] / med[r]:.2f}x   torch / {r} = "
                     f"{med['torch'] / med[r]:.2f}x ({'beats' if med[r] < med['torch'] else 'does not beat'} "
                     f"the yardstick)")


if __name__ == "__main__":
    main()
