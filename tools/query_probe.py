"""A/B of the query kNN and of inductive evaluation (GPU only: fails without a device).

    knn    A : torch.cdist(Xq, Xdb) + topk(k, largest=False), in query chunks that fit --chunk-mb
           B : GLL.knn_query(Xq, Xdb, k)                              (query.hip, 3 launches a panel)
           at the evaluation shape Q = 10,000, N = 50,250, d = 128, k = 50 and at a minibatch-sized
           Q = 1,250, N = 250.  The report also counts the rows whose cdist + topk set differs from
           knn_query's (cdist ranks fp32 expanded-form distances: it is a yardstick for time, not
           for the sets).
    eval   A : utils.gl_accuracy on the 60,250-node graph (250 labeled + 50,000 unlabeled + 10,000
               test rows of the `synth` mixture, k = 50, eps = 1, tau = 1e-8)
           B : utils.laplace_fit on the 50,250 train rows + utils.laplace_predict of the 10,000
           time and accuracy of both, and of the predict step alone.

Every route is warmed up, then timed in alternating windows of at least --window seconds (a host
clock around a device synchronise), --rounds rounds in one process; the report gives each route's
median and spread (min .. max) over its windows.

    python tools/query_probe.py [--rounds 5] [--window 0.5] [--what knn eval] [--out profiles/x.txt]

Kernel lists (a separate run, the tracer slows the host):

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- \
        python tools/query_probe.py --trace b --calls 5

runs `--calls` calls of one knn route at the evaluation shape (after 2 warm-up calls, counted
too) and prints the library's build id; `--summarize OUT LABEL=CSV ... --build ID` turns the
kernel_stats.csv files of such runs into the launch summary (no GPU needed).
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

from graphlearninglayer_amd import GLL, _lib, utils  # noqa: E402
from graphlearninglayer_amd.synth import synth  # noqa: E402

SHAPES = {"eval": (10_000, 50_250, 128, 50), "minibatch": (1_250, 250, 128, 50)}
NL, NU, NT, D, K = 250, 50_000, 10_000, 128, 50
WARM = 2


def data():
    """The synth mixture at the evaluation size: labeled, unlabeled train, test."""
    X, labels = synth(NL, NU + NT, D, C=10, r=1.0, seed=3)
    return X, labels


def cdist_topk(Xq, Xdb, k, chunk_mb):
    rows = max(1, int(chunk_mb * 2 ** 20 // (4 * Xdb.shape[0])))
    idx, d2 = [], []
    for q0 in range(0, Xq.shape[0], rows):
        dist = torch.cdist(Xq[q0:q0 + rows], Xdb)
        v, i = torch.topk(dist, k, dim=1, largest=False)
        idx.append(i)
        d2.append(v * v)
    return torch.cat(idx), torch.cat(d2)


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


def knn_ab(name, rounds, seconds, chunk_mb, emit):
    Q, N, d, k = SHAPES[name]
    X, _ = data()
    dev = torch.device("cuda", 0)
    Xdb = torch.from_numpy(X[:N]).to(dev)
    Xq = torch.from_numpy(X[NL + NU:NL + NU + Q] if name == "eval" else X[N:N + Q]).to(dev)
    tag = f"[knn {name}]"
    ia, _ = cdist_topk(Xq, Xdb, k, chunk_mb)
    ib, _, st = GLL.knn_query(Xq, Xdb, k, return_status=True)
    differ = int((torch.sort(ia, dim=1).values != torch.sort(ib, dim=1).values).any(dim=1).sum())
    ws = _lib.lib().gll_query_workspace_bytes(Q, N, d, k, 0)
    emit(f"{tag} Q {Q}, N {N}, d {d}, k {k}; knn_query workspace {ws / 2**20:.1f} MiB, status "
         f"{st.cpu().tolist()}; cdist chunks of {chunk_mb} MiB; rows whose cdist+topk set differs "
         f"from the exact one: {differ}")
    med = alternate({"A(cdist+topk)": lambda: cdist_topk(Xq, Xdb, k, chunk_mb),
                     "B(knn_query)": lambda: GLL.knn_query(Xq, Xdb, k)}, rounds, seconds, emit, tag)
    a, b = med["A(cdist+topk)"], med["B(knn_query)"]
    emit(f"{tag} A / B = {a / b:.2f}x ({'knn_query' if b < a else 'the yardstick'} is faster)")


def eval_ab(rounds, seconds, emit):
    X, labels = data()
    train, lab = X[:NL], labels[:NL]
    unl, test, tlab = X[NL:NL + NU], X[NL + NU:], labels[NL + NU:]
    tag = "[eval]"
    acc = {}

    def a():
        acc["A"] = utils.gl_accuracy(train, lab, test, tlab, unlabeled_data=unl, epsilon=1.0, knn_num=K)

    def b():
        acc["B"] = utils.gl_accuracy_inductive(train, lab, test, tlab, unlabeled_data=unl,
                                               epsilon=1.0, knn_num=K)

    fit = utils.laplace_fit(X[:NL + NU], lab, knn_num=K, epsilon=1.0)
    tq = torch.from_numpy(test).cuda()

    def p():
        utils.laplace_predict(fit, tq, knn_num=K)

    alternate({"A(gl_accuracy 60,250)": a, "B(fit 50,250 + predict 10,000)": b,
               "predict alone": p}, rounds, seconds, emit, tag)
    emit(f"{tag} accuracy on the 10,000 test rows: A (transductive) {acc['A']:.2f}%  "
         f"B (inductive) {acc['B']:.2f}%")


def trace(route, calls, chunk_mb):
    Q, N, d, k = SHAPES["eval"]
    X, _ = data()
    Xdb = torch.from_numpy(X[:N]).cuda()
    Xq = torch.from_numpy(X[NL + NU:NL + NU + Q]).cuda()
    for _ in range(WARM + calls):
        if route == "a":
            cdist_topk(Xq, Xdb, k, chunk_mb)
        else:
            GLL.knn_query(Xq, Xdb, k)
    torch.cuda.synchronize()
    print(f"traced {WARM + calls} calls of route {route.upper()}; build {_lib.build_id()}")


def summarize(out, pairs, calls, build):
    total = WARM + calls
    lines = [f"Kernels of one kNN call at Q 10,000, N 50,250, d 128, k 50: rocprofv3 --kernel-trace "
             f"--stats over {total} calls", f"({WARM} warm-up + {calls}) of one route of "
             f"tools/query_probe.py per run (build {build}).", ""]
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
    ap.add_argument("--what", nargs="+", default=["knn", "eval"], choices=["knn", "eval"])
    ap.add_argument("--chunk-mb", type=int, default=1024, help="cdist distance chunk (MiB)")
    ap.add_argument("--trace", choices=("a", "b"), help="run one knn route only (under rocprofv3)")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", help="also write the report to this file")
    ap.add_argument("--summarize", nargs="+", metavar=("OUT", "LABEL=CSV"))
    ap.add_argument("--build", default="?")
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize[0], a.summarize[1:], a.calls, a.build)
        return
    if not torch.cuda.is_available():
        sys.exit("query_probe: needs a GPU (no CPU fallback, nothing measured)")
    if a.trace:
        trace(a.trace, a.calls, a.chunk_mb)
        return
    if a.rounds < 5 or a.window < 0.5:
        sys.exit("query_probe: at least 5 rounds of windows of at least 0.5 s")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:   # kept current: a run cut short still leaves what it measured
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    emit(f"query_probe: build {_lib.build_id()}, torch {torch.__version__}, "
         f"{torch.cuda.get_device_name(0)}; {a.rounds} rounds, windows >= {a.window} s")
    if "knn" in a.what:
        for name in SHAPES:
            knn_ab(name, a.rounds, a.window, a.chunk_mb, emit)
    if "eval" in a.what:
        eval_ab(a.rounds, a.window, emit)


if __name__ == "__main__":
    main()
