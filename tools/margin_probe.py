"""A/B of one Carlini-Wagner attack step's margin head (GPU only: fails without a device).

    A: U = apply(X, Y, tau, eps, k); loss = cw_margin(U, other); loss.backward()
    B: loss, pred, labels, second, row_margin, moved = margin_loss(X, Y, other, tau, eps, k);
       loss.backward()

at the NS shape (synth.CONFIGS["ns"]) and at FullySup, eps = 1, tau = 0.07, X a leaf that
requires grad, `other` the second-best class of a clean call (adversarial.py:688-692).  Both
steps are warmed up, then timed in alternating windows of at least --window seconds (a host
clock around a device synchronise), --rounds rounds in one process; the report gives each step's
median and spread (min .. max) over its windows.

    python tools/margin_probe.py [--rounds 5] [--window 0.5] [--out profiles/x.txt]

Kernel lists of one step (a separate run, the tracer slows the host):

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- \
        python tools/margin_probe.py --trace a --shape ns --steps 20

runs `--steps` steps of one route only (after 3 warm-up steps, counted too, and the one clean call
that picks `other`) and prints the library's build id.  `--summarize OUT LABEL=CSV ... --build ID`
turns the kernel_stats.csv files of such runs into the launch-count summary (no GPU needed).
"""
import argparse
import csv
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EPS, TAU = 1.0, 0.07
WARM = 3


def make(shape):
    import torch

    from graphlearninglayer_amd import GLL
    from graphlearninglayer_amd.synth import CONFIGS, one_hot, synth

    c = CONFIGS[shape]
    X, lab = synth(c["base"], c["batch"], c["d"], r=c["r"], seed=0)
    dev = torch.device("cuda", 0)
    Xt = torch.from_numpy(X).to(dev).requires_grad_(True)
    Y = torch.from_numpy(one_hot(lab[: c["base"]])).to(dev)
    L = GLL.LaplaceLearningSparseHard
    with torch.no_grad():
        other = L.margin_loss(Xt, Y, None, TAU, EPS, c["k"])[3]

    def step_a():
        Xt.grad = None
        U = L.apply(Xt, Y, TAU, EPS, c["k"])
        loss = GLL.cw_margin(U, other)
        loss.backward()
        return loss

    def step_b():
        Xt.grad = None
        loss = L.margin_loss(Xt, Y, other, TAU, EPS, c["k"])[0]
        loss.backward()
        return loss

    return c, Xt, step_a, step_b


def window(step, seconds):
    """Microseconds per step over a window of at least `seconds`, ended by a synchronise."""
    import torch

    torch.cuda.synchronize()
    n, chunk = 0, 50
    t0 = time.perf_counter()
    while True:
        for _ in range(chunk):
            step()
        n += chunk
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return dt / n * 1e6   # us per step


def ab(shape, rounds, seconds, emit):
    import torch

    c, Xt, step_a, step_b = make(shape)
    for _ in range(WARM * 10):
        la = step_a()
        ga = Xt.grad.clone()
        lb = step_b()
        gb = Xt.grad.clone()
    torch.cuda.synchronize()
    rel = float(torch.linalg.vector_norm(ga - gb) / torch.linalg.vector_norm(ga))
    emit(f"[{shape}] base {c['base']} + batch {c['batch']} x d {c['d']}, k {c['k']}, eps {EPS}, "
         f"tau {TAU}; loss A {float(la.detach()):.12g}  B {float(lb.detach()):.12g}; "
         f"grad_X B against A, normwise: {rel:.2e}")
    ta, tb = [], []
    for r in range(rounds):
        ta.append(window(step_a, seconds))
        tb.append(window(step_b, seconds))
        emit(f"[{shape}] round {r}: A {ta[-1]:8.2f} us/step   B {tb[-1]:8.2f} us/step")
    ma, mb = statistics.median(ta), statistics.median(tb)
    emit(f"[{shape}] A median {ma:.2f} us (min {min(ta):.2f} .. max {max(ta):.2f})")
    emit(f"[{shape}] B median {mb:.2f} us (min {min(tb):.2f} .. max {max(tb):.2f})")
    spread = max(max(ta) - min(ta), max(tb) - min(tb))
    emit(f"[{shape}] A - B = {ma - mb:.2f} us ({(ma - mb) / ma * 100:.1f}% of A); largest spread "
         f"of one step over its windows {spread:.2f} us; B faster beyond the spread: "
         f"{ma - mb > spread}; every window of B below every window of A: {max(tb) < min(ta)}")


def trace(route, shape, steps):
    import torch

    _, _, step_a, step_b = make(shape)
    step = step_a if route == "a" else step_b
    for _ in range(WARM + steps):
        step()
    torch.cuda.synchronize()
    from graphlearninglayer_amd import _lib

    print(f"traced {WARM + steps} steps of route {route.upper()} at {shape}, build {_lib.build_id()}")


def summarize(out, pairs, steps, build):
    """Launch counts and kernel time per step from rocprofv3 kernel_stats.csv files; `build`: the
    build id the traced runs printed."""
    calls = WARM + steps
    lines = [f"One attack step's kernels, rocprofv3 --kernel-trace --stats over {calls} steps "
             f"({WARM} warm-up + {steps}) of one",
             f"route of tools/margin_probe.py per run (build {build}).  A: apply -> cw_margin -> "
             "backward.  B: margin_loss -> backward.",
             f"Rows with fewer than {calls} calls are the clean call that picks `other`, the "
             "status sink's periodic copy /",
             "clear and one-time set-up, not part of a step.", ""]
    for pair in pairs:
        label, path = pair.split("=", 1)
        with open(path, newline="") as fh:
            rows = [(r["Name"], int(r["Calls"]), float(r["TotalDurationNs"]),
                     float(r["AverageNs"])) for r in csv.DictReader(fh)]
        step_rows = [r for r in rows if r[1] >= calls]   # calls + 1: the clean call ran it too
        n = sum(r[1] // calls for r in step_rows)
        us = sum(r[3] * (r[1] // calls) for r in step_rows) / 1e3
        lines.append(f"{label}: {n} kernel launches per step, {us:.1f} us of kernel time per step")
        for name, cnt, _, avg in rows:
            name = name[5:] if name.startswith("void ") else name
            lines.append(f"    {cnt:2d} calls  {avg / 1e3:7.2f} us avg  {name[:110]}")
        lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("\n".join(lines))
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--shape", choices=["ns", "fullysup", "both"], default="both")
    ap.add_argument("--trace", choices=["a", "b"], help="run one route only (under rocprofv3)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", help="also write the report to this file")
    ap.add_argument("--summarize", nargs="+", metavar=("OUT", "LABEL=CSV"),
                    help="write the launch-count summary of traced runs to OUT")
    ap.add_argument("--build", help="with --summarize: the build id the traced runs printed")
    a = ap.parse_args()
    if a.summarize:
        if not a.build:
            sys.exit("margin_probe: --summarize needs --build (the id the traced runs printed)")
        summarize(a.summarize[0], a.summarize[1:], a.steps, a.build)
        return
    import torch

    from graphlearninglayer_amd import _lib

    if not torch.cuda.is_available():
        sys.exit("margin_probe: needs a GPU (no CPU fallback, nothing measured)")
    if a.rounds < 5 or a.window < 0.5:
        sys.exit("margin_probe: at least 5 rounds of windows of at least 0.5 s")
    shapes = ["ns", "fullysup"] if a.shape == "both" else [a.shape]
    if a.trace:
        for s in shapes:
            trace(a.trace, s, a.steps)
        return
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"margin_probe: build {_lib.build_id()}, torch {torch.__version__}, "
         f"{torch.cuda.get_device_name(0)}; {a.rounds} rounds, windows >= {a.window} s")
    for s in shapes:
        ab(s, a.rounds, a.window, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
