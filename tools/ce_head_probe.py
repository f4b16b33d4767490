"""A/B of one training step's loss head (GPU only: fails without a device).

    A: U = apply(X, Y, tau, eps, k); loss = custom_ce_loss(U, t); U.argmax(1); loss.backward()
    B: loss, pred, labels, row_loss, correct = ce_loss(X, Y, t, tau, eps, k); loss.backward()

at the NS shape (synth.CONFIGS["ns"]) and at FullySup, eps = 1, tau = 0.07, X a leaf that
requires grad.  Both steps are warmed up, then timed in alternating windows of at least
--window seconds (a host clock around a device synchronise), --rounds rounds in one process;
the report gives each step's median and spread (min .. max) over its windows.

    python tools/ce_head_probe.py [--rounds 5] [--window 0.5] [--out profiles/x.txt]

Kernel lists of one step (a separate run, the tracer slows the host):

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- \
        python tools/ce_head_probe.py --trace a --shape ns --steps 20

runs `--steps` steps of one route only (after 3 warm-up steps, counted too: divide the stats'
call counts by steps + 3).
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from graphlearninglayer_amd import GLL, _lib  # noqa: E402
from graphlearninglayer_amd.synth import CONFIGS, one_hot, synth  # noqa: E402

EPS, TAU = 1.0, 0.07
WARM = 3


def make(shape):
    c = CONFIGS[shape]
    X, lab = synth(c["base"], c["batch"], c["d"], r=c["r"], seed=0)
    dev = torch.device("cuda", 0)
    Xt = torch.from_numpy(X).to(dev).requires_grad_(True)
    Y = torch.from_numpy(one_hot(lab[: c["base"]])).to(dev)
    t = torch.from_numpy(lab[c["base"]:]).to(dev)
    L = GLL.LaplaceLearningSparseHard

    def step_a():
        Xt.grad = None
        U = L.apply(Xt, Y, TAU, EPS, c["k"])
        loss = GLL.custom_ce_loss(U, t)
        labels = U.argmax(1)
        loss.backward()
        return loss, labels

    def step_b():
        Xt.grad = None
        loss, _, labels, _, _ = L.ce_loss(Xt, Y, t, TAU, EPS, c["k"])
        loss.backward()
        return loss, labels

    return c, Xt, step_a, step_b


def window(step, seconds):
    """Microseconds per step over a window of at least `seconds`, ended by a synchronise."""
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
    c, Xt, step_a, step_b = make(shape)
    for _ in range(WARM * 10):
        la, laba = step_a()
        lb, labb = step_b()
    torch.cuda.synchronize()
    same = bool((laba == labb).all())
    emit(f"[{shape}] base {c['base']} + batch {c['batch']} x d {c['d']}, k {c['k']}, eps {EPS}, "
         f"tau {TAU}; loss A {float(la.detach()):.12g}  B {float(lb.detach()):.12g}; "
         f"labels equal: {same}")
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
         f"{ma - mb > spread}")


def trace(route, shape, steps):
    _, _, step_a, step_b = make(shape)
    step = step_a if route == "a" else step_b
    for _ in range(WARM + steps):
        step()
    torch.cuda.synchronize()
    print(f"traced {WARM + steps} steps of route {route.upper()} at {shape}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--shape", choices=["ns", "fullysup", "both"], default="both")
    ap.add_argument("--trace", choices=["a", "b"], help="run one route only (under rocprofv3)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", help="also write the report to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ce_head_probe: needs a GPU (no CPU fallback, nothing measured)")
    if a.rounds < 5 or a.window < 0.5:
        sys.exit("ce_head_probe: at least 5 rounds of windows of at least 0.5 s")
    shapes = ["ns", "fullysup"] if a.shape == "both" else [a.shape]
    if a.trace:
        for s in shapes:
            trace(a.trace, s, a.steps)
        return
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"ce_head_probe: build {_lib.build_id()}, torch {torch.__version__}, "
         f"{torch.cuda.get_device_name(0)}; {a.rounds} rounds, windows >= {a.window} s")
    for s in shapes:
        ab(s, a.rounds, a.window, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
