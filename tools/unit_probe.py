"""A/B of one training step's feature normalisation (GPU only: fails without a device).

    A: loss = ce_loss(F.normalize(z, dim=1), Y, t, tau, eps, k)[0]; loss.backward()
    B: loss = ce_loss(z, Y, t, tau, eps, k, normalize=True)[0];     loss.backward()

at the NS shape (synth.CONFIGS["ns"]) and at FullySup, eps = 1, tau = 0.07, z a leaf that requires
grad (un-normalised features: synth's rows times a per-row scale), first as fp32 and then as bf16.
A is what a caller writes today.  With fp32 features its layer call takes the route that has not
changed (no front-end launch), so A is the yardstick the new route is measured against, on the same
build.  With bf16 features the layer call of A converts through the new front end as well; the
step on the unchanged route is A32, which casts by hand:

    A32: loss = ce_loss(F.normalize(z, dim=1).float(), Y, t, tau, eps, k)[0]; loss.backward()

Every step is warmed up, then timed in alternating windows of at least --window seconds (a host
clock around a device synchronise), --rounds rounds in one process; the report gives each step's
median and spread (min .. max) over its windows.

    python tools/unit_probe.py [--rounds 5] [--window 0.5] [--out profiles/x.txt]

Kernel lists of one step (a separate run, the tracer slows the host):

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- \
        python tools/unit_probe.py --trace a --shape ns --dtype float32 --steps 20

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

import numpy as np  # noqa: E402
import torch  # noqa: E402

from graphlearninglayer_amd import GLL, _lib  # noqa: E402
from graphlearninglayer_amd.synth import CONFIGS, one_hot, synth  # noqa: E402

EPS, TAU = 1.0, 0.07
WARM = 3
DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16}


def make(shape, dtype):
    c = CONFIGS[shape]
    X, lab = synth(c["base"], c["batch"], c["d"], r=c["r"], seed=0)
    scale = np.random.Generator(np.random.PCG64(1)).uniform(0.25, 4.0, size=(X.shape[0], 1))
    dev = torch.device("cuda", 0)
    z = torch.from_numpy(X * scale.astype(np.float32)).to(dev, DTYPES[dtype]).requires_grad_(True)
    Y = torch.from_numpy(one_hot(lab[: c["base"]])).to(dev)
    t = torch.from_numpy(lab[c["base"]:]).to(dev)
    L = GLL.LaplaceLearningSparseHard
    normalize = torch.nn.functional.normalize

    def step_a():
        z.grad = None
        loss = L.ce_loss(normalize(z, dim=1), Y, t, TAU, EPS, c["k"])[0]
        loss.backward()
        return loss

    def step_a32():
        z.grad = None
        loss = L.ce_loss(normalize(z, dim=1).float(), Y, t, TAU, EPS, c["k"])[0]
        loss.backward()
        return loss

    def step_b():
        z.grad = None
        loss = L.ce_loss(z, Y, t, TAU, EPS, c["k"], normalize=True)[0]
        loss.backward()
        return loss

    steps = {"A": step_a, "B": step_b}
    if dtype != "float32":
        steps = {"A32": step_a32, **steps}
    return c, z, steps


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


def ab(shape, dtype, rounds, seconds, emit):
    c, z, steps = make(shape, dtype)
    tag = f"[{shape} {dtype}]"
    losses, calls = {}, {}
    for name, step in steps.items():
        for _ in range(WARM * 10):
            loss = step()
        c0 = _lib.lib().gll_features_calls()
        step()
        calls[name] = _lib.lib().gll_features_calls() - c0
        losses[name] = float(loss.detach())
    torch.cuda.synchronize()
    emit(f"{tag} base {c['base']} + batch {c['batch']} x d {c['d']}, k {c['k']}, eps {EPS}, tau "
         f"{TAU}; loss " + "  ".join(f"{n} {v:.12g}" for n, v in losses.items())
         + "; front-end launches a step: " + "  ".join(f"{n} {v}" for n, v in calls.items()))
    times = {name: [] for name in steps}
    for r in range(rounds):
        for name, step in steps.items():
            times[name].append(window(step, seconds))
        emit(f"{tag} round {r}: " + "   ".join(f"{n} {times[n][-1]:8.2f} us/step" for n in steps))
    med = {n: statistics.median(v) for n, v in times.items()}
    for n, v in times.items():
        emit(f"{tag} {n} median {med[n]:.2f} us (min {min(v):.2f} .. max {max(v):.2f})")
    yard = "A" if dtype == "float32" else "A32"
    spread = max(times[yard]) - min(times[yard])
    diff = med[yard] - med["B"]
    emit(f"{tag} {yard} - B = {diff:.2f} us ({diff / med[yard] * 100:.1f}% of {yard}); spread of "
         f"{yard} over its windows {spread:.2f} us; B no slower than {yard} within that spread: "
         f"{med['B'] <= med[yard] + spread}; B faster beyond it: {diff > spread}")


def trace(route, shape, dtype, steps):
    _, _, fns = make(shape, dtype)
    step = fns[route.upper()]
    for _ in range(WARM + steps):
        step()
    torch.cuda.synchronize()
    print(f"traced {WARM + steps} steps of route {route.upper()} at {shape} {dtype}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--shape", choices=["ns", "fullysup", "both"], default="both")
    ap.add_argument("--dtype", choices=[*DTYPES, "both"], default="both")
    ap.add_argument("--trace", choices=["a", "a32", "b"],
                    help="run one route only (under rocprofv3)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", help="also write the report to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("unit_probe: needs a GPU (no CPU fallback, nothing measured)")
    if a.rounds < 5 or a.window < 0.5:
        sys.exit("unit_probe: at least 5 rounds of windows of at least 0.5 s")
    shapes = ["ns", "fullysup"] if a.shape == "both" else [a.shape]
    dtypes = list(DTYPES) if a.dtype == "both" else [a.dtype]
    if a.trace:
        if a.trace == "a32" and "float32" in dtypes:
            sys.exit("unit_probe: route A32 exists for bfloat16 only (--dtype bfloat16)")
        for s in shapes:
            for dt in dtypes:
                trace(a.trace, s, dt, a.steps)
        return
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"unit_probe: build {_lib.build_id()}, torch {torch.__version__}, "
         f"{torch.cuda.get_device_name(0)}; {a.rounds} rounds, windows >= {a.window} s")
    for s in shapes:
        for dt in dtypes:
            ab(s, dt, a.rounds, a.window, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
