"""A/B of one pre-training step's contrastive loss (GPU only: fails without a device).

    A : loss = supcon_loss_torch(f, y); loss.backward()                 (plain torch, R x R logits)
    B : loss = supcon_loss(f, y); loss.backward()                       (supcon.hip, 2 + 2 launches)
    An: loss = supcon_loss_torch(F.normalize(z, dim=-1), y); loss.backward()
    Bn: loss = supcon_loss(z, y, normalize=True); loss.backward()

at bsz 256 and 1,250 (the reference's batch, config/cli.py:28), 2 views, d = 128, 10 classes,
T = Tb = 0.07, mode 'all', features a leaf that requires grad.  All steps are warmed up, then timed
in alternating windows of at least --window seconds (a host clock around a device synchronise),
--rounds rounds in one process; the report gives each step's median and spread (min .. max) over
its windows and the peak device memory of one step above its inputs.

    python tools/supcon_probe.py [--rounds 5] [--window 0.5] [--out profiles/x.txt]

Kernel lists of one step (a separate run, the tracer slows the host):

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- \
        python tools/supcon_probe.py --trace b --bsz 1250 --steps 20

runs `--steps` steps of one route only (after 3 warm-up steps, counted too) and prints the
library's build id.  `--summarize OUT LABEL=CSV ... --build ID` turns the kernel_stats.csv files of
such runs into the launch-count summary (no GPU needed).
"""
import argparse
import csv
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from graphlearninglayer_amd import _lib  # noqa: E402
from graphlearninglayer_amd.losses import supcon_loss, supcon_loss_torch  # noqa: E402

V, D, CLASSES, T = 2, 128, 10, 0.07
WARM = 3
ROUTES = ("a", "b", "an", "bn")


def make(bsz):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(bsz)
    y = (torch.arange(bsz) % CLASSES)
    z = torch.randn(bsz, V, D, generator=g) + 1.5 * torch.randn(CLASSES, 1, D, generator=g)[y]
    y = y.to(dev)
    raw = z.to(dev).requires_grad_(True)
    unit = torch.nn.functional.normalize(z, dim=-1).to(dev).requires_grad_(True)

    def step_a():
        unit.grad = None
        loss = supcon_loss_torch(unit, y, temperature=T, base_temperature=T)
        loss.backward()
        return loss

    def step_b():
        unit.grad = None
        loss = supcon_loss(unit, y, T, T)
        loss.backward()
        return loss

    def step_an():
        raw.grad = None
        loss = supcon_loss_torch(torch.nn.functional.normalize(raw, dim=-1), y, temperature=T,
                                 base_temperature=T)
        loss.backward()
        return loss

    def step_bn():
        raw.grad = None
        loss = supcon_loss(raw, y, T, T, normalize=True)
        loss.backward()
        return loss

    return dict(a=step_a, b=step_b, an=step_an, bn=step_bn)


def window(step, seconds):
    """Microseconds per step over a window of at least `seconds`, ended by a synchronise."""
    torch.cuda.synchronize()
    n, chunk = 0, 20
    t0 = time.perf_counter()
    while True:
        for _ in range(chunk):
            step()
        n += chunk
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return dt / n * 1e6


def peak(step):
    """Peak device bytes of one step above what is allocated before it."""
    step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    step()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def ab(bsz, rounds, seconds, emit):
    steps = make(bsz)
    tag = f"[bsz {bsz}]"
    for _ in range(WARM * 5):
        last = {k: s() for k, s in steps.items()}
    torch.cuda.synchronize()
    emit(f"{tag} {bsz} x {V} views = {bsz * V} rows, d {D}, {CLASSES} classes, T = Tb = {T}; loss "
         + "  ".join(f"{k.upper()} {float(v.detach()):.9g}" for k, v in last.items()))
    emit(f"{tag} peak bytes of one step above its inputs: "
         + "  ".join(f"{k.upper()} {peak(s) / 2**20:.1f} MiB" for k, s in steps.items())
         + f"  (R x R floats: {4 * (bsz * V) ** 2 / 2**20:.1f} MiB)")
    t = {k: [] for k in steps}
    for r in range(rounds):
        for k, s in steps.items():
            t[k].append(window(s, seconds))
        emit(f"{tag} round {r}: " + "  ".join(f"{k.upper()} {t[k][-1]:8.2f}" for k in steps) + "  us/step")
    med = {k: statistics.median(v) for k, v in t.items()}
    for k, v in t.items():
        emit(f"{tag} {k.upper():2s} median {med[k]:.2f} us (min {min(v):.2f} .. max {max(v):.2f})")
    for x, f in (("a", "b"), ("an", "bn")):
        spreads = (max(t[x]) - min(t[x])) + (max(t[f]) - min(t[f]))
        emit(f"{tag} {x.upper()} - {f.upper()} = {med[x] - med[f]:.2f} us ({med[x] / med[f]:.2f}x); the two "
             f"spreads together {spreads:.2f} us; fused faster beyond them: {med[x] - med[f] > spreads}")


def trace(route, bsz, steps):
    step = make(bsz)[route]
    for _ in range(WARM + steps):
        step()
    torch.cuda.synchronize()
    print(f"traced {WARM + steps} steps of route {route.upper()} at bsz {bsz}; build {_lib.build_id()}")


def summarize(out, pairs, steps, build):
    """Launch counts and kernel time per step from rocprofv3 kernel_stats.csv files; `build`: the
    build id the traced runs printed."""
    calls = WARM + steps
    lines = [f"One step's kernels, rocprofv3 --kernel-trace --stats over {calls} steps ({WARM} warm-up + "
             f"{steps}) of one route of",
             f"tools/supcon_probe.py per run (build {build}).  A: supcon_loss_torch -> backward.  "
             "B: supcon_loss -> backward.",
             f"Rows with fewer than {calls} calls are one-time set-up, not part of a step.", ""]
    for pair in pairs:
        label, path = pair.split("=", 1)
        with open(path, newline="") as fh:
            rows = [(r["Name"], int(r["Calls"]), float(r["TotalDurationNs"]),
                     float(r["AverageNs"])) for r in csv.DictReader(fh)]
        step_rows = [r for r in rows if r[1] >= calls]
        n = sum(r[1] // calls for r in step_rows)
        us = sum(r[3] * (r[1] // calls) for r in step_rows) / 1e3
        lines.append(f"{label}: {n} kernel launches per step, {us:.1f} us of kernel time per step")
        for name, cnt, _, avg in rows:
            name = name[5:] if name.startswith("void ") else name
            lines.append(f"    {cnt:3d} calls  {avg / 1e3:7.2f} us avg  {name[:110]}")
        lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("\n".join(lines))
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--bsz", type=int, nargs="+", default=[256, 1250])
    ap.add_argument("--trace", choices=ROUTES, help="run one route only (under rocprofv3)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", help="also write the report to this file")
    ap.add_argument("--summarize", nargs="+", metavar=("OUT", "LABEL=CSV"),
                    help="summarise kernel_stats.csv files instead of measuring")
    ap.add_argument("--build", default="?")
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize[0], a.summarize[1:], a.steps, a.build)
        return
    if not torch.cuda.is_available():
        sys.exit("supcon_probe: needs a GPU (no CPU fallback, nothing measured)")
    if a.trace:
        for b in a.bsz:
            trace(a.trace, b, a.steps)
        return
    if a.rounds < 5 or a.window < 0.5:
        sys.exit("supcon_probe: at least 5 rounds of windows of at least 0.5 s")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"supcon_probe: build {_lib.build_id()}, torch {torch.__version__}, "
         f"{torch.cuda.get_device_name(0)}; {a.rounds} rounds, windows >= {a.window} s")
    for b in a.bsz:
        ab(b, a.rounds, a.window, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
