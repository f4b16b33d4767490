"""A/B of one score-mode training step's head (GPU only: fails without a device).

    A: loss, pred, labels, row_loss, correct = ce_loss(X, Y, t, tau, eps, k)
       s = row_loss.float()                          ('entropy')
       s = (1 - torch.sum(pred ** 2, 1)).float()     ('l2')
       scores[indices] = s; loss.backward()
    B: loss, ... = objective(X, Y, t, tau, eps, k, score=, score_out=scores, indices=indices)
       loss.backward()

A is what a caller of this library writes without `objective`; B is the fused call.  Both at the
NS shape (synth.CONFIGS["ns"]) and at FullySup, eps = 1, tau = 0.07, X a leaf that requires
grad, for both scores.  Both steps are warmed up, then timed in alternating windows of at least
--window seconds (a host clock around a device synchronise), --rounds rounds in one process; the
report gives each step's median and spread (min .. max) over its windows and A - B beside the
largest spread.  The reference's own store -- one `scores_cpu[i] = s_i` per sample with a 0-d
device tensor on the right (FullySup.py:174-175, utils.py:765-766) -- is timed once over
--loop-steps steps, for the record.  The head kernels' own times come from the library's event
brackets (gll_prof_enable(GLL_K_LOSS)) around `ce_loss` and around `objective`.

    python tools/score_probe.py [--rounds 5] [--window 0.5] [--out profiles/x.txt]
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
from graphlearninglayer_amd.base_data import DeviceScoreStore  # noqa: E402
from graphlearninglayer_amd.synth import CONFIGS, one_hot, synth  # noqa: E402

EPS, TAU = 1.0, 0.07
WARM = 3
N_STORE = 50000    # the CIFAR training set the reference scores


def make(shape, score):
    c = CONFIGS[shape]
    X, lab = synth(c["base"], c["batch"], c["d"], r=c["r"], seed=0)
    dev = torch.device("cuda", 0)
    Xt = torch.from_numpy(X).to(dev).requires_grad_(True)
    Y = torch.from_numpy(one_hot(lab[: c["base"]])).to(dev)
    t = torch.from_numpy(lab[c["base"]:]).to(dev)
    store = DeviceScoreStore(torch.arange(N_STORE) % 10, device=dev, seed=0)
    ind = torch.randperm(N_STORE, device=dev,
                         generator=torch.Generator(device=dev).manual_seed(1))[: c["batch"]]
    ind_cpu = ind.cpu()
    L = GLL.LaplaceLearningSparseHard

    def torch_scores(pred, row_loss):
        if score == "entropy":
            return row_loss.float()
        return (1 - torch.sum(pred ** 2, 1)).float()

    def step_a():
        Xt.grad = None
        loss, pred, labels, row_loss, _ = L.ce_loss(Xt, Y, t, TAU, EPS, c["k"])
        store.scores[ind] = torch_scores(pred, row_loss)
        loss.backward()
        return loss

    def step_b():
        Xt.grad = None
        loss = L.objective(Xt, Y, t, TAU, EPS, c["k"], score=score, score_out=store.scores,
                           indices=ind)[0]
        loss.backward()
        return loss

    def step_loop(scores_cpu):
        """The reference's store: one assignment per sample into a CPU tensor."""
        Xt.grad = None
        loss, pred, labels, row_loss, _ = L.ce_loss(Xt, Y, t, TAU, EPS, c["k"])
        for i, s in zip(ind_cpu, torch_scores(pred, row_loss)):   # the loader's indices: CPU
            scores_cpu[i] = s
        loss.backward()
        return loss

    return c, store, ind, step_a, step_b, step_loop


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


def kernel_us(step, n=200):
    """Mean time of the GLL_K_LOSS bracket over n steps (microseconds)."""
    for _ in range(WARM):
        step()
    torch.cuda.synchronize()
    _lib.prof_read(_lib.K_LOSS)
    _lib.prof_enable(_lib.K_LOSS, 1)
    try:
        for _ in range(n):
            step()
        torch.cuda.synchronize()
        ms, cnt = _lib.prof_read(_lib.K_LOSS)
    finally:
        _lib.prof_enable(_lib.K_LOSS, 0)
    return ms / max(cnt, 1) * 1e3, cnt


def ab(shape, score, rounds, seconds, loop_steps, emit):
    c, store, ind, step_a, step_b, step_loop = make(shape, score)
    tag = f"[{shape} {score}]"
    for _ in range(WARM * 10):
        la = step_a()
    sa = store.scores[ind].clone()
    store.scores.zero_()
    for _ in range(WARM * 10):
        lb = step_b()
    torch.cuda.synchronize()
    sb = store.scores[ind]
    emit(f"{tag} base {c['base']} + batch {c['batch']} x d {c['d']}, k {c['k']}, eps {EPS}, "
         f"tau {TAU}; loss A {float(la.detach()):.12g}  B {float(lb.detach()):.12g}; "
         f"stored scores max |A - B| {float((sa - sb).abs().max()):.3g}")
    ta, tb = [], []
    for r in range(rounds):
        ta.append(window(step_a, seconds))
        tb.append(window(step_b, seconds))
        emit(f"{tag} round {r}: A {ta[-1]:8.2f} us/step   B {tb[-1]:8.2f} us/step")
    ma, mb = statistics.median(ta), statistics.median(tb)
    emit(f"{tag} A median {ma:.2f} us (min {min(ta):.2f} .. max {max(ta):.2f})")
    emit(f"{tag} B median {mb:.2f} us (min {min(tb):.2f} .. max {max(tb):.2f})")
    spread = max(max(ta) - min(ta), max(tb) - min(tb))
    emit(f"{tag} A - B = {ma - mb:.2f} us ({(ma - mb) / ma * 100:.1f}% of A); largest spread "
         f"of one step over its windows {spread:.2f} us; B faster beyond the spread: "
         f"{ma - mb > spread}")
    ka, na = kernel_us(step_a)
    kb, nb = kernel_us(step_b)
    emit(f"{tag} head kernel (GLL_K_LOSS bracket, mean of {na} / {nb}): ce_head_kernel "
         f"{ka:.2f} us, objective_head_kernel {kb:.2f} us")
    scores_cpu = torch.zeros(N_STORE)
    step_loop(scores_cpu)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(loop_steps):
        step_loop(scores_cpu)
    torch.cuda.synchronize()
    emit(f"{tag} the reference's per-sample store loop: {(time.perf_counter() - t0) / loop_steps * 1e6:.0f} "
         f"us/step over {loop_steps} steps ({c['batch']} assignments a step)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--shape", choices=["ns", "fullysup", "both"], default="both")
    ap.add_argument("--score", choices=["entropy", "l2", "both"], default="both")
    ap.add_argument("--loop-steps", type=int, default=20)
    ap.add_argument("--out", help="also write the report to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("score_probe: needs a GPU (no CPU fallback, nothing measured)")
    if a.rounds < 5 or a.window < 0.5:
        sys.exit("score_probe: at least 5 rounds of windows of at least 0.5 s")
    shapes = ["ns", "fullysup"] if a.shape == "both" else [a.shape]
    scores = ["entropy", "l2"] if a.score == "both" else [a.score]
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"score_probe: build {_lib.build_id()}, torch {torch.__version__}, "
         f"{torch.cuda.get_device_name(0)}; {a.rounds} rounds, windows >= {a.window} s")
    for s in shapes:
        for sc in scores:
            ab(s, sc, a.rounds, a.window, a.loop_steps, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
