"""What the parity tests (tests/test_gpu_parity.py, _cg, _backward, _laplace) share:
the parity bar, the layer through autograd, the GPU's own kNN lists, and forward / backward runs
through the C ABI (tests/abi.py Run) -- a test helper, not a test."""
import contextlib

import numpy as np
import torch

from graphlearninglayer_amd import GLL
from graphlearninglayer_amd import _lib as L
from oracle import gll_oracle as O
from tests import abi as A
from tests.launch_counts import counted

TOL = 1e-4


def run_layer(X, Y, tau, eps, k, gbar, dev="cuda"):
    Xt = torch.from_numpy(np.ascontiguousarray(X)).to(dev).requires_grad_(True)
    Yt = torch.from_numpy(np.ascontiguousarray(Y)).to(dev)
    U = GLL.LaplaceLearningSparseHard.apply(Xt, Yt, tau, eps, k)
    U.backward(torch.from_numpy(gbar).to(U.device))
    torch.cuda.synchronize()
    return U.detach().cpu().numpy(), Xt.grad.detach().cpu().numpy()


def gpu_knn(X, k, eps="auto"):
    return GLL.device_graph(torch.from_numpy(np.ascontiguousarray(X)).cuda(), k, eps)


def synth_batch(cfg, B, seed0=0):
    from graphlearninglayer_amd.synth import CONFIGS, one_hot, synth
    c = CONFIGS[cfg]
    Xs, Ys = [], []
    for g in range(B):
        X, lab = synth(c["base"], c["batch"], c["d"], r=c["r"], seed=seed0 + g)
        Xs.append(X)
        Ys.append(one_hot(lab[: c["base"]]))
    return np.stack(Xs), np.stack(Ys), c


def exact_knn_rows(X, ind, k):
    """Rows whose GPU kNN set differs from the exact float64 set (ties at 1e-12 excused)."""
    return O.knn_set_mismatch(X, ind, k, rel_gap=1e-12)


def forward_c_abi(X, Y, k, tau, eps, flags=0, status=None):
    """gll_forward with explicit problem flags: (U, fwd iterations, non-converged columns);
    `status` (a list) receives the public status words."""
    run = A.Run(X, Y, k, tau, eps, flags)
    U = run.forward()
    st = run.status()
    if status is not None:
        status.extend(st)
    return U, st[L.ST_FWD_ITERS], st[L.ST_FWD_NONCONV]


def fwd_bwd_c_abi(X, Y, k, tau, eps, gbar, flags=0, bwd_flags=None, ws_fill=None, counts=False):
    """gll_forward + gll_backward with explicit problem flags: (U, grad_X).  `bwd_flags`: the
    backward's own flags (default: the forward's); `ws_fill`: a byte value the workspace holds
    before the forward; `counts`: also return the backward's launches (tests/launch_counts.py)."""
    run = A.Run(X, Y, k, tau, eps, flags, ws_fill=ws_fill)
    U = run.forward()
    with (counted() if counts else contextlib.nullcontext()) as got:
        gx = run.backward(gbar, flags=flags if bwd_flags is None else bwd_flags)
    return (U, gx, got) if counts else (U, gx)


def fwd_bwds_c_abi(X, Y, k, tau, eps, gbar, flags=0, backward_calls=1, counts=False):
    """gll_forward then `backward_calls` x gll_backward (NULL labels) on ONE workspace:
    (U, [grad_X], status words) and, with `counts`, the launches of each backward."""
    run = A.Run(X, Y, k, tau, eps, flags)
    U = run.forward()
    grads, ran = [], []
    for _ in range(backward_calls):
        with (counted() if counts else contextlib.nullcontext()) as got:
            grads.append(run.backward(gbar, labels=False))
        ran.append(got.counts if counts else None)
    return (U, grads, run.status(), ran) if counts else (U, grads, run.status())


def fwd_bwd_batched_c_abi(Xs, Ys, k, tau, eps, G, flags=0, ws=None):
    """gll_forward_batched + gll_backward_batched: (U[B], grad_X[B], the Run).  `ws`: a workspace
    to reuse (default: a fresh torch.empty one)."""
    run = A.Run(Xs, Ys, k, tau, eps, flags, ws=ws)
    U = run.forward()
    return U, run.backward(G), run


def batched_knn_lists(run):
    """Each graph's kNN list (n x K int64) read from its block of a batched Run's workspace: the
    lists the batched select kernel itself wrote."""
    K = min(run.k, run.n)
    return [run.array(run.view(g).knn_idx, run.n * K, np.int32, g).reshape(run.n, K)
            .astype(np.int64) for g in range(run.B)]
