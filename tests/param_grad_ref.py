"""Float64 closed form of the label_matrix / tau / epsilon gradients -- a test helper, not a test.

For a frozen kNN graph (oracle.gll_oracle: State, Graph.W, Graph.dist, edge_coefficients' wU),
with w = [0; wU], P = [Y; U] and the loss <gbar, U>:

    grad_Y[j, c] = sum_{i in N(j)} W_ji w_ic                                  rows j < base
    grad_tau     = - sum_{i >= base, c} w_ic U_ic
    grad_eps     = 1/2 sum_{directed edges (i, j)} G_ij W_ij 8 d_ij^2 / eps^3  fixed eps only
    G_ij         = sum_c (w_ic - w_jc)(P_jc - P_ic)

tests/test_param_grad_cpu.py pins these against central finite differences of oracle.forward.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from oracle import gll_oracle as O


@dataclass
class ParamGrads:
    grad_Y: np.ndarray      # base x C
    grad_tau: float
    tau_terms: float        # sum |w_ic U_ic|: the magnitude that does not cancel
    grad_eps: float | None  # None for epsilon = 'auto' (no epsilon input)
    eps_terms: float | None  # sum |edge terms|


def param_grads(state: O.State, gbar) -> ParamGrads:
    g = state.graph
    base = state.Y.shape[0]
    _, _, wU = O.edge_coefficients(state, gbar)
    w = np.concatenate([np.zeros_like(state.Y), wU], axis=0)
    P = np.concatenate([state.Y, state.U], axis=0)
    grad_Y = np.asarray(g.csr(g.W)[:base] @ w)
    t = wU * state.U
    grad_eps = eps_terms = None
    if not g.auto:
        r, c = g.rows, g.cols
        G = np.sum((w[r] - w[c]) * (P[c] - P[r]), axis=1)
        terms = 0.5 * G * g.W * 8.0 * g.dist ** 2 / g.eps[r] ** 3
        grad_eps, eps_terms = float(terms.sum()), float(np.abs(terms).sum())
    return ParamGrads(grad_Y, float(-t.sum()), float(np.abs(t).sum()), grad_eps, eps_terms)


def reference(X, Y, tau, eps, k, gbar, knn_idx):
    """(U, State, ParamGrads) of the oracle on the given kNN lists (exact float64 distances)."""
    U, st = O.forward(X, Y, tau, eps, k, knn=(np.asarray(knn_idx, dtype=np.int64), None))
    return U, st, param_grads(st, gbar)
