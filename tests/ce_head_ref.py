"""Float64 numpy reference of the cross-entropy head (include/gll.h gll_ce_head_batched) and the
inputs its tests share.

    p_i = U[i, t_i] + 1e-8;  row_loss_i = -log(p_i);  loss = sum_i row_loss_i / m
    gbar[i, c] = -(1 / m) / p_i at c == t_i, 0 elsewhere;  pred_i = first argmax of row i
A target outside [0, C) masks its row: row_loss 0, a zero gbar row, not counted as correct; the
divisor stays m.
"""
import collections
import functools

import numpy as np

from graphlearninglayer_amd.synth import CONFIGS, one_hot, synth

CeRef = collections.namedtuple("CeRef", "loss row_loss gbar pred_label correct")
CeCase = collections.namedtuple("CeCase", "base batch d C r seed k")

# tag -> synth arguments and k (the table of the feature's issue); eps / tau vary per test
CASES = {
    "T1": CeCase(32, 64, 16, 3, 0.75, 0, 6),
    "T1s1": CeCase(32, 64, 16, 3, 0.75, 1, 6),
    "T1s2": CeCase(32, 64, 16, 3, 0.75, 2, 6),
    "T2": CeCase(32, 65, 16, 3, 0.75, 0, 6),
    "T3": CeCase(32, 1, 16, 3, 0.75, 0, 6),
    "T4": CeCase(68, 130, 32, 17, 1.0, 0, 8),
    "T5": CeCase(400, 257, 32, 100, 2.0, 0, 8),
    "T6": CeCase(CONFIGS["plumbing"]["base"], CONFIGS["plumbing"]["batch"],
                 CONFIGS["plumbing"]["d"], 10, CONFIGS["plumbing"]["r"], 0, CONFIGS["plumbing"]["k"]),
    # just past the launcher's switch from one workgroup to the row pass + reduce (m > 4096)
    "T7": CeCase(32, 4100, 16, 3, 0.75, 0, 6),
    # the NS shape (500 + 500 x 512, k = 10): a single graph with fixed eps takes the fused
    # adjoint + gradient launch
    "NS": CeCase(CONFIGS["ns"]["base"], CONFIGS["ns"]["batch"], CONFIGS["ns"]["d"], 10,
                 CONFIGS["ns"]["r"], 0, CONFIGS["ns"]["k"]),
}
PAST_SWITCH = ("T7", 1.0, 0.07)
NS = ("NS", 1.0, 0.07)
# (tag, eps, tau) of the table, in its order
SETTINGS = [("T1", 1.0, 0.07), ("T1s1", 1.0, 0.07), ("T1s2", 1.0, 0.07), ("T2", "auto", 0.0),
            ("T3", 1.0, 0.07), ("T3", "auto", 0.0), ("T4", "auto", 0.07), ("T5", 1.0, 0.07),
            ("T5", "auto", 0.07), ("T6", 1.0, 0.07)]


@functools.lru_cache(maxsize=None)
def inputs(tag):
    """(X float32 n x d, Y float32 base x C one-hot, targets int64 m = labels of the unlabeled
    rows) of a case; shared, read-only."""
    c = CASES[tag]
    X, lab = synth(c.base, c.batch, c.d, C=c.C, r=c.r, seed=c.seed)
    Y = one_hot(lab[:c.base], c.C)
    t = lab[c.base:].copy()
    for a in (X, Y, t):
        a.setflags(write=False)
    return X, Y, t


def ce_head(U, targets):
    """The head on a float64 m x C prediction; targets int (m,), any value."""
    U = np.asarray(U, dtype=np.float64)
    t = np.asarray(targets, dtype=np.int64)
    m, C = U.shape
    valid = (t >= 0) & (t < C)
    rows = np.nonzero(valid)[0]
    row_loss = np.zeros(m)
    gbar = np.zeros((m, C))
    with np.errstate(divide="ignore", invalid="ignore"):
        p = U[rows, t[rows]] + 1e-8
        row_loss[rows] = -np.log(p)
        gbar[rows, t[rows]] = -(1.0 / m) / p
    pred = np.argmax(U, axis=1).astype(np.int64) if m else np.zeros(0, np.int64)
    loss = float(np.sum(row_loss) / m) if m else 0.0
    return CeRef(loss, row_loss, gbar, pred, int(np.sum(valid & (pred == t))))


def top2_gap(U):
    """Smallest difference between the two largest entries of a row."""
    s = np.sort(np.asarray(U, dtype=np.float64), axis=1)
    return float(np.min(s[:, -1] - s[:, -2]))
