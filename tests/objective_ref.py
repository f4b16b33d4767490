"""Float64 numpy reference of the score/objective head (include/gll.h
gll_objective_head_batched) and the plain-Python selection rule of DeviceScoreStore.

    p_i   = U[i, t_i] + 1e-8;  ce_i = -log(p_i)          (t_i outside [0, C): masked, ce_i = 0)
    ent_i = -sum_c U[i, c] log(U[i, c] + 1e-8);  sq_i = sum_c U[i, c]^2;  row_l2_i = 1 - sq_i
    loss  = (w_ce sum_i ce_i + w_ent sum_i ent_i - w_l2 sum_i sq_i) / m
    gbar[i, c] = (1 / m) (w_ce (-1 / p_i) [c == t_i]
                          - w_ent (log(U[i, c] + 1e-8) + U[i, c] / (U[i, c] + 1e-8))
                          - w_l2 2 U[i, c])
A term whose weight is exactly 0 is left out (it contributes exactly 0, even where it would be NaN);
masking touches the ce term, row_ce and correct alone; the divisor stays m.  Inputs: the cases
of tests/ce_head_ref.py.
"""
import collections

import numpy as np

WEIGHTS = [(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 0.3, 0.1)]

# row_abs: |w_ce ce_i| + |w_ent ent_i| + |w_l2 sq_i| per row (the scale of the loss sum's rounding);
# gbar_abs: the sum of the absolute terms of every gbar entry
ObRef = collections.namedtuple(
    "ObRef", "loss row_ce row_entropy row_l2 gbar pred_label correct row_abs gbar_abs ent_abs sq")


def objective(U, targets, weights=(1.0, 0.0, 0.0)):
    """The head on a float64 m x C prediction; targets int (m,) of any value, or None (every row
    masked)."""
    U = np.asarray(U, dtype=np.float64)
    m, C = U.shape
    t = np.full(m, -1, dtype=np.int64) if targets is None else np.asarray(targets, dtype=np.int64)
    w_ce, w_ent, w_l2 = (float(w) for w in weights)
    valid = (t >= 0) & (t < C)
    rows = np.nonzero(valid)[0]
    row_ce = np.zeros(m)
    inv_p = np.zeros(m)
    with np.errstate(divide="ignore", invalid="ignore"):
        p = U[rows, t[rows]] + 1e-8
        row_ce[rows] = -np.log(p)
        inv_p[rows] = 1.0 / p
        lg = np.log(U + 1e-8)
        row_entropy = -np.sum(U * lg, axis=1)
        ent_abs = np.sum(np.abs(U * lg), axis=1)
        sq = np.sum(U * U, axis=1)
        total = 0.0
        row_abs = np.zeros(m)
        gbar = np.zeros((m, C))
        gbar_abs = np.zeros((m, C))
        if w_ce != 0.0:
            total = total + w_ce * np.sum(row_ce)
            row_abs = row_abs + np.abs(w_ce * row_ce)
            gbar[rows, t[rows]] += w_ce * -inv_p[rows]
            gbar_abs[rows, t[rows]] += np.abs(w_ce * inv_p[rows])
        if w_ent != 0.0:
            total = total + w_ent * np.sum(row_entropy)
            row_abs = row_abs + np.abs(w_ent * row_entropy)
            gbar -= w_ent * (lg + U / (U + 1e-8))
            gbar_abs += np.abs(w_ent) * (np.abs(lg) + np.abs(U / (U + 1e-8)))
        if w_l2 != 0.0:
            total = total - w_l2 * np.sum(sq)
            row_abs = row_abs + np.abs(w_l2 * sq)
            gbar -= w_l2 * 2.0 * U
            gbar_abs += np.abs(w_l2 * 2.0 * U)
        loss = float(total / m) if m else 0.0
        gbar = gbar / m if m else gbar
        gbar_abs = gbar_abs / m if m else gbar_abs
    pred = np.argmax(U, axis=1).astype(np.int64) if m else np.zeros(0, np.int64)
    return ObRef(loss, row_ce, row_entropy, 1.0 - sq, gbar, pred, int(np.sum(valid & (pred == t))),
                 row_abs, gbar_abs, ent_abs, sq)


def select_by_score(scores, labels, num_samples, class_uniform_sample):
    """The selection of DeviceScoreStore.select_indices(mode='score') in plain Python: scores
    descending, equal scores by ascending index, NaN after every number (-inf included); with
    class_uniform_sample num_samples // (classes present) per class -- or the class's size --
    classes in the order of their first appearance in `labels`."""
    scores = [float(s) for s in scores]
    labels = [int(v) for v in labels]

    def ranked(idx):
        numbers = [i for i in idx if scores[i] == scores[i]]
        nans = [i for i in idx if scores[i] != scores[i]]
        # Python's sort is stable; reverse=True keeps the original order of equal keys
        return sorted(numbers, key=lambda i: scores[i], reverse=True) + nans

    if not class_uniform_sample:
        return ranked(range(len(scores)))[:max(num_samples, 0)]
    classes = {}
    for i, c in enumerate(labels):
        classes.setdefault(c, []).append(i)   # insertion order = first appearance
    per_class = num_samples // len(classes)
    out = []
    for idx in classes.values():
        out.extend(ranked(idx)[:min(per_class, len(idx))])
    return out
