"""Float64 numpy reference of the Carlini-Wagner margin head (include/gll.h
gll_margin_head_batched).

    a_i = lowest index among the maxima of row i
    s_i = lowest index among the maxima of the row with entry a_i removed; 0 for C = 1
    d_i = U[i, a_i] - U[i, other_i];  row_margin_i = d_i if d_i >= 0 or d_i is NaN, else 0
    loss = sum_i row_margin_i / m;  gbar[i, c] = float32(1 / m) * ([c == a_i] - [c == other_i])
    moved = #{i : a_i == other_i}
Ranking: numbers by value descending, NaN entries after every number, each by index ascending (a
NaN is never a maximum while a number is left; a row of NaN has a = 0, s = 1).  An other_i
outside [0, C) -- or other = None: every row -- masks the row: margin 0, a zero gbar row, not
counted as moved; labels and second are still written and the divisor stays m.
"""
import collections

import numpy as np

from tests import ce_head_ref as R

MarginRef = collections.namedtuple("MarginRef", "loss row_margin gbar labels second moved")

# (tag, eps, tau) of tests/ce_head_ref.py the layer-level GPU tests run
LAYER_CASES = [("T1", 1.0, 0.07), ("T2", "auto", 0.0), ("T4", "auto", 0.07), ("T5", 1.0, 0.07),
               ("T5", "auto", 0.07), R.PAST_SWITCH, R.NS]
# of those, the cases whose float64 oracle keeps the top-1/top-2 and the top-2/top-3 gap of every
# row above 1e-4 (asserted in test_margin_head_cpu.py)
WELL_SEPARATED = [("T1", 1.0, 0.07), ("T5", 1.0, 0.07)]


def rank(U):
    """The class indices of every row in ranking order (m x C): sorted by (is NaN, -value,
    index).  -0.0 and 0.0 are equal values, so their indices decide."""
    U = np.asarray(U, dtype=np.float64)
    nan = np.isnan(U)
    neg = np.where(nan, 0.0, -U) + 0.0            # + 0.0: -0.0 becomes 0.0
    idx = np.broadcast_to(np.arange(U.shape[1]), U.shape)
    return np.lexsort((idx, neg, nan), axis=1)    # the last key is the primary one


def margin_head(U, other=None):
    """The head on an m x C prediction (float32 or float64; evaluated in float64); other: int
    (m,), any value, or None.  gbar is float32, as the kernel writes it."""
    U = np.asarray(U, dtype=np.float64)
    m, C = U.shape
    o = np.full(m, -1, dtype=np.int64) if other is None else np.asarray(other, dtype=np.int64)
    assert o.shape == (m,)
    order = rank(U)
    labels = order[:, 0].astype(np.int64) if m else np.zeros(0, np.int64)
    second = order[:, 1].astype(np.int64) if C > 1 else np.zeros(m, np.int64)
    valid = (o >= 0) & (o < C)
    rows = np.nonzero(valid)[0]
    row_margin = np.zeros(m)
    with np.errstate(invalid="ignore"):
        d = U[rows, labels[rows]] - U[rows, o[rows]]      # inf - inf = NaN, as the kernel's
    row_margin[rows] = np.where((d >= 0) | np.isnan(d), d, 0.0)
    hit = valid & (labels == o)
    live = np.nonzero(valid & ~hit)[0]
    gbar = np.zeros((m, C), dtype=np.float32)
    if m:
        gbar[live, labels[live]] = np.float32(1.0 / m)
        gbar[live, o[live]] = -np.float32(1.0 / m)
    loss = float(np.sum(row_margin) / m) if m else 0.0
    return MarginRef(loss, row_margin, gbar, labels, second, int(hit.sum()))


def top3_gaps(U):
    """(smallest top-1/top-2 gap, smallest top-2/top-3 gap) over the rows; the second is inf for
    C < 3."""
    s = np.sort(np.asarray(U, dtype=np.float64), axis=1)
    g12 = float(np.min(s[:, -1] - s[:, -2]))
    g23 = float(np.min(s[:, -2] - s[:, -3])) if s.shape[1] >= 3 else float("inf")
    return g12, g23
