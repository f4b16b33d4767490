"""The kNN select's variants as test inputs: the sweep that must reach every row of the table of
instantiated kernels (select.hip; gll_select_route reports the row a problem takes, on the CPU)
and one small problem per row for the GPU test that runs every variant."""
import ctypes as ct

import numpy as np

from graphlearninglayer_amd import GLL as G
from graphlearninglayer_amd import _lib
from graphlearninglayer_amd.synth import synth

SWEEP = dict(
    n=(66, 520, 1000, 1024, 1025, 2048, 2049, 3000),
    d=(37, 64, 128, 129, 256, 257, 512, 513, 1024, 1028),
    K=(2, 13, 14, 29, 30, 57, 58, 129, 130, 257),
    B=(1, 2, 18, 64),
    aligned=(0, 1),
    panel=(0, 1),                                   # rows = n, or 1,024 with GLL_FLAG_KNN_PANEL
    flags=(0, _lib.FLAG_D2_F32, _lib.FLAG_GRAM_INLINE),
    form=(0, 1, 2),                                 # GLL_KNOB_SEL_FORM
)


def route(n, d, K, B=1, aligned=1, panel=0, flags=0, form=0):
    """(return code, the GLL_SEL_ROUTE_WORDS words) of gll_select_route, or None when the problem
    is not supported (no workspace, or row panels of a batch).  Sets and restores the knob."""
    lib = _lib.lib()
    p = G.make_problem(n, d, 0, 1, K, 0.0, "auto",
                       flags=flags | (_lib.FLAG_KNN_PANEL if panel else 0))
    if lib.gll_workspace_bytes(ct.byref(p)) == 0:
        return None
    rows = n
    if panel and n > 1024:   # panels of 1,024 rows: the buffer holds fewer rows than the graph
        if B > 1:
            return None
        rows = 1024
    out = (ct.c_int32 * 12)()
    _lib.set_knob(_lib.KNOB_SEL_FORM, form)
    try:
        rc = lib.gll_select_route(ct.byref(p), B, aligned, rows, out)
    finally:
        _lib.set_knob(_lib.KNOB_SEL_FORM, 0)
    return rc, list(out)


# One problem per table row, the cheapest of a small pool: (n, d, K, B, panel, form).  n = 520 /
# 1,025 / 2,049 hold the D2 row in one / two / no register chunks (CH), and 520 rows with
# 256 < d <= 512 take two planes (NP); d walks the ladder of (NU, XQ) and 37, 129, 257, 1030 the
# scalar loads; K = 10 / 20 / 40 are the three list capacities (KC), 70 and 140 the two tiers of
# the wide kernel; B = 18 x 520, 6 x 1,025 and 2 x 2,049 rows are the smallest batches on the
# pre-split Gram route (fp16 rows, H); a panel or form 2 reaches what the defaults do not.
POINTS = (
    (520, 512, 10, 1, 0, 0), (520, 64, 10, 1, 0, 0), (1025, 64, 10, 1, 0, 0),
    (1025, 64, 10, 1, 1, 0), (520, 256, 10, 1, 0, 0), (1025, 256, 10, 1, 0, 0),
    (1025, 256, 10, 1, 1, 0), (520, 257, 10, 1, 0, 0), (520, 37, 10, 1, 0, 0),
    (520, 129, 10, 1, 0, 0), (520, 512, 20, 1, 0, 0), (520, 64, 20, 1, 0, 0),
    (1025, 64, 20, 1, 0, 0), (1025, 64, 20, 1, 1, 0), (520, 256, 20, 1, 0, 0),
    (1025, 256, 20, 1, 0, 0), (1025, 256, 20, 1, 1, 0), (520, 257, 20, 1, 0, 0),
    (520, 37, 20, 1, 0, 0), (520, 129, 20, 1, 0, 0), (520, 512, 40, 1, 0, 0),
    (520, 64, 40, 1, 0, 0), (520, 256, 40, 1, 0, 0), (520, 257, 40, 1, 0, 0),
    (520, 37, 40, 1, 0, 0), (520, 129, 40, 1, 0, 0), (520, 512, 10, 1, 0, 2),
    (520, 64, 10, 1, 0, 2), (520, 64, 10, 18, 0, 0), (1025, 64, 10, 1, 0, 2),
    (1025, 64, 10, 6, 0, 0), (1025, 64, 10, 1, 1, 2), (2049, 64, 10, 2, 0, 0),
    (520, 512, 10, 2, 0, 0), (520, 512, 10, 18, 0, 0), (1025, 512, 10, 1, 0, 2),
    (1025, 512, 10, 6, 0, 0), (1025, 512, 10, 1, 1, 2), (2049, 512, 10, 2, 0, 0),
    (520, 1024, 10, 1, 0, 2), (520, 1024, 10, 18, 0, 0), (1025, 1024, 10, 1, 0, 2),
    (1025, 1024, 10, 6, 0, 0), (1025, 1024, 10, 1, 1, 2), (2049, 1024, 10, 2, 0, 0),
    (520, 1028, 10, 1, 0, 2), (520, 1028, 10, 18, 0, 0), (1025, 1028, 10, 1, 0, 2),
    (1025, 1028, 10, 6, 0, 0), (1025, 1028, 10, 1, 1, 2), (2049, 1028, 10, 2, 0, 0),
    (520, 257, 10, 1, 0, 2), (520, 37, 10, 1, 0, 2), (520, 37, 10, 18, 0, 0),
    (520, 1030, 10, 1, 0, 2), (2049, 1030, 10, 2, 0, 0), (520, 512, 20, 1, 0, 2),
    (520, 64, 20, 1, 0, 2), (520, 64, 20, 18, 0, 0), (1025, 64, 20, 1, 0, 2),
    (1025, 64, 20, 6, 0, 0), (1025, 64, 20, 1, 1, 2), (2049, 64, 20, 2, 0, 0),
    (520, 512, 20, 2, 0, 0), (520, 512, 20, 18, 0, 0), (1025, 512, 20, 1, 0, 2),
    (1025, 512, 20, 6, 0, 0), (1025, 512, 20, 1, 1, 2), (2049, 512, 20, 2, 0, 0),
    (520, 1024, 20, 1, 0, 2), (520, 1024, 20, 18, 0, 0), (1025, 1024, 20, 1, 0, 2),
    (1025, 1024, 20, 6, 0, 0), (1025, 1024, 20, 1, 1, 2), (2049, 1024, 20, 2, 0, 0),
    (520, 1028, 20, 1, 0, 2), (520, 1028, 20, 18, 0, 0), (1025, 1028, 20, 1, 0, 2),
    (1025, 1028, 20, 6, 0, 0), (1025, 1028, 20, 1, 1, 2), (2049, 1028, 20, 2, 0, 0),
    (520, 257, 20, 1, 0, 2), (520, 37, 20, 1, 0, 2), (520, 37, 20, 18, 0, 0),
    (520, 1030, 20, 1, 0, 2), (2049, 1030, 20, 2, 0, 0), (520, 512, 40, 1, 0, 2),
    (520, 64, 40, 1, 0, 2), (520, 64, 40, 18, 0, 0), (520, 512, 40, 2, 0, 0),
    (1025, 512, 40, 6, 0, 0), (520, 1024, 40, 1, 0, 2), (2049, 1024, 40, 2, 0, 0),
    (520, 1028, 40, 1, 0, 2), (2049, 1028, 40, 2, 0, 0), (520, 257, 40, 1, 0, 2),
    (520, 37, 40, 1, 0, 2), (520, 37, 40, 18, 0, 0), (520, 1030, 40, 1, 0, 2),
    (2049, 1030, 40, 2, 0, 0), (520, 64, 70, 1, 0, 0), (520, 512, 70, 1, 0, 0),
    (520, 37, 70, 1, 0, 0), (520, 257, 70, 1, 0, 0), (520, 64, 140, 1, 0, 0),
    (520, 512, 140, 1, 0, 0), (520, 37, 140, 1, 0, 0), (520, 257, 140, 1, 0, 0),
)


def features(n, d, B):
    """The B graphs of a point: synth features, seeds fixed by the shape."""
    return [synth(n // 2, n - n // 2, d, r=1.0, seed=4000 + 7 * g + n + d)[0] for g in range(B)]


def tie_rows(X, Ks, gap=1e-12):
    """{K: rows of X whose (K-1)-th and K-th nearest neighbours are within `gap` relative in
    exact float64 squared distance}: the rows on which two correct kNN sets could differ."""
    from oracle.graphlearning_standin import knn_exact
    dist = knn_exact(X, min(max(Ks) + 1, X.shape[0]))[1] ** 2
    out = {}
    for K in Ks:
        a, b = dist[:, K - 1], dist[:, K]
        out[K] = np.nonzero(b - a <= gap * b)[0].tolist()
    return out
