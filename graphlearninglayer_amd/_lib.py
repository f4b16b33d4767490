"""ctypes binding of libgll.so (the C ABI of include/gll.h).

The shared library is built in-tree by `graphlearninglayer_amd.build` (or
`__graft_entry__.build()`).  There is no fallback: if it is missing, `lib()` raises.
"""
from __future__ import annotations

import ctypes as ct
import os
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GLL_LIB_PATH") or os.path.join(HERE, "libgll.so")  # env: A/B builds

GLL_OK = 0
GLL_DT_F32, GLL_DT_F64, GLL_DT_I64 = 0, 1, 2
# gll_problem.flags (include/gll.h): code-path choices for tests and A/B runs
FLAG_CG_GRID = 1          # force the whole-GPU CG
FLAG_CG_PERCOL = 8        # per-column CG for large single graphs
FLAG_DIAG_GRID_OVERSUB = 128   # tests: whole-GPU CG grid past co-residency (launch refused)
FLAG_DIAG_GRID_FAIL = 256      # tests: injected grid-barrier failure
FLAG_CG_ELL = 512         # register-ELL per-column CG where the balanced one runs
FLAG_CG_VR = 1024         # balanced (virtual-row) per-column CG wherever it fits
FLAG_GRAD_ROWS = 2048     # whole-row feature-gradient kernel
FLAG_GRAD_CHUNK = 4096    # feature-chunked gradient kernel wherever it runs
FLAG_GRAM_INLINE = 8192   # 128-tile Gram with the inline split
FLAG_BWD_UNFUSED = 16384  # adjoint CG and gradient as two launches
FLAG_KNN_PANEL = 65536    # kNN in row panels (O(panel x n) distances)
FLAG_D2_F32 = 131072      # fp32 distance matrix on the pre-split Gram route
FLAG_ROW_ORDER_OFF = 262144   # large single graphs: row-index order instead of the locality order
FLAG_KNN_GIVEN = 524288   # caller-supplied neighbour lists (gll_forward_lists_batched): no n x n buffer
# process-wide test knobs (gll_set_knob): force a code path, 0 = automatic
KNOB_VR_RV, KNOB_GRID_CAP, KNOB_GRAM_TILE, KNOB_SEL_FORM, KNOB_GRAM_TAIL, KNOB_ROW_PRE = 0, 1, 2, 3, 4, 5
KNOB_GRAD_SPLIT = 6   # fused backward: long rows in feature parts (0 automatic, 1 on, 2 off)
ST_TINY_EPS, ST_FWD_NONCONV, ST_FWD_ITERS, ST_BWD_NONCONV, ST_BWD_ITERS = 0, 1, 2, 3, 4
ST_KNN_RESCAN = 5   # kNN rows re-ranked over every column under the Gram error bound
ST_SOLVE_FAILED = 6   # the fused backward gave up on its adjoint solves: grad NaN, raised
ST_GRID_RESCUED = 10  # whole-GPU CG solves rescued by one workgroup after a lost grid barrier
ST_KNN_MERGE = 7   # kNN rows that took the full-row select fallback (diagnostic)
ST_GRAD_SPLIT = 12  # rows the last fused backward ran as 2 or 4 waves over feature parts (diagnostic)
ST_LIST_DROPPED = 13  # caller-supplied list entries dropped as out of range or repeated (count)
ST_NWORDS = 16
K_GRAM, K_SELECT, K_FINALIZE, K_CG, K_EDGE, K_GRAD = range(6)
K_BWD = 6     # cg_grad_fused_kernel
K_PARAM = 7   # param_grad_kernel: label_matrix / tau / eps gradients
K_LOSS = 8    # ce_head_kernel: cross-entropy head (gll_ce_head_batched)
K_COUNT = 9
PG_Y, PG_TAU, PG_EPS = 1, 2, 4   # gll_param_grad_batched `what` bits
SCORE_NONE, SCORE_ENTROPY, SCORE_L2 = 0, 1, 2   # gll_objective_head_batched score_kind
XT_F32, XT_F16, XT_BF16 = 0, 1, 2  # gll_features_* element types of Z / gZ
UF_NORMALIZE = 1                 # gll_features_* flag: unit-norm rows
MAX_D_FEATURES = 4096            # gll_features_*: 1 <= d <= 4096 (one wave holds a row)
SC_ALL, SC_ONE = 0, 1            # gll_supcon_* mode
# supcon.hip tiling (csrc/gll_internal.h kSc*): an MFMA tile is SC_TILE x SC_TILE logits, a
# workgroup owns SC_ROWS anchor rows and one chunk of column tiles, features go SC_KC at a time
SC_TILE, SC_ROWS, SC_KC, SC_TARGET_WG, SC_PART_BYTES, SC_MIN_BUDGET = 32, 64, 128, 512, 32, 3 << 20
SC_TARGET_WG_FWD = 1024
SC_MAX_ROWS = 65536
QF_SMALL_PANELS = 1              # gll_knn_query flag: 64-row panels (tests: the multi-panel path)
QUERY_MAX_K, QUERY_MAX_C = 256, 256   # gll_knn_query k / gll_extend kn and C
QUERY_MAX_N = (2**31 - 1) // 2
QST_RESCAN, QST_NONFINITE, QST_ZERO_SUM = 0, 1, 2   # gll_knn_query / gll_extend status words
QST_NWORDS = 4
RR_KEEP_ORDER = 1                # gll_knn_rerank flag: list mode, the caller's order kept (c == k)
RERANK_MAX_C = 512               # gll_knn_rerank: candidates per row (the wave's slots)
QST_SHORT_ROW = 3                # gll_knn_rerank: pool rows with fewer than k valid candidates
EG_XQ, EG_XDB, EG_P, EG_EPS = 1, 2, 4, 8   # gll_extend_backward `what` bits
EGF_SMALL_LISTS = 1              # gll_extend_backward flag: 64-entry in-LDS lists (tests: the long-list path)
EGST_ZERO_SUM, EGST_LONG_LIST = 2, 3   # gll_extend_backward status words


def supcon_plan(rows: int, d: int):
    """(column tiles, row blocks, chunks, tiles per chunk, forward chunks, tiles per forward
    chunk) of gll_supcon_* for (rows, d): the host-side mirror of supcon.hip supcon_plan;
    gll_supcon_scratch_bytes = 32 rows fchunks + 4 d rows chunks, the second term only for
    chunks > 1."""
    ntiles, rowblocks = -(-rows // SC_TILE), -(-rows // SC_ROWS)
    per = rows * (4 * d + SC_PART_BYTES)
    nc = max(1, min(-(-SC_TARGET_WG // rowblocks), max(2 * rows * rows, SC_MIN_BUDGET) // per, ntiles))
    tpc = -(-ntiles // nc)
    ftpc = -(-ntiles // min(-(-SC_TARGET_WG_FWD // rowblocks), ntiles))
    return ntiles, rowblocks, -(-ntiles // tpc), tpc, -(-ntiles // ftpc), ftpc

# every symbol include/gll.h declares (tests check the library exports all of them)
EXPORTS = (
    "gll_workspace_bytes", "gll_forward", "gll_backward", "gll_forward_batched",
    "gll_backward_batched", "gll_param_grad_scratch_bytes", "gll_param_grad_batched",
    "gll_ce_head_scratch_bytes", "gll_ce_head_batched", "gll_margin_head_scratch_bytes",
    "gll_margin_head_batched", "gll_graph", "gll_workspace_view",
    "gll_cg_csr_workspace_bytes", "gll_cg_csr", "gll_prof_enable", "gll_prof_read",
    "gll_kernel_name", "gll_strerror", "gll_set_knob", "gll_build_id", "gll_select_route",
    "gll_workspace_solve_view", "gll_workspace_knn_view", "gll_gram_route",
    "gll_features_forward", "gll_features_backward", "gll_features_calls", "gll_fused_plan",
    "gll_objective_head_scratch_bytes", "gll_objective_head_batched",
    "gll_supcon_scratch_bytes", "gll_supcon_forward", "gll_supcon_backward", "gll_supcon_launches",
    "gll_query_workspace_bytes", "gll_knn_query", "gll_extend", "gll_query_launches",
    "gll_extend_grad_workspace_bytes", "gll_extend_backward", "gll_extend_grad_launches",
    "gll_forward_lists_batched", "gll_graph_lists", "gll_cg_route", "gll_knn_rerank",
)


class Problem(ct.Structure):
    _fields_ = [
        ("n", ct.c_int32), ("d", ct.c_int32), ("base", ct.c_int32), ("C", ct.c_int32),
        ("K", ct.c_int32), ("max_iter", ct.c_int32), ("tau", ct.c_float), ("eps", ct.c_float),
        ("rtol", ct.c_float), ("flags", ct.c_int32), ("status_sink", ct.c_void_p),
    ]


class View(ct.Structure):
    _fields_ = [(name, ct.c_void_p) for name in (
        "knn_idx", "knn_d2", "eps", "row_start", "row_len", "col", "w", "d2", "deg", "U32",
        "wadj", "status")]


class SolveView(ct.Structure):
    """gll_solve_view: what the row build writes for the Luu solves (include/gll.h)."""
    _fields_ = [(name, ct.c_void_p) for name in ("ucnt", "diag", "rhs", "P", "ell", "vr")] + [
        (name, ct.c_int32) for name in ("SE", "VRM", "Wcap", "RCAP")]


class KnnView(ct.Structure):
    """gll_knn_view: what the Gram and the locality order leave in a workspace (include/gll.h)."""
    _fields_ = [(name, ct.c_void_p) for name in (
        "D2", "d2_scale", "xhi", "xlo", "xnrm", "pid", "perm")] + [("plane_stride", ct.c_int64)] + [
        (name, ct.c_int32) for name in ("planes", "ldD", "rows", "d2_half", "dp", "order")]


GRAM_ROUTE_WORDS = 9
# gll_gram_route out[0]
GRAM_BF3, GRAM_BF3H, GRAM_BF3S, GRAM_BF3W, GRAM_PK, GRAM_PK2 = range(6)

_lock = threading.Lock()
_lib = None


def _declare(lib):
    P = ct.POINTER(Problem)
    vp, i32, sz = ct.c_void_p, ct.c_int, ct.c_size_t
    lib.gll_workspace_bytes.argtypes = [P]
    lib.gll_workspace_bytes.restype = sz
    lib.gll_forward.argtypes = [P, vp, vp, i32, vp, vp, vp]
    lib.gll_forward.restype = i32
    lib.gll_backward.argtypes = [P, vp, vp, i32, vp, vp, i32, vp, vp]
    lib.gll_backward.restype = i32
    lib.gll_forward_batched.argtypes = [P, i32, vp, vp, i32, vp, vp, vp]
    lib.gll_forward_batched.restype = i32
    lib.gll_backward_batched.argtypes = [P, i32, vp, vp, vp, i32, vp, vp]
    lib.gll_backward_batched.restype = i32
    lib.gll_param_grad_scratch_bytes.argtypes = [P, i32]
    lib.gll_param_grad_scratch_bytes.restype = sz
    lib.gll_param_grad_batched.argtypes = [P, i32, vp, i32, vp, vp, vp, vp, vp]
    lib.gll_param_grad_batched.restype = i32
    lib.gll_ce_head_scratch_bytes.argtypes = [P, i32]
    lib.gll_ce_head_scratch_bytes.restype = sz
    lib.gll_ce_head_batched.argtypes = [P, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.gll_ce_head_batched.restype = i32
    lib.gll_margin_head_scratch_bytes.argtypes = [P, i32]
    lib.gll_margin_head_scratch_bytes.restype = sz
    lib.gll_margin_head_batched.argtypes = [P, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.gll_margin_head_batched.restype = i32
    lib.gll_objective_head_scratch_bytes.argtypes = [P, i32]
    lib.gll_objective_head_scratch_bytes.restype = sz
    f64 = ct.c_double
    lib.gll_objective_head_batched.argtypes = [P, i32, vp, vp, f64, f64, f64, vp, vp, vp, vp, vp,
                                               vp, vp, i32, vp, ct.c_int64, vp, vp, vp]
    lib.gll_objective_head_batched.restype = i32
    lib.gll_graph.argtypes = [P, vp, vp, vp]
    lib.gll_graph.restype = i32
    lib.gll_workspace_view.argtypes = [P, vp, ct.POINTER(View)]
    lib.gll_workspace_view.restype = i32
    lib.gll_workspace_solve_view.argtypes = [P, vp, ct.POINTER(SolveView)]
    lib.gll_workspace_solve_view.restype = i32
    lib.gll_workspace_knn_view.argtypes = [P, i32, vp, ct.POINTER(KnnView)]
    lib.gll_workspace_knn_view.restype = i32
    lib.gll_gram_route.argtypes = [P, i32, i32, i32, ct.POINTER(ct.c_int32)]
    lib.gll_gram_route.restype = i32
    lib.gll_cg_csr_workspace_bytes.argtypes = [i32, i32]
    lib.gll_cg_csr_workspace_bytes.restype = sz
    lib.gll_cg_csr.argtypes = [i32, i32, vp, vp, vp, vp, vp, ct.c_float, i32, vp, vp, vp, vp]
    lib.gll_cg_csr.restype = i32
    lib.gll_prof_enable.argtypes = [i32, i32]
    lib.gll_prof_enable.restype = i32
    lib.gll_prof_read.argtypes = [i32, ct.POINTER(ct.c_double), ct.POINTER(ct.c_int)]
    lib.gll_prof_read.restype = i32
    lib.gll_kernel_name.argtypes = [i32]
    lib.gll_kernel_name.restype = ct.c_char_p
    lib.gll_select_route.argtypes = [ct.POINTER(Problem), i32, i32, i32, ct.POINTER(ct.c_int32)]
    lib.gll_select_route.restype = i32
    lib.gll_cg_route.argtypes = [ct.POINTER(Problem), i32, ct.POINTER(ct.c_int32)]
    lib.gll_cg_route.restype = i32
    lib.gll_fused_plan.argtypes = [ct.POINTER(Problem), i32, i32, ct.POINTER(ct.c_int32)]
    lib.gll_fused_plan.restype = i32
    lib.gll_set_knob.argtypes = [i32, i32]
    lib.gll_set_knob.restype = i32
    lib.gll_strerror.argtypes = [i32]
    lib.gll_strerror.restype = ct.c_char_p
    lib.gll_build_id.argtypes = []
    lib.gll_build_id.restype = ct.c_char_p
    lib.gll_features_forward.argtypes = [ct.c_int64, ct.c_int32, vp, i32, i32, vp, vp, vp]
    lib.gll_features_forward.restype = i32
    lib.gll_features_backward.argtypes = [ct.c_int64, ct.c_int32, vp, vp, vp, i32, vp, i32, vp]
    lib.gll_features_backward.restype = i32
    lib.gll_features_calls.argtypes = []
    lib.gll_features_calls.restype = ct.c_int64
    f32 = ct.c_float
    lib.gll_supcon_scratch_bytes.argtypes = [ct.c_int64, ct.c_int32]
    lib.gll_supcon_scratch_bytes.restype = sz
    lib.gll_supcon_forward.argtypes = [ct.c_int64, ct.c_int32, ct.c_int32, vp, vp, i32, f32, f32,
                                       vp, vp, vp, vp, vp]
    lib.gll_supcon_forward.restype = i32
    lib.gll_supcon_backward.argtypes = [ct.c_int64, ct.c_int32, ct.c_int32, vp, vp, i32, f32, f32,
                                        vp, vp, vp, vp, vp]
    lib.gll_supcon_backward.restype = i32
    lib.gll_supcon_launches.argtypes = []
    lib.gll_supcon_launches.restype = ct.c_int64
    i64 = ct.c_int64
    lib.gll_query_workspace_bytes.argtypes = [i64, i64, ct.c_int32, ct.c_int32, i32]
    lib.gll_query_workspace_bytes.restype = sz
    lib.gll_knn_query.argtypes = [i64, i64, ct.c_int32, ct.c_int32, i32, vp, vp, vp, vp, vp, vp, vp]
    lib.gll_knn_query.restype = i32
    lib.gll_extend.argtypes = [i64, i64, ct.c_int32, ct.c_int32, vp, vp, vp, vp, f32, vp, vp, vp, vp]
    lib.gll_extend.restype = i32
    lib.gll_knn_rerank.argtypes = [i64, i64, ct.c_int32, ct.c_int32, ct.c_int32, i32, vp, vp, vp, vp,
                                   vp, vp, vp]
    lib.gll_knn_rerank.restype = i32
    lib.gll_query_launches.argtypes = []
    lib.gll_query_launches.restype = ct.c_int64
    i32s = ct.c_int32
    lib.gll_extend_grad_workspace_bytes.argtypes = [i64, i64, i32s, i32s, i32s, i32, i32]
    lib.gll_extend_grad_workspace_bytes.restype = sz
    lib.gll_extend_backward.argtypes = [i64, i64, i32s, i32s, i32s, vp, vp, vp, vp, vp, vp, f32, vp,
                                        i32, i32, vp, vp, vp, vp, vp, vp, vp]
    lib.gll_extend_backward.restype = i32
    lib.gll_extend_grad_launches.argtypes = []
    lib.gll_extend_grad_launches.restype = ct.c_int64
    lib.gll_forward_lists_batched.argtypes = [P, i32, vp, vp, vp, i32, vp, vp, vp]
    lib.gll_forward_lists_batched.restype = i32
    lib.gll_graph_lists.argtypes = [P, vp, vp, vp, vp]
    lib.gll_graph_lists.restype = i32
    return lib


def build_id() -> str:
    """The loaded library's build identity (build.py source_digest at its build)."""
    return lib().gll_build_id().decode()


def lib():
    """The loaded libgll.so.  Raises if the HIP library was not built."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise RuntimeError(
                        f"{LIB_PATH} is missing: build the HIP extension first "
                        "(python graphlearninglayer_amd/build.py). There is no CPU fallback.")
                _lib = _declare(ct.CDLL(LIB_PATH))
    return _lib


def check(rc: int, what: str):
    if rc != GLL_OK:
        raise RuntimeError(f"{what} failed: {lib().gll_strerror(rc).decode()} (code {rc})")


def kernel_name(kid: int) -> str:
    return lib().gll_kernel_name(kid).decode()


def prof_enable(kid: int, period: int = 1):
    """Bracket every `period`-th launch of kernel `kid` with HIP events (0 disables)."""
    check(lib().gll_prof_enable(kid, int(period)), "gll_prof_enable")


def prof_read(kid: int):
    ms, cnt = ct.c_double(0.0), ct.c_int(0)
    check(lib().gll_prof_read(kid, ct.byref(ms), ct.byref(cnt)), "gll_prof_read")
    return ms.value, cnt.value


def set_knob(knob: int, value: int):
    """Force a code path for tests (include/gll.h GLL_KNOB_*); 0 restores the automatic one."""
    check(lib().gll_set_knob(int(knob), int(value)), "gll_set_knob")
