"""The one place the GPU tests call the C ABI -- a test helper, not a test.

Small helpers (need_gpu, stream, nan, dev, host, bits, raw_bytes, same_bits, features_buffer), two scopes for
process-wide state (knobs, launches) and `Run`: one problem on the device -- features, labels,
workspace blocks, NaN-filled outputs -- driven through gll_forward / gll_backward / gll_graph (a
2-D X) or their batched forms (a 3-D X), with bounds-checked reads of the workspace views.
"""
from __future__ import annotations

import contextlib
import ctypes as ct

import numpy as np
import pytest
import torch

from graphlearninglayer_amd import GLL
from graphlearninglayer_amd import _lib as L


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    L.lib()  # fail loudly when the HIP library is missing


def stream():
    return torch.cuda.current_stream().cuda_stream


def nan(*shape, dtype):
    """An output buffer no kernel has written: NaN everywhere (a caching-allocator block from
    torch.empty usually still holds the previous, correct result of the same shape)."""
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a, order="C")).cuda()   # a copy: shared inputs are read-only
    return t if dtype is None else t.to(dtype)


def host(t):
    return t.detach().cpu().numpy()


_UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
_TORCH_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def bits(a):
    """The array's (or tensor's) elements as unsigned integers of the same width, on the host."""
    if isinstance(a, torch.Tensor):
        a = host(a.contiguous().view(_TORCH_INT[a.element_size()]))
    a = np.ascontiguousarray(a)
    return a.view(_UINT[a.dtype.itemsize])


def raw_bytes(t):
    """The tensor's bytes, or None for None: for `==` between outputs that may be absent."""
    return None if t is None else host(t).tobytes()


def same_bits(a, b, msg=""):
    """Assert equal dtype, shape and bits (arrays or tensors); True, so it chains in an assert."""
    assert a.dtype == b.dtype and a.shape == b.shape, msg
    np.testing.assert_array_equal(bits(a), bits(b), err_msg=msg)
    return True


def features_buffer(X, aligned=True):
    """X (float32, any shape) on the device, its base 16-byte aligned or 4 bytes past such a
    boundary (the kernels' scalar-load paths)."""
    X = np.array(X, dtype=np.float32, order="C")   # a copy: shared inputs are read-only
    buf = torch.zeros(X.size + 4, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    o = 0 if aligned else 1
    v = buf[o: o + X.size].view(X.shape)
    v.copy_(torch.from_numpy(X))
    assert v.data_ptr() % 16 == (0 if aligned else 4)
    return v


@contextlib.contextmanager
def knobs(values):
    """{GLL_KNOB_* id: value} set for the block; every one back to 0 (automatic) after it,
    exceptions included.  gll_set_knob is process-wide."""
    try:
        for k, v in values.items():
            L.set_knob(k, v)
        yield
    finally:
        for k in values:
            L.set_knob(k, 0)


@contextlib.contextmanager
def launches(*kernel_ids):
    """Bracket every launch of the given kernel ids (gll_prof_enable, period 1) while the block
    runs; on exit synchronise and fill the yielded list with the launches of each id.  The brackets
    are process-wide (one pending list per id, emptied by gll_prof_read): pairs an earlier bracket
    left unread are dropped first, and nested use of one id is not supported."""
    counts = []
    for k in kernel_ids:
        L.prof_read(k)
        L.prof_enable(k, 1)
    try:
        yield counts
        torch.cuda.synchronize()
        counts.extend(L.prof_read(k)[1] for k in kernel_ids)
    finally:
        for k in kernel_ids:
            L.prof_enable(k, 0)


_Y_DT = {"f32": (np.float32, L.GLL_DT_F32), "f64": (np.float64, L.GLL_DT_F64),
         "i64": (np.int64, L.GLL_DT_I64)}


class Run:
    """One problem on the device.  X: n x d (the single-graph entry points) or B x n x d (the
    batched ones), float32 on the host; Y: base x C or B x base x C, or None for base = 0 (then
    `C`).  Options: rtol / max_iter (default: make_problem's), aligned (False: X 4 bytes off a
    16-byte boundary), ws_fill (a byte value the workspace holds before the first call; default
    torch.empty's contents), ws (a workspace tensor to reuse), sink (a private status sink:
    self.sink), y_dtype, neighbors (n x (K-1) or B x n x (K-1) int32 lists with GLL_FLAG_KNN_GIVEN
    in flags: the lists route).  Every output is NaN-filled before its call."""

    def __init__(self, X, Y, k, tau, eps, flags=0, *, C=None, rtol=None, max_iter=None,
                 aligned=True, ws_fill=None, ws=None, sink=False, y_dtype="f32", neighbors=None):
        X = np.asarray(X)
        self.batched = X.ndim == 3
        self.B = X.shape[0] if self.batched else 1
        self.n, self.d = X.shape[-2:]
        self.base = 0 if Y is None else np.shape(Y)[-2]
        self.C = C if C is not None else np.shape(Y)[-1]
        self.m = self.n - self.base
        self.k, self.tau, self.eps, self.flags = k, tau, eps, flags
        self.solver = {q: v for q, v in (("rtol", rtol), ("max_iter", max_iter)) if v is not None}
        self.X = features_buffer(X, aligned)
        np_dt, self.y_dt = _Y_DT[y_dtype]
        self.Y = None if Y is None else dev(np.asarray(Y, dtype=np_dt))
        self.nbr = None if neighbors is None else dev(neighbors, torch.int32)
        self.sink = torch.zeros(L.ST_NWORDS, dtype=torch.int32, device="cuda") if sink else None
        self.wb = self.workspace_bytes()
        assert self.wb > 0
        if ws is None:
            ws = torch.empty(self.B * self.wb, dtype=torch.uint8, device="cuda")
            if ws_fill is not None:
                ws.fill_(ws_fill)
        assert ws.numel() >= self.B * self.wb
        self.ws = ws
        self.U = None

    # -- the problem ---------------------------------------------------------------------------
    def problem(self, **overrides):
        """The gll_problem; overrides: flags, rtol, max_iter."""
        kw = dict(self.solver, flags=self.flags)
        kw.update(overrides)
        p = GLL.make_problem(self.n, self.d, self.base, self.C, self.k, self.tau, self.eps, **kw)
        if self.sink is not None:
            p.status_sink = self.sink.data_ptr()
        return p

    def workspace_bytes(self, **overrides):
        return L.lib().gll_workspace_bytes(ct.byref(self.problem(**overrides)))

    def _yp(self):
        return None if self.Y is None else self.Y.data_ptr()

    # -- the calls -----------------------------------------------------------------------------
    def forward(self, **overrides):
        """gll_forward(_batched), or gll_forward_lists_batched with neighbors: U (m x C, or
        B x m x C) on the host; the device tensor stays in self.U."""
        p = self.problem(**overrides)
        lead = (self.B,) if self.batched else ()
        self.U = nan(*lead, self.m, self.C, dtype=torch.float64)
        lib, ws, U = L.lib(), self.ws.data_ptr(), self.U.data_ptr()
        if self.nbr is not None:
            rc, what = lib.gll_forward_lists_batched(
                ct.byref(p), self.B, self.X.data_ptr(), self.nbr.data_ptr(), self._yp(), self.y_dt,
                ws, U, stream()), "gll_forward_lists_batched"
        elif self.batched:
            rc, what = lib.gll_forward_batched(ct.byref(p), self.B, self.X.data_ptr(), self._yp(),
                                               self.y_dt, ws, U, stream()), "gll_forward_batched"
        else:
            rc, what = lib.gll_forward(ct.byref(p), self.X.data_ptr(), self._yp(), self.y_dt, ws, U,
                                       stream()), "gll_forward"
        L.check(rc, what)
        return host(self.U)

    def backward(self, gbar, g_dtype=L.GLL_DT_F64, labels=True, **overrides):
        """gll_backward(_batched) on the workspace a forward left: grad_X on the host (self.gx on
        the device).  gbar is converted to g_dtype; labels=False passes the single-graph entry a
        NULL label matrix; overrides as in problem(): the backward's own flags, rtol, max_iter."""
        p = self.problem(**overrides)
        gd = dev(np.asarray(gbar, dtype=np.float32 if g_dtype == L.GLL_DT_F32 else np.float64))
        self.gx = nan(*self.X.shape, dtype=torch.float32)
        lib, ws = L.lib(), self.ws.data_ptr()
        if self.batched:
            rc, what = lib.gll_backward_batched(ct.byref(p), self.B, self.X.data_ptr(), ws,
                                                gd.data_ptr(), g_dtype, self.gx.data_ptr(),
                                                stream()), "gll_backward_batched"
        else:
            rc, what = lib.gll_backward(ct.byref(p), self.X.data_ptr(),
                                        self._yp() if labels else None,
                                        self.y_dt if labels else 0, ws, gd.data_ptr(), g_dtype,
                                        self.gx.data_ptr(), stream()), "gll_backward"
        L.check(rc, what)
        return host(self.gx)

    def graph(self, **overrides):
        """gll_graph, or gll_graph_lists with neighbors (one graph); synchronises."""
        assert not self.batched
        p = self.problem(**overrides)
        if self.nbr is not None:
            rc, what = L.lib().gll_graph_lists(ct.byref(p), self.X.data_ptr(), self.nbr.data_ptr(),
                                               self.ws.data_ptr(), stream()), "gll_graph_lists"
        else:
            rc, what = L.lib().gll_graph(ct.byref(p), self.X.data_ptr(), self.ws.data_ptr(),
                                         stream()), "gll_graph"
        torch.cuda.synchronize()
        L.check(rc, what)

    # -- reading the workspace -----------------------------------------------------------------
    def block(self, g=0):
        return self.ws.data_ptr() + g * self.wb

    def status(self, g=0):
        """The status words at the front of block g."""
        return self.ws[g * self.wb: g * self.wb + 4 * L.ST_NWORDS].view(torch.int32).cpu().tolist()

    def view(self, g=0):
        v = L.View()
        L.check(L.lib().gll_workspace_view(ct.byref(self.problem()), self.block(g), ct.byref(v)),
                "gll_workspace_view")
        return v

    def solve_view(self, g=0):
        v = L.SolveView()
        L.check(L.lib().gll_workspace_solve_view(ct.byref(self.problem()), self.block(g),
                                                 ct.byref(v)), "gll_workspace_solve_view")
        return v

    def knn_view(self):
        """gll_workspace_knn_view of the B blocks: pointers into block 0, the same offsets in the
        others."""
        v = L.KnnView()
        L.check(L.lib().gll_workspace_knn_view(ct.byref(self.problem()), self.B, self.ws.data_ptr(),
                                               ct.byref(v)), "gll_workspace_knn_view")
        return v

    def blocks(self, ptr, nbytes):
        """[B][nbytes] bytes on the host: those at `ptr`, which must lie inside block 0, and at
        the same offset of every other block (how knn_view's pointers are meant)."""
        off = ptr - self.ws.data_ptr()
        assert 0 <= off and off + nbytes <= self.wb, (off, nbytes, self.wb)
        return host(self.ws[: self.B * self.wb].view(self.B, self.wb)[:, off: off + nbytes]
                    .contiguous())

    def host_copy(self):
        """The whole workspace on the host, for array(..., snapshot=) of stage tests that read
        many arrays."""
        return host(self.ws)

    def array(self, ptr, count, dtype, g=0, snapshot=None):
        """`count` elements of numpy `dtype` at device pointer `ptr`, which must lie inside block
        g; read from the device, or from a host_copy()."""
        nb = count * np.dtype(dtype).itemsize
        off = ptr - self.ws.data_ptr()
        assert g * self.wb <= off and off + nb <= (g + 1) * self.wb, (g, off, nb, self.wb)
        src = host(self.ws[off: off + nb]) if snapshot is None else snapshot[off: off + nb]
        return src.view(dtype)
