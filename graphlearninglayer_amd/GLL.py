"""Host-side mirror of /root/reference/GLL.py on the MI355X HIP path.

Same names, argument meaning and error behaviour as the reference module:

  LaplaceLearningSparseHard.apply(X, label_matrix, tau=0, epsilon='auto'[, k=25])
                                                           GLL.py:10-177
  knn_sym_dist(data, k=25, epsilon='auto') -> W, V, mod_V, C, knn_ind   GLL.py:180-244
  stable_conjgrad(A, b, x0=None, max_iter=1e5, tol=1e-10)              GLL.py:247-276

Every numerical step runs in libgll.so (include/gll.h): exact kNN on fp32 MFMA, CSR graph
build, Jacobi-CG solves, edge gradient and Laplacian SpMM.  PyTorch provides device memory
(the caching allocator hands out the per-call workspace), the current stream and autograd.
There is no CPU fallback: a missing library or a missing GPU raises.

Deliberate differences from the reference (all documented in DESIGN.md):
  * kNN is exact (the reference's annoy index is approximate);
  * the solves are fp32 Jacobi-CG to rtol 1e-6 instead of float64 SuperLU;
  * outputs are placed on X.device (the reference uses the *current* device, GLL.py:15-18);
  * an optional 5th positional argument `k` replaces the hard-coded k=25 (GLL.py:27);
  * X may carry a leading batch dimension (B x n x d, labels B x base x C or shared):
    B independent graphs in one launch per kernel, U is B x m x C;
  * LaplaceLearningSparseHard.ce_loss(X, label_matrix, targets, ...) is apply followed by the
    callers' custom_ce_loss (losses.py:128-136) and argmax accuracy (FullySup.py:156-171) with
    one extra kernel (gll_ce_head_batched);
  * LaplaceLearningSparseHard.margin_loss(X, label_matrix, other, ...) is apply followed by the
    Carlini-Wagner attack's top-2 labels and clamped margin (adversarial.py:688-751) with one
    extra kernel (gll_margin_head_batched);
  * LaplaceLearningSparseHard.objective(X, label_matrix, targets, ..., weights, score, score_out,
    indices) is apply followed by the head of a score-driven step (FullySup.py:156-175): the
    weighted cross-entropy / entropy / l2 loss (losses.py:128-136, :100-101, :111-112) and the
    per-sample score scattered into a device store, with one extra kernel
    (gll_objective_head_batched);
  * label_matrix (floating point), tau and a fixed epsilon are differentiable as well as X
    (the reference returns None for them, GLL.py:177): tau / epsilon may be one-element
    tensors, whose value is read once in the forward (a host sync when on the GPU), and their
    gradients come from one extra pass over the graph (gll_param_grad_batched, DESIGN.md
    §3.6); epsilon='auto' has no epsilon input and so no epsilon gradient;
  * an optional last argument `normalize` (bool, False by default) of apply / ce_loss scales
    the rows of X to unit length inside the layer -- what every network of the reference does
    with F.normalize(feat, dim=1) in its last line (networks/BuildNet.py:101) -- and float16 /
    bfloat16 features are read as they are: one launch in front of the graph build, one behind
    its backward, the gradient in X's dtype (gll_features_forward / _backward, DESIGN.md §3.8;
    unit_features / unit_features_backward are the two stages on their own);
  * an optional last argument `neighbors` of apply / ce_loss / margin_loss / objective (and of
    device_graph, utils.laplace, utils.laplace_fit, utils.gl_accuracy) gives the neighbour lists
    instead of the search: an integer tensor n x k (the reference's knn_ind, GLL.py:186, column
    0 = self and not read) or n x (k - 1), in the caller's order, which is kept -- the last
    column is knn_ind[:, -1] of GLL.py:205.  The graph is built from them with exact distances
    and no n x n buffer (gll_forward_lists_batched); the lists are frozen, as
    the searched graph is.
"""
from __future__ import annotations

import ctypes as ct
import warnings

import numpy as np
import torch

from . import _lib

DEFAULT_K = 25          # GLL.py:27
MAX_K = 257             # include/gll.h: 2 <= K <= 257 (neighbours incl. self; kMaxKm1Huge = 256)
DEFAULT_RTOL = 1e-6     # fp32 Jacobi-CG at 1e-6 matches SuperLU to <1e-5
DEFAULT_MAX_ITER = 1000


def _check_k(k, n):
    """The kNN count the C ABI supports (include/gll.h gll_problem.K): a clear error here
    instead of the ABI's generic 'unsupported problem size'."""
    kk = min(int(k), int(n))
    if kk < 2 or kk > MAX_K:
        raise ValueError(f"k = {k} (n = {n}): the kNN count incl. self must satisfy "
                         f"2 <= min(k, n) <= {MAX_K}")


def _load_ext():
    """_gll_torch.so: LaplaceLearningSparseHard.apply in native code (csrc/torch_ext.cpp) and
    the per-device status sink.  Built in-tree with libgll.so; there is no fallback."""
    try:
        from . import _gll_torch
    except ImportError as e:
        raise ImportError("graphlearninglayer_amd: _gll_torch.so is missing or does not load "
                          "(build it: python graphlearninglayer_amd/build.py). There is no "
                          f"CPU fallback. ({e})") from e
    return _gll_torch


_ext_mod = _load_ext()


def _ext():
    return _ext_mod


# Device status -> the reference's warnings, without a host sync on the hot path: every call's
# kernels OR/max/add their status words into a sticky per-device sink (gll_problem.status_sink,
# owned by _gll_torch); every 64 calls the sink is copied to pinned memory and cleared on the
# stream, and completed copies are turned into warnings (GLL.py:240-241, 273-274) at a later
# call, or at check_status().
def check_status():
    """Flush every device's status sink now and raise the pending warnings (syncs)."""
    _ext_mod.check_status()


def _warn_from(st):
    """The warnings / error of one copy of the status words (as _gll_torch raises them), for
    callers of the C ABI that read the words themselves."""
    if st[_lib.ST_SOLVE_FAILED]:
        raise RuntimeError("GLL: the fused backward's gradient gave up waiting for the adjoint "
                           "solves; its grad_X was written as NaN")
    if st[_lib.ST_GRID_RESCUED]:
        warnings.warn(f"GLL: {st[_lib.ST_GRID_RESCUED]} whole-GPU CG solve(s) lost their grid "
                      "barrier (other kernels held the CUs) and were solved by one workgroup "
                      "instead: correct, slower", RuntimeWarning)
    if st[_lib.ST_TINY_EPS]:
        warnings.warn("Epsilon in KNN is very close to zero.", UserWarning)  # GLL.py:240-241
    if st[_lib.ST_LIST_DROPPED]:
        warnings.warn(f"GLL neighbors: {st[_lib.ST_LIST_DROPPED]} list entries were dropped (an "
                      "index outside [0, n) or a repeat within a row)", UserWarning)
    if st[_lib.ST_FWD_NONCONV]:
        warnings.warn(f"GLL forward CG: {st[_lib.ST_FWD_NONCONV]} column solve(s) reached "
                      f"max_iter ({st[_lib.ST_FWD_ITERS]} iterations)", RuntimeWarning)
    if st[_lib.ST_BWD_NONCONV]:
        warnings.warn(f"GLL adjoint CG: {st[_lib.ST_BWD_NONCONV]} column solve(s) reached "
                      f"max_iter ({st[_lib.ST_BWD_ITERS]} iterations)", RuntimeWarning)


def _poll_status(dev=None):
    idx = torch.cuda.current_device() if dev is None else dev.index
    _ext_mod.poll_status(idx)


def set_grad_diagnostics(threshold=10.0):
    """Print the reference's 'possible exploding gradient' report when ||grad_X||_F exceeds
    `threshold` (the inline copy of train_and_adversarial.py:177-183 uses 10) for calls made
    from now on; None switches the check off (the default).  The check synchronises."""
    _ext_mod.set_grad_diagnostics(-1.0 if threshold is None else float(threshold))


def _device_for(X: torch.Tensor) -> torch.device:
    if X.is_cuda:
        return X.device
    if not torch.cuda.is_available():
        raise RuntimeError("graphlearninglayer_amd needs a ROCm GPU (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def _features(X: torch.Tensor, dev) -> torch.Tensor:
    X32 = X.detach().to(device=dev, dtype=torch.float32).contiguous()
    if X32.data_ptr() % 16:      # the 16-B vector path needs an aligned base
        X32 = X32.clone()
    return X32


def _typed(t: torch.Tensor, dev):
    t = t.detach().to(dev)
    if t.dtype == torch.float32:
        code = _lib.GLL_DT_F32
    elif t.dtype == torch.float64:
        code = _lib.GLL_DT_F64
    elif t.dtype == torch.int64:
        code = _lib.GLL_DT_I64
    else:
        t, code = t.float(), _lib.GLL_DT_F32
    return t.contiguous(), code


def _scalar_tensor(v, what):
    """True when tau / epsilon is given as a tensor: it must hold one floating-point value."""
    if not torch.is_tensor(v):
        return False
    if v.numel() != 1 or not v.is_floating_point():
        raise TypeError(f"{what} as a tensor must hold one floating-point value")
    return True


def _eps_value(epsilon) -> float:
    if isinstance(epsilon, str):
        if epsilon != "auto":
            raise ValueError(f"epsilon must be a number or 'auto', got {epsilon!r}")
        return 0.0
    if _scalar_tensor(epsilon, "epsilon"):
        e = epsilon.item()
        if epsilon.requires_grad and not e > 0.0:
            raise ValueError("epsilon as a tensor that requires grad must be > 0")
    else:
        e = float(epsilon)
    if not e > 0.0:
        # GLL.py:240-241 warns for any eps < 1e-10.  The reference uses eps only as the product
        # eps[rows] * eps[cols] (GLL.py:233-234), so a negative eps builds the graph of |eps|;
        # eps = 0 (or NaN) divides by zero there, here it disconnects the graph (W = 0)
        warnings.warn("Epsilon in KNN is very close to zero.", UserWarning)
        return -e if e < 0.0 else 1e-30
    return e


def _check_neighbors(neighbors, lead, n, k):
    """The caller's neighbour lists: an integer tensor lead x n x K (column 0, the self column,
    is not read) or lead x n x (K - 1), K = min(k, n).  Metadata alone: no GPU call, no host
    sync."""
    K = min(int(k), int(n))
    if not torch.is_tensor(neighbors):
        raise TypeError("neighbors must be a Tensor")
    if neighbors.is_floating_point() or neighbors.is_complex() or neighbors.dtype == torch.bool:
        raise ValueError("neighbors must hold integers (int32 or int64)")
    want = tuple(lead) + (n,)
    if neighbors.dim() != len(want) + 1 or tuple(neighbors.shape[:-1]) != want \
            or neighbors.shape[-1] not in (K, K - 1):
        raise ValueError(f"neighbors must be {'B x ' if lead else ''}n x k or n x (k - 1) = "
                         f"{n} x {K} or {K - 1}")


def _neighbors_arg(neighbors, lead, n, k, dev):
    """The lists as the C ABI takes them: int32, contiguous, on `dev`, lead x n x (K - 1)."""
    _check_neighbors(neighbors, lead, n, k)
    nb = neighbors.detach()
    if nb.shape[-1] == min(int(k), int(n)):
        nb = nb[..., 1:]
    return nb.to(device=dev, dtype=torch.int32).contiguous()


def make_problem(n, d, base, C, k=DEFAULT_K, tau=0.0, epsilon="auto",
                 rtol=DEFAULT_RTOL, max_iter=DEFAULT_MAX_ITER, flags=0) -> _lib.Problem:
    return _lib.Problem(n=int(n), d=int(d), base=int(base), C=int(C), K=int(min(k, n)),
                        max_iter=int(max_iter),
                        tau=tau.item() if _scalar_tensor(tau, "tau") else float(tau),
                        eps=_eps_value(epsilon),
                        rtol=float(rtol), flags=int(flags))


def _stream(dev) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


class LaplaceLearningSparseHard(torch.autograd.Function):
    """Graph Laplace learning layer; labeled rows of X come first (GLL.py:11).

    `LaplaceLearningSparseHard.apply(X, label_matrix, tau=0, epsilon='auto'[, k=25[,
    normalize=False]])` is the
    native function of _gll_torch.so (csrc/torch_ext.cpp): argument checks, the forward
    kernels and one autograd node whose backward runs the backward kernels -- the whole host
    side of a call in C++.  `apply_python` is the same call as a Python
    torch.autograd.Function over the ctypes binding of the same C ABI (tests compare the two
    bitwise).  Both execute only the HIP kernels of libgll.so."""

    apply = staticmethod(_ext_mod.apply)

    @classmethod
    def apply_python(cls, X, label_matrix, tau=0, epsilon="auto", k=DEFAULT_K, neighbors=None):
        """The Python torch.autograd.Function path (ctypes onto the same C ABI)."""
        _check_k(k, X.shape[-2])
        return super().apply(X, label_matrix, tau, epsilon, k, neighbors)

    ce_loss = staticmethod(_ext_mod.ce_loss)

    @classmethod
    def ce_loss_python(cls, X, label_matrix, targets, tau=0, epsilon="auto", k=DEFAULT_K):
        """`ce_loss` on the Python torch.autograd.Function path (ctypes onto the same C ABI)."""
        _check_k(k, X.shape[-2])
        need = torch.is_grad_enabled() and any(
            torch.is_tensor(t) and t.requires_grad for t in (X, label_matrix, tau, epsilon))
        return _CeLossPython.apply(X, label_matrix, targets, tau, epsilon, k, need)

    margin_loss = staticmethod(_ext_mod.margin_loss)

    @classmethod
    def margin_loss_python(cls, X, label_matrix, other, tau=0, epsilon="auto", k=DEFAULT_K):
        """`margin_loss` on the Python torch.autograd.Function path (ctypes onto the same C ABI)."""
        _check_k(k, X.shape[-2])
        need = torch.is_grad_enabled() and any(
            torch.is_tensor(t) and t.requires_grad for t in (X, label_matrix, tau, epsilon))
        return _MarginLossPython.apply(X, label_matrix, other, tau, epsilon, k, need)

    objective = staticmethod(_ext_mod.objective)

    @classmethod
    def objective_python(cls, X, label_matrix, targets, tau=0, epsilon="auto", k=DEFAULT_K,
                         weights=(1.0, 0.0, 0.0), score=None, score_out=None, indices=None):
        """`objective` on the Python torch.autograd.Function path (ctypes onto the same C ABI)."""
        _check_k(k, X.shape[-2])
        need = torch.is_grad_enabled() and any(
            torch.is_tensor(t) and t.requires_grad for t in (X, label_matrix, tau, epsilon))
        return _ObjectivePython.apply(X, label_matrix, targets, tau, epsilon, k, need, weights,
                                      score, score_out, indices)

    @staticmethod
    def forward(ctx, X, label_matrix, tau=0, epsilon="auto", k=DEFAULT_K, neighbors=None):
        U = _layer_forward(ctx, X, label_matrix, tau, epsilon, k, neighbors)
        return U if X.is_cuda else U.cpu()

    @staticmethod
    def backward(ctx, grad_output):
        return (*_layer_backward(ctx, grad_output, ctx.needs_input_grad), None, None)


def _layer_forward(ctx, X, label_matrix, tau, epsilon, k, neighbors=None):
    """The forward of the Python path; returns U on the device and leaves the state of
    _layer_backward on ctx."""
    if X.dim() not in (2, 3) or label_matrix.dim() not in (2, X.dim()):
        raise ValueError("X must be n x d (or B x n x d), label_matrix base x C "
                         "(or B x base x C)")
    if neighbors is not None:
        _check_neighbors(neighbors, X.shape[:-2], X.shape[-2], k)
    dev = _device_for(X)
    _poll_status(dev)
    B = X.shape[0] if X.dim() == 3 else 1
    n, d = X.shape[-2:]
    base, C = label_matrix.shape[-2:]
    with torch.cuda.device(dev):
        X32 = _features(X, dev)
        Y, ydt = _typed(label_matrix, dev)
        if X.dim() == 3 and Y.dim() == 2:
            Y = Y.unsqueeze(0).expand(B, base, C).contiguous()   # shared labels
        if X.dim() == 3 and Y.shape[0] != B:
            raise ValueError(f"label_matrix batch {Y.shape[0]} != {B}")
        nb = None if neighbors is None else _neighbors_arg(neighbors, X.shape[:-2], n, k, dev)
        prob = make_problem(n, d, base, C, k, tau, epsilon,
                            flags=0 if nb is None else _lib.FLAG_KNN_GIVEN)
        prob.status_sink = _ext_mod.status_sink(dev.index)
        nbytes = _lib.lib().gll_workspace_bytes(ct.byref(prob))
        if nbytes == 0:
            raise ValueError(f"unsupported GLL problem n={n} d={d} base={base} C={C} k={k}")
        ws = torch.empty(nbytes * B, dtype=torch.uint8, device=dev)
        U = torch.empty(X.shape[:-2] + (n - base, C), dtype=torch.float64, device=dev)
        if nb is None:
            _lib.check(_lib.lib().gll_forward_batched(ct.byref(prob), B, X32.data_ptr(),
                                                      Y.data_ptr(), ydt, ws.data_ptr(),
                                                      U.data_ptr(), _stream(dev)),
                       "gll_forward")
        else:
            _lib.check(_lib.lib().gll_forward_lists_batched(ct.byref(prob), B, X32.data_ptr(),
                                                            nb.data_ptr(), Y.data_ptr(), ydt,
                                                            ws.data_ptr(), U.data_ptr(),
                                                            _stream(dev)),
                       "gll_forward_lists")
        _ext_mod.note_call(dev.index)
    ctx.save_for_backward(X)
    ctx.prob, ctx.ws, ctx.dev, ctx.B = prob, ws, dev, B
    # what the label_matrix / tau / epsilon gradients take after: (dtype, device, shape)
    ctx.like = [(t.dtype, t.device, t.shape) if torch.is_tensor(t) else None
                for t in (label_matrix, tau, epsilon)]
    ctx.Y_shared = X.dim() == 3 and label_matrix.dim() == 2
    return U


def _layer_backward(ctx, grad_output, need):
    """gll_backward_batched (+ gll_param_grad_batched) over the workspace on ctx; `need`: which
    of (X, label_matrix, tau, epsilon) want a gradient.  Returns their four gradients."""
    (X,) = ctx.saved_tensors
    dev, prob = ctx.dev, ctx.prob
    with torch.cuda.device(dev):
        X32 = _features(X, dev)
        g, gdt = _typed(grad_output, dev)
        if gdt == _lib.GLL_DT_I64:
            g, gdt = g.double(), _lib.GLL_DT_F64
        gradX = torch.empty(X.shape, dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().gll_backward_batched(ct.byref(prob), ctx.B, X32.data_ptr(),
                                                   ctx.ws.data_ptr(), g.data_ptr(), gdt,
                                                   gradX.data_ptr(), _stream(dev)),
                   "gll_backward")
        what = ((_lib.PG_Y if need[1] and ctx.like[0][0].is_floating_point else 0)
                | (_lib.PG_TAU if need[2] else 0)
                | (_lib.PG_EPS if need[3] and prob.eps > 0.0 else 0))
        gY = gtau = geps = None
        if what:   # one more pass over the graph the backward just completed
            B = ctx.B
            f64 = dict(dtype=torch.float64, device=dev)
            bufY = torch.empty((B, prob.base, prob.C), dtype=torch.float32, device=dev) \
                if what & _lib.PG_Y else None
            btau = torch.empty(B, **f64) if what & _lib.PG_TAU else None
            beps = torch.empty(B, **f64) if what & _lib.PG_EPS else None
            scratch = torch.empty(_lib.lib().gll_param_grad_scratch_bytes(ct.byref(prob), B),
                                  dtype=torch.uint8, device=dev) \
                if what & (_lib.PG_TAU | _lib.PG_EPS) else None

            def ptr(t):
                return None if t is None else t.data_ptr()

            _lib.check(_lib.lib().gll_param_grad_batched(ct.byref(prob), B, ctx.ws.data_ptr(),
                                                         what, ptr(bufY), ptr(btau), ptr(beps),
                                                         ptr(scratch), _stream(dev)),
                       "gll_param_grad")

            def like(v, meta):   # the input's dtype, device and shape
                return v.to(device=meta[1], dtype=meta[0]).reshape(meta[2])

            # batched input: shared labels and the scalars sum over graphs (float64)
            if bufY is not None:
                gY = like(bufY.double().sum(0) if ctx.Y_shared else bufY, ctx.like[0])
            if btau is not None:
                gtau = like(btau.sum() if B > 1 else btau, ctx.like[1])
            if beps is not None:
                geps = like(beps.sum() if B > 1 else beps, ctx.like[2])
    if not need[0]:
        gradX = None
    elif gradX.device != X.device or gradX.dtype != X.dtype:
        gradX = gradX.to(device=X.device, dtype=X.dtype)
    return gradX, gY, gtau, geps


class _CeLossPython(torch.autograd.Function):
    """LaplaceLearningSparseHard.ce_loss_python: the layer's Python path followed by
    gll_ce_head_batched; the backward feeds gbar * grad_loss to the layer's backward."""

    @staticmethod
    def forward(ctx, X, label_matrix, targets, tau, epsilon, k, need_grad):
        if not torch.is_tensor(targets) or targets.is_floating_point() or targets.is_complex() \
                or targets.dtype == torch.bool:
            raise TypeError("targets must hold integers")
        U = _layer_forward(ctx, X, label_matrix, tau, epsilon, k)
        dev, prob, B = ctx.dev, ctx.prob, ctx.B
        m = prob.n - prob.base
        lead = tuple(U.shape[:-2])
        if tuple(targets.shape) != lead + (m,):
            raise ValueError("targets must have shape "
                             + (f"B x m = {B} x {m}" if lead else f"m = {m}"))
        with torch.cuda.device(dev):
            t = targets.detach().to(device=dev, dtype=torch.int64).contiguous()
            loss = torch.empty(lead, dtype=torch.float64, device=dev)
            correct = torch.empty(lead, dtype=torch.int64, device=dev)
            row_loss = torch.empty(lead + (m,), dtype=torch.float64, device=dev)
            labels = torch.empty(lead + (m,), dtype=torch.int64, device=dev)
            gbar = torch.empty(U.shape, dtype=torch.float32, device=dev) if need_grad else None
            sb = _lib.lib().gll_ce_head_scratch_bytes(ct.byref(prob), B)
            scratch = torch.empty(sb, dtype=torch.uint8, device=dev) if sb else None
            _lib.check(_lib.lib().gll_ce_head_batched(
                ct.byref(prob), B, ctx.ws.data_ptr(), t.data_ptr(), loss.data_ptr(),
                None if gbar is None else gbar.data_ptr(), row_loss.data_ptr(), labels.data_ptr(),
                correct.data_ptr(), None if scratch is None else scratch.data_ptr(),
                _stream(dev)), "gll_ce_head")
        ctx.gbar = gbar
        out = (loss, U, labels, row_loss, correct)
        if not X.is_cuda:
            out = tuple(o.cpu() for o in out)
        ctx.mark_non_differentiable(*out[1:])
        return out

    @staticmethod
    def backward(ctx, grad_loss, *_):
        gl = grad_loss.to(ctx.dev)
        g = torch.empty_like(ctx.gbar)
        torch.mul(ctx.gbar, gl.reshape(-1, 1, 1) if ctx.gbar.dim() == 3 else gl.reshape(()), out=g)
        need = ctx.needs_input_grad
        gX, gY, gtau, geps = _layer_backward(ctx, g, (need[0], need[1], need[3], need[4]))
        return gX, gY, None, gtau, geps, None, None


class _MarginLossPython(torch.autograd.Function):
    """LaplaceLearningSparseHard.margin_loss_python: the layer's Python path followed by
    gll_margin_head_batched; the backward is _CeLossPython's."""

    @staticmethod
    def forward(ctx, X, label_matrix, other, tau, epsilon, k, need_grad):
        if other is not None and (not torch.is_tensor(other) or other.is_floating_point()
                                  or other.is_complex() or other.dtype == torch.bool):
            raise TypeError("other must hold integers (or be None)")
        U = _layer_forward(ctx, X, label_matrix, tau, epsilon, k)
        dev, prob, B = ctx.dev, ctx.prob, ctx.B
        m = prob.n - prob.base
        lead = tuple(U.shape[:-2])
        if other is not None and tuple(other.shape) != lead + (m,):
            raise ValueError("other must have shape "
                             + (f"B x m = {B} x {m}" if lead else f"m = {m}"))
        with torch.cuda.device(dev):
            o = None if other is None else \
                other.detach().to(device=dev, dtype=torch.int64).contiguous()
            loss = torch.empty(lead, dtype=torch.float64, device=dev)
            moved = torch.empty(lead, dtype=torch.int64, device=dev)
            row_margin = torch.empty(lead + (m,), dtype=torch.float64, device=dev)
            labels = torch.empty(lead + (m,), dtype=torch.int64, device=dev)
            second = torch.empty(lead + (m,), dtype=torch.int64, device=dev)
            gbar = torch.empty(U.shape, dtype=torch.float32, device=dev) if need_grad else None
            sb = _lib.lib().gll_margin_head_scratch_bytes(ct.byref(prob), B)
            scratch = torch.empty(sb, dtype=torch.uint8, device=dev) if sb else None
            _lib.check(_lib.lib().gll_margin_head_batched(
                ct.byref(prob), B, ctx.ws.data_ptr(), None if o is None else o.data_ptr(),
                loss.data_ptr(), None if gbar is None else gbar.data_ptr(),
                row_margin.data_ptr(), labels.data_ptr(), second.data_ptr(), moved.data_ptr(),
                None if scratch is None else scratch.data_ptr(), _stream(dev)),
                "gll_margin_head")
        ctx.gbar = gbar
        out = (loss, U, labels, second, row_margin, moved)
        if not X.is_cuda:
            out = tuple(t.cpu() for t in out)
        ctx.mark_non_differentiable(*out[1:])
        return out

    backward = staticmethod(_CeLossPython.backward)   # the same seven inputs, the same gbar


_SCORE_KINDS = {None: _lib.SCORE_NONE, "entropy": _lib.SCORE_ENTROPY, "l2": _lib.SCORE_L2}


class _ObjectivePython(torch.autograd.Function):
    """LaplaceLearningSparseHard.objective_python: the layer's Python path followed by
    gll_objective_head_batched; the backward is _CeLossPython's."""

    @staticmethod
    def forward(ctx, X, label_matrix, targets, tau, epsilon, k, need_grad, weights, score,
                score_out, indices):
        if targets is not None and (not torch.is_tensor(targets) or targets.is_floating_point()
                                    or targets.is_complex() or targets.dtype == torch.bool):
            raise TypeError("targets must hold integers (or be None)")
        try:
            w_ce, w_ent, w_l2 = (float(w) for w in weights)
        except (TypeError, ValueError):
            raise ValueError("weights must be three numbers (w_ce, w_ent, w_l2)") from None
        if isinstance(score, torch.Tensor) or score not in _SCORE_KINDS:
            raise ValueError("score must be None, 'entropy' or 'l2'")
        kind = _SCORE_KINDS[score]
        if (score_out is None) != (indices is None):
            raise ValueError("score_out and indices go together: give both or neither")
        if score_out is not None and kind == _lib.SCORE_NONE:
            raise ValueError("score_out needs score='entropy' or score='l2'")
        dev = _device_for(X)
        if score_out is not None:
            if not torch.is_tensor(score_out) or score_out.dtype != torch.float32 \
                    or score_out.dim() != 1 or not score_out.is_contiguous() \
                    or score_out.device != dev:
                raise ValueError("score_out must be a contiguous float32 tensor of shape N on the "
                                 "layer's device")
            if not torch.is_tensor(indices) or indices.is_floating_point() \
                    or indices.is_complex() or indices.dtype == torch.bool:
                raise TypeError("indices must hold integers")
        else:
            kind = _lib.SCORE_NONE   # a score without a store: nothing to scatter
        U = _layer_forward(ctx, X, label_matrix, tau, epsilon, k)
        prob, B = ctx.prob, ctx.B
        m = prob.n - prob.base
        lead = tuple(U.shape[:-2])
        for name, v in (("targets", targets), ("indices", indices)):
            if v is not None and tuple(v.shape) != lead + (m,):
                raise ValueError(f"{name} must have shape "
                                 + (f"B x m = {B} x {m}" if lead else f"m = {m}"))
        with torch.cuda.device(dev):
            def rows_arg(v):
                return None if v is None else \
                    v.detach().to(device=dev, dtype=torch.int64).contiguous()

            t, ind = rows_arg(targets), rows_arg(indices)
            f64 = dict(dtype=torch.float64, device=dev)
            i64 = dict(dtype=torch.int64, device=dev)
            loss, correct = torch.empty(lead, **f64), torch.empty(lead, **i64)
            row_loss, row_ent, row_l2 = (torch.empty(lead + (m,), **f64) for _ in range(3))
            labels = torch.empty(lead + (m,), **i64)
            gbar = torch.empty(U.shape, dtype=torch.float32, device=dev) if need_grad else None
            sb = _lib.lib().gll_objective_head_scratch_bytes(ct.byref(prob), B)
            scratch = torch.empty(sb, dtype=torch.uint8, device=dev) if sb else None

            def ptr(v):
                return None if v is None else v.data_ptr()

            _lib.check(_lib.lib().gll_objective_head_batched(
                ct.byref(prob), B, ctx.ws.data_ptr(), ptr(t), w_ce, w_ent, w_l2, loss.data_ptr(),
                ptr(gbar), row_loss.data_ptr(), row_ent.data_ptr(), row_l2.data_ptr(),
                labels.data_ptr(), correct.data_ptr(), kind, ptr(score_out),
                0 if score_out is None else score_out.shape[0], ptr(ind), ptr(scratch),
                _stream(dev)), "gll_objective_head")
        ctx.gbar = gbar
        out = (loss, U, labels, row_loss, correct, row_ent, row_l2)
        if not X.is_cuda:
            out = tuple(o.cpu() for o in out)
        ctx.mark_non_differentiable(*out[1:])
        return out

    @staticmethod
    def backward(ctx, grad_loss, *_):
        # ce_loss's seven inputs first, then weights, score, score_out, indices
        return (*_CeLossPython.backward(ctx, grad_loss), None, None, None, None)


def cw_margin(pred, other):
    """The Carlini-Wagner margin in plain torch (loss2 of adversarial.py:725 without its `c`, divided
    by the rows of `pred`): clamp(max_c pred[i, c] - pred[i, other_i], min=0).sum() / m.  The
    yardstick of LaplaceLearningSparseHard.margin_loss, which computes it in one kernel."""
    idx = torch.arange(pred.shape[0], device=pred.device)
    return torch.clamp(pred.max(1)[0] - pred[idx, other], min=0).sum() / pred.shape[0]


# ----------------------------------------------------------------------------------------
# The front end on its own (gll_features_forward / gll_features_backward): what
# apply / ce_loss run in front of the graph build for normalize=True or fp16 / bf16 features
# ----------------------------------------------------------------------------------------
_XT_CODES = {torch.float32: _lib.XT_F32, torch.float16: _lib.XT_F16, torch.bfloat16: _lib.XT_BF16}


def _xt_code(dtype):
    try:
        return _XT_CODES[dtype]
    except KeyError:
        raise TypeError(f"features must be float32, float16 or bfloat16, got {dtype}") from None


def _rows_of(t: torch.Tensor, what: str):
    if t.dim() not in (2, 3):
        raise ValueError(f"{what} must be n x d or B x n x d")
    d = t.shape[-1]
    if not 1 <= d <= _lib.MAX_D_FEATURES:
        raise ValueError(f"d = {d}: the front end holds rows of 1 <= d <= {_lib.MAX_D_FEATURES}")
    return t.numel() // d, d


def unit_features(Z: torch.Tensor, normalize: bool = True):
    """X^, rnorm = unit_features(Z): the fp32 rows the layer builds its graph on, from Z
    (n x d or B x n x d; float32, float16 or bfloat16) in one launch on the current stream.
    normalize=True: X^ = F.normalize(Z.float(), dim=-1) and rnorm = 1 / max(|z_i|, 1e-12) per
    row (Z's shape without the last dimension); False: X^ = Z.float() and rnorm is None.  For
    callers who cache features; apply(X^, ...) is bitwise apply(Z, ..., normalize=True)."""
    if not isinstance(normalize, bool):
        raise TypeError("normalize must be a bool")
    code = _xt_code(Z.dtype)
    rows, d = _rows_of(Z, "Z")
    dev = _device_for(Z)
    with torch.cuda.device(dev):
        Zd = Z.detach().to(dev).contiguous()
        X = torch.empty(Z.shape, dtype=torch.float32, device=dev)
        rnorm = torch.empty(Z.shape[:-1], dtype=torch.float32, device=dev) if normalize else None
        _lib.check(_lib.lib().gll_features_forward(
            rows, d, Zd.data_ptr(), code, _lib.UF_NORMALIZE if normalize else 0, X.data_ptr(),
            None if rnorm is None else rnorm.data_ptr(), _stream(dev)), "gll_features_forward")
    return X, rnorm


def unit_features_backward(gX: torch.Tensor, X: torch.Tensor, rnorm, dtype,
                           normalize: bool = True):
    """gZ = unit_features_backward(gX, X^, rnorm, dtype): the gradient with respect to the Z
    that unit_features turned into (X^, rnorm), from gX = dloss/dX^ (fp32, X^'s shape), rounded
    once to `dtype` (Z's: float32, float16 or bfloat16); one launch on the current stream.
    normalize=False: gZ = gX.to(dtype), X^ and rnorm are not read and may be None."""
    if not isinstance(normalize, bool):
        raise TypeError("normalize must be a bool")
    code = _xt_code(dtype)
    rows, d = _rows_of(gX, "gX")
    dev = _device_for(gX)

    def f32(t, shape, what):
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{what} must have shape {tuple(shape)}, got {tuple(t.shape)}")
        return t.detach().to(device=dev, dtype=torch.float32).contiguous()

    with torch.cuda.device(dev):
        g = f32(gX, gX.shape, "gX")
        Xd = f32(X, gX.shape, "X") if normalize else None
        rn = f32(rnorm, gX.shape[:-1], "rnorm") if normalize else None
        gZ = torch.empty(gX.shape, dtype=dtype, device=dev)
        _lib.check(_lib.lib().gll_features_backward(
            rows, d, g.data_ptr(), None if Xd is None else Xd.data_ptr(),
            None if rn is None else rn.data_ptr(), _lib.UF_NORMALIZE if normalize else 0,
            gZ.data_ptr(), code, _stream(dev)), "gll_features_backward")
    return gZ


def custom_ce_loss(pred, targets):
    """The callers' loss in plain torch (losses.py:128-136): -sum(one_hot(targets) *
    log(pred + 1e-8)) / batch_size for pred m x C with rows that sum to 1.  The yardstick of
    LaplaceLearningSparseHard.ce_loss, which computes it in one kernel."""
    onehot = torch.nn.functional.one_hot(targets, num_classes=pred.shape[1]).to(pred.dtype)
    return -(onehot * torch.log(pred + 1e-8)).sum() / pred.shape[0]


# ----------------------------------------------------------------------------------------
# knn_sym_dist: device graph, returned as the reference's scipy objects
# ----------------------------------------------------------------------------------------
def device_graph(X: torch.Tensor, k: int = DEFAULT_K, epsilon="auto", flags: int = 0,
                 neighbors=None):
    """Build the symmetric kNN graph on the GPU; returns a dict of device tensors
    (knn_idx, knn_d2, eps, row_ptr, col, w, d2, deg).  `flags`: gll_problem.flags
    (e.g. _lib.FLAG_KNN_PANEL, row panels instead of the n x n distances).  `neighbors`: the
    caller's lists (n x k or n x (k - 1) integers) instead of the search -- no n x n buffer;
    knn_idx then holds them in the caller's order (dropped entries padded with the row itself)."""
    _check_k(k, X.shape[0])
    if neighbors is not None:
        _check_neighbors(neighbors, (), X.shape[0], k)
    dev = _device_for(X)
    n, d = X.shape
    with torch.cuda.device(dev):
        X32 = _features(X, dev)
        nb = None if neighbors is None else _neighbors_arg(neighbors, (), n, k, dev)
        prob = make_problem(n, d, 0, 1, k, 0.0, epsilon,
                            flags=flags | (0 if nb is None else _lib.FLAG_KNN_GIVEN))
        nbytes = _lib.lib().gll_workspace_bytes(ct.byref(prob))
        if nbytes == 0:
            raise ValueError(f"unsupported graph problem n={n} d={d} k={k}")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        if nb is None:
            _lib.check(_lib.lib().gll_graph(ct.byref(prob), X32.data_ptr(), ws.data_ptr(),
                                            _stream(dev)), "gll_graph")
        else:
            _lib.check(_lib.lib().gll_graph_lists(ct.byref(prob), X32.data_ptr(), nb.data_ptr(),
                                                  ws.data_ptr(), _stream(dev)), "gll_graph_lists")
        view = _lib.View()
        _lib.check(_lib.lib().gll_workspace_view(ct.byref(prob), ws.data_ptr(), ct.byref(view)),
                   "gll_workspace_view")
        K = prob.K
        base_ptr = ws.data_ptr()

        def arr(ptr, count, dtype):
            off = ptr - base_ptr
            esz = torch.empty(0, dtype=dtype).element_size()
            return ws[off: off + count * esz].view(dtype)

        # padded device rows (row_start, row_len) -> compact CSR
        starts = arr(view.row_start, n, torch.int32).long()
        lens = arr(view.row_len, n, torch.int32).long()
        span = int((starts + lens).max().item())
        row_ptr = torch.zeros(n + 1, dtype=torch.long, device=dev)
        row_ptr[1:] = torch.cumsum(lens, 0)
        E = int(row_ptr[-1].item())
        rows = torch.repeat_interleave(torch.arange(n, device=dev), lens)
        src = starts[rows] + (torch.arange(E, device=dev) - row_ptr[rows])
        out = dict(
            knn_idx=arr(view.knn_idx, n * K, torch.int32).view(n, K),
            knn_d2=arr(view.knn_d2, n * K, torch.float32).view(n, K),
            eps=arr(view.eps, n, torch.float32),
            row_ptr=row_ptr.int(),
            col=arr(view.col, span, torch.int32)[src],
            w=arr(view.w, span, torch.float32)[src],
            d2=arr(view.d2, span, torch.float32)[src],
            deg=arr(view.deg, n, torch.float32),
            status=arr(view.status, _lib.ST_NWORDS, torch.int32),
            workspace=ws,
        )
    return out


def knn_sym_dist(data, k=DEFAULT_K, epsilon="auto"):
    """Mirror of GLL.py:180-244: returns (W, V, mod_V, C, knn_ind) as scipy/numpy objects.

    The graph is built on the GPU (exact kNN); only the final arrays travel to the host."""
    import scipy.sparse as sparse

    X = data if torch.is_tensor(data) else torch.from_numpy(np.ascontiguousarray(data))
    g = device_graph(X, k, epsilon)
    n = X.shape[0]
    rp = g["row_ptr"].cpu().numpy().astype(np.int64)
    col = g["col"].cpu().numpy().astype(np.int64)
    w = g["w"].cpu().numpy().astype(np.float64)
    d2 = g["d2"].cpu().numpy().astype(np.float64)
    eps = g["eps"].cpu().numpy().astype(np.float64)
    knn_ind = g["knn_idx"].cpu().numpy().astype(np.int64)
    rows = np.repeat(np.arange(n), np.diff(rp))
    W = sparse.csr_matrix((w, col, rp), shape=(n, n))
    Vv = -8.0 * w / (eps[rows] * eps[col])
    V = sparse.csr_matrix((Vv, col, rp), shape=(n, n))
    if isinstance(epsilon, str):
        mod_V = sparse.csr_matrix((d2 * Vv / eps[rows] ** 2 / 2, col, rp), shape=(n, n))
        C = sparse.csr_matrix((np.ones(n), (knn_ind[:, -1], knn_ind[:, 0])), shape=(n, n))
    else:
        mod_V, C = 0, 0
    _poll_status()
    return W, V, mod_V, C, knn_ind


# ----------------------------------------------------------------------------------------
# stable_conjgrad: device multi-RHS CG
# ----------------------------------------------------------------------------------------
def refined_solve(rp, ci, val64, B, x=None, tol=1e-10, max_iter=100000, weight=None):
    """Solve A x = B (A SPD, device CSR: int32 row_ptr / col, float64 values; B m x C float64)
    to max_c ||weight * (B - A x)_c||_2 <= tol.

    fp32 Jacobi-CG corrections (libgll gll_cg_csr: the whole-GPU CG for m > 2048) inside
    float64 iterative refinement; the float64 residual uses torch sparse on the GPU.
    Returns (x, err, CG iterations)."""
    dev = B.device
    m, C = B.shape
    val32 = val64.float().contiguous()
    with warnings.catch_warnings():   # "sparse CSR support is in beta" (torch 2.10)
        warnings.simplefilter("ignore", UserWarning)
        A64 = torch.sparse_csr_tensor(rp.long(), ci.long(), val64, size=(m, m))
    x = torch.zeros_like(B) if x is None else x
    ws = torch.empty(_lib.lib().gll_cg_csr_workspace_bytes(m, C), dtype=torch.uint8, device=dev)
    counters = torch.zeros(2, dtype=torch.int32, device=dev)
    total = 0
    max_iter = int(max_iter)

    def residual(x):
        r = B - (A64 @ x)
        rw = r if weight is None else r * weight[:, None]
        return r, torch.linalg.vector_norm(rw, dim=0).max().item()

    r, err = residual(x)
    for _ in range(32):  # refinement sweeps
        if err <= tol or total >= max_iter:
            break
        scale = max(torch.linalg.vector_norm(r, dim=0).max().item(), 1e-300)
        r32 = (r / scale).float().contiguous()
        d32 = torch.empty_like(r32)
        counters.zero_()
        _lib.check(_lib.lib().gll_cg_csr(m, C, rp.data_ptr(), ci.data_ptr(), val32.data_ptr(),
                                         r32.data_ptr(), d32.data_ptr(),
                                         ct.c_float(1e-6), max_iter - total,
                                         counters.data_ptr(), counters[1:].data_ptr(),
                                         ws.data_ptr(), _stream(dev)), "gll_cg_csr")
        total += int(counters[0].item())
        x = x + scale * d32.double()
        r, err = residual(x)
    return x, err, total


def stable_conjgrad(A, b, x0=None, max_iter=1e5, tol=1e-10):
    """Mirror of GLL.py:247-276: solve A x = b (A SPD, b n x C) to max_col ||r||_2 <= tol.

    Mixed precision on the device: fp32 Jacobi-CG (libgll gll_cg_csr) inside float64
    iterative refinement (residual r = b - A x in float64 with torch sparse on the GPU),
    so the float64 tolerance of the reference is reachable."""
    import scipy.sparse as sparse

    if not torch.cuda.is_available():
        raise RuntimeError("graphlearninglayer_amd needs a ROCm GPU (no CPU fallback)")
    dev = torch.device("cuda", torch.cuda.current_device())
    A = sparse.csr_matrix(A)
    b_np = np.asarray(b, dtype=np.float64)
    vec = b_np.ndim == 1
    B = torch.from_numpy(b_np.reshape(b_np.shape[0], -1)).to(dev)
    m, C = B.shape
    rp = torch.from_numpy(A.indptr.astype(np.int32)).to(dev)
    ci = torch.from_numpy(A.indices.astype(np.int32)).to(dev)
    val64 = torch.from_numpy(A.data.astype(np.float64)).to(dev)
    x = None if x0 is None else torch.from_numpy(
        np.asarray(x0, dtype=np.float64).reshape(m, C)).to(dev)
    x, err, total = refined_solve(rp, ci, val64, B, x, tol, max_iter)
    if err > tol:
        print("max iter reached: ", total, " iters")  # GLL.py:273-274
    out = x.cpu().numpy()
    return out.ravel() if vec else out


# ----------------------------------------------------------------------------------------
# Query-vs-database kNN and the out-of-sample extension (gll_knn_query / gll_extend,
# DESIGN.md §3.12).  knn_query has no gradient (the lists are frozen); extend is differentiable
# in Xq, Xdb, P and a fixed epsilon given as a tensor (gll_extend_backward).
# ----------------------------------------------------------------------------------------
def _check_query(Xq, Xdb, k, what):
    if not (torch.is_tensor(Xq) and torch.is_tensor(Xdb)):
        raise TypeError(f"{what}: Xq and Xdb must be tensors")
    if Xq.dim() != 2 or Xdb.dim() != 2:
        raise ValueError(f"{what}: Xq must be Q x d and Xdb N x d")
    N, d = Xdb.shape
    if Xq.shape[1] != d:
        raise ValueError(f"{what}: Xq has {Xq.shape[1]} features, Xdb has {d}")
    if not 1 <= d <= _lib.MAX_D_FEATURES:
        raise ValueError(f"{what}: d = {d}, need 1 <= d <= {_lib.MAX_D_FEATURES}")
    if not 1 <= N <= _lib.QUERY_MAX_N:
        raise ValueError(f"{what}: N = {N}, need 1 <= N <= {_lib.QUERY_MAX_N}")
    if int(k) != k or not 1 <= k <= min(N, _lib.QUERY_MAX_K):
        raise ValueError(f"{what}: k = {k} (N = {N}), need 1 <= k <= min(N, {_lib.QUERY_MAX_K})")


def _knn_query_device(Xq32, Xdb32, k, flags, status, dev):
    """gll_knn_query on prepared fp32 device rows: (idx int32 Q x k, d2 float32 Q x k)."""
    Q, d = Xq32.shape
    N = Xdb32.shape[0]
    lib = _lib.lib()
    nbytes = lib.gll_query_workspace_bytes(Q, N, d, k, flags)
    if nbytes == 0:
        raise ValueError(f"unsupported query Q={Q} N={N} d={d} k={k} flags={flags}")
    idx = torch.empty((Q, k), dtype=torch.int32, device=dev)
    d2 = torch.empty((Q, k), dtype=torch.float32, device=dev)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _lib.check(lib.gll_knn_query(Q, N, d, k, flags, Xq32.data_ptr(), Xdb32.data_ptr(),
                                 idx.data_ptr(), d2.data_ptr(), status.data_ptr(), ws.data_ptr(),
                                 _stream(dev)), "gll_knn_query")
    return idx, d2


def _check_candidates(cand, Q, lo, what, name):
    """Caller-supplied candidates of the query calls: an integer tensor Q x c, lo <= c <=
    _lib.RERANK_MAX_C.  Metadata alone: no GPU call, no host sync."""
    if not torch.is_tensor(cand):
        raise TypeError(f"{what}: {name} must be a Tensor")
    if cand.is_floating_point() or cand.is_complex() or cand.dtype == torch.bool:
        raise ValueError(f"{what}: {name} must hold integers (int32 or int64)")
    if cand.dim() != 2 or cand.shape[0] != Q or not lo <= cand.shape[1] <= _lib.RERANK_MAX_C:
        raise ValueError(f"{what}: {name} must be Q x c = {Q} x c with {lo} <= c <= "
                         f"{_lib.RERANK_MAX_C}, got {tuple(cand.shape)}")


def _knn_rerank_device(Xq32, Xdb32, cand, k, flags, status, dev):
    """gll_knn_rerank on prepared fp32 device rows and the caller's candidates (narrowed to int32
    as the layer's neighbors are): (idx int32 Q x k, d2 float32 Q x k)."""
    Q, d = Xq32.shape
    N = Xdb32.shape[0]
    c32 = cand.detach().to(device=dev, dtype=torch.int32).contiguous()
    idx = torch.empty((Q, k), dtype=torch.int32, device=dev)
    d2 = torch.empty((Q, k), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().gll_knn_rerank(Q, N, d, c32.shape[1], k, flags, Xq32.data_ptr(),
                                         Xdb32.data_ptr(), c32.data_ptr(), idx.data_ptr(),
                                         d2.data_ptr(), status.data_ptr(), _stream(dev)),
               "gll_knn_rerank")
    return idx, d2


def knn_query(Xq: torch.Tensor, Xdb: torch.Tensor, k: int, flags: int = 0,
              return_status: bool = False, candidates=None, keep_order: bool = False):
    """idx, d2 = knn_query(Xq, Xdb, k): for every row of Xq (Q x d) the k rows of Xdb (N x d) with
    the smallest float64 sum_f (q_f - x_f)^2 of the fp32 features, equal distances to the lower
    index -- exact, like the graph build's kNN.  idx int64 Q x k, d2 float32 Q x k (the fp32
    difference-form distances), each list ordered by (d2, idx), on Xdb's device.  float16 /
    bfloat16 / float64 features are converted to float32 first.  flags: _lib.QF_SMALL_PANELS.
    return_status=True adds the 4 int32 status words of the call (_lib.QST_*, a device tensor).
    candidates: an integer tensor Q x c (any device), k <= c <= 512 -- no search: one launch
    (gll_knn_rerank) picks each row's k nearest among its own candidates, with the search's
    distance bits; entries outside [0, N) and repeats are never chosen, and a row with fewer than
    k valid ones ends in (-1, +inf) and is counted in status[_lib.QST_SHORT_ROW].
    keep_order=True (c == k): the lists as they are, in the caller's order, with their distances
    (+inf for an index outside [0, N))."""
    _check_query(Xq, Xdb, k, "knn_query")
    k, flags = int(k), int(flags)
    if flags & ~_lib.QF_SMALL_PANELS:
        raise ValueError(f"knn_query: unknown flags {flags}")
    if candidates is None:
        if keep_order:
            raise ValueError("knn_query: keep_order needs candidates")
    else:
        _check_candidates(candidates, Xq.shape[0], k, "knn_query", "candidates")
        if keep_order and candidates.shape[1] != k:
            raise ValueError(f"knn_query: keep_order needs candidates of k = {k} columns, got "
                             f"{candidates.shape[1]}")
        if flags:
            raise ValueError("knn_query: flags steer the search; candidates take none")
    dev = _device_for(Xdb)
    with torch.cuda.device(dev):
        status = torch.zeros(_lib.QST_NWORDS, dtype=torch.int32, device=dev)
        if Xq.shape[0] == 0:
            idx = torch.empty((0, k), dtype=torch.int64, device=dev)
            d2 = torch.empty((0, k), dtype=torch.float32, device=dev)
        elif candidates is not None:
            idx32, d2 = _knn_rerank_device(_features(Xq, dev), _features(Xdb, dev), candidates, k,
                                           _lib.RR_KEEP_ORDER if keep_order else 0, status, dev)
            idx = idx32.long()
        else:
            idx32, d2 = _knn_query_device(_features(Xq, dev), _features(Xdb, dev), k, flags,
                                          status, dev)
            idx = idx32.long()
    return (idx, d2, status) if return_status else (idx, d2)


def extend(Xq: torch.Tensor, Xdb: torch.Tensor, P: torch.Tensor, k: int = DEFAULT_K,
           epsilon="auto", eps_db=None, return_status: bool = False, neighbors=None):
    """Uq, labels = extend(Xq, Xdb, P, k): the harmonic (Nadaraya-Watson) out-of-sample extension
    of a solved graph, u(q) = sum_j w_qj P_j / sum_j w_qj over q's k - 1 nearest rows of Xdb
    (k has the layer's meaning, neighbours including the point itself; a query is not in the
    database), w = exp(-4 d^2 / (eps_q eps_j)): a fixed epsilon for both, or 'auto': eps_q the
    distance to the (k - 1)-th nearest and eps_j = eps_db[j] (the database graph's eps, required).
    P: N x C predictions of the database rows ([Y; U]), read as float32.  Uq float64 Q x C,
    labels int64 Q (lowest index among the maxima), on Xdb's device.
    Differentiable: with grad mode on and Xq, Xdb, P or a one-element tensor epsilon requiring
    grad, Uq carries a grad_fn (gll_extend_backward: the neighbour lists frozen, as the layer's
    graph is; gradients in each input's dtype).  eps_db is a constant of the fitted graph and
    never gets a gradient; labels are not differentiable.
    neighbors: an integer tensor Q x c (any device), k - 1 <= c <= 512, in place of the search:
    re-rank + extension, two launches.  c == k - 1: each row's list as it is, in the caller's order
    (the last column gives 'auto' its eps_q, as knn_ind[:, -1] does for the layer); c > k - 1: a
    pool, of which every call takes the k - 1 nearest -- what the search gives while the pool
    still holds them.  The backward runs on the re-ranked lists, frozen.  An index outside [0, N)
    in a list, or a pool row with fewer than k - 1 valid entries (status[_lib.QST_SHORT_ROW]),
    makes its row NaN."""
    if not isinstance(k, (int, np.integer)) or not 2 <= k <= MAX_K:
        raise ValueError(f"extend: k = {k}, need 2 <= k <= {MAX_K} (neighbours incl. self)")
    _check_query(Xq, Xdb, int(k) - 1, "extend")
    N = Xdb.shape[0]
    if not torch.is_tensor(P) or P.dim() != 2 or P.shape[0] != N:
        raise ValueError(f"extend: P must be N x C with N = {N}")
    C = P.shape[1]
    if not 1 <= C <= _lib.QUERY_MAX_C:
        raise ValueError(f"extend: C = {C}, need 1 <= C <= {_lib.QUERY_MAX_C}")
    eps = _eps_value(epsilon)
    if eps == 0.0:
        if eps_db is None:
            raise ValueError("extend: epsilon='auto' needs eps_db (the database graph's eps)")
        if not torch.is_tensor(eps_db) or eps_db.numel() != N:
            raise ValueError(f"extend: eps_db must hold N = {N} values")
    kn = int(k) - 1
    Q = Xq.shape[0]
    if neighbors is not None:
        _check_candidates(neighbors, Q, kn, "extend", "neighbors")
    dev = _device_for(Xdb)
    eps_t = epsilon if torch.is_tensor(epsilon) else None
    if Q > 0 and torch.is_grad_enabled() and any(
            t is not None and t.requires_grad for t in (Xq, Xdb, P, eps_t)):
        Uq, labels, status = _Extend.apply(Xq, Xdb, P, eps_t, kn, eps, eps_db, dev, neighbors)
    else:
        Uq, labels, status = _extend_forward(Xq, Xdb, P, kn, eps, eps_db, dev, neighbors)[:3]
    return (Uq, labels, status) if return_status else (Uq, labels)


def _extend_forward(Xq, Xdb, P, kn, eps, eps_db, dev, neighbors=None):
    """gll_knn_query (or, on the caller's neighbors, gll_knn_rerank: a list of kn columns as it is,
    the kn nearest of a wider pool) + gll_extend: (Uq, labels, status) and what the backward
    reads."""
    Q, N, C = Xq.shape[0], Xdb.shape[0], P.shape[1]
    with torch.cuda.device(dev):
        status = torch.zeros(_lib.QST_NWORDS, dtype=torch.int32, device=dev)
        Uq = torch.empty((Q, C), dtype=torch.float64, device=dev)
        labels = torch.empty(Q, dtype=torch.int64, device=dev)
        saved = None
        if Q > 0:
            P32 = P.detach().to(device=dev, dtype=torch.float32).contiguous()
            e32 = None
            if eps == 0.0:
                e32 = eps_db.detach().to(device=dev, dtype=torch.float32).contiguous().view(-1)
            Xq32, Xdb32 = _features(Xq, dev), _features(Xdb, dev)
            if neighbors is None:
                idx, d2 = _knn_query_device(Xq32, Xdb32, kn, 0, status, dev)
            else:
                idx, d2 = _knn_rerank_device(
                    Xq32, Xdb32, neighbors, kn,
                    _lib.RR_KEEP_ORDER if neighbors.shape[1] == kn else 0, status, dev)
            _lib.check(_lib.lib().gll_extend(
                Q, N, kn, C, idx.data_ptr(), d2.data_ptr(), P32.data_ptr(),
                None if e32 is None else e32.data_ptr(), ct.c_float(eps), Uq.data_ptr(),
                labels.data_ptr(), status.data_ptr(), _stream(dev)), "gll_extend")
            saved = (Xq32, Xdb32, idx, d2, P32, e32)
    return Uq, labels, status, saved


def _extend_backward_device(Xq32, Xdb32, idx, d2, P32, e32, eps, gU, what, flags=0):
    """gll_extend_backward on prepared device arrays: (gXq, gXdb, gP fp32, grad_eps float64 --
    None where not selected -- and the call's 4 status words)."""
    Q, d = Xq32.shape
    N, C = P32.shape
    kn = idx.shape[1]
    dev = Xdb32.device
    lib = _lib.lib()
    with torch.cuda.device(dev):
        nbytes = lib.gll_extend_grad_workspace_bytes(Q, N, kn, d, C, what, flags)
        if nbytes == 0:
            raise ValueError(f"unsupported extend backward Q={Q} N={N} kn={kn} d={d} C={C} "
                             f"what={what} flags={flags}")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        status = torch.zeros(_lib.QST_NWORDS, dtype=torch.int32, device=dev)
        gXq = torch.empty((Q, d), dtype=torch.float32, device=dev) if what & _lib.EG_XQ else None
        gXdb = torch.empty((N, d), dtype=torch.float32, device=dev) if what & _lib.EG_XDB else None
        gP = torch.empty((N, C), dtype=torch.float32, device=dev) if what & _lib.EG_P else None
        geps = torch.empty(1, dtype=torch.float64, device=dev) if what & _lib.EG_EPS else None
        ptr = lambda t: None if t is None else t.data_ptr()
        _lib.check(lib.gll_extend_backward(
            Q, N, kn, d, C, Xq32.data_ptr(), Xdb32.data_ptr(), idx.data_ptr(), d2.data_ptr(),
            P32.data_ptr(), ptr(e32), ct.c_float(eps), gU.data_ptr(), what, flags, ptr(gXq),
            ptr(gXdb), ptr(gP), ptr(geps), status.data_ptr(), ws.data_ptr(), _stream(dev)),
            "gll_extend_backward")
    return gXq, gXdb, gP, geps, status


class _Extend(torch.autograd.Function):
    """extend with its hand-written backward (gll_extend_backward): the neighbour
    lists are frozen, eps_db is a constant, labels and status carry no gradient."""

    @staticmethod
    def forward(ctx, Xq, Xdb, P, eps_t, kn, eps, eps_db, dev, neighbors=None):
        Uq, labels, status, saved = _extend_forward(Xq, Xdb, P, kn, eps, eps_db, dev, neighbors)
        ctx.save_for_backward(*saved)   # (Uq is recomputed by the kernel, bit for bit)
        ctx.eps = eps
        ctx.like = tuple(None if t is None else (t.dtype, t.device, t.shape)
                         for t in (Xq, Xdb, P, eps_t))
        ctx.mark_non_differentiable(labels, status)
        return Uq, labels, status

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gU, *_):
        Xq32, Xdb32, idx, d2, P32, e32 = ctx.saved_tensors
        need = ctx.needs_input_grad
        what = ((_lib.EG_XQ if need[0] else 0) | (_lib.EG_XDB if need[1] else 0) |
                (_lib.EG_P if need[2] else 0) | (_lib.EG_EPS if need[3] else 0))
        if what == 0:
            return (None,) * 9
        dev = Xdb32.device
        with torch.cuda.device(dev):
            g64 = gU.detach().to(device=dev, dtype=torch.float64).contiguous()
            outs = _extend_backward_device(Xq32, Xdb32, idx, d2, P32, e32, ctx.eps, g64, what)[:4]

        def back(g, like):
            if g is None:
                return None
            dtype, device, shape = like
            return g.to(device=device, dtype=dtype).reshape(shape)

        return tuple(back(g, like) for g, like in zip(outs, ctx.like)) + (None,) * 5


def extend_torch(Xq, Xdb, P, idx, epsilon="auto", eps_db=None):
    """The extension's formula in plain PyTorch on given neighbour lists idx (Q x kn, nearest
    first): Uq = sum_i w_i P[idx_i] / sum_i w_i, w_i = exp(-4 d_i^2 / (eps_q eps_j)), d_i^2 =
    sum_f (q_f - x_f)^2, eps_q = d_(kn-1) and eps_j = eps_db[j] for 'auto'.  Everything in the
    inputs' dtype and differentiable by autograd: the yardstick of extend and its backward (as
    cw_margin and supcon_loss_torch are for theirs), not a code path of the package."""
    idx = idx.long()
    diff = Xq[:, None, :] - Xdb[idx]
    d2 = (diff * diff).sum(-1)
    if isinstance(epsilon, str):
        if epsilon != "auto":
            raise ValueError(f"epsilon must be a number or 'auto', got {epsilon!r}")
        den = d2[:, -1:].sqrt() * eps_db.to(d2.dtype).view(-1)[idx]
    else:
        den = epsilon * epsilon
    w = torch.exp(-4.0 * d2 / den)
    return (w[:, :, None] * P[idx]).sum(1) / w.sum(1, keepdim=True)
