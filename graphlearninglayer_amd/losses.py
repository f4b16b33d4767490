"""SupCon / SimCLR loss on the device (include/gll.h gll_supcon_*).

Drop-in for the reference's `losses.py` SupConLoss: `from losses import *` (FullySup.py:13)
becomes `from graphlearninglayer_amd.losses import SupConLoss`.  The R x R logits are never in
memory: two launches forward and two backward, with the unit-norm / half-precision front end
(gll_features_*) in front of and behind them on request.  There is no CPU fallback.
"""
from __future__ import annotations

import torch

from . import _lib
from .GLL import _device_for, _stream, _xt_code

__all__ = ["SupConLoss", "supcon_loss", "supcon_loss_torch"]

_MODES = {"all": _lib.SC_ALL, "one": _lib.SC_ONE}


def _mode_code(contrast_mode):
    try:
        return _MODES[contrast_mode]
    except (KeyError, TypeError):
        raise ValueError(f"Unknown mode: {contrast_mode}") from None


def _check_features(features, labels, mask):
    """The reference's argument handling (losses.py:38-55): features as [bsz, V, d]."""
    if features.dim() < 3:
        raise ValueError("`features` needs to be [bsz, n_views, ...], at least 3 dimensions are required")
    if features.dim() > 3:
        features = features.reshape(features.shape[0], features.shape[1], -1)
    if labels is not None and mask is not None:
        raise ValueError("Cannot define both `labels` and `mask`")
    if labels is not None:
        labels = labels.contiguous().view(-1)
        if labels.shape[0] != features.shape[0]:
            raise ValueError("Num of labels does not match num of features")
    return features, labels


class _SupConPython(torch.autograd.Function):
    """loss (and the anchors' losses) of features [bsz, V, d]; saves Z (or X^ and rnorm) and the
    per-row statistics only."""

    @staticmethod
    def forward(ctx, features, labels, T, Tb, mode, normalize):
        code = _xt_code(features.dtype)
        bsz, V, d = features.shape
        rows = bsz * V
        if not 1 <= d <= _lib.MAX_D_FEATURES:
            raise ValueError(f"d = {d}: supcon_loss holds rows of 1 <= d <= {_lib.MAX_D_FEATURES}")
        if not 2 <= rows <= _lib.SC_MAX_ROWS:
            raise ValueError(f"bsz * n_views = {rows}: supcon_loss needs 2 <= rows <= {_lib.SC_MAX_ROWS}")
        dev = _device_for(features)
        lib = _lib.lib()
        front = normalize or code != _lib.XT_F32
        with torch.cuda.device(dev):
            Zd = features.detach().to(dev).contiguous()
            rnorm = None
            if front:
                X = torch.empty((bsz, V, d), dtype=torch.float32, device=dev)
                rnorm = torch.empty((bsz, V), dtype=torch.float32, device=dev) if normalize else None
                _lib.check(lib.gll_features_forward(
                    rows, d, Zd.data_ptr(), code, _lib.UF_NORMALIZE if normalize else 0,
                    X.data_ptr(), None if rnorm is None else rnorm.data_ptr(), _stream(dev)),
                    "gll_features_forward")
            else:
                X = Zd    # fp32, read in place (16-B loads when aligned, scalar ones otherwise)
            lab = None if labels is None else labels.detach().to(device=dev, dtype=torch.int64).contiguous()
            A = rows if mode == _lib.SC_ALL else bsz
            loss = torch.empty((), dtype=torch.float64, device=dev)
            row_loss = torch.empty(A, dtype=torch.float32, device=dev)
            stats = torch.empty((rows, 4), dtype=torch.float32, device=dev)
            scratch = torch.empty(lib.gll_supcon_scratch_bytes(rows, d), dtype=torch.uint8, device=dev)
            _lib.check(lib.gll_supcon_forward(
                rows, V, d, X.data_ptr(), None if lab is None else lab.data_ptr(), mode, T, Tb,
                loss.data_ptr(), row_loss.data_ptr(), stats.data_ptr(), scratch.data_ptr(),
                _stream(dev)), "gll_supcon_forward")
            out = loss.to(torch.float32)
        ctx.save_for_backward(X, rnorm, stats, lab)
        ctx.args = (rows, V, d, mode, T, Tb, normalize, front, features.dtype, features.device, dev)
        ctx.mark_non_differentiable(row_loss)
        if features.device != dev:
            out, row_loss = out.to(features.device), row_loss.to(features.device)
        return out, row_loss

    @staticmethod
    def backward(ctx, grad_loss, _grad_rows):
        X, rnorm, stats, lab = ctx.saved_tensors
        rows, V, d, mode, T, Tb, normalize, front, dtype, src_dev, dev = ctx.args
        lib = _lib.lib()
        with torch.cuda.device(dev):
            gl = grad_loss.detach().to(device=dev, dtype=torch.float64).contiguous()   # stays on the device
            gX = torch.empty((rows // V, V, d), dtype=torch.float32, device=dev)
            scratch = torch.empty(lib.gll_supcon_scratch_bytes(rows, d), dtype=torch.uint8, device=dev)
            _lib.check(lib.gll_supcon_backward(
                rows, V, d, X.data_ptr(), None if lab is None else lab.data_ptr(), mode, T, Tb,
                stats.data_ptr(), gl.data_ptr(), gX.data_ptr(), scratch.data_ptr(), _stream(dev)),
                "gll_supcon_backward")
            if front:
                gZ = torch.empty((rows // V, V, d), dtype=dtype, device=dev)
                _lib.check(lib.gll_features_backward(
                    rows, d, gX.data_ptr(), X.data_ptr() if normalize else None,
                    rnorm.data_ptr() if normalize else None, _lib.UF_NORMALIZE if normalize else 0,
                    gZ.data_ptr(), _xt_code(dtype), _stream(dev)), "gll_features_backward")
            else:
                gZ = gX
        if src_dev != dev:
            gZ = gZ.to(src_dev)
        return gZ, None, None, None, None, None


def supcon_loss(features, labels=None, temperature=0.07, base_temperature=0.07,
                contrast_mode="all", normalize=False, return_rows=False):
    """The SupCon loss of features [bsz, n_views, ...] (float32, float16 or bfloat16) under
    `labels` [bsz], or the SimCLR loss when labels is None, as losses.py:11-98 computes it, in
    two launches forward and two backward (include/gll.h gll_supcon_forward).  normalize=True
    takes raw features and runs F.normalize(dim=-1) and its backward on the device in one more
    launch each way; half-precision features take the same front end and get their gradient back
    in their dtype.  return_rows=True also returns the anchors' losses (float32, the reference's
    view-major order; not differentiable).  A 0-dim float32 tensor on features.device."""
    if not isinstance(normalize, bool):
        raise TypeError("normalize must be a bool")
    features, labels = _check_features(features, labels, None)
    mode = _mode_code(contrast_mode)
    T, Tb = float(temperature), float(base_temperature)
    loss, rows = _SupConPython.apply(features, labels, T, Tb, mode, normalize)
    return (loss, rows) if return_rows else loss


class SupConLoss(torch.nn.Module):
    """The reference's SupConLoss (losses.py:11-98) on the device: forward(features, labels=None,
    mask=None) with features [bsz, n_views, ...] already unit-norm, as every network of the
    reference returns them.  SimCLR when labels is None.  An explicit mask is not built:
    supcon_loss_torch takes one."""

    def __init__(self, temperature=0.07, contrast_mode="all", base_temperature=0.07):
        super().__init__()
        self.temperature = temperature
        self.contrast_mode = contrast_mode
        self.base_temperature = base_temperature

    def forward(self, features, labels=None, mask=None):
        _check_features(features, labels, mask)
        if mask is not None:
            raise NotImplementedError(
                "SupConLoss(mask=...) has no device kernel: use supcon_loss_torch(features, mask=mask)")
        return supcon_loss(features, labels, self.temperature, self.base_temperature,
                           self.contrast_mode)


def supcon_loss_torch(features, labels=None, mask=None, temperature=0.07, base_temperature=0.07,
                      contrast_mode="all"):
    """The same loss in plain torch, from the closed form of include/gll.h: the yardstick of
    supcon_loss, and the form that takes an explicit `mask` [bsz, bsz] (mask[a, b] = 1: every
    view of sample b is a positive of the views of sample a).  Differentiable by autograd;
    materialises the R x R logits."""
    features, labels = _check_features(features, labels, mask)
    mode = _mode_code(contrast_mode)
    bsz, V, d = features.shape
    R = bsz * V
    z = features.reshape(R, d)                       # row r = b V + v
    sample = torch.arange(R, device=z.device) // V
    if mask is not None:
        same = mask.to(device=z.device, dtype=z.dtype)[sample][:, sample]
    else:
        key = sample if labels is None else labels.to(z.device)[sample]
        same = (key[:, None] == key[None, :]).to(z.dtype)
    off = 1.0 - torch.eye(R, dtype=z.dtype, device=z.device)
    logits = (z @ z.T) / temperature
    m = logits.max(dim=1, keepdim=True)[0].detach()
    logE = torch.log((torch.exp(logits - m) * off).sum(1))
    pos = same * off
    row = -(temperature / base_temperature) * ((pos * logits).sum(1) / pos.sum(1) - m[:, 0] - logE)
    if mode == _lib.SC_ONE:
        row = row.view(bsz, V)[:, 0]
    return row.mean()
