"""Count the backward's kernel launches -- a test helper, not a test.

`with counted() as got:` brackets every launch of the edge pass, the gradient, the fused backward
and the CG (gll_prof_enable with period 1) while the block runs; on exit it synchronises and `got`
holds the number of launches of each, in the order tests/grad_ref.py route() names them:

    got.counts == (GLL_K_EDGE, GLL_K_GRAD, GLL_K_BWD, GLL_K_CG)

The brackets are process-wide (one pending list per kernel id, emptied by gll_prof_read), so
nested use is not supported.
"""
from __future__ import annotations

from contextlib import contextmanager


class Launches:
    edge = grad = bwd = cg = -1

    @property
    def counts(self):
        return (self.edge, self.grad, self.bwd, self.cg)

    def __repr__(self):
        return f"Launches(edge={self.edge}, grad={self.grad}, bwd={self.bwd}, cg={self.cg})"


@contextmanager
def counted():
    import torch

    from graphlearninglayer_amd import _lib as L
    kids = (L.K_EDGE, L.K_GRAD, L.K_BWD, L.K_CG)
    got = Launches()
    for k in kids:
        L.prof_read(k)          # drop pairs an earlier bracket left unread
        L.prof_enable(k, 1)
    try:
        yield got
        torch.cuda.synchronize()
        got.edge, got.grad, got.bwd, got.cg = (L.prof_read(k)[1] for k in kids)
    finally:
        for k in kids:
            L.prof_enable(k, 0)
