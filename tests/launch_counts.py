"""Count the backward's kernel launches -- a test helper, not a test.

`with counted() as got:` brackets every launch of the edge pass, the gradient, the fused backward
and the CG (tests/abi.py launches) while the block runs; on exit it synchronises and `got` holds
the number of launches of each, in the order tests/grad_ref.py route() names them:

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
    from graphlearninglayer_amd import _lib as L
    from tests.abi import launches
    got = Launches()
    with launches(L.K_EDGE, L.K_GRAD, L.K_BWD, L.K_CG) as n:
        yield got
    got.edge, got.grad, got.bwd, got.cg = n
