"""CPU checks of the extension's backward (extend_grad.hip): the closed form of
tests/extend_grad_ref.py against float64 autograd of the plain formula and against central finite
differences, the case table's boundary gaps and list shapes, extend_torch against the forward
reference, and the C ABI's header, exports and argument checks through ctypes (no GPU call)."""
import ctypes as ct

import numpy as np
import pytest
import torch

from graphlearninglayer_amd import _lib
from tests import extend_grad_ref as E
from tests import query_ref as R

OK, INVALID, UNSUPPORTED = 0, -1, -2
CASES = list(E.GRAD_CASES)


def _autograd(name, eps_as_tensor=False):
    """float64 torch.autograd of extend_torch on the case's exact lists."""
    from graphlearninglayer_amd import GLL
    Xq, Xdb, P, k, epsilon, eps_db, gU, idx, d2 = E.grad_case(name)
    t = lambda a: torch.from_numpy(np.array(a, dtype=np.float64)).requires_grad_(True)
    xq, xdb, p = t(Xq), t(Xdb), t(P)
    eps = epsilon
    if epsilon != "auto" and eps_as_tensor:
        eps = torch.tensor(float(epsilon), dtype=torch.float64, requires_grad=True)
    Uq = GLL.extend_torch(xq, xdb, p, torch.from_numpy(np.array(idx)), eps,
                          None if eps_db is None else torch.from_numpy(np.array(eps_db)))
    (Uq * torch.from_numpy(np.array(gU))).sum().backward()
    geps = eps.grad.item() if torch.is_tensor(eps) else None
    return Uq.detach().numpy(), xq.grad.numpy(), xdb.grad.numpy(), p.grad.numpy(), geps


def _rel(got, ref):
    return np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300)


@pytest.mark.parametrize("name", CASES)
def test_closed_form_matches_float64_autograd(name):
    Xq, Xdb, P, k, epsilon, eps_db, gU, idx, d2 = E.grad_case(name)
    ref = E.closed_form(Xq, Xdb, P, idx, d2, gU, epsilon, eps_db)
    Uq, gq, gdb, gp, geps = _autograd(name, eps_as_tensor=True)
    for key, got in (("gXq", gq), ("gXdb", gdb), ("gP", gp)):
        if name == "tiny" and key != "gP":   # C = 1: u = P[j], the feature gradients are rounding noise around 0
            assert np.abs(ref[key]).max() <= 1e-15 and np.abs(got).max() <= 1e-15
            continue
        err = _rel(ref[key], got)
        print(name, key, err)
        assert err <= 1e-12
    if epsilon == "auto":
        assert ref["geps"] is None and geps is None
    else:                                   # a fixed eps passed as a tensor
        assert abs(ref["geps"] - geps) <= 1e-12 * max(abs(geps), 1e-300)


@pytest.mark.parametrize("name", CASES)
def test_extend_torch_in_float64_equals_the_forward_reference(name):
    Xq, Xdb, P, k, epsilon, eps_db, gU, idx, d2 = E.grad_case(name)
    Uq = _autograd(name)[0]
    ref = R.extend_ref(idx, d2, P, k - 1, epsilon, eps_db)[0]
    assert np.allclose(Uq, ref, rtol=1e-12, atol=1e-14)
    assert np.allclose(E.forward_np(Xq, Xdb, P, idx, epsilon, eps_db), ref, rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("name", ["fixed", "auto", "auto_wide", "hub_auto", "long_d"])
def test_closed_form_matches_central_differences(name):
    """L = sum(gU * Uq) moved along a handful of coordinates of each input: h = 1e-5 of the
    coordinate's scale, truncation O(h^2) and float64 rounding O(1e-16 / h), both far under the
    1e-6 of the largest gradient entry asked for here."""
    Xq, Xdb, P, k, epsilon, eps_db, gU, idx, d2 = E.grad_case(name)
    ref = E.closed_form(Xq, Xdb, P, idx, d2, gU, epsilon, eps_db)
    base = [np.array(a, dtype=np.float64) for a in (Xq, Xdb, P)]
    rng = np.random.default_rng(5)
    h = 1e-5

    def loss(arrs, eps):
        return float((E.forward_np(arrs[0], arrs[1], arrs[2], idx, eps, eps_db) * gU).sum())

    listed = np.unique(idx)
    for which, key in enumerate(("gXq", "gXdb", "gP")):
        rows = rng.choice(listed, size=3) if which else rng.integers(0, len(Xq), size=3)
        for row in rows:
            col = int(rng.integers(0, base[which].shape[1]))
            up = [a.copy() for a in base]
            dn = [a.copy() for a in base]
            up[which][row, col] += h
            dn[which][row, col] -= h
            fd = (loss(up, epsilon) - loss(dn, epsilon)) / (2 * h)
            assert abs(fd - ref[key][row, col]) <= 1e-6 * np.abs(ref[key]).max(), (key, row, col)
    if epsilon != "auto":
        fd = (loss(base, epsilon + h) - loss(base, epsilon - h)) / (2 * h)
        assert abs(fd - ref["geps"]) <= 1e-6 * abs(ref["geps"])


def test_no_case_has_a_boundary_tie_and_the_lists_have_the_shapes_the_gpu_test_needs():
    """With no row at a float64 boundary tie the GPU's lists are the reference's sets and the GPU
    test excuses no row.  The hub case: row 0 in every list, lists longer than a wave (and than
    the 64 entries of GLL_EGF_SMALL_LISTS), most rows empty."""
    for name in CASES:
        Xq, Xdb, P, k, epsilon, eps_db, gU, idx, d2 = E.grad_case(name)
        gap = R.boundary_gap(Xq, Xdb, k - 1)
        assert gap.min() > R.tie_gap(Xq.shape[1]), (name, gap.min())
        assert (d2 > 0).all()
    Xq, Xdb, P, k, *_, idx, d2 = E.grad_case("hub_fixed")
    lists = E.transposed_lists(idx, len(Xdb))
    lens = np.array([len(v) for v in lists])
    assert lens.sum() == idx.size and lens[0] == len(Xq) == 300
    assert (lens > 64).sum() == 9 and (lens == 0).sum() == 486
    for v in lists:
        assert (np.diff(v[:, 0]) > 0).all()          # ascending q, a query at most once
    assert E.transposed_lists(np.array([[0, -1], [5, 1]]), 5)[1].tolist() == [[1, 1]]
    # the paths the table is there for
    assert E.grad_case("auto_wide")[7].shape[1] == 79 and E.grad_case("auto_wide")[0].shape[1] % 4
    assert E.grad_case("kmax")[7].shape[1] == 256 and E.grad_case("kmax")[2].shape[1] == 256
    assert E.grad_case("long_d")[0].shape[1] > 2 * 256


@pytest.mark.parametrize("name", CASES)
def test_stage_bound_is_finite_and_dominated_by_the_fp32_store(name):
    Xq, Xdb, P, k, epsilon, eps_db, gU, idx, d2 = E.grad_case(name)
    ref = E.closed_form(Xq, Xdb, P, idx, d2.astype(np.float32), gU, epsilon, eps_db, bounds=True)
    for key in ("gXq", "gXdb", "gP"):
        b = ref["b_" + key]
        assert np.isfinite(b).all() and (b > 0).all()
        if name == "tiny":      # C = 1: the feature gradients cancel to 0, the bound is all noise
            continue
        # float64 noise: far below single precision relative to the output's scale
        assert b.max() <= 2.0 ** -20 * max(np.abs(ref[key]).max(), 1e-30) + 2.0 ** -148
    assert (ref["b_geps"] is None) == (epsilon == "auto")


def test_header_symbols_are_exported_and_bound():
    lib = _lib.lib()
    for name in ("gll_extend_grad_workspace_bytes", "gll_extend_backward", "gll_extend_grad_launches"):
        assert name in _lib.EXPORTS
        assert hasattr(lib, name)
    assert (_lib.EG_XQ, _lib.EG_XDB, _lib.EG_P, _lib.EG_EPS, _lib.EGF_SMALL_LISTS) == (1, 2, 4, 8, 1)
    src = open(_lib.HERE + "/../include/gll.h").read()
    for text in ("#define GLL_EG_XQ 1", "#define GLL_EG_XDB 2", "#define GLL_EG_P 4",
                 "#define GLL_EG_EPS 8", "#define GLL_EGF_SMALL_LISTS 1"):
        assert text in src
    assert lib.gll_extend_grad_launches() >= 0
    import graphlearninglayer_amd as pkg
    assert callable(pkg.extend_torch) and "extend_torch" in pkg.__all__


def test_argument_limits_without_a_gpu():
    lib = _lib.lib()
    nb = lib.gll_extend_grad_workspace_bytes
    n0 = lib.gll_extend_grad_launches()

    def b(Q=8, N=100, kn=5, d=16, C=3, what=15, flags=0, eps=1.0, eps_db=None, null=(), p=256):
        # pointers are never dereferenced: every check comes before any HIP call
        a = {n: p for n in ("Xq", "Xdb", "idx", "d2", "P", "gU", "gXq", "gXdb", "gP", "geps", "st", "ws")}
        for n in null:
            a[n] = None
        return lib.gll_extend_backward(Q, N, kn, d, C, a["Xq"], a["Xdb"], a["idx"], a["d2"], a["P"],
                                       eps_db, ct.c_float(eps), a["gU"], what, flags, a["gXq"],
                                       a["gXdb"], a["gP"], a["geps"], a["st"], a["ws"], None)

    good = dict(Q=8, N=100, kn=5, d=16, C=3, what=15, flags=0)
    assert nb(*good.values()) > 0
    for kw in (dict(Q=0), dict(N=0), dict(kn=0), dict(d=0), dict(C=0), dict(what=0), dict(what=16),
               dict(flags=2)):
        assert b(**kw) == INVALID, kw
        assert nb(*{**good, **kw}.values()) == 0
    for kw in (dict(kn=257), dict(C=257), dict(d=4097), dict(N=(2 ** 31 - 1) // 2 + 1)):
        assert b(**kw) == UNSUPPORTED, kw
        assert nb(*{**good, **kw}.values()) == 0
    assert nb(1, 1, 1, 1, 1, 1, 0) > 0 and nb(8, 300, 256, 4096, 256, 15, 1) > 0   # the limits
    # required pointers, and the outputs that `what` selects
    for n in ("Xq", "Xdb", "idx", "d2", "P", "gU", "st", "ws", "gXq", "gXdb", "gP", "geps"):
        assert b(null=(n,)) == INVALID, n
    # 'auto': eps_db is required and there is no eps gradient
    for eps in (0.0, -1.0, float("nan")):
        assert b(eps=eps, what=7) == INVALID
        assert b(eps=eps, what=8, eps_db=256) == INVALID
        assert b(eps=eps, what=15, eps_db=256) == INVALID
    assert b(p=258) == INVALID                      # misaligned pointers
    assert lib.gll_extend_grad_launches() == n0     # nothing was launched
    # an output that is not selected may be NULL: such a call passes every check and reaches the
    # launch (GLL_ERR_HIP without a device); only where no GPU is present, never on a GPU machine
    if not torch.cuda.is_available():
        assert b(what=1, null=("gXdb", "gP", "geps")) not in (INVALID, UNSUPPORTED)
        assert b(what=4, eps=0.0, eps_db=256, null=("gXq", "gXdb", "geps")) not in (INVALID, UNSUPPORTED)


def test_front_end_rejects_a_bad_epsilon_tensor():
    from graphlearninglayer_amd import GLL
    Xq, Xdb, P = torch.zeros(3, 4), torch.zeros(10, 4), torch.zeros(10, 3)
    with pytest.raises(TypeError):
        GLL.extend(Xq, Xdb, P, k=5, epsilon=torch.ones(2))
    with pytest.raises(ValueError):
        GLL.extend(Xq, Xdb, P, k=5, epsilon=torch.tensor(-1.0, requires_grad=True))
