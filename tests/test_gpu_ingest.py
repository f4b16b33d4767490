"""The graph build from caller-supplied neighbour lists on the MI355X (-m gpu): ingest.hip against
the float64 stage reference of tests/ingest_ref.py, and the layer with `neighbors=` against the
oracle on the same lists (oracle.forward(..., knn=(ind, None)) / oracle.backward) at the project's
parity bar ||a - b||_inf / ||b||_inf <= 1e-4 for U and grad_X (README).

Stage test: through the C ABI (gll_graph_lists) into a workspace of 0xFF bytes.  knn_idx, the
kept counts, the padding and the dropped count equal the reference; knn_d2 lies within
ingest_ref.d2_bound (tests/query_ref.py's) and the 'auto' eps within ingest_ref.eps_bound; the
reverse entries are checked as per-row sets through the rows the row build makes of them (col
exact, d2 under the same bound): forward entries U reverse entries, the larger directed d2.

Every oracle comparison prints its figures before it asserts and is recorded in
profiles/nl01_parity.json by the module's teardown."""
import ctypes as ct
import functools
import json
import os
import warnings

import numpy as np
import pytest
import torch

from graphlearninglayer_amd.synth import seeded_gbar
from oracle import gll_oracle as O
from tests import abi as A
from tests import ingest_ref as IR
from tests.param_grad_ref import param_grads

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4
PARITY = {}


def _L():
    from graphlearninglayer_amd import _lib
    return _lib


def _G():
    from graphlearninglayer_amd import GLL
    return GLL


def _LL():
    return _G().LaplaceLearningSparseHard


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    A.need_gpu()
    yield
    try:
        with open(os.path.join(ROOT, "profiles", "nl01_parity.json"), "w") as fh:
            json.dump(PARITY, fh, indent=1, sort_keys=True)
    except OSError:
        pass


def _record(tag, eU, eg):
    PARITY[tag] = {"U": eU, "grad_X": eg}
    print(f"{tag}: U rel err {eU:.3e}, grad_X rel err {eg:.3e}")


# ------------------------------------------------------------------------------------------------
# 1. the stage against its reference
# ------------------------------------------------------------------------------------------------
def _stage_run(X, nbr, epsilon):
    """gll_graph_lists on a 0xFF workspace: the arrays of gll_workspace_view on the host."""
    L = _L()
    n, K = X.shape[0], nbr.shape[1] + 1
    run = A.Run(X, None, K, 0.0, epsilon, L.FLAG_KNN_GIVEN, C=1, ws_fill=0xFF, neighbors=nbr)
    run.graph()
    v, host = run.view(), run.host_copy()

    def arr(ptr, count, dtype):
        return run.array(ptr, count, dtype, snapshot=host).copy()

    start, length = arr(v.row_start, n, np.int32), arr(v.row_len, n, np.int32)
    span = int((start.astype(np.int64) + length).max())
    col, d2 = arr(v.col, span, np.int32), arr(v.d2, span, np.float32)
    rows = [dict(zip(col[s:s + l].tolist(), d2[s:s + l].tolist())) for s, l in zip(start, length)]
    return dict(knn_idx=arr(v.knn_idx, n * K, np.int32).reshape(n, K),
                knn_d2=arr(v.knn_d2, n * K, np.float32).reshape(n, K),
                eps=arr(v.eps, n, np.float32), rows=rows, length=length,
                status=arr(v.status, L.ST_NWORDS, np.int32))


def _check_stage(name, epsilon):
    L = _L()
    X, nbr = IR.case(name)
    ref = IR.stage(name, epsilon)
    out = _stage_run(X, nbr, epsilon)
    d = X.shape[1]
    assert (out["knn_idx"] == ref.knn_idx).all()
    assert (out["knn_idx"][:, 0] == np.arange(X.shape[0])).all() and (out["knn_d2"][:, 0] == 0).all()
    pad = ref.knn_d2 == 0
    assert (out["knn_d2"][pad] == 0).all()                 # the self slot and the padding
    rel = np.abs(out["knn_d2"].astype(np.float64) - ref.knn_d2)[~pad] / ref.knn_d2[~pad]
    worst_d2 = float(rel.max())
    assert worst_d2 <= IR.d2_bound(d), worst_d2
    if isinstance(epsilon, str):
        z = ref.eps == 0
        assert (out["eps"][z] == 0).all()
        e = np.abs(out["eps"].astype(np.float64) - ref.eps)[~z] / ref.eps[~z]
        assert e.max() <= IR.eps_bound(d), e.max()
    else:
        assert (out["eps"] == np.float32(epsilon)).all()
    assert int(out["status"][L.ST_LIST_DROPPED]) == ref.dropped
    assert bool(out["status"][L.ST_TINY_EPS]) == ref.tiny_eps
    # reverse entries, as per-row sets, through the symmetric rows
    want = IR.sym_rows(ref)
    worst_e = 0.0
    for i, (g, w) in enumerate(zip(out["rows"], want)):
        assert sorted(g) == sorted(w), i
        for j, v in w.items():
            worst_e = max(worst_e, abs(g[j] - v) / v)
    assert worst_e <= IR.d2_bound(d), worst_e
    print(f"ingest stage {name} eps={epsilon}: d2 err/bound {worst_d2 / IR.d2_bound(d):.4f}, "
          f"edges err/bound {worst_e / IR.d2_bound(d):.4f}, dropped {ref.dropped}, "
          f"longest row {int(out['length'].max())}")
    return out, ref


@pytest.mark.parametrize("epsilon", [1.0, "auto"])
@pytest.mark.parametrize("name", ["ragged", "ns", "parts2", "parts4"])
def test_stage_matches_reference(name, epsilon):
    _check_stage(name, epsilon)


@pytest.mark.parametrize("epsilon", [1.0, "auto"])
def test_stage_reverse_overflow(epsilon):
    """Column 0 of every list is row 0: 199 reverse entries on one row, RCAP = 24."""
    out, _ = _check_stage("hub", epsilon)
    p = _G().make_problem(200, 16, 0, 1, 3, 0.0, 1.0, flags=_L().FLAG_KNN_GIVEN)
    sv = _L().SolveView()
    assert _L().lib().gll_workspace_solve_view(ct.byref(p), ct.c_void_p(256), ct.byref(sv)) == 0
    assert sv.RCAP == 24 and out["length"][0] == 199 > sv.RCAP


@pytest.mark.parametrize("epsilon", [1.0, "auto"])
def test_stage_drops(epsilon):
    """Entries of -1, n, a repeat, the row itself and a duplicated point: the dropped count and the
    padded form."""
    out, ref = _check_stage("bad", epsilon)
    assert ref.dropped >= 8      # -1, n, one repeat, k - 2 repeats, the out-of-range last column
    n, K = out["knn_idx"].shape
    for i in range(n):
        kept = int(ref.kept[i])
        assert (out["knn_idx"][i, 1 + kept:] == i).all() and (out["knn_d2"][i, 1 + kept:] == 0).all()
        assert (out["knn_d2"][i, 1:1 + kept] > 0).all()
    assert ref.kept.min() == 1 and (ref.kept < K - 1).sum() >= 6


# ------------------------------------------------------------------------------------------------
# 2. oracle parity on shuffled approximate lists
# ------------------------------------------------------------------------------------------------
def _apply(X, Y, nbr, tau, eps, k, gbar, fn="apply", **kw):
    """(U, grad_X) on the device; X, Y, nbr device tensors."""
    Xt = X.detach().clone().requires_grad_(True)
    f = getattr(_LL(), fn)
    U = f(Xt, Y, tau, eps, k, nbr) if fn == "apply_python" else \
        f(Xt, Y, tau, eps, k, neighbors=nbr, **kw)
    (gX,) = torch.autograd.grad(U, Xt, gbar)
    return U.detach(), gX


@functools.lru_cache(maxsize=None)
def _oracle(config, eps, tau):
    X, Y, nbr, k = IR.layer_case(config)
    U, st = O.forward(X, Y, tau, eps, k, knn=(IR.with_self(nbr), None))
    gbar = seeded_gbar(U.shape[0], U.shape[1])
    return U, O.backward(st, gbar), st, gbar


@pytest.mark.parametrize("tau", [0.0, 0.07])
@pytest.mark.parametrize("eps", [1.0, "auto"])
@pytest.mark.parametrize("config", ["plumbing", "ns", "fullysup"])
def test_oracle_parity_on_shuffled_lists(config, eps, tau):
    X, Y, nbr, k = IR.layer_case(config)
    assert IR.components(nbr) == 1 and Y.shape[0] > 0
    Uo, go, _, gbar = _oracle(config, eps, tau)
    U, gX = _apply(A.dev(X), A.dev(Y), A.dev(nbr), tau, eps, k, A.dev(gbar))
    eU, eg = O.rel_err(U.cpu().numpy(), Uo), O.rel_err(gX.cpu().numpy(), go)
    _record(f"{config}_eps{eps}_tau{tau}", eU, eg)
    assert eU <= TOL and eg <= TOL, (eU, eg)


def test_self_column_and_int32_lists_are_the_same_call():
    """n x k with the self column (the reference's knn_ind, device_graph()['knn_idx']) and
    n x (k - 1), int32 or int64, on the host or the device: bitwise one result."""
    X, Y, nbr, k = IR.layer_case("plumbing")
    _, _, _, gbar = _oracle("plumbing", "auto", 0.07)
    Xd, Yd, gd = A.dev(X), A.dev(Y), A.dev(gbar)
    U0, g0 = _apply(Xd, Yd, A.dev(nbr), 0.07, "auto", k, gd)
    for other in (A.dev(IR.with_self(nbr)), A.dev(nbr, torch.int32),
                  torch.from_numpy(IR.with_self(nbr).astype(np.int32)),
                  A.dev(IR.with_self(nbr))[:, 1:]):            # not contiguous
        U1, g1 = _apply(Xd, Yd, other, 0.07, "auto", k, gd)
        assert torch.equal(U0, U1) and torch.equal(g0, g1)


def test_batch_of_three_is_bitwise_the_single_calls():
    from graphlearninglayer_amd.synth import CONFIGS, one_hot, synth
    c = CONFIGS["plumbing"]
    Xs, Ys, Ns = [], [], []
    for seed in (0, 1, 2):
        X, lab = synth(c["base"], c["batch"], c["d"], r=c["r"], seed=seed)
        Xs.append(X), Ys.append(one_hot(lab[: c["base"]])), Ns.append(IR.approx_lists(X, c["k"], seed))
    gbar = np.stack([seeded_gbar(c["batch"], 10, seed=s) for s in (5, 6, 7)])
    for eps in (1.0, "auto"):
        Ub, gb = _apply(A.dev(np.stack(Xs)), A.dev(np.stack(Ys)), A.dev(np.stack(Ns)), 0.07, eps,
                        c["k"], A.dev(gbar))
        for b in range(3):
            U1, g1 = _apply(A.dev(Xs[b]), A.dev(Ys[b]), A.dev(Ns[b]), 0.07, eps, c["k"], A.dev(gbar[b]))
            assert torch.equal(Ub[b], U1) and torch.equal(gb[b], g1), (eps, b)
        Uo, st = O.forward(Xs[1], Ys[1], 0.07, eps, c["k"], knn=(IR.with_self(Ns[1]), None))
        eU = O.rel_err(Ub[1].cpu().numpy(), Uo)
        eg = O.rel_err(gb[1].cpu().numpy(), O.backward(st, gbar[1]))
        _record(f"batch3_graph1_eps{eps}", eU, eg)
        assert eU <= TOL and eg <= TOL


def test_normalize_and_bf16_features():
    """Distances come from the front end's fp32 rows: the call equals the layer on
    unit_features(Z) bitwise, which is held to the oracle on those rows."""
    G = _G()
    X, Y, nbr, k = IR.layer_case("plumbing")
    gbar = A.dev(seeded_gbar(64, 10))
    Z = A.dev(X * 3.0).to(torch.bfloat16)
    Xh, rnorm = G.unit_features(Z, True)
    Zt = Z.clone().requires_grad_(True)
    U = _LL().apply(Zt, A.dev(Y), 0.07, "auto", k, True, neighbors=A.dev(nbr))
    (gZ,) = torch.autograd.grad(U, Zt, gbar)
    U1, gX1 = _apply(Xh, A.dev(Y), A.dev(nbr), 0.07, "auto", k, gbar)
    assert torch.equal(U.detach(), U1)
    assert gZ.dtype == torch.bfloat16
    assert torch.equal(gZ, G.unit_features_backward(gX1, Xh, rnorm, torch.bfloat16, True))
    Xn = Xh.cpu().numpy()
    Uo, st = O.forward(Xn, Y, 0.07, "auto", k, knn=(IR.with_self(nbr), None))
    eU = O.rel_err(U1.cpu().numpy(), Uo)
    eg = O.rel_err(gX1.cpu().numpy(), O.backward(st, gbar.cpu().numpy()))
    _record("plumbing_normalize_bf16_epsauto_tau0.07", eU, eg)
    assert eU <= TOL and eg <= TOL


def test_label_tau_and_epsilon_gradients():
    X, Y, nbr, k = IR.layer_case("plumbing")
    Uo, go, st, gbar = _oracle("plumbing", 1.0, 0.07)
    ref = param_grads(st, gbar)
    Xt = A.dev(X).requires_grad_(True)
    Yt = A.dev(Y).requires_grad_(True)
    tt = torch.tensor(0.07, dtype=torch.float64, device="cuda", requires_grad=True)
    et = torch.tensor(1.0, dtype=torch.float64, device="cuda", requires_grad=True)
    U = _LL().apply(Xt, Yt, tt, et, k, neighbors=A.dev(nbr))
    gX, gY, gt, ge = torch.autograd.grad(U, (Xt, Yt, tt, et), A.dev(gbar))
    eU, eg = O.rel_err(U.detach().cpu().numpy(), Uo), O.rel_err(gX.cpu().numpy(), go)
    eY = O.rel_err(gY.cpu().numpy(), ref.grad_Y)
    e_tau = abs(float(gt) - ref.grad_tau) / ref.tau_terms
    e_eps = abs(float(ge) - ref.grad_eps) / ref.eps_terms
    _record("plumbing_param_grads_eps1.0_tau0.07", eU, eg)
    print(f"grad_Y rel err {eY:.3e}, grad_tau err / sum|terms| {e_tau:.3e}, grad_eps err / "
          f"sum|terms| {e_eps:.3e}")
    assert max(eU, eg, eY, e_tau, e_eps) <= TOL


# ------------------------------------------------------------------------------------------------
# 3. hub: one column in every row's list
# ------------------------------------------------------------------------------------------------
def test_hub_column_against_the_oracle():
    """n = 600, k = 5: row 599 is in every other row's list, a row of 599 entries -- past the LDS
    staging of the row build, through the overflow triples and the bump region, and a CG row of
    ~n entries."""
    from graphlearninglayer_amd.synth import one_hot, synth
    X, lab = synth(300, 300, 32, r=0.75, seed=3)
    Y = one_hot(lab[:300])
    nbr = IR.approx_lists(X, 5, 3).copy()
    hub = 599
    for i in range(599):
        if hub not in nbr[i]:
            nbr[i, 0] = hub
    assert (nbr[:599] == hub).sum() == 599 and IR.components(nbr) == 1
    gbar = seeded_gbar(300, 10)
    for eps in (1.0, "auto"):
        Uo, st = O.forward(X, Y, 0.07, eps, 5, knn=(IR.with_self(nbr), None))
        go = O.backward(st, gbar)
        U, gX = _apply(A.dev(X), A.dev(Y), A.dev(nbr), 0.07, eps, 5, A.dev(gbar))
        eU, eg = O.rel_err(U.cpu().numpy(), Uo), O.rel_err(gX.cpu().numpy(), go)
        _record(f"hub600_eps{eps}_tau0.07", eU, eg)
        assert eU <= TOL and eg <= TOL, (eps, eU, eg)


# ------------------------------------------------------------------------------------------------
# 4. exact lists reproduce the searched layer
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [10, 100])
def test_exact_lists_reproduce_the_search(k):
    from graphlearninglayer_amd.synth import CONFIGS, one_hot, synth
    G = _G()
    c = CONFIGS["ns"]
    X, lab = synth(c["base"], c["batch"], c["d"], r=c["r"], seed=0)
    Y = one_hot(lab[: c["base"]])
    nbr = IR.exact_lists(X, k)
    # Two neighbours of a row whose float64 distances differ by less than twice the searching
    # kernel's own d2 bound may come out of the search in either order: the narrow select
    # (k - 1 <= 56) ranks a row's interior by its fp32 sums (tests/query_ref.py d2_bound), the wide
    # one by float64 sums in another order (query_ref.tie_gap).  Such rows are held to the same set
    # and the same last column; every other row to the identical list.
    from tests import query_ref as Q
    dl = np.take_along_axis(Q.dist2(X, X), nbr, axis=1)
    sep = 2 * IR.d2_bound(X.shape[1]) if k - 1 <= 56 else Q.tie_gap(X.shape[1])
    tie = ((dl[:, 1:] - dl[:, :-1]) <= sep * dl[:, 1:]).any(axis=1)
    assert tie.sum() <= 5, tie.sum()                  # NS: 4 rows at k = 10, none at k = 100
    gbar = seeded_gbar(c["batch"], 10)
    Xd, Yd, gd = A.dev(X), A.dev(Y), A.dev(gbar)
    for eps in (1.0, "auto"):
        gs = G.device_graph(Xd, k, eps)
        gl = G.device_graph(Xd, k, eps, neighbors=A.dev(nbr))
        assert (gl["knn_idx"][:, 1:].cpu().numpy() == nbr).all()
        si = gs["knn_idx"].cpu().numpy()
        assert (si[~tie, 1:] == nbr[~tie]).all()
        assert (np.sort(si[tie, 1:], axis=1) == np.sort(nbr[tie], axis=1)).all()
        if tie.any():      # the d2 comparison below pairs entries by column
            order = np.argsort(si[:, 1:], axis=1)
            back = np.argsort(np.argsort(nbr, axis=1), axis=1)
            perm = np.take_along_axis(order, back, axis=1)
            sd = np.take_along_axis(gs["knn_d2"].cpu().numpy()[:, 1:], perm, axis=1)
            gs = dict(gs, knn_d2=torch.from_numpy(np.concatenate([np.zeros((len(X), 1), np.float32),
                                                                   sd], axis=1)).cuda())
        # each kernel's d2 is within its own derived bound of float64: the narrow select's fp32
        # sums (tests/query_ref.py d2_bound) or the wide select's float64 sum, and the ingest's
        a, b = gs["knn_d2"].double(), gl["knn_d2"].double()
        rel = ((a - b).abs()[:, 1:] / b[:, 1:]).max().item()
        assert rel <= 2 * IR.d2_bound(X.shape[1]), rel
        Xt = Xd.clone().requires_grad_(True)
        Us = _LL().apply(Xt, Yd, 0.07, eps, k)
        (gXs,) = torch.autograd.grad(Us, Xt, gd)
        Ul, gXl = _apply(Xd, Yd, A.dev(nbr), 0.07, eps, k, gd)
        eU = O.rel_err(Ul.cpu().numpy(), Us.detach().cpu().numpy())
        eg = O.rel_err(gXl.cpu().numpy(), gXs.cpu().numpy())
        Uo, st = O.forward(X, Y, 0.07, eps, k, knn=(IR.with_self(nbr), None))
        eUo, ego = O.rel_err(Ul.cpu().numpy(), Uo), O.rel_err(gXl.cpu().numpy(), O.backward(st, gbar))
        print(f"exact lists k={k} eps={eps}: vs apply() U {eU:.3e} grad_X {eg:.3e}; d2 rel {rel:.3e}")
        _record(f"ns_exact_k{k}_eps{eps}_tau0.07", eUo, ego)
        assert max(eU, eg, eUo, ego) <= TOL


# ------------------------------------------------------------------------------------------------
# 5. bitwise: the two host paths, two runs
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [1.0, "auto"])
def test_native_and_python_paths_agree_bitwise(eps):
    X, Y, nbr, k = IR.layer_case("plumbing")
    gbar = A.dev(seeded_gbar(64, 10))
    a = _apply(A.dev(X), A.dev(Y), A.dev(nbr), 0.07, eps, k, gbar)
    b = _apply(A.dev(X), A.dev(Y), A.dev(nbr), 0.07, eps, k, gbar, fn="apply_python")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("config", ["plumbing", "fullysup"])
def test_two_runs_are_bitwise_equal(config):
    G = _G()
    X, Y, nbr, k = IR.layer_case(config)
    gbar = A.dev(seeded_gbar(X.shape[0] - Y.shape[0], 10))
    for eps in (1.0, "auto"):
        runs = []
        for _ in range(2):
            g = G.device_graph(A.dev(X), k, eps, neighbors=A.dev(nbr))
            U, gX = _apply(A.dev(X), A.dev(Y), A.dev(nbr), 0.07, eps, k, gbar)
            runs.append((g["knn_idx"].clone(), g["knn_d2"].clone(), g["eps"].clone(), U, gX))
        for x, y in zip(*runs):
            assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------
# 6. the heads
# ------------------------------------------------------------------------------------------------
def test_heads_equal_apply_followed_by_the_torch_formulas():
    G = _G()
    X, Y, nbr, k = IR.layer_case("plumbing")
    Xd, Yd, nd = A.dev(X), A.dev(Y), A.dev(nbr)
    m, C = 64, 10
    rng = np.random.default_rng(11)
    tgt = A.dev(rng.integers(0, C, size=m))
    for eps in (1.0, "auto"):
        Xa = Xd.clone().requires_grad_(True)
        Ua = _LL().apply(Xa, Yd, 0.07, eps, k, neighbors=nd)
        # cross-entropy
        Xt = Xd.clone().requires_grad_(True)
        loss, pred, labels, row_loss, correct = _LL().ce_loss(Xt, Yd, tgt, 0.07, eps, k, neighbors=nd)
        assert torch.equal(pred, Ua.detach())
        want = G.custom_ce_loss(Ua, tgt)
        assert abs(float(loss.detach()) - float(want.detach())) <= 1e-12 * abs(float(want.detach()))
        assert torch.equal(labels, Ua.argmax(1)) and int(correct) == int((labels == tgt).sum())
        (g1,) = torch.autograd.grad(loss, Xt)
        (g2,) = torch.autograd.grad(want, Xa, retain_graph=True)
        assert O.rel_err(g1.cpu().numpy(), g2.cpu().numpy()) <= TOL
        # margin
        Xt = Xd.clone().requires_grad_(True)
        out = _LL().margin_loss(Xt, Yd, tgt, 0.07, eps, k, neighbors=nd)
        assert torch.equal(out[1], Ua.detach())
        want = G.cw_margin(Ua, tgt)
        assert abs(float(out[0].detach()) - float(want.detach())) <= 1e-12 * max(abs(float(want.detach())), 1e-30)
        (g1,) = torch.autograd.grad(out[0], Xt)
        (g2,) = torch.autograd.grad(want, Xa, retain_graph=True)
        assert O.rel_err(g1.cpu().numpy(), g2.cpu().numpy()) <= TOL
        # objective with the three weights
        Xt = Xd.clone().requires_grad_(True)
        w = (1.0, 0.3, 0.2)
        out = _LL().objective(Xt, Yd, tgt, 0.07, eps, k, weights=w, neighbors=nd)
        assert torch.equal(out[1], Ua.detach())
        ent = -(Ua * torch.log(Ua + 1e-8)).sum()
        want = (w[0] * G.custom_ce_loss(Ua, tgt) * m + w[1] * ent - w[2] * (Ua * Ua).sum()) / m
        assert abs(float(out[0].detach()) - float(want.detach())) <= 1e-12 * abs(float(want.detach()))
        (g1,) = torch.autograd.grad(out[0], Xt)
        (g2,) = torch.autograd.grad(want, Xa)
        assert O.rel_err(g1.cpu().numpy(), g2.cpu().numpy()) <= TOL


# ------------------------------------------------------------------------------------------------
# 7. a frozen graph over an attack loop
# ------------------------------------------------------------------------------------------------
def test_frozen_graph_sign_gradient_steps():
    """Lists from device_graph of the clean features, weights from the perturbed ones: three
    sign-gradient steps, each against the oracle on the same lists."""
    G = _G()
    X, Y, _, k = IR.layer_case("plumbing")
    Xd, Yd = A.dev(X), A.dev(Y)
    knn_idx = G.device_graph(Xd, k, "auto")["knn_idx"].clone()     # n x k, self first
    ind = knn_idx.cpu().numpy().astype(np.int64)
    gbar = seeded_gbar(64, 10)
    gd = A.dev(gbar)
    Xp = Xd.clone()
    for step in range(3):
        U, gX = _apply(Xp, Yd, knn_idx, 0.07, "auto", k, gd)
        Xh = Xp.cpu().numpy()
        Uo, st = O.forward(Xh, Y, 0.07, "auto", k, knn=(ind, None))
        eU, eg = O.rel_err(U.cpu().numpy(), Uo), O.rel_err(gX.cpu().numpy(), O.backward(st, gbar))
        _record(f"frozen_step{step}_epsauto_tau0.07", eU, eg)
        assert eU <= TOL and eg <= TOL, (step, eU, eg)
        Xp = Xp + 0.01 * gX.sign()
    assert not torch.equal(Xp, Xd)


# ------------------------------------------------------------------------------------------------
# 8. library paths
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [1.0, "auto"])
def test_device_graph_matches_the_oracles_csr(eps):
    G = _G()
    X, _, nbr, k = IR.layer_case("plumbing")
    g = G.device_graph(A.dev(X), k, eps, neighbors=A.dev(nbr))
    Xd = X.astype(np.float64)
    ind = IR.with_self(nbr)
    dist = np.sqrt(((Xd[:, None, :] - Xd[ind]) ** 2).sum(-1))
    og = O.graph_from_knn(ind, dist, eps)
    rp = g["row_ptr"].cpu().numpy()
    rows = np.repeat(np.arange(X.shape[0]), np.diff(rp))
    assert (rows == og.rows).all() and (g["col"].cpu().numpy() == og.cols).all()
    np.testing.assert_allclose(g["d2"].cpu().numpy(), og.dist ** 2, rtol=IR.d2_bound(X.shape[1]))
    # W = exp(-4 d2 / (eps_i eps_j)): the exponent t carries the d2 and eps bounds and fp32 steps
    t = 4.0 * og.dist ** 2 / (og.eps[og.rows] * og.eps[og.cols])
    tolw = t * (IR.d2_bound(X.shape[1]) + 2 * IR.eps_bound(X.shape[1]) + 4 * IR.U32) + 4 * IR.U32
    assert (np.abs(g["w"].cpu().numpy() - og.W) <= tolw * og.W + 1e-38).all()
    assert int(g["status"][_L().ST_LIST_DROPPED]) == 0


def test_utils_laplace_with_lists():
    from graphlearninglayer_amd import utils
    from graphlearninglayer_amd.synth import synth
    X, lab = synth(100, 1900, 64, r=1.0, seed=4)
    nbr = IR.approx_lists(X, 20, 4)
    assert IR.components(nbr) == 1
    U = utils.laplace(X, lab[:100], knn_num=20, epsilon="auto", neighbors=torch.from_numpy(nbr))
    Uo = O.laplace(X, lab[:100], knn_num=20, epsilon="auto", knn=(IR.with_self(nbr), None))
    e = O.rel_err(U, Uo)
    PARITY["utils_laplace_n2000_k20"] = {"U": e}
    print(f"utils.laplace(neighbors=) n=2000: U rel err {e:.3e}")
    assert e <= TOL
    fit = utils.laplace_fit(X, lab[:100], knn_num=20, epsilon="auto",
                            neighbors=torch.from_numpy(nbr))
    assert O.rel_err(fit.P[100:].cpu().numpy(), Uo) <= TOL
    acc = utils.gl_accuracy(X[:100], lab[:100], X[1000:], lab[1000:], X[100:1000], epsilon="auto",
                            knn_num=20, neighbors=torch.from_numpy(nbr))
    assert abs(acc - 100.0 * np.mean(np.argmax(Uo, 1)[-1000:] == lab[1000:])) < 1e-9


def test_dropped_entries_warn_through_the_sink():
    G = _G()
    X, Y, nbr, k = IR.layer_case("plumbing")
    bad = nbr.copy()
    bad[3, 0] = -1
    bad[9, 1] = bad[9, 0]
    G.check_status()
    _LL().apply(A.dev(X), A.dev(Y), 0.07, 1.0, k, neighbors=A.dev(bad))
    with pytest.warns(UserWarning, match="2 list entries were dropped"):
        G.check_status()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        _LL().apply(A.dev(X), A.dev(Y), 0.07, 1.0, k, neighbors=A.dev(nbr))
        G.check_status()


# ------------------------------------------------------------------------------------------------
# 9. argument errors
# ------------------------------------------------------------------------------------------------
def test_argument_errors_on_the_device():
    X, Y, nbr, k = IR.layer_case("plumbing")
    Xd, Yd = A.dev(X), A.dev(Y)
    n = X.shape[0]
    for bad in (torch.zeros(n, k + 1, dtype=torch.int64, device="cuda"),
                torch.zeros(n, k - 2, dtype=torch.int64, device="cuda"),
                torch.zeros(n - 1, k - 1, dtype=torch.int64, device="cuda"),
                torch.zeros(n, k - 1, dtype=torch.float32, device="cuda"),
                torch.zeros(2, n, k - 1, dtype=torch.int64, device="cuda")):
        for fn in ("apply", "apply_python"):
            with pytest.raises(ValueError, match="neighbors"):
                _apply(Xd, Yd, bad, 0.07, 1.0, k, None, fn=fn)
        with pytest.raises(ValueError, match="neighbors"):
            _LL().ce_loss(Xd, Yd, torch.zeros(64, dtype=torch.int64, device="cuda"), 0.07, 1.0, k,
                          neighbors=bad)
    with pytest.raises(ValueError, match="neighbors"):
        _G().device_graph(Xd, k, 1.0, neighbors=torch.zeros(n, k + 3, dtype=torch.int32))
    Xb = torch.stack([Xd, Xd])
    with pytest.raises(ValueError, match="neighbors"):
        _LL().apply(Xb, Yd, 0.07, 1.0, k, neighbors=A.dev(nbr))      # batched X needs B x n x (k-1)
