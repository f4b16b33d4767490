"""HIP path vs the oracle and the reference fixtures (run on the MI355X: -m gpu).

Parity bar (BASELINE.json north_star): forward U and backward grad_X within 1e-4
relative (||a - b||_inf / ||b||_inf) of the reference CPU path on fixed inputs.
  * graph-level parity: the oracle (float64 closed form, pinned to the reference in
    test_oracle_golden.py) is fed the GPU's own kNN lists, so parity of the graph, the
    solves and the gradient is tested independently of fp32 near-ties in the kNN search;
  * fixture parity: the GPU kNN sets must equal the reference's in every row, and U and
    grad_X are compared with the reference outputs directly for every fixture case;
  * kNN parity: index sets equal the exact float64 sets (float64 re-rank + the Gram-error
    certificate); the older near-tie allowance (rel gap < 1e-5) remains only as a looser
    check beside the exact one where the reference itself is not run.
"""
import numpy as np
import pytest
import torch

from graphlearninglayer_amd import GLL
from oracle import gll_oracle as O
from tests import abi as A
from tests.golden_io import Case, nan_aware, names
from tests.parity_runs import (TOL, batched_knn_lists, exact_knn_rows, forward_c_abi,
                                fwd_bwd_batched_c_abi, fwd_bwd_c_abi, gpu_knn, run_layer,
                                synth_batch)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    A.need_gpu()


@pytest.mark.parametrize("name", names())
def test_parity_against_reference_fixture(name):
    c = Case(name)
    assert c.x_ok
    Y = c.Y if c.meta["ydtype"] == "f32" else c.Y.astype(np.int64)
    U, grad = run_layer(c.X, Y, c.tau, c.eps, c.k, c.gbar)
    assert U.dtype == np.float64 and U.shape == c.U.shape
    # graph-level parity with the GPU's own kNN
    g = gpu_knn(c.X, c.k)
    ind = g["knn_idx"].cpu().numpy().astype(np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):   # eps = 0 divides by zero
        Uo, st = O.forward(c.X, c.Y, c.tau, c.eps, c.k, knn=(ind, None))
        go = O.backward(st, c.gbar)
    # NaN where the reference has NaN (eps = 0, GLL.py:234), the metric over the rest
    eU, eg = nan_aware(O.rel_err)(U, Uo), nan_aware(O.rel_err)(grad, go)
    assert eU < TOL, f"U vs oracle(gpu knn): {eU:.3e}"
    assert eg < TOL, f"grad vs oracle(gpu knn): {eg:.3e}"
    # kNN parity against the reference's own lists: identical sets in every row (the float64
    # re-rank and the Gram-error certificate make the GPU search exact), so U and grad_X are
    # compared with the reference outputs directly, in every case -- never skipped
    bad = [i for i, (a, b) in enumerate(zip(ind.tolist(), c.knn.tolist())) if set(a) != set(b)]
    assert bad == [], f"{len(bad)} rows differ from the reference kNN, first {bad[:8]}"
    eU_ref, eg_ref = nan_aware(O.rel_err)(U, c.U), c.grad_error(grad, O.rel_err)
    print(f"{name}: U vs reference {eU_ref:.2e}, grad vs reference {eg_ref:.2e}")
    assert eU_ref < TOL, f"U vs reference: {eU_ref:.3e}"
    assert eg_ref < TOL, f"grad vs reference: {eg_ref:.3e}"


def test_knn_lists_ordered_and_self_first():
    c = Case("ns_eps1p0_tau0p07_f32")
    g = gpu_knn(c.X, c.k)
    ind = g["knn_idx"].cpu().numpy()
    d2 = g["knn_d2"].cpu().numpy()
    assert (ind[:, 0] == np.arange(ind.shape[0])).all()
    assert (d2[:, 0] == 0).all()
    assert (np.diff(d2[:, 1:], axis=1) >= 0).all()
    exact = np.sum((c.X[:, None, :].astype(np.float64) - c.X[ind].astype(np.float64)) ** 2, 2)
    assert np.max(np.abs(exact - d2)) < 1e-5


def test_graph_symmetric_sorted_and_weights():
    from tests import rows_ref as R
    c = Case("ns_epsauto_tau0p07_f32")
    g = gpu_knn(c.X, c.k, "auto")
    rp = g["row_ptr"].cpu().numpy()
    col = g["col"].cpu().numpy()
    w = g["w"].cpu().numpy()
    n = c.X.shape[0]
    rows = np.repeat(np.arange(n), np.diff(rp))
    for i in range(n):                                   # every row's order
        seg = col[rp[i]:rp[i + 1]]
        assert (np.diff(seg) > 0).all()
    import scipy.sparse as sp
    W = sp.csr_matrix((w, col, rp), shape=(n, n))
    assert abs(W - W.T).max() == 0                       # the two directions are bitwise equal
    ind = g["knn_idx"].cpu().numpy()
    d2k = g["knn_d2"].cpu().numpy()
    ref = O.graph_from_knn(ind, np.sqrt(d2k.astype(np.float64)), "auto")
    assert np.array_equal(ref.rows, rows) and np.array_equal(ref.cols, col)
    # W, d2 and deg against the float64 stage reference on the GPU's own lists and eps, under its
    # relative elementwise bounds (tests/rows_ref.py): a weight of 1e-6 is held to ~1e-12
    st = R.rows_stage(ind, d2k, g["eps"].cpu().numpy(), np.zeros((0, 1), np.float32), 0.0, 0, c.k,
                      R.layout(n, 0, c.k))
    assert np.array_equal(st.row, rows) and np.array_equal(st.col, col)
    assert np.array_equal(g["d2"].cpu().numpy().view(np.uint32), st.d2.view(np.uint32))
    np.testing.assert_allclose(st.W, ref.W, rtol=1e-5)   # the oracle's eps are float64 roots
    assert (np.abs(w.astype(np.float64) - st.W) <= st.wb).all()
    deg = g["deg"].cpu().numpy()
    assert (np.abs(deg.astype(np.float64) - st.deg) <= st.deg_b).all()
    assert np.max(np.abs(ref.W - w)) < 1e-5


def test_deterministic_bitwise():
    c = Case("ns_epsauto_tau0p0_i64")
    U1, g1 = run_layer(c.X, c.Y.astype(np.int64), c.tau, c.eps, c.k, c.gbar)
    U2, g2 = run_layer(c.X, c.Y.astype(np.int64), c.tau, c.eps, c.k, c.gbar)
    assert np.array_equal(U1, U2) and np.array_equal(g1, g2)


def test_cpu_tensor_input_roundtrips_to_cpu():
    c = Case("plumbing_eps1p0_tau0p07_f32")
    X = torch.from_numpy(c.X).requires_grad_(True)
    U = GLL.LaplaceLearningSparseHard.apply(X, torch.from_numpy(c.Y), c.tau, c.eps, c.k)
    assert U.device.type == "cpu" and U.dtype == torch.float64
    U.backward(torch.from_numpy(c.gbar))
    assert X.grad.device.type == "cpu" and X.grad.dtype == torch.float32
    assert O.rel_err(U.detach().numpy(), c.U) < TOL
    assert c.grad_error(X.grad.numpy(), O.rel_err) < TOL


def test_float64_and_noncontiguous_features():
    c = Case("plumbing_epsauto_tau0p07_f32")
    wide = np.zeros((c.X.shape[0], 2 * c.X.shape[1]))
    wide[:, ::2] = c.X
    X = torch.from_numpy(wide).cuda()[:, ::2].requires_grad_(True)   # strided float64 view
    assert not X.is_contiguous()
    U = GLL.LaplaceLearningSparseHard.apply(X, torch.from_numpy(c.Y).cuda(), c.tau, c.eps, c.k)
    U.backward(torch.from_numpy(c.gbar).cuda())
    assert X.grad.dtype == torch.float64
    assert O.rel_err(U.detach().cpu().numpy(), c.U) < TOL
    assert c.grad_error(X.grad.cpu().numpy(), O.rel_err) < TOL


@pytest.mark.parametrize("d", [30, 37, 200, 1100])
def test_scalar_and_wide_feature_paths(d):
    from graphlearninglayer_amd.synth import one_hot, seeded_gbar, synth
    X, lab = synth(60, 140, d, r=1.0, seed=5)
    Y = one_hot(lab[:60])
    g = seeded_gbar(140, 10, 7)
    U, grad = run_layer(X, Y, 0.07, "auto", 8, g)
    ind = gpu_knn(X, 8)["knn_idx"].cpu().numpy()
    Uo, st = O.forward(X, Y, 0.07, "auto", 8, knn=(ind, None))
    assert O.rel_err(U, Uo) < TOL
    assert O.rel_err(grad, O.backward(st, g)) < TOL


@pytest.mark.parametrize("n,d,eps", [(777, 333, "auto"), (1024, 512, 1.0), (900, 300, 1.0),
                                     (1025, 512, 1.0)])
def test_split_phase_gram_shapes(n, d, eps):
    """Single graphs with ceil(n/64) <= 16 and 256 < d <= 512 take the split-phase Gram (two
    partial D2 planes, diagonal tiles zeroing plane 1 of an uninitialised workspace): ragged
    tiles (777, 900), the largest split grid (1024 = 16 tiles), a scalar-load feature width (333)
    and a half-empty second phase (300).  n = 1025 is the first shape past the split (17 tiles)."""
    from graphlearninglayer_amd.synth import one_hot, seeded_gbar, synth
    base = n // 5
    X, lab = synth(base, n - base, d, r=1.0, seed=11)
    Y = one_hot(lab[:base])
    g = seeded_gbar(n - base, 10, 3)
    U, grad = run_layer(X, Y, 0.07, eps, 10, g)
    ind = gpu_knn(X, 10, eps)["knn_idx"].cpu().numpy()
    assert O.knn_set_mismatch(X, ind, 10) == []
    Uo, st = O.forward(X, Y, 0.07, eps, 10, knn=(ind, None))
    assert O.rel_err(U, Uo) < TOL
    assert O.rel_err(grad, O.backward(st, g)) < TOL


@pytest.mark.parametrize("n,d,eps", [(1500, 128, 1.0), (777, 37, "auto"), (1984, 125, 1.0),
                                     (130, 128, "auto"), (300, 2, 1.0)])
def test_half_tile_gram_shapes(n, d, eps):
    """Single graphs with d <= 128 and fewer than 512 64-tiles take the 512-thread half tile
    (gram.hip gram_bf3h_kernel): FullySup's shape, a scalar-load ragged shape (777 x 37), the
    largest triangle on this route (31 tiles a side: 496), d = 125 (lanes past d in the last
    feature group), two tiles of which one nearly empty (130) and d = 2 (unit rows on a circle;
    at d = 1 every row is +-1, all ties).  Exact kNN sets against float64 and U / grad_X
    against the oracle."""
    from graphlearninglayer_amd.synth import one_hot, seeded_gbar, synth
    base = n // 5
    X, lab = synth(base, n - base, d, r=1.0, latent=min(16, d), seed=13)
    Y = one_hot(lab[:base])
    g = seeded_gbar(n - base, 10, 5)
    U, grad = run_layer(X, Y, 0.07, eps, 10, g)
    ind = gpu_knn(X, 10, eps)["knn_idx"].cpu().numpy()
    assert O.knn_set_mismatch(X, ind, 10) == []
    Uo, st = O.forward(X, Y, 0.07, eps, 10, knn=(ind, None))
    assert O.rel_err(U, Uo) < TOL
    assert O.rel_err(grad, O.backward(st, g)) < TOL


@pytest.mark.parametrize("k,eps", [(13, 1.0), (14, "auto"), (29, 1.0), (30, "auto"),
                                   (57, 1.0), (57, "auto")])
def test_candidate_capacity_boundaries(k, eps):
    """k at each edge of the select's candidate capacity (select.hip launch_select: the smallest of
    16 / 32 / 64 keeping a re-rank margin >= 4, so 13 | 14 and 29 | 30 switch lists; k = 57 is
    the largest k include/gll.h accepts): exact kNN sets
    and U / grad_X against the oracle, fixed and automatic eps (GLL.py:183, utils.py:574)."""
    from graphlearninglayer_amd.synth import one_hot, seeded_gbar, synth
    X, lab = synth(120, 380, 64, r=1.0, seed=k)
    Y = one_hot(lab[:120])
    g = seeded_gbar(380, 10, k)
    U, grad = run_layer(X, Y, 0.07, eps, k, g)
    ind = gpu_knn(X, k, eps)["knn_idx"].cpu().numpy()
    assert O.knn_set_mismatch(X, ind, k) == []
    Uo, st = O.forward(X, Y, 0.07, eps, k, knn=(ind, None))
    assert O.rel_err(U, Uo) < TOL
    assert O.rel_err(grad, O.backward(st, g)) < TOL


@pytest.mark.parametrize("n,base,k", [(12, 3, 10), (8, 2, 10), (5, 1, 2), (70, 64, 10),
                                      (66, 1, 10)])
@pytest.mark.parametrize("eps", [1.0, "auto"])
def test_tiny_graphs(n, base, k, eps):
    """Graphs of a handful of points: k clipped to n (every point a neighbour: 8 points, k =
    10), k = 2 (one neighbour, disconnected pieces held by tau), six unlabeled rows among 64
    labeled, one labeled row among 66 -- U and grad_X against the oracle (GLL.py:183,205)."""
    from graphlearninglayer_amd.synth import one_hot, seeded_gbar, synth
    X, lab = synth(base, n - base, 16, r=1.0, seed=n)
    Y = one_hot(lab[:base])
    g = seeded_gbar(n - base, 10, 3)
    kk = min(k, n)
    U, grad = run_layer(X, Y, 0.07, eps, k, g)
    ind = gpu_knn(X, kk, eps)["knn_idx"].cpu().numpy()
    assert O.knn_set_mismatch(X, ind, kk) == []
    Uo, st = O.forward(X, Y, 0.07, eps, kk, knn=(ind, None))
    assert O.rel_err(U, Uo) < TOL
    assert O.rel_err(grad, O.backward(st, g)) < TOL


@pytest.mark.parametrize("n,base,d,C,k", [(40, 39, 16, 10, 10), (60, 20, 1, 10, 10),
                                          (60, 20, 3, 10, 10), (60, 20, 16, 1, 10),
                                          (300, 100, 2, 1, 7)])
@pytest.mark.parametrize("eps", [1.0, "auto"])
def test_odd_shapes(n, base, d, C, k, eps):
    """Shapes at the edge of the ABI: one unlabeled row, one or three features (ties in the
    distances), a single class (label_matrix of shape [base, 1], GLL.py:32) -- U and grad_X
    against the oracle on the GPU's own kNN lists."""
    rng = np.random.default_rng(n + d + C)
    X = rng.standard_normal((n, d)).astype(np.float32)
    lab = rng.integers(0, C, base)
    Y = np.eye(C, dtype=np.float32)[lab]
    g = rng.standard_normal((n - base, C))
    U, grad = run_layer(X, Y, 0.07, eps, k, g)
    ind = gpu_knn(X, k, eps)["knn_idx"].cpu().numpy().astype(np.int64)
    assert O.knn_set_mismatch(X, ind, k) == []
    Uo, st = O.forward(X, Y, 0.07, eps, k, knn=(ind, None))
    assert U.shape == (n - base, C)
    assert O.rel_err(U, Uo) < TOL
    assert O.rel_err(grad, O.backward(st, g)) < TOL


@pytest.mark.parametrize("d", [1028, 2048, 4096])
def test_wide_features_up_to_the_limit(d):
    """Features past the fused backward's 1,024 and up to include/gll.h's 4,096: the Gram's
    feature phases, the exact re-rank over d-float rows and the feature gradient past the
    register-row form, against the oracle."""
    rng = np.random.default_rng(d)
    n, base, k = 300, 100, 10
    X = rng.standard_normal((n, d)).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    lab = rng.integers(0, 10, base)
    Y = np.eye(10, dtype=np.float32)[lab]
    g = rng.standard_normal((n - base, 10))
    U, grad = run_layer(X, Y, 0.07, 1.0, k, g)
    ind = gpu_knn(X, k, 1.0)["knn_idx"].cpu().numpy().astype(np.int64)
    assert O.knn_set_mismatch(X, ind, k) == []
    Uo, st = O.forward(X, Y, 0.07, 1.0, k, knn=(ind, None))
    assert O.rel_err(U, Uo) < TOL
    assert O.rel_err(grad, O.backward(st, g)) < TOL


@pytest.mark.parametrize("eps", [1.0, "auto"])
def test_batch_of_one_equals_the_single_graph(eps):
    """X of shape [1, n, d] through the batched entry against X [n, d] through the single-graph
    one: the same predictions and feature gradient (1e-5: the batched launch may run another CG
    geometry), U of shape [1, m, C]."""
    from graphlearninglayer_amd.synth import CONFIGS, one_hot, seeded_gbar, synth
    c = CONFIGS["ns"]
    X, lab = synth(c["base"], c["batch"], c["d"], r=c["r"], seed=31)
    Y = one_hot(lab[: c["base"]])
    g = seeded_gbar(c["batch"], 10, 37)
    U1, g1 = run_layer(X, Y, 0.07, eps, c["k"], g)
    Xb = torch.from_numpy(X[None]).cuda().requires_grad_(True)
    Ub = GLL.LaplaceLearningSparseHard.apply(Xb, torch.from_numpy(Y[None]).cuda(), 0.07, eps,
                                             c["k"])
    assert tuple(Ub.shape) == (1,) + U1.shape
    Ub.backward(torch.from_numpy(g[None]).cuda())
    assert O.rel_err(Ub[0].detach().cpu().numpy(), U1) <= 1e-5
    assert O.rel_err(Xb.grad[0].cpu().numpy(), g1) <= 1e-5


@pytest.mark.parametrize("n,base,k", [(8, 2, 10), (12, 3, 10), (66, 1, 57)])
def test_batched_tiny_graphs(n, base, k):
    """The batched entry on three graphs of a handful of points (k clipped to n; k = 57 on 66
    points): every graph's U and grad_X against the oracle on the GPU's own kNN lists, auto
    eps (GLL.py:14-177)."""
    from graphlearninglayer_amd.synth import one_hot, seeded_gbar, synth
    B, kk = 3, min(k, n)
    Xs, Ys = [], []
    for g in range(B):
        X, lab = synth(base, n - base, 16, r=1.0, seed=40 + g)
        Xs.append(X)
        Ys.append(one_hot(lab[:base]))
    Xs, Ys = np.stack(Xs), np.stack(Ys)
    G = np.stack([seeded_gbar(n - base, 10, 500 + g) for g in range(B)])
    Xb = torch.from_numpy(Xs).cuda().requires_grad_(True)
    Ub = GLL.LaplaceLearningSparseHard.apply(Xb, torch.from_numpy(Ys).cuda(), 0.07, "auto", k)
    Ub.backward(torch.from_numpy(G).cuda())
    for g in range(B):
        ind = gpu_knn(Xs[g], kk, "auto")["knn_idx"].cpu().numpy().astype(np.int64)
        assert O.knn_set_mismatch(Xs[g], ind, kk) == []
        Uo, st = O.forward(Xs[g], Ys[g], tau=0.07, epsilon="auto", K=kk, knn=(ind, None))
        assert O.rel_err(Ub[g].detach().cpu().numpy(), Uo) <= TOL
        assert O.rel_err(Xb.grad[g].cpu().numpy(), O.backward(st, G[g])) <= TOL


def test_hub_row_longer_than_lds_chunk():
    """One point is a neighbour of everybody: its CSR row exceeds the 256-entry chunk."""
    rng = np.random.default_rng(0)
    n, d = 700, 64
    X = rng.standard_normal((n, d)).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)   # pairwise distances ~ sqrt(2)
    X[0] = 0.0    # centre: distance 1 to every unit vector -> in every kNN list
    lab = np.arange(n) % 10
    base = 100
    Y = np.eye(10, dtype=np.float32)[lab[:base]]
    gb = rng.standard_normal((n - base, 10))
    U, grad = run_layer(X, Y, 0.07, 1.0, 6, gb)
    g = gpu_knn(X, 6, 1.0)
    rp = g["row_ptr"].cpu().numpy()
    ind = g["knn_idx"].cpu().numpy()
    Uo, st = O.forward(X, Y, 0.07, 1.0, 6, knn=(ind, None))
    assert O.rel_err(U, Uo) < TOL
    assert O.rel_err(grad, O.backward(st, gb)) < TOL
    assert np.diff(rp).max() > 256


def test_hub_row_overflow_within_lds_staging():
    """An unlabeled hub whose reverse list passes its capacity (8(K-1)+8 = 48 at k = 6,
    gll_internal.h Layout::RCAP) while the row still fits the 256-entry LDS staging: its extra
    reverse entries come from the global overflow list (rows.hip build_row, batched scan), it
    stages more than 64 entries (the rhs loads labels past the prefetched 64, 32 per step) and
    more than 32 of them are labeled."""
    rng = np.random.default_rng(3)
    n, d, base, k = 700, 64, 100, 6
    X = rng.standard_normal((n, d))
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    hub = 300
    v = X[hub].copy()
    members = np.r_[10:100, 301:341]   # 90 labeled and 40 unlabeled rows around the hub
    X[members] = v + 0.15 * rng.standard_normal((len(members), d)) / np.sqrt(d)
    X = X.astype(np.float32)
    lab = np.arange(n) % 10
    Y = np.eye(10, dtype=np.float32)[lab[:base]]
    gb = rng.standard_normal((n - base, 10))
    U, grad = run_layer(X, Y, 0.07, 1.0, k, gb)
    ind = gpu_knn(X, k, 1.0)["knn_idx"].cpu().numpy()
    rc = int((ind[:, 1:] == hub).sum())
    assert 8 * (k - 1) + 8 < rc <= 250, rc
    assert O.knn_set_mismatch(X, ind, k) == []
    Uo, st = O.forward(X, Y, 0.07, 1.0, k, knn=(ind, None))
    assert O.rel_err(U, Uo) < TOL
    assert O.rel_err(grad, O.backward(st, gb)) < TOL


@pytest.mark.parametrize("k", [10, 30])
def test_duplicate_points_and_ties(k):
    """Clusters of exact duplicates: more tied candidates than the re-rank margin (the threshold
    scan takes every tie at its threshold; more than 64 ties fall back to select_fallback's
    full-row bisection), and zero-distance pairs drop out of the graph as sparse.find drops them
    (GLL.py:198).  k = 30: the 64-slot candidate list."""
    rng = np.random.default_rng(5)
    n, d, base = 600, 40, 100
    X = rng.standard_normal((n, d)).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    X[200:230] = X[199]     # 31 copies: ties beyond K - 1 + margin
    X[400:480] = X[399]     # 81 copies: more than 64 tied candidates
    X[5:8] = X[4]           # duplicates among the labeled rows
    lab = np.arange(n) % 10
    Y = np.eye(10, dtype=np.float32)[lab[:base]]
    gb = rng.standard_normal((n - base, 10))
    U, grad = run_layer(X, Y, 0.07, 1.0, k, gb)
    from graphlearninglayer_amd import _lib
    g = gpu_knn(X, k, 1.0)
    ind = g["knn_idx"].cpu().numpy()
    assert int(g["status"][_lib.ST_KNN_MERGE].item()) > 0   # > 64 ties: the fallback ran
    assert O.knn_set_mismatch(X, ind, k) == []
    Uo, st = O.forward(X, Y, 0.07, 1.0, k, knn=(ind, None))
    assert O.rel_err(U, Uo) < TOL
    assert O.rel_err(grad, O.backward(st, gb)) < TOL


def test_no_labeled_rows_gives_zero_predictions():
    c = Case("plumbing_eps1p0_tau0p07_f32")
    X = torch.from_numpy(c.X).cuda().requires_grad_(True)
    U = GLL.LaplaceLearningSparseHard.apply(X, torch.zeros(0, 10).cuda(), 0.07, 1.0, 5)
    assert U.shape == (128, 10) and torch.count_nonzero(U) == 0


def test_status_sink_raises_reference_warning():
    """Duplicate points make eps_i = 0 in auto mode: the reference warns (GLL.py:240-241)."""
    c = Case("plumbing_epsauto_tau0p07_f32")
    GLL.check_status()
    X = c.X.copy()
    X[70:80] = X[70]          # ten identical rows: their 4th neighbour is at distance 0
    Xt = torch.from_numpy(X).cuda()
    GLL.LaplaceLearningSparseHard.apply(Xt, torch.from_numpy(c.Y).cuda(), 0.07, "auto", 5)
    with pytest.warns(UserWarning, match="very close to zero"):
        GLL.check_status()
    U = GLL.LaplaceLearningSparseHard.apply(Xt, torch.from_numpy(c.Y).cuda(), 0.07, 1.0, 5)
    assert torch.isfinite(U).all()


def test_negative_epsilon_is_its_absolute_value():
    """GLL.py:233-234 use a fixed epsilon only as eps_i * eps_j, so eps < 0 gives the weights of
    |eps| (plus the reference's 'very close to zero' style warning here): the native apply maps it
    to |eps| with a warning, U and grad_X bitwise those of |eps| and within 1e-4 of the oracle."""
    c = Case("ns_eps1p0_tau0p07_f32")
    gb = np.random.default_rng(4).standard_normal(c.U.shape)
    outs = []
    for e in (-1.0, 1.0):
        X = torch.from_numpy(c.X).cuda().requires_grad_(True)
        if e < 0:
            with pytest.warns(UserWarning):
                U = GLL.LaplaceLearningSparseHard.apply(X, torch.from_numpy(c.Y).cuda(), 0.07, e,
                                                        c.k)
        else:
            U = GLL.LaplaceLearningSparseHard.apply(X, torch.from_numpy(c.Y).cuda(), 0.07, e, c.k)
        U.backward(torch.from_numpy(gb).cuda())
        outs.append((U.detach().cpu().numpy(), X.grad.cpu().numpy()))
    np.testing.assert_array_equal(outs[0][0], outs[1][0])
    np.testing.assert_array_equal(outs[0][1], outs[1][1])
    assert O.rel_err(outs[0][0], c.U) <= TOL


def test_knn_sym_dist_mirror_matches_oracle():
    c = Case("ns_epsauto_tau0p07_f32")
    W, V, mod_V, C, knn_ind = GLL.knn_sym_dist(c.X, k=c.k, epsilon="auto")
    assert np.array_equal(knn_ind, c.knn)
    ref = O.graph_from_knn(*O.knn_exact(c.X, c.k), "auto")
    Wr = ref.csr(ref.W)
    assert abs(W - Wr).max() < 1e-5 * abs(Wr).max()
    assert C.shape == (c.X.shape[0],) * 2 and C.nnz == c.X.shape[0]


def test_stable_conjgrad_mirror_reaches_float64_tolerance():
    import scipy.sparse as sp
    rng = np.random.default_rng(1)
    m = 300
    M = sp.random(m, m, density=0.02, random_state=2)
    M = M + M.T
    M = sp.diags(np.asarray(abs(M).sum(1)).ravel() + 0.5) - M
    b = rng.standard_normal((m, 3))
    x = GLL.stable_conjgrad(M, b, tol=1e-10)
    assert np.max(np.linalg.norm(b - M @ x, axis=0)) <= 1e-10


def test_stress_shape_graph_parity():
    """base=4096 batch=4096 d=1024 k=30 eps=auto (BASELINE config 5), graph-level parity."""
    from graphlearninglayer_amd.synth import CONFIGS, one_hot, seeded_gbar, synth
    s = CONFIGS["stress"]
    X, lab = synth(s["base"], s["batch"], s["d"], r=s["r"], seed=0)
    Y = one_hot(lab[: s["base"]])
    gb = seeded_gbar(s["batch"], 10)
    U, grad = run_layer(X, Y, 0.07, "auto", s["k"], gb)
    ind = gpu_knn(X, s["k"])["knn_idx"].cpu().numpy()
    rows = np.arange(0, X.shape[0], 128)
    # kNN: exact float64 distances of sampled rows
    X64 = X.astype(np.float64)
    for i in rows:
        d2 = np.sum((X64 - X64[i]) ** 2, axis=1)
        d2[i] = -1
        ref = np.argsort(d2, kind="stable")[: s["k"]]
        if set(ref) != set(ind[i]):
            kth = np.sort(d2)[s["k"] - 1]
            extra = list(set(ind[i]) - set(ref))
            assert np.all(np.abs(d2[extra] - kth) <= 1e-5 * kth)
    Uo, st = O.forward(X, Y, 0.07, "auto", s["k"], knn=(ind, None))
    assert O.rel_err(U, Uo) < TOL
    assert O.rel_err(grad, O.backward(st, gb)) < TOL


def test_cpp_node_and_python_function_agree_bitwise():
    """The C++ autograd node (what .apply runs) and the ctypes Python Function are the
    same kernels: identical outputs and gradients."""
    assert GLL._ext() is not None
    c = Case("ns_epsauto_tau0p07_f32")
    X = torch.from_numpy(c.X).cuda().requires_grad_(True)
    Y = torch.from_numpy(c.Y).cuda()
    g = torch.from_numpy(c.gbar).cuda()
    U1 = GLL.LaplaceLearningSparseHard.apply(X, Y, c.tau, c.eps, c.k)
    (g1,) = torch.autograd.grad(U1, X, g)
    U2 = GLL.LaplaceLearningSparseHard.apply_python(X, Y, c.tau, c.eps, c.k)
    (g2,) = torch.autograd.grad(U2, X, g)
    assert U1.grad_fn is not None and U2.grad_fn is not None
    assert torch.equal(U1, U2) and torch.equal(g1, g2)


def test_output_does_not_alias_saved_state():
    """Callers edit the output in place (adversarial.py:691); backward must not change."""
    c = Case("plumbing_eps1p0_tau0p07_f32")
    X = torch.from_numpy(c.X).cuda().requires_grad_(True)
    Y = torch.from_numpy(c.Y).cuda()
    g = torch.from_numpy(c.gbar).cuda()
    U = GLL.LaplaceLearningSparseHard.apply(X, Y, c.tau, c.eps, c.k)
    (ref,) = torch.autograd.grad(U, X, g, retain_graph=True)
    with torch.no_grad():
        U.mul_(0.5).add_(1.0)
    (again,) = torch.autograd.grad(U, X, g)
    assert torch.equal(ref, again)


@pytest.mark.parametrize("cfg,eps,ydt,exact", [("plumbing", "auto", "i64", True),
                                               ("ns", 1.0, "f32", False),
                                               ("fullysup", 1.0, "f32", False)])
def test_batched_graphs_equal_single_calls_bitwise(cfg, eps, ydt, exact):
    """B graphs in one launch per kernel give B single calls.  Bitwise at
    plumbing; at NS and FullySup the batched launch takes other kernel variants than a single
    graph (the unfused backward instead of cg_grad_fused_kernel, the batched select and
    gradient forms), so there the bar is 1e-5 relative (10x below the 1e-4 parity bar)."""
    from graphlearninglayer_amd.synth import seeded_gbar
    B = 5
    Xs, Ys, c = synth_batch(cfg, B, seed0=11)
    if ydt == "i64":
        Ys = Ys.astype(np.int64)
    G = np.stack([seeded_gbar(c["batch"], 10, 100 + g) for g in range(B)])
    Xb = torch.from_numpy(Xs).cuda().requires_grad_(True)
    Ub = GLL.LaplaceLearningSparseHard.apply(Xb, torch.from_numpy(Ys).cuda(), 0.07, eps, c["k"])
    assert Ub.shape == (B, c["batch"], 10) and Ub.dtype == torch.float64
    Ub.backward(torch.from_numpy(G).cuda())
    for g in range(B):
        U1, gx1 = run_layer(Xs[g], Ys[g], 0.07, eps, c["k"], G[g])
        if exact:
            np.testing.assert_array_equal(Ub[g].detach().cpu().numpy(), U1)
            np.testing.assert_array_equal(Xb.grad[g].cpu().numpy(), gx1)
        else:
            assert O.rel_err(Ub[g].detach().cpu().numpy(), U1) <= 1e-5
            assert O.rel_err(Xb.grad[g].cpu().numpy(), gx1) <= 1e-5


@pytest.mark.parametrize("cfg,B", [("ns", 3), ("stress", 2)])
def test_batched_auto_eps_matches_oracle(cfg, B):
    """The batched entry with auto epsilon (the inline-copy callers' default) at NS and at the
    stress shape: every graph's U and grad_X against the float64 oracle on the GPU's own kNN
    lists, forward and adjoint (GLL.py:14-177)."""
    from graphlearninglayer_amd.synth import seeded_gbar
    Xs, Ys, c = synth_batch(cfg, B, seed0=21)
    G = np.stack([seeded_gbar(c["batch"], 10, 300 + g) for g in range(B)])
    Xb = torch.from_numpy(Xs).cuda().requires_grad_(True)
    Ub = GLL.LaplaceLearningSparseHard.apply(Xb, torch.from_numpy(Ys).cuda(), 0.07, "auto", c["k"])
    Ub.backward(torch.from_numpy(G).cuda())
    for g in range(B):
        ind = gpu_knn(Xs[g], c["k"], "auto")["knn_idx"].cpu().numpy().astype(np.int64)
        Uo, st = O.forward(Xs[g], Ys[g], tau=0.07, epsilon="auto", K=c["k"], knn=(ind, None))
        assert O.rel_err(Ub[g].detach().cpu().numpy(), Uo) <= TOL
        assert O.rel_err(Xb.grad[g].cpu().numpy(), O.backward(st, G[g])) <= TOL


def test_batched_duplicates_match_single_calls():
    """Batched selection (the occupancy form: x_i staged in LDS, 8 waves per SIMD) on graphs with
    > 64 tied candidates, where the full-row fallback runs: each graph's kNN, U and grad_X agree
    with its single call (the latency form)."""
    rng = np.random.default_rng(8)
    n, d, base, k, B = 600, 40, 100, 10, 2
    Xs = rng.standard_normal((B, n, d)).astype(np.float32)
    Xs /= np.linalg.norm(Xs, axis=2, keepdims=True)
    Xs[:, 400:480] = Xs[:, 399:400]
    Xs[1, 200:230] = Xs[1, 199]
    Y = np.eye(10, dtype=np.float32)[np.arange(base) % 10]
    G = rng.standard_normal((B, n - base, 10))
    Xb = torch.from_numpy(Xs).cuda().requires_grad_(True)
    Ub = GLL.LaplaceLearningSparseHard.apply(Xb, torch.from_numpy(Y).cuda(), 0.07, 1.0, k)
    Ub.backward(torch.from_numpy(G).cuda())
    for g in range(B):
        U1, gx1 = run_layer(Xs[g], Y, 0.07, 1.0, k, G[g])
        assert O.rel_err(Ub[g].detach().cpu().numpy(), U1) <= 1e-5
        assert O.rel_err(Xb.grad[g].cpu().numpy(), gx1) <= 1e-5


def test_batched_shared_labels_python_and_cpp_paths_agree():
    B = 3
    Xs, Ys, c = synth_batch("plumbing", B, seed0=3)
    Y = torch.from_numpy(Ys[0]).cuda()            # one label matrix shared by the batch
    outs = []
    for fn in (GLL.LaplaceLearningSparseHard.apply, GLL.LaplaceLearningSparseHard.apply_python):
        Xb = torch.from_numpy(Xs).cuda().requires_grad_(True)
        U = fn(Xb, Y, 0.0, 1.0, c["k"])
        (gx,) = torch.autograd.grad(U.sum(), Xb)
        outs.append((U.detach().cpu().numpy(), gx.cpu().numpy()))
    np.testing.assert_array_equal(outs[0][0], outs[1][0])
    np.testing.assert_array_equal(outs[0][1], outs[1][1])
    # every graph against the float64 oracle on the GPU's own kNN lists
    for g in range(B):
        ind = gpu_knn(Xs[g], c["k"], 1.0)["knn_idx"].cpu().numpy().astype(np.int64)
        Uo, _ = O.forward(Xs[g], Ys[0], tau=0.0, epsilon=1.0, K=c["k"], knn=(ind, None))
        assert O.rel_err(outs[0][0][g], Uo) <= TOL


@pytest.mark.parametrize("offset", [100.0, 1000.0])
def test_translated_features_exact_knn(offset):
    """NS features plus a common offset of norm `offset`: |x|^2 >> d^2, the case where an
    uncentred split-bf16 Gram nominates wrong candidates.  The Gram works on rows centred on
    row 0 (distance-invariant), the certificate holds, and the kNN sets, U and grad_X match
    the float64 oracle; no row needs the rescan."""
    from graphlearninglayer_amd import _lib
    c = Case("ns_eps1p0_tau0p07_f32")
    rng = np.random.default_rng(17)
    v = rng.standard_normal(c.X.shape[1])
    Xs = (c.X.astype(np.float64) + offset * v / np.linalg.norm(v)).astype(np.float32)
    g = gpu_knn(Xs, c.k, c.eps)
    ind = g["knn_idx"].cpu().numpy()
    assert exact_knn_rows(Xs, ind, c.k) == []
    assert int(g["status"][_lib.ST_KNN_RESCAN].item()) == 0
    U, grad = run_layer(Xs, c.Y, c.tau, c.eps, c.k, c.gbar)
    Uo, st = O.forward(Xs, c.Y, c.tau, c.eps, c.k, knn=(ind.astype(np.int64), None))
    assert O.rel_err(U, Uo) < TOL
    assert O.rel_err(grad, O.backward(st, c.gbar)) < TOL


def test_far_centre_row_takes_exact_rescan():
    """Row 0 (the Gram's centre) far from every other row: the split-bf16 error bound then
    exceeds the neighbour gaps, the certificate fails in (nearly) every row and the exact
    rescan under the bound runs -- the kNN is still exact and the solve still matches."""
    from graphlearninglayer_amd import _lib
    from graphlearninglayer_amd.synth import one_hot, seeded_gbar, synth
    X, lab = synth(100, 400, 64, r=1.0, seed=23)
    X = X.astype(np.float32)
    X[0] = 300.0 / np.sqrt(64)      # |x_0 - x_i| ~ 300
    k = 10
    g = gpu_knn(X, k, "auto")
    ind = g["knn_idx"].cpu().numpy()
    assert int(g["status"][_lib.ST_KNN_RESCAN].item()) > 100
    assert exact_knn_rows(X, ind, k) == []
    Y = one_hot(lab[:100])
    gb = seeded_gbar(400, 10, 5)
    U, grad = run_layer(X, Y, 0.07, "auto", k, gb)
    Uo, st = O.forward(X, Y, 0.07, "auto", k, knn=(ind.astype(np.int64), None))
    assert O.rel_err(U, Uo) < TOL
    assert O.rel_err(grad, O.backward(st, gb)) < TOL


@pytest.mark.parametrize("cfg", ["plumbing", "ns", "fullysup"])
def test_knn_exact_against_float64(cfg):
    """kNN sets equal the exact float64 sets (no near-tie allowance) at the bench configs."""
    from graphlearninglayer_amd.synth import CONFIGS, synth
    c = CONFIGS[cfg]
    X, _ = synth(c["base"], c["batch"], c["d"], r=c["r"], seed=3)
    ind = gpu_knn(X, c["k"], 1.0)["knn_idx"].cpu().numpy()
    assert exact_knn_rows(X, ind, c["k"]) == []


@pytest.mark.parametrize("d,eps", [(64, 1.0), (256, "auto"), (100, "auto")])
def test_knn_row_panels_match_whole_matrix(d, eps):
    """kNN in row panels (GLL_FLAG_KNN_PANEL: 1,024-row panels of rectangular Gram tiles, each
    panel selected before the next is computed -- the path graphs past 32 GiB of n x n distances
    take) against the whole n x n matrix: the Gram only nominates candidates and the select is
    exact, so the kNN lists, distances, eps, the CSR and then U and grad_X agree bitwise (ragged
    last panel; d not a multiple of 64, and of 4: the scalar loads)."""
    from graphlearninglayer_amd import _lib
    from graphlearninglayer_amd.synth import one_hot, seeded_gbar, synth
    base, m, k = 900, 3300, 10
    X, lab = synth(base, m, d, r=1.0, seed=31)
    Xd = torch.from_numpy(X).cuda()
    gw = GLL.device_graph(Xd, k, eps)
    gp = GLL.device_graph(Xd, k, eps, flags=_lib.FLAG_KNN_PANEL)
    for key in ("knn_idx", "knn_d2", "eps", "row_ptr", "col", "w", "deg"):
        assert torch.equal(gw[key], gp[key]), key
    Y = one_hot(lab[:base])
    g = seeded_gbar(m, 10, 77)
    Uw, gxw = fwd_bwd_c_abi(X, Y, k, 0.07, eps, g)
    Up, gxp = fwd_bwd_c_abi(X, Y, k, 0.07, eps, g, flags=_lib.FLAG_KNN_PANEL)
    np.testing.assert_array_equal(Up, Uw)
    np.testing.assert_array_equal(gxp, gxw)


def test_knn_row_panels_automatic_past_the_n2_buffer():
    """A graph whose n x n distances (40 GB at n = 100,000) pass the 32 GiB line: the workspace
    holds an 8 GiB row panel instead (gll_workspace_bytes far below n^2 x 4), and the kNN of
    sampled rows is the exact float64 kNN, as is eps for auto epsilon."""
    import ctypes as ct
    from graphlearninglayer_amd import _lib
    n, d, k = 100_000, 64, 10
    rng = np.random.default_rng(5)
    centres = rng.standard_normal((50, d))
    X = (centres[rng.integers(0, 50, n)] + 0.6 * rng.standard_normal((n, d))).astype(np.float32)
    prob = GLL.make_problem(n, d, 0, 1, k, 0.0, "auto")
    # the raw call: the size itself is the subject, and no 100,000-row Run is wanted for it
    nbytes = _lib.lib().gll_workspace_bytes(ct.byref(prob))
    assert nbytes < n * n * 4 // 4, nbytes
    g = GLL.device_graph(torch.from_numpy(X).cuda(), k, "auto")
    ind = g["knn_idx"].cpu().numpy()
    eps = g["eps"].cpu().numpy()
    X64 = X.astype(np.float64)
    for i in rng.choice(n, 48, replace=False):
        d2 = np.sum((X64 - X64[i]) ** 2, axis=1)
        d2[i] = np.inf
        order = np.argsort(d2, kind="stable")[: k - 1]
        got = ind[i, 1:]
        assert ind[i, 0] == i
        if set(order.tolist()) != set(got.tolist()):
            # excused only at exact ties of the boundary distance
            assert abs(np.max(d2[got]) - d2[order[-1]]) <= 1e-12 * d2[order[-1]], i
        assert abs(eps[i] - np.sqrt(d2[order[-1]])) <= 1e-6 * np.sqrt(d2[order[-1]]), i


@pytest.mark.parametrize("cfg,B,scale", [("ns", 8, 1.0), ("ns", 8, 1e3), ("ns", 8, 1e-3),
                                           ("fullysup", 8, 1.0), ("stress", 2, 1.0)])
def test_fp16_distance_storage_matches_fp32(cfg, B, scale):
    """Batches on the pre-split Gram route store D2 as fp16 x 2^e (gram.hip dput): every GEMM tile
    recomputes e itself from the graph's row norms (a max-reduction over nrm, |x - x_0|^2) and
    stores it as a plain word -- the same value from every tile, nothing carried over from an
    earlier call -- so features scaled by 1e3 or 1e-3 stay in range, and a workspace reused by a
    batch of another scale (the second call below) leaks nothing in.  The select widens its error
    bounds by the fp16 rounding.  D2 only nominates candidates and the select is exact, so U and
    grad_X are bitwise those of fp32 storage (GLL_FLAG_D2_F32), whose batched results the other
    batched tests hold to single calls and the oracle."""
    from graphlearninglayer_amd import _lib
    from graphlearninglayer_amd.synth import seeded_gbar
    Xs, Ys, c = synth_batch(cfg, B, seed0=61)
    Xs = (Xs * scale).astype(np.float32)
    G = np.stack([seeded_gbar(c["batch"], 10, 700 + g) for g in range(B)])
    eps = "auto"
    Uh, gh = fwd_bwd_batched_c_abi(Xs, Ys, c["k"], 0.07, eps, G)[:2]
    Uf, gf = fwd_bwd_batched_c_abi(Xs, Ys, c["k"], 0.07, eps, G, flags=_lib.FLAG_D2_F32)[:2]
    np.testing.assert_array_equal(Uh, Uf)
    np.testing.assert_array_equal(gh, gf)
    if scale != 1.0:   # one workspace, first a batch at 1/scale of these features, then these
        ws = fwd_bwd_batched_c_abi((Xs / scale).astype(np.float32), Ys, c["k"], 0.07, eps, G)[2].ws
        Ur, gr = fwd_bwd_batched_c_abi(Xs, Ys, c["k"], 0.07, eps, G, ws=ws)[:2]
        np.testing.assert_array_equal(Ur, Uf)
        np.testing.assert_array_equal(gr, gf)


def test_batched_graphs_stay_independent_with_non_finite_and_large_features():
    """Per-graph state of a batched launch (workspace block, fp16 D2 scale, CG columns): one
    graph with a NaN feature row and another scaled by 1e4 leave the other graphs' U and grad_X
    bitwise what they are in a batch without them, and the call returns (no hang, no fault)."""
    from graphlearninglayer_amd.synth import seeded_gbar
    B = 8
    Xs, Ys, c = synth_batch("ns", B, seed0=81)
    G = np.stack([seeded_gbar(c["batch"], 10, 900 + g) for g in range(B)])
    U0, g0 = fwd_bwd_batched_c_abi(Xs, Ys, c["k"], 0.07, 1.0, G)[:2]
    Xb = Xs.copy()
    Xb[2, 700, :] = np.nan
    Xb[5] *= 1e4
    U1, g1 = fwd_bwd_batched_c_abi(Xb, Ys, c["k"], 0.07, 1.0, G)[:2]
    for g in (0, 1, 3, 4, 6, 7):
        np.testing.assert_array_equal(U1[g], U0[g])
        np.testing.assert_array_equal(g1[g], g0[g])
    assert np.isfinite(U1[5]).all()


def test_batched_bench_route_matches_oracle_every_graph():
    """The exact route bench.py's `batched` line times (B = 64 NS graphs, fixed eps, tau 0.07):
    B x C = 640 column solves > 256 CUs, so the per-column CG runs 256 threads x 2 rows with the
    single-reduction recurrence (solve.hip cg_dispatch); the distances are stored fp16 x 2^e and
    the Gram takes the pre-split route (knn_route.h d2_half, gram_tile256).  Every graph's U and
    grad_X against the float64 oracle at the 1e-4 bar (GLL.py:53,93,146-159), the oracle fed each
    graph's own GPU kNN lists."""
    from graphlearninglayer_amd.synth import seeded_gbar
    B = 64
    Xs, Ys, c = synth_batch("ns", B, seed0=300)
    G = np.stack([seeded_gbar(c["batch"], 10, 700 + g) for g in range(B)])
    U, gx, run = fwd_bwd_batched_c_abi(Xs, Ys, c["k"], 0.07, 1.0, G)
    assert np.isfinite(U).all() and np.isfinite(gx).all()
    # the oracle is fed the kNN lists the batched launch wrote (each graph's workspace block),
    # and those lists are the exact float64 kNN
    inds = batched_knn_lists(run)
    worst_u = worst_g = 0.0
    for g in range(B):
        ind = inds[g]
        assert exact_knn_rows(Xs[g], ind, c["k"]) == [], g
        Uo, st = O.forward(Xs[g], Ys[g], tau=0.07, epsilon=1.0, K=c["k"], knn=(ind, None))
        worst_u = max(worst_u, O.rel_err(U[g], Uo))
        worst_g = max(worst_g, O.rel_err(gx[g], O.backward(st, G[g])))
    assert worst_u <= TOL and worst_g <= TOL, (worst_u, worst_g)


@pytest.mark.parametrize("d", [100, 37, 256])
def test_presplit_gram_matches_inline_split(d):
    """The 128-tile Gram on pre-split hi/lo planes with LDS-DMA staging (gram.hip gram_split_kernel
    + gram_pk_kernel, the default for batches and for large graphs with d > 128) against the
    inline-split kernel (GLL_FLAG_GRAM_INLINE): both only nominate candidates, so the kNN (exact
    against float64) and every output agree bitwise; ragged n (not a multiple of 128) and d (not
    of 64, and not of 4: the scalar load path).  For d <= 128 the pre-split path runs batched."""
    from graphlearninglayer_amd import _lib
    from graphlearninglayer_amd.synth import one_hot, synth
    base, m, k = 1000, 3037, 10   # 32 128-row tiles a side: 528 tiles, the 128-tile path
    X, lab = synth(base, m, d, r=1.0, seed=8)
    Y = one_hot(lab[:base])
    Ui, iti, nci = forward_c_abi(X, Y, k, 0.07, "auto", flags=_lib.FLAG_GRAM_INLINE)
    assert nci == 0
    ind = gpu_knn(X, k, "auto")["knn_idx"].cpu().numpy()
    assert exact_knn_rows(X, ind, k) == []
    if d > 128:
        Up, itp, ncp = forward_c_abi(X, Y, k, 0.07, "auto")
        assert ncp == 0
        np.testing.assert_array_equal(Up, Ui)
        return
    # single graphs with d <= 128 take the inline kernel (gram.hip launch_gram); batches keep the
    # pre-split one: a batch of two (this graph and a second) against the single calls, at the
    # batched-parity bar (the batched launch runs a different CG configuration)
    X2, lab2 = synth(base, m, d, r=1.0, seed=9)
    Xb = torch.from_numpy(np.stack([X, X2])).cuda()
    Yb = torch.from_numpy(np.stack([Y, one_hot(lab2[:base])])).cuda()
    Ub = GLL.LaplaceLearningSparseHard.apply(Xb, Yb, 0.07, "auto", k).cpu().numpy()
    assert O.rel_err(Ub[0], Ui) <= 1e-5
    U2, _, _ = forward_c_abi(X2, one_hot(lab2[:base]), k, 0.07, "auto")
    assert O.rel_err(Ub[1], U2) <= 1e-5


@pytest.mark.parametrize("cfg,B,n_extra,d", [("ns", 3, 0, None), ("fullysup", 2, 0, None),
                                             ("ns", 2, 37, 100), ("ns", 26, 0, None),
                                             ("ns", 26, 37, 100), ("ns", 64, 0, None)])
def test_gram_256_tiles_match_128_tiles(cfg, B, n_extra, d, monkeypatch):
    """The 256-tile pre-split Gram (gram.hip gram_pk2_kernel, 8 waves) against the 128-tile one
    (gram_pk_kernel) on batches, ragged n and d included: the same k order and epilogue, so U
    and grad_X agree bitwise (the GLL_KNOB_GRAM_TILE test knob forces either).  B = 26 (n 1,000
    and 1,037): 260 256-tiles on a 256-CU device, whose short last round runs as 64-subtiles (the
    launch's tail); B = 64: 640 256-tiles, a third round of 256-tiles."""
    from graphlearninglayer_amd.synth import CONFIGS, one_hot, seeded_gbar, synth
    c = dict(CONFIGS[cfg])
    if d is not None:
        c["d"] = d
    Xs, Ys = [], []
    for g in range(B):
        X, lab = synth(c["base"], c["batch"] + n_extra, c["d"], r=c["r"], seed=40 + g)
        Xs.append(X)
        Ys.append(one_hot(lab[: c["base"]]))
    G = torch.from_numpy(np.stack([seeded_gbar(c["batch"] + n_extra, 10, 50 + g)
                                   for g in range(B)])).cuda()
    from graphlearninglayer_amd import _lib
    outs = []
    for tile in (128, 256):
        with A.knobs({_lib.KNOB_GRAM_TILE: tile}):
            Xb = torch.from_numpy(np.stack(Xs)).cuda().requires_grad_(True)
            U = GLL.LaplaceLearningSparseHard.apply(Xb, torch.from_numpy(np.stack(Ys)).cuda(),
                                                    0.07, 1.0, c["k"])
            U.backward(G)
            outs.append((U.detach().cpu().numpy(), Xb.grad.cpu().numpy()))
    np.testing.assert_array_equal(outs[0][0], outs[1][0])
    np.testing.assert_array_equal(outs[0][1], outs[1][1])


def test_gram_tail_changes_no_result():
    """The stress Gram (8,192 x 1024: 528 256-tiles on 256 CUs) runs its 16-tile last round as 256
    64-subtiles (gram_pk_kernel<H, 64>, round 6; bitwise the 256-tile kernel's D2);
    GLL_KNOB_GRAM_TAIL = 2 runs it as 64 128-subtiles (round 5), 1 as a third 256-tile round.  The
    kNN lists, distances and eps are bitwise the same, and no row needs the exact rescan
    (GLL.py:183,205)."""
    from graphlearninglayer_amd import _lib
    from graphlearninglayer_amd.synth import CONFIGS, synth
    c = CONFIGS["stress"]
    X, _ = synth(c["base"], c["batch"], c["d"], r=c["r"], seed=5)
    outs = []
    for tail in (0, 1, 2):
        with A.knobs({_lib.KNOB_GRAM_TAIL: tail}):
            g = gpu_knn(X, c["k"], "auto")
            outs.append({key: g[key].cpu().numpy() for key in ("knn_idx", "knn_d2", "eps")})
            assert int(g["status"][_lib.ST_KNN_RESCAN].item()) == 0, tail
    for key in outs[0]:
        np.testing.assert_array_equal(outs[1][key], outs[0][key])
        np.testing.assert_array_equal(outs[2][key], outs[0][key])


@pytest.mark.parametrize("eps", [1.0, "auto"])
def test_locality_order_changes_no_result(eps):
    """Large single graphs process the kNN select and the chunked gradient in a pivot-grouped
    row order (gll_internal.h locality_order: speed only).  At the stress shape (X 32 MB, past an
    XCD's L2) U and grad_X are bitwise those of row-index order (GLL_FLAG_ROW_ORDER_OFF), and the
    kNN lists, eps and CSR too (GLL.py:183,205)."""
    from graphlearninglayer_amd import _lib
    from graphlearninglayer_amd.synth import CONFIGS, one_hot, seeded_gbar, synth
    c = CONFIGS["stress"]
    X, lab = synth(c["base"], c["batch"], c["d"], r=c["r"], seed=5)
    Y = one_hot(lab[: c["base"]])
    g = seeded_gbar(c["batch"], 10, 6)
    U0, g0 = fwd_bwd_c_abi(X, Y, c["k"], 0.07, eps, g)
    U1, g1 = fwd_bwd_c_abi(X, Y, c["k"], 0.07, eps, g, flags=_lib.FLAG_ROW_ORDER_OFF)
    np.testing.assert_array_equal(U0, U1)
    np.testing.assert_array_equal(g0, g1)


@pytest.mark.parametrize("k,d", [(10, 256), (30, 1024), (14, 37), (57, 64)])
def test_select_forms_agree_bitwise(k, d):
    """The kNN select's latency form (two candidate groups in flight; single graphs of at most
    2,048 rows) and its occupancy form (x_i staged in LDS, one group; larger graphs and batches),
    forced through GLL_KNOB_SEL_FORM: the same kNN lists, distances and eps bitwise on one
    3,000-row graph -- k = 30 takes the 64-slot candidate list of the stress config -- and the
    lists are the exact float64 kNN (GLL.py:183,205)."""
    from graphlearninglayer_amd import _lib
    from graphlearninglayer_amd.synth import synth
    X, _ = synth(1000, 2000, d, r=1.0, seed=71)
    outs = []
    for form in (1, 2):
        with A.knobs({_lib.KNOB_SEL_FORM: form}):
            g = gpu_knn(X, k, "auto")
            outs.append({key: g[key].cpu().numpy() for key in ("knn_idx", "knn_d2", "eps")})
    for key in outs[0]:
        np.testing.assert_array_equal(outs[0][key], outs[1][key])
    assert exact_knn_rows(X, outs[0]["knn_idx"], k) == []


# ----------------------------------------------------------------------------------------
# Class counts other than 10.  The reference takes any label_matrix.shape[1] (GLL.py:32,85),
# and utils.one_hot_encode(..., 'auto') (utils.py:556-568) yields whatever C the labels have.
# C = 10 runs the specialised forms (the fused backward, the register-form coefficient);
# these cases reach the edge-coefficient instantiations (grad.hip launch_backward_grad: exact
# even C, the 4 / 8 / 16 bounds and the generic loop), the generic-C gradient and the
# two-launch backward.
# ----------------------------------------------------------------------------------------
def _classes_case(C, eps, seed, base=500, batch=500, d=512, k=10):
    from graphlearninglayer_amd.synth import one_hot, seeded_gbar, synth
    X, lab = synth(base, batch, d, C=C, r=1.0, seed=seed)
    return X, one_hot(lab[:base], C), seeded_gbar(batch, C, seed + 1)


@pytest.mark.parametrize("C", [2, 3, 16, 17, 100])
@pytest.mark.parametrize("eps", [1.0, "auto"])
def test_class_counts_match_oracle(C, eps):
    """NS shape (500 + 500 x 512, k = 10), C classes: U and grad_X through apply against the
    float64 oracle on the GPU's own kNN lists (GLL.py:14-177)."""
    X, Y, g = _classes_case(C, eps, seed=40 + C)
    U, gx = run_layer(X, Y, 0.07, eps, 10, g)
    assert U.shape == (500, C)
    ind = gpu_knn(X, 10, eps)["knn_idx"].cpu().numpy().astype(np.int64)
    Uo, st = O.forward(X, Y, tau=0.07, epsilon=eps, K=10, knn=(ind, None))
    assert O.rel_err(U, Uo) <= TOL
    assert O.rel_err(gx, O.backward(st, g)) <= TOL


@pytest.mark.parametrize("C,eps,shape", [(3, 1.0, "fullysup"), (16, "auto", "fullysup"),
                                         (17, "auto", "ns"), (6, 1.0, "ns")])
def test_class_counts_batched_match_oracle(C, eps, shape):
    """The batched entry at C != 10: FullySup-shape batches take the feature-chunked gradient
    with the per-edge coefficient pass (edge_coef_kernel<4>/<-16>), NS batches the whole-row
    gradient's generic-C form; every graph against the oracle."""
    from graphlearninglayer_amd.synth import CONFIGS, one_hot, seeded_gbar, synth
    c = CONFIGS[shape]
    B = 2
    Xs, Ys, Gs = [], [], []
    for g_ in range(B):
        X, lab = synth(c["base"], c["batch"], c["d"], C=C, r=c["r"], seed=60 + g_)
        Xs.append(X)
        Ys.append(one_hot(lab[: c["base"]], C))
        Gs.append(seeded_gbar(c["batch"], C, 70 + g_))
    Xb = torch.from_numpy(np.stack(Xs)).cuda().requires_grad_(True)
    Ub = GLL.LaplaceLearningSparseHard.apply(Xb, torch.from_numpy(np.stack(Ys)).cuda(), 0.07, eps,
                                             c["k"])
    Ub.backward(torch.from_numpy(np.stack(Gs)).cuda())
    for g_ in range(B):
        ind = gpu_knn(Xs[g_], c["k"], eps)["knn_idx"].cpu().numpy().astype(np.int64)
        Uo, st = O.forward(Xs[g_], Ys[g_], tau=0.07, epsilon=eps, K=c["k"], knn=(ind, None))
        assert O.rel_err(Ub[g_].detach().cpu().numpy(), Uo) <= TOL
        assert O.rel_err(Xb.grad[g_].cpu().numpy(), O.backward(st, Gs[g_])) <= TOL


def test_class_count_past_the_grid_cg_large_single_graph():
    """A single graph with m > 2048 and C = 17: the whole-GPU CG holds C <= 16, so the solves
    take the per-column kernels; U and grad_X against the oracle."""
    X, Y, g = _classes_case(17, 1.0, seed=81, base=500, batch=2500, d=64, k=10)
    U, gx = run_layer(X, Y, 0.07, 1.0, 10, g)
    ind = gpu_knn(X, 10, 1.0)["knn_idx"].cpu().numpy().astype(np.int64)
    Uo, st = O.forward(X, Y, tau=0.07, epsilon=1.0, K=10, knn=(ind, None))
    assert O.rel_err(U, Uo) <= TOL
    assert O.rel_err(gx, O.backward(st, g)) <= TOL


# ----------------------------------------------------------------------------------------
# k past one candidate per lane (kMaxKm1 = 56 < K - 1 <= 256): knn_select_wide_kernel (256
# candidate slots up to K - 1 = 128, 512 past it).  The reference takes any k (the constant at
# GLL.py:27, knn_num in utils.py:574).
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,eps", [(64, 1.0), (100, "auto"), (129, 1.0), (130, "auto"),
                                   (200, 1.0), (257, "auto")])
def test_wide_k_exact_knn_and_oracle(k, eps):
    """NS shape (500 + 500 x 512): the kNN lists are the exact float64 kNN, and U and grad_X
    match the float64 oracle on them (GLL.py:14-177)."""
    from graphlearninglayer_amd.synth import CONFIGS, one_hot, seeded_gbar, synth
    c = CONFIGS["ns"]
    X, lab = synth(c["base"], c["batch"], c["d"], r=c["r"], seed=31)
    Y = one_hot(lab[: c["base"]])
    g = seeded_gbar(c["batch"], 10, 32)
    ind = gpu_knn(X, k, eps)["knn_idx"].cpu().numpy()
    assert ind.shape == (c["base"] + c["batch"], k)
    assert (ind[:, 0] == np.arange(ind.shape[0])).all()
    assert exact_knn_rows(X, ind, k) == []
    U, gx = run_layer(X, Y, 0.07, eps, k, g)
    Uo, st = O.forward(X, Y, 0.07, eps, k, knn=(ind.astype(np.int64), None))
    assert O.rel_err(U, Uo) <= TOL
    assert O.rel_err(gx, O.backward(st, g)) <= TOL


def test_wide_k_batched_and_rescan():
    """k = 64 through the batched entry (fp32 distance rows: d2_half keeps them for the wide
    select) against single calls, and a graph whose row 0 -- the Gram's centre -- is far from
    the rest, so the certificate fails and the exact rescan under the bound runs: still the
    exact float64 kNN and the oracle's solve."""
    from graphlearninglayer_amd import _lib
    from graphlearninglayer_amd.synth import one_hot, seeded_gbar, synth
    k, B = 64, 3
    Xs, Ys, c = synth_batch("ns", B, seed0=41)
    G = np.stack([seeded_gbar(c["batch"], 10, 42 + g) for g in range(B)])
    Xb = torch.from_numpy(Xs).cuda().requires_grad_(True)
    Ub = GLL.LaplaceLearningSparseHard.apply(Xb, torch.from_numpy(Ys).cuda(), 0.07, 1.0, k)
    Ub.backward(torch.from_numpy(G).cuda())
    for g in range(B):
        U1, gx1 = run_layer(Xs[g], Ys[g], 0.07, 1.0, k, G[g])
        assert O.rel_err(Ub[g].detach().cpu().numpy(), U1) <= 1e-5
        assert O.rel_err(Xb.grad[g].cpu().numpy(), gx1) <= 1e-5
    X, lab = synth(100, 400, 64, r=1.0, seed=23)
    X[0] = 300.0 / np.sqrt(64)
    gg = gpu_knn(X, 80, "auto")
    ind = gg["knn_idx"].cpu().numpy()
    assert int(gg["status"][_lib.ST_KNN_RESCAN].item()) > 100
    assert exact_knn_rows(X, ind, 80) == []
    Y = one_hot(lab[:100])
    gb = seeded_gbar(400, 10, 5)
    U, grad = run_layer(X, Y, 0.07, "auto", 80, gb)
    Uo, st = O.forward(X, Y, 0.07, "auto", 80, knn=(ind.astype(np.int64), None))
    assert O.rel_err(U, Uo) < TOL
    assert O.rel_err(grad, O.backward(st, gb)) < TOL


@pytest.mark.parametrize("k", [100, 200])
def test_wide_k_ties_past_the_candidate_slots(k):
    """Advisor (round 5): more tied columns than the wide select's candidate slots (256 / 512):
    a cluster of 600 exact duplicates, so the threshold scan's compaction overflows and the
    full-row bisection for T' with ties in index order runs (GLL_ST_KNN_MERGE); the lists are
    still the exact float64 kNN (ties by index) and U, grad_X the oracle's."""
    from graphlearninglayer_amd import _lib
    rng = np.random.default_rng(7)
    n, d, base = 1400, 48, 200
    X = rng.standard_normal((n, d)).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    X[600:1200] = X[599]     # 601 copies of one point
    lab = np.arange(n) % 10
    Y = np.eye(10, dtype=np.float32)[lab[:base]]
    gb = rng.standard_normal((n - base, 10))
    g = gpu_knn(X, k, 1.0)
    ind = g["knn_idx"].cpu().numpy()
    assert int(g["status"][_lib.ST_KNN_MERGE].item()) > 0
    assert O.knn_set_mismatch(X, ind, k) == []
    U, grad = run_layer(X, Y, 0.07, 1.0, k, gb)
    Uo, st = O.forward(X, Y, 0.07, 1.0, k, knn=(ind.astype(np.int64), None))
    assert O.rel_err(U, Uo) < TOL
    assert O.rel_err(grad, O.backward(st, gb)) < TOL


@pytest.mark.parametrize("k,eps", [(100, 1.0), (200, "auto")])
def test_wide_k_row_panels_match_whole_matrix(k, eps):
    """Advisor (round 5): the wide select on the row-panel route (GLL_FLAG_KNN_PANEL: 1,024-row
    panels, a ragged last one): bitwise the whole-matrix path, and the oracle."""
    from graphlearninglayer_amd import _lib
    from graphlearninglayer_amd.synth import one_hot, seeded_gbar, synth
    X, lab = synth(300, 2200, 64, C=10, r=1.0, seed=61)
    Y = one_hot(lab[:300])
    g = seeded_gbar(2200, 10, 62)
    U0, gr0 = fwd_bwd_c_abi(X, Y, k, 0.07, eps, g)
    U1, gr1 = fwd_bwd_c_abi(X, Y, k, 0.07, eps, g, flags=_lib.FLAG_KNN_PANEL)
    np.testing.assert_array_equal(U0, U1)
    np.testing.assert_array_equal(gr0, gr1)
    ind = gpu_knn(X, k, eps)["knn_idx"].cpu().numpy().astype(np.int64)
    Uo, st = O.forward(X, Y, 0.07, eps, k, knn=(ind, None))
    assert O.rel_err(U1, Uo) <= TOL
    assert O.rel_err(gr1, O.backward(st, g)) <= TOL


def _select_point_id(pt):
    return "n{}-d{}-K{}-B{}-panel{}-form{}".format(*pt)


def _check_exact_lists(X, ind, d2, k):
    """The float64 kNN sets in every row (no row excused past the 1e-12 tie gap, and the point
    list holds no such tie: tests/test_lib_cpu.py), ordered by (d^2, index) with self first."""
    assert O.knn_set_mismatch(X, ind, k, rel_gap=1e-12) == []
    assert (ind[:, 0] == np.arange(ind.shape[0])).all() and (d2[:, 0] == 0).all()
    dd, di = d2[:, 1:], ind[:, 1:]
    assert (np.diff(dd, axis=1) >= 0).all()
    # equal fp32 distances: by index, unless the float64 distances the select ranked by differ
    X64 = X.astype(np.float64)
    for i, r in zip(*np.nonzero((np.diff(dd, axis=1) == 0) & (np.diff(di, axis=1) < 0))):
        a, b = (np.sum((X64[i] - X64[di[i, r + q]]) ** 2) for q in (0, 1))
        assert a < b, (i, r)


@pytest.mark.parametrize("pt", __import__("tests.select_points", fromlist=["POINTS"]).POINTS,
                         ids=_select_point_id)
def test_every_select_variant_is_exact(pt):
    """One small problem per row of the select's table of instantiated kernels (select.hip;
    tests/select_points.py lists them and the CPU suite proves the list reaches every row).
    Single graphs: the float64 kNN sets, ordered lists.  Batches (the rows with fp16 distance
    storage among them): every graph's lists, distances and eps, read from its workspace block,
    are bitwise those of the single-graph call on that graph's rows under GLL_FLAG_D2_F32, and
    the float64 sets."""
    from graphlearninglayer_amd import _lib
    from tests import select_points as SP
    n, d, k, B, panel, form = pt
    Xs = SP.features(n, d, B)
    if B == 1:
        with A.knobs({_lib.KNOB_SEL_FORM: form}):
            g = GLL.device_graph(torch.from_numpy(Xs[0]).cuda(), k, "auto",
                                 flags=_lib.FLAG_KNN_PANEL if panel else 0)
            ind, d2 = g["knn_idx"].cpu().numpy(), g["knn_d2"].cpu().numpy()
        _check_exact_lists(Xs[0], ind, d2, k)
        return
    base, C = 8, 2
    Y = np.zeros((B, base, C), dtype=np.float32)
    Y[:, :, 0] = 1.0
    run = A.Run(np.stack(Xs), Y, k, 0.07, "auto", max_iter=2)   # the solve is not read here
    run.forward()
    K = run.problem().K
    for g in range(B):
        view = run.view(g)
        ind = run.array(view.knn_idx, n * K, np.int32, g).reshape(n, K)
        d2 = run.array(view.knn_d2, n * K, np.float32, g).reshape(n, K)
        eps = run.array(view.eps, n, np.float32, g)
        one = GLL.device_graph(run.X[g], k, "auto", flags=_lib.FLAG_D2_F32)
        np.testing.assert_array_equal(ind, one["knn_idx"].cpu().numpy())
        np.testing.assert_array_equal(d2, one["knn_d2"].cpu().numpy())
        np.testing.assert_array_equal(eps, one["eps"].cpu().numpy())
        _check_exact_lists(Xs[g], ind, d2, k)
