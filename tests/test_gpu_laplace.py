"""utils.laplace on the HIP path (run on the MI355X: -m gpu) against the reference pipeline's
fixtures and the float64 oracle.  The parity bar is that of tests/test_gpu_parity.py.
"""
import numpy as np
import pytest
import torch

from oracle import gll_oracle as O
from tests import abi as A
from tests.parity_runs import TOL, gpu_knn

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    A.need_gpu()


@pytest.mark.parametrize("fname", ["laplace_small", "laplace_k64"])
def test_utils_laplace_matches_reference_fixture(fname):
    """utils.laplace on the GPU vs the reference pipeline's fixture
    (laplace_k64: knn_num = 64, the wide kNN select, pinned by the reference itself)."""
    import json
    import os
    from graphlearninglayer_amd import utils as U_
    from graphlearninglayer_amd.synth import synth
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                             fname + ".npz"))
    p = json.loads(str(z["meta"]))
    X, labels = synth(p["labeled"], p["unlabeled"], p["d"], C=10, r=p["r"], seed=p["seed"])
    train = labels[: p["labeled"]]
    U = U_.laplace(X, train, knn_num=p["knn_num"], epsilon=p["epsilon"], tau=p["tau"])
    assert U.shape == z["U"].shape and U.dtype == np.float64
    ind = gpu_knn(X, p["knn_num"], p["epsilon"])["knn_idx"].cpu().numpy().astype(np.int64)
    Uo = O.laplace(X, train, knn_num=p["knn_num"], epsilon=p["epsilon"], tau=p["tau"],
                   knn=(ind, None))
    assert O.rel_err(U, Uo) <= TOL
    ref_ind = z["knn"].astype(np.int64)
    bad = [i for i, (a, b) in enumerate(zip(ind.tolist(), ref_ind.tolist())) if set(a) != set(b)]
    assert bad == [], f"{len(bad)} rows differ from the reference kNN, first {bad[:8]}"
    assert O.rel_err(U, z["U"]) <= TOL          # against the reference pipeline's output
    assert np.mean(U.argmax(1) == z["U"].argmax(1)) >= 0.999


def test_utils_laplace_large_graph_matches_oracle():
    """n = 20,250 (250 labeled), d = 128, k = 50: the whole-GPU CG + float64 refinement."""
    from graphlearninglayer_amd import utils as U_
    from graphlearninglayer_amd.synth import synth
    X, labels = synth(250, 20000, 128, C=10, r=1.0, seed=8)
    train = labels[:250]
    U = U_.laplace(X, train, knn_num=50, epsilon=1.0, tau=1e-8)
    ind = gpu_knn(X, 50, 1.0)["knn_idx"].cpu().numpy().astype(np.int64)
    Uo = O.laplace(X, train, knn_num=50, epsilon=1.0, tau=1e-8, knn=(ind, None))
    assert O.rel_err(U, Uo) <= TOL
    acc = U_.gl_accuracy(X[:250], train, X[250:], labels[250:])
    assert acc == pytest.approx(100.0 * np.mean(Uo.argmax(1) == labels[250:]), abs=0.05)


def test_utils_laplace_reference_size_properties():
    """utils.laplace at the reference's evaluation size (250 labeled + 50,000 unlabeled train +
    10,000 test, d = 128, k = 50, utils.py:570-593): too large for the SuperLU oracle, so
    size-independent properties instead.  (1) kNN lists of 64 sampled rows equal the exact
    float64 sets over all 60,250 points; (2) the reference's own stopping criterion holds in
    float64 on the host, recomputed from the GPU graph: max_c ||M (rhs - Luu x)|| <= 1e-10 with
    M = diag(Luu + 1e-10)^(-1/2) (utils.py:586-591, GLL.py:259); (3) every prediction row is
    a convex combination of the labels (rows sum to 1, entries in [0, 1], maximum principle)."""
    import scipy.sparse as sp
    from graphlearninglayer_amd import utils as U_
    from graphlearninglayer_amd.synth import synth
    nl, nu, k = 250, 60000, 50
    X, labels = synth(nl, nu, 128, C=10, r=1.0, seed=3)
    Xd = torch.from_numpy(X).cuda()
    U = U_.laplace(Xd, labels[:nl], knn_num=k, epsilon=1.0, tau=1e-8)
    n, m = nl + nu, nu
    assert U.shape == (m, 10) and np.isfinite(U).all()
    g = gpu_knn(X, k, 1.0)
    ind = g["knn_idx"].cpu().numpy()
    rng = np.random.default_rng(0)
    X64 = X.astype(np.float64)
    for i in rng.choice(n, 64, replace=False):
        d2 = np.sum((X64 - X64[i]) ** 2, axis=1)
        order = np.argsort(d2, kind="stable")
        gap = d2[order[k]] - d2[order[k - 1]]
        if gap > 1e-12 * max(d2[order[k]], 1e-30):     # no exact tie at the boundary
            assert set(ind[i].tolist()) == set(order[:k].tolist()), f"row {i}"
    rp, col = g["row_ptr"].cpu().numpy(), g["col"].cpu().numpy()
    W = sp.csr_matrix((g["w"].cpu().numpy().astype(np.float64), col, rp), shape=(n, n))
    deg = np.asarray(W.sum(axis=1)).ravel()
    L = (sp.diags(deg) - W).tocsr()
    Luu = L[nl:, nl:] + 1e-8 * sp.eye(m)
    Y = U_.one_hot_encode(labels[:nl])
    rhs = -(L[nl:, :nl] @ Y)
    Mv = 1.0 / np.sqrt(Luu.diagonal() + 1e-10)
    res = np.linalg.norm(Mv[:, None] * (rhs - Luu @ U), axis=0)
    assert res.max() <= 2e-10, f"scaled residual {res.max():.3e}"
    # Luu is an M-matrix and W_ul Y >= 0, so 0 <= U and U 1 = 1 - tau Luu^-1 1 <= 1
    assert U.min() >= -1e-7 and U.sum(1).max() <= 1.0 + 1e-7
    acc = 100.0 * np.mean(U.argmax(1) == labels[nl:])
    print(f"n={n}: scaled residual {res.max():.2e}, GL accuracy {acc:.2f}%")


@pytest.mark.parametrize("C,nu", [(3, 2750), (17, 2750)])
def test_utils_laplace_auto_class_count(C, nu):
    """utils.laplace with n_classes = 'auto' on labels of C classes (utils.py:556-568,570-593):
    the one-hot width follows the labels, the CSR solve (gll_cg_csr: the whole-GPU CG for
    C <= 16, per-column kernels past it) against the oracle."""
    from graphlearninglayer_amd import utils as U_
    from graphlearninglayer_amd.synth import synth
    X, labels = synth(250, nu, 64, C=C, r=1.0, seed=90 + C)
    train = labels[:250]
    U = U_.laplace(X, train, knn_num=20, epsilon=1.0, tau=1e-8)
    assert U.shape == (nu, C)
    ind = gpu_knn(X, 20, 1.0)["knn_idx"].cpu().numpy().astype(np.int64)
    Uo = O.laplace(X, train, knn_num=20, epsilon=1.0, tau=1e-8, knn=(ind, None))
    assert Uo.shape == (nu, C)
    assert O.rel_err(U, Uo) <= TOL


@pytest.mark.parametrize("knn_num", [64, 100, 200])
def test_utils_laplace_wide_knn_num(knn_num):
    """utils.laplace with knn_num = 64 / 100 (utils.py:574) on 250 + 4,000 points: exact kNN
    on sampled rows and the oracle's solution."""
    from graphlearninglayer_amd import utils as U_
    from graphlearninglayer_amd.synth import synth
    X, labels = synth(250, 4000, 64, C=10, r=1.0, seed=50 + knn_num)
    train = labels[:250]
    U = U_.laplace(X, train, knn_num=knn_num, epsilon=1.0, tau=1e-8)
    ind = gpu_knn(X, knn_num, 1.0)["knn_idx"].cpu().numpy()
    Uo = O.laplace(X, train, knn_num=knn_num, epsilon=1.0, tau=1e-8,
                   knn=(ind.astype(np.int64), None))
    assert O.rel_err(U, Uo) <= TOL
    rng = np.random.default_rng(1)
    X64 = X.astype(np.float64)
    for i in rng.choice(X.shape[0], 48, replace=False):
        d2 = np.sum((X64 - X64[i]) ** 2, axis=1)
        order = np.argsort(d2, kind="stable")
        assert set(ind[i].tolist()) == set(order[:knn_num].tolist()), i
