"""Float64 stage reference of the fused SupCon / SimCLR loss (include/gll.h gll_supcon_*,
graphlearninglayer_amd/csrc/supcon.hip) and an elementwise bound on how far its fp32 evaluation
may stray from it.  numpy throughout; tests/test_supcon_cpu.py runs this module on the CPU and
pins it to fixtures the reference's losses.py generated, tests/test_gpu_supcon.py holds the
kernels to it.

Model, in the memory order of features [bsz, V, d] (row r = b V + v, R = bsz V, lab(r) =
labels[r // V] or r // V; anchors: every row ('all') or the rows with v == 0 ('one'); A anchors):
    l_rj = z_r . z_j / T,  m_r = max_j l_rj,  E_r = sum_{j != r} exp(l_rj - m_r)
    pos(r) = {j != r: lab(j) == lab(r)},  c_r = |pos(r)|,  P_r = sum_pos l_rj
    row_loss_r = -(T / Tb) (P_r / c_r - m_r - log E_r),  loss = sum_anchors row_loss / A
    q_rj = ([j != r] exp(l_rj - m_r) / E_r - [j in pos(r)] / c_r) / (A Tb) for an anchor r, else 0
    gZ_r = gl sum_j (q_rj + q_jr) z_j
stats = (m_r, log E_r, c_r, 1 / E_r) of every row; row_loss in the reference's order (v bsz + b,
'one': b).  c_r = 0 gives 0/0: NaN, by plain IEEE arithmetic here too.

bound(): first-order, counted from the code of supcon.hip, u = 2^-24, gamma(n) = n u / (1 - n u),
every result widened by SLOP for the second-order terms.  Nothing is tuned to a measurement.
  * logits: the fp32-input MFMA is an fmaf chain over the d features, then one division by the
    fp32-rounded T: |dl_rj| <= gamma(d + 2) S_rj / T, S_rj = sum_k |z_rk z_jk|.
    delta_r = max_j |dl_rj|; the maximum of perturbed values moves by at most delta_r.
  * one exp term expf(fl(l - m)): its argument is off by at most 2 delta_r + u spread_r
    (spread_r = max_j (m_r - l_rj)), expf itself by EXP_ULPS u relative:
    rho_r = 2 delta_r + u spread_r + EXP_ULPS u.
  * E_r is a float64 sum of such terms (no fp32 addition); a term is rescaled by
    expf(fl(m_old - m_new)) at most `nresc` times on its way (once per tile of its chunk, once for
    the lane halves, once per chunk), each (spread_r + EXP_ULPS) u relative:
    relE_r = rho_r + nresc (spread_r + EXP_ULPS) u, and |d log E_r| <= relE_r.
  * P_r is a float64 sum of the logits: |d (P_r / c_r)| <= delta_r.
  * row_loss: (T / Tb) (2 delta_r + relE_r) + 3 u |row_loss| (T and Tb rounded to fp32, the result
    once); loss: the anchors' mean of that, + u |loss| for a float32 result.
  * stats as floats: + u |value| each; 1 / E_r: (relE_r + u) / E_r.
  * softmax weight p_rj = exp(l_rj - m_r) / E_r as fl(expf(.) fl(1 / E)): kappa_r = rho_r +
    relE_r + 3 u relative; q^_rj = fl(p^ - pos fl(1 / c)): p kappa_r + pos 2 u / c + u |q|;
    h_rj = fl(q_rj + q_jr): the two sides' errors + u |h|.
  * gZ_r = sum_j h_rj z_j as an fmaf chain of `chain` terms per chunk (32 per column tile), the
    chunks summed in float64, times gl / (A Tb) (Tb in fp32) and rounded once:
    |dgZ_rf| <= |gl| / (A Tb) (sum_j dh_rj |z_jf| + gamma(chain) sum_j |h_rj| |z_jf|) + 3 u |gZ_rf|.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

U = 2.0 ** -24
EXP_ULPS = 4.0            # expf: within 1 ulp by its documentation; 4 leaves room, not tuned
SLOP = 1.0 + 2.0 ** -10


def gamma(n):
    return n * U / (1.0 - n * U)


class SupCon(NamedTuple):
    loss: float
    row_loss: np.ndarray      # A, reference order
    stats: np.ndarray         # R x 4: m, log E, c, 1 / E
    gZ: np.ndarray            # bsz x V x d, for grad_loss = gl
    anchors: np.ndarray       # R bool
    order: np.ndarray         # A: row index r of row_loss[i]


def _rows(features, labels, mode):
    f = np.asarray(features, dtype=np.float64)
    bsz, V = f.shape[:2]
    Z = f.reshape(bsz * V, -1)
    R = bsz * V
    sample = np.arange(R) // V
    lab = sample if labels is None else np.asarray(labels).reshape(-1)[sample]
    if mode == "all":
        anch = np.ones(R, bool)
        order = (np.arange(bsz)[None, :] * V + np.arange(V)[:, None]).reshape(-1)   # v bsz + b -> r
    elif mode == "one":
        anch = np.arange(R) % V == 0
        order = np.arange(bsz) * V
    else:
        raise ValueError(mode)
    return Z, lab, anch, order


def supcon(features, labels=None, T=0.07, Tb=0.07, mode="all", gl=1.0) -> SupCon:
    Z, lab, anch, order = _rows(features, labels, mode)
    R = Z.shape[0]
    A = int(anch.sum())
    off = ~np.eye(R, dtype=bool)
    L = Z @ Z.T / T
    m = L.max(1)
    ex = np.where(off, np.exp(L - m[:, None]), 0.0)
    E = ex.sum(1)
    pos = (lab[:, None] == lab[None, :]) & off
    c = pos.sum(1).astype(np.float64)
    P = np.where(pos, L, 0.0).sum(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        rl = -(T / Tb) * (P / c - m - np.log(E))
        q = (ex / E[:, None] - pos / c[:, None]) / (A * Tb)
    q = np.where(anch[:, None], q, 0.0)
    gZ = gl * ((q + q.T) @ Z)
    stats = np.stack([m, np.log(E), c, 1.0 / E], 1)
    return SupCon(float(rl[anch].sum() / A), rl[order], stats, gZ.reshape(np.shape(features)[0], -1, Z.shape[1]),
                  anch, order)


class Bound(NamedTuple):
    loss: float
    row_loss: np.ndarray      # A, reference order
    stats: np.ndarray         # R x 4
    gZ: np.ndarray            # bsz x V x d


def bound(features, labels=None, T=0.07, Tb=0.07, mode="all", gl=1.0, chain=None, nresc=None) -> Bound:
    """|fp32 evaluation - supcon()| per element (module docstring).  chain: fmaf terms of one
    chunk's gZ accumulation (32 tiles-per-chunk; default: all R rows in one chain); nresc:
    rescalings a term of E_r can meet (tiles per chunk + 1 + chunks; default R / 32 + 2)."""
    Z, lab, anch, order = _rows(features, labels, mode)
    R, d = Z.shape
    A = int(anch.sum())
    chain = R + 32 if chain is None else chain
    nresc = R // 32 + 3 if nresc is None else nresc
    ref = supcon(features, labels, T, Tb, mode, gl)
    off = ~np.eye(R, dtype=bool)
    aZ = np.abs(Z)
    L = Z @ Z.T / T
    m = L.max(1)
    delta = (gamma(d + 2) * (aZ @ aZ.T) / T).max(1)
    spread = (m[:, None] - L).max(1)
    rho = 2 * delta + U * spread + EXP_ULPS * U
    relE = rho + nresc * (spread + EXP_ULPS) * U
    E = np.where(off, np.exp(L - m[:, None]), 0.0).sum(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        rl_all = -(T / Tb) * ((np.where((lab[:, None] == lab[None, :]) & off, L, 0.0).sum(1))
                              / ref.stats[:, 2] - m - np.log(E))
        b_rl = (T / Tb) * (2 * delta + relE) + 3 * U * np.abs(rl_all)
        b_loss = b_rl[anch].sum() / A + U * abs(ref.loss)
        b_stats = np.stack([delta + U * np.abs(m), relE + U * np.abs(np.log(E)), np.zeros(R),
                            (relE + U) / E], 1)
        pos = (lab[:, None] == lab[None, :]) & off
        c = ref.stats[:, 2]
        p = np.where(off, np.exp(L - m[:, None]), 0.0) / E[:, None]
        kappa = rho + relE + 3 * U
        q = p - pos / c[:, None]
        dq = p * kappa[:, None] + pos * (2 * U / c[:, None]) + U * np.abs(q)
        q = np.where(anch[:, None], q, 0.0)
        dq = np.where(anch[:, None], dq, 0.0)
        h = q + q.T
        dh = dq + dq.T + U * np.abs(h)
        w = abs(gl) / (A * Tb)
        b_g = w * (dh @ aZ + gamma(chain) * (np.abs(h) @ aZ)) + 3 * U * np.abs(ref.gZ.reshape(R, d))
    return Bound(SLOP * b_loss, SLOP * b_rl[order], SLOP * b_stats,
                 SLOP * b_g.reshape(ref.gZ.shape))


def finite_difference(features, labels, T, Tb, mode, idx, eps=1e-6):
    """Central difference of the loss in the entries `idx` (flat indices) of features."""
    f = np.asarray(features, dtype=np.float64)
    out = np.empty(len(idx))
    for n, i in enumerate(idx):
        fp, fm = f.copy(), f.copy()
        fp.reshape(-1)[i] += eps
        fm.reshape(-1)[i] -= eps
        out[n] = (supcon(fp, labels, T, Tb, mode).loss - supcon(fm, labels, T, Tb, mode).loss) / (2 * eps)
    return out
