"""The Python-integer model of the native periodic gradient calls and their strain derivative (test infrastructure, CPU only).

tests/gradient_native_util.py extended by the `disp` form of the contribution rule and by W (include/loco_hd_hip.h, "under periodic
boundaries, and the strain derivative"), in numpy float64, one IEEE operation at a time:

    use   = k >= 1  &&  idx[p][k] >= 0  &&  dist[p][k] > 0  &&  isfinite(g[p][k])
    coef  = (v_p * g[p][k]) / dist[p][k]
    step_c = coef * disp[p][k][c]
    grad[m][c] += step_c ;  grad[a][c] += -step_c        m = idx[p][k];  a = idx[p][0] (thresholded) or p (dense)
    W[i][j]   += step_i * disp[p][k][j]                  i <= j;  W[j][i] = W[i][j]

Every sum is the exact accumulator of gradient_native_util (quantize, integer sum, one rounding).
"""
from __future__ import annotations

import numpy as np

import gradient_native_util as gn

COMPONENTS = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]  # the order of lchd_strain_sum.h


def side_terms(idx, dist, g, disp, n_atoms, weights=None, dense=False):
    """The used slots of one side, row-major over (pair, slot): (members [M], anchors [M], steps [M][3], W terms [M][6])."""
    idx, dist, g = np.asarray(idx), np.asarray(dist, dtype=np.float64), np.asarray(g, dtype=np.float64)
    disp = np.asarray(disp, dtype=np.float64)
    n_pairs = idx.shape[0]
    v = np.ones(n_pairs) if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
    anchor = np.arange(n_pairs) if dense else idx[:, 0].astype(np.int64)
    use = (idx >= 0) & (idx < n_atoms) & (dist > 0.0) & np.isfinite(g) & ((anchor >= 0) & (anchor < n_atoms))[:, None]
    use[:, 0] = False
    p, k = np.nonzero(use)
    with np.errstate(over="ignore", invalid="ignore"):
        coef = (v[p] * g[p, k]) / dist[p, k]
        d = disp[p, k]
        step = coef[:, None] * d
        terms = np.stack([step[:, i] * d[:, j] for i, j in COMPONENTS], axis=1) if len(p) else np.zeros((0, 6))
    return idx[p, k].astype(np.int64), anchor[p], step, terms


def exact_totals(columns):
    """Per column of a float64 array [M][C]: (the integer sum of the quantized values, flag)."""
    totals, flag = [0] * columns.shape[1], 0
    for row in columns.tolist():
        for c, s in enumerate(row):
            t = gn.quantize(s)
            if t is None:
                flag |= 1
            else:
                totals[c] += t
    return totals, flag


def strain_from_totals(totals) -> np.ndarray:
    w = np.zeros((3, 3))
    for (i, j), t in zip(COMPONENTS, totals):
        w[i, j] = w[j, i] = gn.round_total(t)
    return w


def side_result(idx, dist, g, disp, n_atoms, weights=None, dense=False):
    """One side of a native periodic gradient call: (grad [n_atoms][3], W [3][3], flag)."""
    m, a, step, terms = side_terms(idx, dist, g, disp, n_atoms, weights, dense)
    total = [[0, 0, 0] for _ in range(n_atoms)]
    flag = 0
    for mi, ai, st in zip(m.tolist(), a.tolist(), step.tolist()):
        for c in range(3):
            t = gn.quantize(st[c])
            if t is None:
                flag |= 1
                continue
            total[mi][c] += t
            total[ai][c] -= t
    grad = np.asarray([[gn.round_total(t) for t in row] for row in total], dtype=np.float64).reshape(n_atoms, 3)
    totals, wflag = exact_totals(terms)
    return grad, strain_from_totals(totals), flag | wflag


def result(sens, n_a, n_b, weights=None, dense=False):
    """(grad_a, grad_b, strain_a, strain_b, flag) from a PeriodicSensitivity / MinImageSensitivity of NumPy arrays."""
    ga, wa, fa = side_result(sens.idx_a, sens.dist_a, sens.g_a, sens.disp_a, n_a, weights, dense)
    gb, wb, fb = side_result(sens.idx_b, sens.dist_b, sens.g_b, sens.disp_b, n_b, weights, dense)
    return ga, gb, wa, wb, fa | fb


def strain_longdouble(sens, weights=None, dense=False):
    """(W_a, W_b) of the same lists summed in long double, full 3 x 3 (no symmetrisation): what a C client or a model compares with."""
    out = []
    ld = np.longdouble
    for idx, dist, g, disp in ((sens.idx_a, sens.dist_a, sens.g_a, sens.disp_a), (sens.idx_b, sens.dist_b, sens.g_b, sens.disp_b)):
        idx = np.asarray(idx)
        n_pairs = idx.shape[0]
        v = np.ones(n_pairs) if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
        use = (idx >= 0) & (np.asarray(dist) > 0.0) & np.isfinite(np.asarray(g))
        use[:, 0] = False
        p, k = np.nonzero(use)
        coef = v[p].astype(ld) * np.asarray(g)[p, k].astype(ld) / np.asarray(dist)[p, k].astype(ld)
        d = np.asarray(disp)[p, k].astype(ld)
        out.append(np.einsum("m,mi,mj->ij", coef, d, d))
    return out[0], out[1]
