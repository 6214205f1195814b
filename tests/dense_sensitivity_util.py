"""Dense-row neighbour sensitivities from their definition (test infrastructure, CPU, NumPy only), on tests/sensitivity_util.py.

Row r of a distance matrix is one environment in which every column is a member.  Its list is the row co-sorted with the column index,
ascending by (distance, column) -- the reference's stable sort of a row with seq -- with no forced anchor: slot 0 is the first of that
order.  sensitivity_util.sensitivity (longdouble) takes the two sorted lists; the gradients are assembled in longdouble from its g.
"""
from __future__ import annotations

import numpy as np

from integral_form import LD, _sqdist
from sensitivity_util import Sens, sensitivity


def coords_rows(xyz):
    """The rows from_coords scores, float64 in the reference's operation order (utils.rs:1-8): row r = distances from atom r."""
    xyz = np.asarray(xyz, dtype=np.float64)
    return np.asarray([np.sqrt(_sqdist(xyz[r], xyz)) for r in range(len(xyz))]).reshape(len(xyz), len(xyz))


def sorted_row(row):
    """(columns, distances) of one row in (distance, column) order."""
    row = np.asarray(row, dtype=np.float64)
    order = np.lexsort((np.arange(len(row)), row))
    return order, row[order]


def from_dmxs(cat_a, dmx_a, cat_b, dmx_b, n_categories, wf, sd=("Hellinger", [2.0]), category_weights=None, width=None):
    """The Sens tuple LoCoHD.sensitivity_from_dmxs returns (g as float64); wf: one (name, params) or one per row."""
    cat_a, cat_b = np.asarray(cat_a), np.asarray(cat_b)
    dmx_a, dmx_b = np.asarray(dmx_a, dtype=np.float64), np.asarray(dmx_b, dtype=np.float64)
    rows, (na, nb) = len(dmx_a), (dmx_a.shape[1], dmx_b.shape[1])
    K = max(na, nb) if width is None else width
    out = Sens(np.zeros(rows), np.full(rows, na, np.int32), np.full((rows, K), -1, np.int32), np.zeros((rows, K)), np.zeros((rows, K)),
               np.full(rows, nb, np.int32), np.full((rows, K), -1, np.int32), np.zeros((rows, K)), np.zeros((rows, K)))
    for r in range(rows):
        ia, da = sorted_row(dmx_a[r])
        ib, db = sorted_row(dmx_b[r])
        s, ga, gb = sensitivity(cat_a[ia], da, cat_b[ib], db, n_categories, wf[r] if isinstance(wf, list) else wf, sd, category_weights)
        out.scores[r] = s
        out.idx_a[r, :na], out.dist_a[r, :na], out.g_a[r, :na] = ia, da, ga.astype(np.float64)
        out.idx_b[r, :nb], out.dist_b[r, :nb], out.g_b[r, :nb] = ib, db, gb.astype(np.float64)
    return out


def scatter(count, idx, values, cols, dtype=LD):
    """out[r][idx[r][k]] = values[r][k] for slots 1 .. count[r] - 1, longdouble: sorted rows back into column order."""
    out = np.zeros((len(count), cols), dtype=dtype)
    for r in range(len(count)):
        for k in range(1, int(count[r])):
            out[r, idx[r, k]] = values[r, k]
    return out


def gradient_dmx(sens, cols_a, cols_b, pair_weights=None):
    """(G_a, G_b): G[r][j] = v_r g of column j; the slot-0 column and non-finite g give 0."""
    v = np.ones(len(sens.scores)) if pair_weights is None else np.asarray(pair_weights, dtype=np.float64)
    out = []
    for cnt, idx, g, cols in ((sens.count_a, sens.idx_a, sens.g_a, cols_a), (sens.count_b, sens.idx_b, sens.g_b, cols_b)):
        vals = np.where(np.isfinite(g), np.asarray(v, dtype=LD)[:, None] * np.asarray(g, dtype=LD), LD(0))
        out.append(scatter(cnt, idx, vals, cols).astype(np.float64))
    return out[0], out[1]


def gradient_coords(sens, xyz_a, xyz_b, pair_weights=None):
    """(grad_a, grad_b), longdouble sums term by term: row r moves member m by v g (x_m - x_r) / d and atom r by the opposite; members
    at d == 0 are skipped.  (The direction is taken from atom r, the row's own atom, whichever tied atom holds slot 0.)"""
    v = np.ones(len(sens.scores)) if pair_weights is None else np.asarray(pair_weights, dtype=np.float64)
    out = []
    for xyz, cnt, idx, dist, g in ((xyz_a, sens.count_a, sens.idx_a, sens.dist_a, sens.g_a), (xyz_b, sens.count_b, sens.idx_b, sens.dist_b, sens.g_b)):
        xyz = np.asarray(xyz, dtype=LD)
        grad = np.zeros(xyz.shape, dtype=LD)
        for r in range(len(cnt)):
            for k in range(1, int(cnt[r])):
                if dist[r, k] > 0.0 and np.isfinite(g[r, k]):
                    step = LD(v[r]) * LD(g[r, k]) / LD(dist[r, k]) * (xyz[idx[r, k]] - xyz[r])
                    grad[idx[r, k]] += step
                    grad[r] -= step
        out.append(grad.astype(np.float64))
    return out[0], out[1]
