"""Score attribution by category from its definition (test infrastructure, CPU, NumPy only), on tests/integral_form.py.

    t_c(r) = |a_c^(1/e) - b_c^(1/e)|^e      T(r) = sum_c t_c(r)      H(r) = (T / 2)^(1/e)
    out[c] = sum_j (F(u_{j+1}) - F(u_j)) * H_j * t_{c,j} / T_j          (a piece with T_j = 0 adds 0 to every column)

over the DISTINCT breakpoints u_j of the pair's two environments, a / b the weighted, normalised count vectors of the points at distance
<= u_j (anchors included): integral_form.score with the Hellinger sum kept per category.  Everything after the environment membership
test is np.longdouble.  Hellinger distances only: no other distance is a sum of per-category terms.
"""
from __future__ import annotations

import numpy as np

from integral_form import LD, _sqdist, cdf
from radial_util import environment


def attribution(cat_a, dist_a, cat_b, dist_b, n_categories, wf, exponent=2.0, category_weights=None):
    """cat_x / dist_x: the two environments as integral_form.score takes them (any order).  Returns a float64 array [n_categories]."""
    w = np.ones(n_categories, dtype=LD) if category_weights is None else np.asarray(category_weights, dtype=LD)
    sides = []
    for cat, dist in ((cat_a, dist_a), (cat_b, dist_b)):
        dist = np.asarray(dist, dtype=np.float64)
        order = np.argsort(dist, kind="stable")
        d = dist[order]
        onehot = np.zeros((len(d) + 1, n_categories), dtype=LD)
        onehot[np.arange(1, len(d) + 1), np.asarray(cat)[order]] = 1
        sides.append((d, np.cumsum(onehot, axis=0) * w[None, :]))
    (da, pa), (db, pb) = sides
    u = np.unique(np.concatenate([[0.0], da, db]))
    A = pa[np.searchsorted(da, u, side="right")]
    B = pb[np.searchsorted(db, u, side="right")]
    P, Q = A / A.sum(-1, keepdims=True), B / B.sum(-1, keepdims=True)
    e = LD(exponent)
    t = np.abs(P ** (1 / e) - Q ** (1 / e)) ** e  # [J + 1][C]
    T = t.sum(-1)
    H = (T / LD(2)) ** (1 / e)
    share = np.where(T[:, None] > 0, t / np.where(T > 0, T, LD(1))[:, None], LD(0))
    F = cdf(wf[0], wf[1], np.concatenate([u, [np.inf]]))
    return ((np.diff(F) * H)[:, None] * share).sum(0).astype(np.float64)


def from_primitives(cat_a, xyz_a, tag_a, cat_b, xyz_b, tag_b, pairs, thr, n_categories, wf, exponent=2.0, category_weights=None,
                    accept_same=True):
    """Thresholded pairs: row p is the attribution of pair p (the environment rule of radial_util.environment); wf: one (name, params)
    or one per pair."""
    rows = []
    for p, (i, j) in enumerate(pairs):
        ca, da = environment(int(i), cat_a, xyz_a, tag_a, thr, accept_same)
        cb, db = environment(int(j), cat_b, xyz_b, tag_b, thr, accept_same)
        rows.append(attribution(ca, da, cb, db, n_categories, wf[p] if isinstance(wf, list) else wf, exponent, category_weights))
    return np.asarray(rows)


def from_rows(cat_a, rows_a, cat_b, rows_b, n_categories, wf, exponent=2.0, category_weights=None):
    """Dense rows (from_dmxs / from_coords): row r of A against row r of B, categories = a prefix of cat_x."""
    return np.asarray([attribution(np.asarray(cat_a)[: len(ra)], ra, np.asarray(cat_b)[: len(rb)], rb, n_categories, wf, exponent, category_weights)
                       for ra, rb in zip(rows_a, rows_b)])


def open_rows(xyz):
    """The distance rows of from_coords without a cell, in the reference's summation order."""
    xyz = np.asarray(xyz, dtype=np.float64)
    return np.sqrt(np.asarray([_sqdist(p, xyz) for p in xyz]))
