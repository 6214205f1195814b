"""The binned form of tests/integral_form.score (test infrastructure, CPU, NumPy only): a pair's radial profile from its definition.

    out[k] = sum_j H_j * max(0, min(F(u_{j+1}), F(e_{k+1})) - max(F(u_j), F(e_k)))

H is constant between two distinct breakpoints u_j, so the finite edges are inserted among the breakpoints: every piece of the refined
grid lies in exactly one bin (or below e_0 / above e_K, where it is dropped), and `np.diff(F) * H` is summed per bin in longdouble.
"""
from __future__ import annotations

import numpy as np

from integral_form import LD, _sqdist, cdf, distance


def profile(cat_a, dist_a, cat_b, dist_b, n_categories, wf, edges, sd=("Hellinger", [2.0]), category_weights=None):
    """cat_x / dist_x: the two environments as integral_form.score takes them (any order); edges: K + 1 ascending distances, the
    last may be inf.  Returns a float64 array [K]."""
    w = np.ones(n_categories, dtype=LD) if category_weights is None else np.asarray(category_weights, dtype=LD)
    edges = np.asarray(edges, dtype=np.float64)
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
    t = np.unique(np.concatenate([u, edges[np.isfinite(edges)]]))  # the breakpoints with the edges among them
    t = t[t >= 0.0]
    A = pa[np.searchsorted(da, t, side="right")]  # counts at distance <= t_i: constant up to the next breakpoint
    B = pb[np.searchsorted(db, t, side="right")]
    H = distance(sd[0], sd[1], A / A.sum(-1, keepdims=True), B / B.sum(-1, keepdims=True))
    F = cdf(wf[0], wf[1], np.concatenate([t, [np.inf]]))
    mass = np.diff(F) * H
    k = np.searchsorted(edges, t, side="right") - 1  # the bin piece i starts (and lies) in
    out = np.zeros(len(edges) - 1, dtype=LD)
    for b in range(len(edges) - 1):
        sel = mass[k == b]
        out[b] = sel.sum() if len(sel) else LD(0)
    return out.astype(np.float64)


def environment(i, cat, xyz, tag, thr, accept_same=True):
    """The environment of anchor i as from_primitives builds it (integral_form.from_primitives): categories and distances."""
    xyz = np.asarray(xyz, dtype=np.float64)
    thr2 = np.float64(thr) * np.float64(thr) if np.isfinite(thr) else np.inf
    d2 = _sqdist(xyz[i], xyz)
    keep = d2 < thr2
    if tag is not None:
        rule = (np.asarray(tag) == tag[i]) == bool(accept_same)
        rule[i] = True
        keep &= rule
    return np.asarray(cat)[keep], np.sqrt(d2[keep])


def from_primitives(cat_a, xyz_a, tag_a, cat_b, xyz_b, tag_b, pairs, thr, n_categories, wf, edges, sd=("Hellinger", [2.0]),
                    category_weights=None, accept_same=True):
    """Row p: the profile of pair p; wf: one (name, params) or one per pair."""
    rows = []
    for p, (i, j) in enumerate(pairs):
        ca, da = environment(int(i), cat_a, xyz_a, tag_a, thr, accept_same)
        cb, db = environment(int(j), cat_b, xyz_b, tag_b, thr, accept_same)
        rows.append(profile(ca, da, cb, db, n_categories, wf[p] if isinstance(wf, list) else wf, edges, sd, category_weights))
    return np.asarray(rows)


def from_rows(cat_a, rows_a, cat_b, rows_b, n_categories, wf, edges, sd=("Hellinger", [2.0]), category_weights=None):
    """Dense rows (from_dmxs / from_coords): row r of A against row r of B, categories = a prefix of cat_x."""
    return np.asarray([profile(np.asarray(cat_a)[: len(ra)], ra, np.asarray(cat_b)[: len(rb)], rb, n_categories, wf, edges, sd, category_weights)
                       for ra, rb in zip(rows_a, rows_b)])


def split(f_lo, f_hi, h, bounds):
    """The additions of ONE interval [f_lo, f_hi] of constant distance h to the bins with bounds E_0 <= ... <= E_K, by the definition:
    h * max(0, min(f_hi, E_{k+1}) - max(f_lo, E_k)) (what loco_hd_amd/csrc/lchd_radial_bins.h walks with a running bin index)."""
    E = np.asarray(bounds, dtype=LD)
    return (LD(h) * np.maximum(LD(0), np.minimum(LD(f_hi), E[1:]) - np.maximum(LD(f_lo), E[:-1]))).astype(np.float64)
