"""Neighbour sensitivities of a LoCoHD score from their definition (test infrastructure, CPU, NumPy only), on tests/integral_form.py.

    S = sum_j (F(u_{j+1}) - F(u_j)) * H_j          g = dS/dd = w(d) * (H- - H+)

w = F' the weight function's density, H- / H+ the statistical distance on the piece that ends / starts at the member.  Every environment
is a list sorted ascending by (distance, atom index) with the anchor first; the non-anchor members of both lists are merged by distance
(side A first at equal distances, list order within a side) and treated one at a time, so at ties the derivative is one-sided.  Members
entering or leaving at the threshold are ignored.  Everything after the environment membership test is np.longdouble.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from integral_form import LD, _sqdist, cdf, distance
from radial_util import environment

Sens = namedtuple("Sens", "scores count_a idx_a dist_a g_a count_b idx_b dist_b g_b")


def pdf(name: str, params, x):
    """The analytic derivative of integral_form.cdf, longdouble; 0 below 0 and outside a bounded support (uniform: on [a, b))."""
    x = np.asarray(x, dtype=LD)
    p = [LD(v) for v in params]
    if name == "hyper_exp":
        k = len(p) // 2
        a, b = np.asarray(p[:k], dtype=LD), np.asarray(p[k:], dtype=LD)
        out = (a[None, :] * b[None, :] * np.exp(-b[None, :] * x[..., None])).sum(-1) / a.sum()
    elif name == "dagum":
        A, B, P = p
        xs = np.where(x > 0, x, LD(1))
        t = np.power(xs / B, -A)
        out = np.where(x > 0, A * P / xs * t * (LD(1) + t) ** (-P - 1), LD(0))
    elif name == "uniform":
        lo, hi = p
        out = np.where((x >= lo) & (x < hi), LD(1) / (hi - lo), LD(0))
    elif name == "kumaraswamy":
        lo, hi, A, B = p
        z = np.clip((x - lo) / (hi - lo), LD(0), LD(1))
        with np.errstate(divide="ignore", invalid="ignore"):
            out = np.where((x >= lo) & (x <= hi), A * B * z ** (A - 1) * (LD(1) - z ** A) ** (B - 1) / (hi - lo), LD(0))
    else:
        raise ValueError(name)
    return np.where(x < 0, LD(0), out)


def indexed_environment(i, cat, xyz, tag, thr, accept_same=True):
    """radial_util.environment with the atom indices, sorted by (distance, index), the anchor first: (idx, cat, dist)."""
    xyz = np.asarray(xyz, dtype=np.float64)
    c, d = environment(i, cat, xyz, tag, thr, accept_same)
    thr2 = np.float64(thr) * np.float64(thr) if np.isfinite(thr) else np.inf
    keep = _sqdist(xyz[i], xyz) < thr2
    if tag is not None:
        rule = (np.asarray(tag) == tag[i]) == bool(accept_same)
        rule[i] = True
        keep &= rule
    idx = np.flatnonzero(keep)
    assert len(idx) == len(d)
    order = np.lexsort((idx, d, idx != i))  # the anchor, then distance, then index
    return idx[order], np.asarray(c)[order], d[order]


def sensitivity(cat_a, dist_a, cat_b, dist_b, n_categories, wf, sd=("Hellinger", [2.0]), category_weights=None):
    """cat_x / dist_x: the two SORTED lists (slot 0 the anchor).  Returns (score, g_a, g_b): float, longdouble arrays per slot."""
    w = np.ones(n_categories, dtype=LD) if category_weights is None else np.asarray(category_weights, dtype=LD)
    da, db = np.asarray(dist_a, dtype=np.float64), np.asarray(dist_b, dtype=np.float64)
    ev = sorted([(da[k], 0, k) for k in range(1, len(da))] + [(db[k], 1, k) for k in range(1, len(db))])
    cnt = np.zeros((2, n_categories), dtype=LD)
    cnt[0, cat_a[0]] += w[cat_a[0]]
    cnt[1, cat_b[0]] += w[cat_b[0]]
    states = [cnt.copy()]
    for d, side, k in ev:
        c = (cat_a if side == 0 else cat_b)[k]
        cnt[side, c] += w[c]
        states.append(cnt.copy())
    st = np.asarray(states)  # [M + 1][2][C]
    H = distance(sd[0], sd[1], st[:, 0] / st[:, 0].sum(-1, keepdims=True), st[:, 1] / st[:, 1].sum(-1, keepdims=True))
    d_ev = np.asarray([e[0] for e in ev], dtype=np.float64)
    F = cdf(wf[0], wf[1], np.concatenate([[0.0], d_ev, [np.inf]]))
    score = float((np.diff(F) * H).sum())
    dens = pdf(wf[0], wf[1], d_ev) if len(ev) else np.zeros(0, dtype=LD)
    g = [np.zeros(len(da), dtype=LD), np.zeros(len(db), dtype=LD)]
    for m, (d, side, k) in enumerate(ev):
        g[side][k] = dens[m] * (H[m] - H[m + 1])
    return score, g[0], g[1]


def from_primitives(cat_a, xyz_a, tag_a, cat_b, xyz_b, tag_b, pairs, thr, n_categories, wf, sd=("Hellinger", [2.0]), category_weights=None,
                    accept_same=True, width=None):
    """The Sens tuple LoCoHD.sensitivity_from_primitives returns (g as float64); wf: one (name, params) or one per pair."""
    rows = []
    for p, (i, j) in enumerate(pairs):
        ia, ca, da = indexed_environment(int(i), cat_a, xyz_a, tag_a, thr, accept_same)
        ib, cb, db = indexed_environment(int(j), cat_b, xyz_b, tag_b, thr, accept_same)
        s, ga, gb = sensitivity(ca, da, cb, db, n_categories, wf[p] if isinstance(wf, list) else wf, sd, category_weights)
        rows.append((s, ia, da, ga, ib, db, gb))
    K = max([max(len(r[1]), len(r[4])) for r in rows], default=1) if width is None else width
    P = len(rows)
    out = Sens(np.zeros(P), np.zeros(P, np.int32), np.full((P, K), -1, np.int32), np.zeros((P, K)), np.zeros((P, K)), np.zeros(P, np.int32),
               np.full((P, K), -1, np.int32), np.zeros((P, K)), np.zeros((P, K)))
    for p, (s, ia, da, ga, ib, db, gb) in enumerate(rows):
        out.scores[p] = s
        out.count_a[p], out.count_b[p] = len(ia), len(ib)
        out.idx_a[p, : len(ia)], out.dist_a[p, : len(ia)], out.g_a[p, : len(ia)] = ia, da, ga.astype(np.float64)
        out.idx_b[p, : len(ib)], out.dist_b[p, : len(ib)], out.g_b[p, : len(ib)] = ib, db, gb.astype(np.float64)
    return out


def gradient(sens, xyz_a, xyz_b, pair_weights=None):
    """(grad_a, grad_b), longdouble sums: member += v g (x_m - x_anchor) / d, anchor -= the same; members at d == 0 skipped."""
    v = np.ones(len(sens.scores)) if pair_weights is None else np.asarray(pair_weights, dtype=np.float64)
    out = []
    for xyz, cnt, idx, dist, g in ((xyz_a, sens.count_a, sens.idx_a, sens.dist_a, sens.g_a), (xyz_b, sens.count_b, sens.idx_b, sens.dist_b, sens.g_b)):
        xyz = np.asarray(xyz, dtype=LD)
        grad = np.zeros(xyz.shape, dtype=LD)
        for p in range(len(cnt)):
            for k in range(1, int(cnt[p])):
                if dist[p, k] > 0.0:
                    step = LD(v[p]) * LD(g[p, k]) / LD(dist[p, k]) * (xyz[idx[p, k]] - xyz[idx[p, 0]])
                    grad[idx[p, k]] += step
                    grad[idx[p, 0]] -= step
        out.append(grad.astype(np.float64))
    return out[0], out[1]
