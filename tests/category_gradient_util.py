"""Category-weight gradients dS/dw_c from their definition (test infrastructure, CPU, NumPy only), on tests/integral_form.py.

Between two DISTINCT breakpoints u_j < u_{j+1} of the pair's two environments (u_0 = 0, u_{J+1} = +inf), with n^A / n^B the category
counts of the points at distance <= u_j (anchors included), p_c = w_c n^A_c / sum_k w_k n^A_k, q_c likewise from n^B, D(p, q) the
statistical distance, x_c = p_c dD/dp_c and y_c = q_c dD/dq_c:

    w_c dD/dw_c = x_c + y_c - p_c sum_k x_k - q_c sum_k y_k              (since w_c dp_k/dw_c = p_c (delta_kc - p_k))
    G[c]        = (1 / w_c) * sum_j (F(u_{j+1}) - F(u_j)) * (w_c dD/dw_c)_j

    Hellinger, exponent e:   d_c = p_c^(1/e) - q_c^(1/e), T = sum_c |d_c|^e, D = (T / 2)^(1/e)
                             x_c = (D / (e T)) |d_c|^(e-1) sgn(d_c) p_c^(1/e)      y_c = -(D / (e T)) |d_c|^(e-1) sgn(d_c) q_c^(1/e)
    Kullback-Leibler, eps:   x_c = p_c [ln((p_c + eps) / (q_c + eps)) + p_c / (p_c + eps)]      y_c = -p_c q_c / (q_c + eps)

Conventions: a Hellinger piece with T = 0 adds 0 to every column; a category with d_c = 0 has x_c = y_c = 0 for every exponent
(sgn 0 = 0); a piece with dF <= 0 adds nothing.  Everything after the environment membership test is np.longdouble (`dtype=`: the
same statements in another floating-point type, for the float64 restatement of the device tests).
"""
from __future__ import annotations

import numpy as np

from integral_form import LD, cdf
from radial_util import environment


# Restatement against Richardson-extrapolated finite differences of the CPU oracle: 10 x the oracle differences' own error estimate,
# measured in tests/test_category_gradient_model.py (its docstring has the figures).
FD_BOUND = 9e-11


def pieces(cat_a, dist_a, cat_b, dist_b, n_categories, wf, category_weights=None, dtype=LD):
    """The pieces of a pair: (dF [J + 1], P [J + 1][C], Q [J + 1][C], w [C]) with P / Q the two sides' PMFs on every piece."""
    w = np.ones(n_categories, dtype=dtype) if category_weights is None else np.asarray(category_weights, dtype=dtype)
    sides = []
    for cat, dist in ((cat_a, dist_a), (cat_b, dist_b)):
        dist = np.asarray(dist, dtype=np.float64)
        order = np.argsort(dist, kind="stable")
        d = dist[order]
        onehot = np.zeros((len(d) + 1, n_categories), dtype=dtype)
        onehot[np.arange(1, len(d) + 1), np.asarray(cat)[order]] = 1
        sides.append((d, np.cumsum(onehot, axis=0) * w[None, :]))
    (da, pa), (db, pb) = sides
    u = np.unique(np.concatenate([[0.0], da, db]))
    A = pa[np.searchsorted(da, u, side="right")]
    B = pb[np.searchsorted(db, u, side="right")]
    P, Q = A / A.sum(-1, keepdims=True), B / B.sum(-1, keepdims=True)
    F = np.asarray(cdf(wf[0], wf[1], np.concatenate([u, [np.inf]])), dtype=dtype)
    return np.diff(F), P, Q, w


def log_terms(P, Q, distance, dtype=LD):
    """(x, y) [J + 1][C] of every piece; distance: ("Hellinger", e) or ("Kullback-Leibler", eps)."""
    name, prm = distance
    prm = dtype(prm)
    if name == "Hellinger":
        a, b = P ** (1 / prm), Q ** (1 / prm)
        d = a - b
        s = np.where(d != 0, np.sign(d) * np.abs(np.where(d != 0, d, dtype(1))) ** (prm - 1), dtype(0))
        T = (np.abs(d) * np.abs(s)).sum(-1)
        ok = T > 0
        Ts = np.where(ok, T, dtype(1))
        k = np.where(ok, (Ts / dtype(2)) ** (1 / prm) / (prm * Ts), dtype(0))[:, None]
        return k * s * a, -(k * s * b)
    if name == "Kullback-Leibler":
        return P * (np.log((P + prm) / (Q + prm)) + P / (P + prm)), -(P * Q) / (Q + prm)
    raise ValueError(name)


def log_gradient(cat_a, dist_a, cat_b, dist_b, n_categories, wf, distance=("Hellinger", 2.0), category_weights=None, dtype=LD, parts=False):
    """w_c * dS/dw_c of one pair, in `dtype` [n_categories].  parts=True: also (integral of x_c + y_c, integral of p_c sum x + q_c sum y)."""
    dF, P, Q, w = pieces(cat_a, dist_a, cat_b, dist_b, n_categories, wf, category_weights, dtype)
    x, y = log_terms(P, Q, distance, dtype)
    direct = x + y
    mean = P * x.sum(-1, keepdims=True) + Q * y.sum(-1, keepdims=True)
    live = (dF > 0)[:, None]
    wg = (np.where(live, dF[:, None] * (direct - mean), dtype(0))).sum(0)
    if parts:
        return wg, np.where(live, dF[:, None] * direct, dtype(0)).sum(0), np.where(live, dF[:, None] * mean, dtype(0)).sum(0)
    return wg


def from_primitives(cat_a, xyz_a, tag_a, cat_b, xyz_b, tag_b, pairs, thr, n_categories, wf, distance=("Hellinger", 2.0), category_weights=None,
                    accept_same=True, dtype=LD, log_form=True):
    """Thresholded pairs (the environment rule of radial_util.environment): row p is w_c * G[p][c] (log_form) or G[p][c], in `dtype`;
    wf: one (name, params) or one per pair."""
    rows = []
    for p, (i, j) in enumerate(pairs):
        ca, da = environment(int(i), cat_a, xyz_a, tag_a, thr, accept_same)
        cb, db = environment(int(j), cat_b, xyz_b, tag_b, thr, accept_same)
        rows.append(log_gradient(ca, da, cb, db, n_categories, wf[p] if isinstance(wf, list) else wf, distance, category_weights, dtype))
    return _finish(rows, n_categories, category_weights, dtype, log_form)


def from_rows(cat_a, rows_a, cat_b, rows_b, n_categories, wf, distance=("Hellinger", 2.0), category_weights=None, dtype=LD, log_form=True):
    """Dense rows (from_dmxs / from_coords): row r of A against row r of B, categories = a prefix of cat_x."""
    rows = [log_gradient(np.asarray(cat_a)[: len(ra)], ra, np.asarray(cat_b)[: len(rb)], rb, n_categories, wf, distance, category_weights, dtype)
            for ra, rb in zip(rows_a, rows_b)]
    return _finish(rows, n_categories, category_weights, dtype, log_form)


def _finish(rows, n_categories, category_weights, dtype, log_form):
    out = np.asarray(rows, dtype=dtype).reshape(-1, n_categories)
    if log_form or category_weights is None:
        return out
    return out / np.asarray(category_weights, dtype=dtype)[None, :]


def richardson(score_of, w, c, rel=1e-3):
    """dS/dw_c by central differences of `score_of(weights) -> [P]` at steps h = rel * w_c, h / 2 and h / 4, Richardson-extrapolated:
    returns (the (h, h/2) extrapolation, |it - the (h/2, h/4) extrapolation|: the estimate of the reference's own error)."""
    w = np.asarray(w, dtype=np.float64)

    def central(h):
        up, dn = w.copy(), w.copy()
        up[c] += h
        dn[c] -= h
        return (np.asarray(score_of(up)) - np.asarray(score_of(dn))) / ((w[c] + h) - (w[c] - h))

    h = rel * w[c]
    d1, d2, d4 = central(h), central(h / 2), central(h / 4)
    r1, r2 = (4.0 * d2 - d1) / 3.0, (4.0 * d4 - d2) / 3.0
    return r1, np.abs(r1 - r2)
