"""Weight-function gradients dS/dtheta_k from their definition (test infrastructure, CPU, NumPy only).

Between the DISTINCT breakpoints u_0 = 0 < u_1 < ... < u_J of a pair's two environments (u_{J+1} = +inf), with H_j the statistical
distance of the two normalised, weighted count vectors of the points at distance <= u_j (anchors included) and G_k = dF/dtheta_k the
derivative of the weight function's CDF with respect to its k-th parameter:

    interval form    dS/dtheta_k = sum_j (G_k(u_{j+1}) - G_k(u_j)) * H_j
    by parts         dS/dtheta_k = sum_{j >= 1} G_k(u_j) * (H_{j-1} - H_j) + G_k(inf) * H_J - G_k(0) * H_0

G_k is written here from the closed forms of the four CDFs; nothing is shared with the library.  Conventions: G(inf) = 0; a dagum at
x = 0 gives 0; 0 * ln 0 = 0; where the limit is infinite (kumaraswamy's bounds with alpha < 1 at z = 0, beta < 1 at z = 1) the value is 0;
a point on a support bound of uniform / kumaraswamy takes the inside branch.  Everything after the environment membership test is
np.longdouble (`dtype=`: the same statements in another floating-point type, for the float64 restatement of the device tests).
"""
from __future__ import annotations

import numpy as np

from integral_form import LD, cdf
from radial_util import environment

# Restatement against Richardson-extrapolated finite differences of the CPU oracle: 10 x the oracle differences' own error estimate,
# measured in tests/test_weight_gradient_model.py (its docstring has the figures).
FD_BOUND = 6.1e-9
# Device against the longdouble restatement, on theta_k * grad[p][k]: the project's parity bound; the float64 restatement deviates from
# the longdouble one by less than 1e-12 on every case of tests/test_gpu_weight_gradient.py (its docstring has the figure).
PARITY = 1e-11


def cdf_param_grad(name, params, x, dtype=LD):
    """G[i][k] = dF/dtheta_k at x[i], in `dtype`."""
    x = np.asarray(x, dtype=dtype).reshape(-1)
    p = [dtype(v) for v in params]
    out = np.zeros((len(x), len(p)), dtype=dtype)
    one = dtype(1)
    with np.errstate(all="ignore"):
        for i, xi in enumerate(x):
            if not np.isfinite(xi) or xi < 0:
                continue
            if name == "uniform":
                a, b = p
                if a <= xi <= b:
                    out[i] = [(xi - b) / (b - a) ** 2, -(xi - a) / (b - a) ** 2]
            elif name == "kumaraswamy":
                lo, hi, al, be = p
                if lo <= xi <= hi:
                    L = hi - lo
                    z = (xi - lo) / L
                    za = z ** al
                    u = one - za
                    dz = al * be * z ** (al - one) * u ** (be - one)
                    d_al = be * u ** (be - one) * za * np.log(z) if 0 < z < 1 else dtype(0)
                    d_be = -(u ** be) * np.log(u) if 0 < u < 1 else dtype(0)
                    out[i] = [dz * (-(one - z) / L), dz * (-z / L), d_al, d_be]
            elif name == "dagum":
                A, B, P = p
                if xi > 0:
                    t = (xi / B) ** (-A)
                    if np.isfinite(t) and t > 0:
                        dt = -P * (one + t) ** (-P - one)
                        out[i] = [dt * (-t * np.log(xi / B)), dt * (A * t / B), -((one + t) ** (-P)) * np.log(one + t)]
            elif name == "hyper_exp":
                n = len(p) // 2
                a, b = np.asarray(p[:n], dtype=dtype), np.asarray(p[n:], dtype=dtype)
                e = np.exp(-b * xi)
                N = a.sum()
                tail = (a * e).sum() / N
                out[i, :n] = (tail - e) / N
                out[i, n:] = a * xi * e / N
            else:
                raise ValueError(name)
    out[~np.isfinite(out)] = 0
    return out


def distance(name, params, P, Q, dtype=LD):
    """The statistical distances from their definitions, in `dtype`; P, Q: [J][C]."""
    if name == "Hellinger":
        e = dtype(params[0])
        return ((np.abs(P ** (1 / e) - Q ** (1 / e)) ** e).sum(-1) / dtype(2)) ** (1 / e)
    if name == "Kolmogorov-Smirnov":
        return np.abs(P - Q).max(-1)
    if name == "Kullback-Leibler":
        eps = dtype(params[0])
        return (P * np.log((P + eps) / (Q + eps))).sum(-1)
    if name == "Renyi":
        alpha, eps = dtype(params[0]), dtype(params[1])
        if alpha == 1:
            return distance("Kullback-Leibler", [eps], P, Q, dtype)
        return np.log((P * ((P + eps) / (Q + eps)) ** (alpha - 1)).sum(-1)) / (alpha - 1)
    raise ValueError(name)


def pieces(cat_a, dist_a, cat_b, dist_b, n_categories, sd, category_weights=None, dtype=LD):
    """(u [J + 1] distinct breakpoints from 0, H [J + 1] the distance on the piece that starts at u_j)."""
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
    return u, distance(sd[0], sd[1], A / A.sum(-1, keepdims=True), B / B.sum(-1, keepdims=True), dtype)


def gradient(cat_a, dist_a, cat_b, dist_b, n_categories, wf, sd=("Hellinger", [2.0]), category_weights=None, dtype=LD, by_parts=False):
    """(score, dS/dtheta [n_params]) of one pair, in `dtype`; wf = (name, params)."""
    u, H = pieces(cat_a, dist_a, cat_b, dist_b, n_categories, sd, category_weights, dtype)
    F = np.asarray(cdf(wf[0], wf[1], np.concatenate([u, [np.inf]])), dtype=dtype)
    G = np.concatenate([cdf_param_grad(wf[0], wf[1], u, dtype), np.zeros((1, len(wf[1])), dtype=dtype)])  # (G(inf) = 0)
    score = (np.diff(F) * H).sum()
    if by_parts:
        grad = (G[1:-1] * (H[:-1] - H[1:])[:, None]).sum(0) + G[-1] * H[-1] - G[0] * H[0]
    else:
        grad = (np.diff(G, axis=0) * H[:, None]).sum(0)
    return score, grad


def from_primitives(cat_a, xyz_a, tag_a, cat_b, xyz_b, tag_b, pairs, thr, n_categories, wf, sd=("Hellinger", [2.0]), category_weights=None,
                    accept_same=True, dtype=LD, by_parts=False, width=None):
    """Thresholded pairs (radial_util.environment): (scores [P], grad [P][width]) in `dtype`; wf: one (name, params) or one per pair;
    rows are zero-padded to `width` columns (default: the most parameters of any function)."""
    wfs = wf if isinstance(wf, list) else [wf] * len(pairs)
    width = max(len(f[1]) for f in wfs) if width is None else width
    scores, rows = np.zeros(len(pairs), dtype=dtype), np.zeros((len(pairs), width), dtype=dtype)
    for p, (i, j) in enumerate(pairs):
        ca, da = environment(int(i), cat_a, xyz_a, tag_a, thr, accept_same)
        cb, db = environment(int(j), cat_b, xyz_b, tag_b, thr, accept_same)
        scores[p], g = gradient(ca, da, cb, db, n_categories, wfs[p], sd, category_weights, dtype, by_parts)
        rows[p, :len(g)] = g
    return scores, rows


def from_rows(cat_a, rows_a, cat_b, rows_b, n_categories, wf, sd=("Hellinger", [2.0]), category_weights=None, dtype=LD, by_parts=False):
    """Dense rows (from_dmxs / from_coords): row r of A against row r of B, categories = a prefix of cat_x."""
    wfs = wf if isinstance(wf, list) else [wf] * len(rows_a)
    width = max(len(f[1]) for f in wfs)
    scores, rows = np.zeros(len(rows_a), dtype=dtype), np.zeros((len(rows_a), width), dtype=dtype)
    for r, (ra, rb) in enumerate(zip(rows_a, rows_b)):
        scores[r], g = gradient(np.asarray(cat_a)[: len(ra)], ra, np.asarray(cat_b)[: len(rb)], rb, n_categories, wfs[r], sd, category_weights,
                                dtype, by_parts)
        rows[r, :len(g)] = g
    return scores, rows


def kink_parameters(name):
    """The parameters whose change moves a kink of F: the support bounds of uniform and kumaraswamy."""
    return (0, 1) if name in ("uniform", "kumaraswamy") else ()


def smooth_within_the_stencil(dists, wf, rel=1e-4):
    """bool [n_params]: a central-difference stencil theta_k +- h, h = rel * theta_k, of a pair whose members lie at `dists` straddles no
    kink of F -- no member lies within h of the support bound theta_k.  Decided from the geometry alone."""
    d = np.asarray(dists, dtype=np.float64)
    keep = np.ones(len(wf[1]), dtype=bool)
    for k in kink_parameters(wf[0]):
        keep[k] = not np.any(np.abs(d - wf[1][k]) <= rel * wf[1][k])
    return keep


def library_leaf_deviation(families):
    """max |theta_k (library's host leaf - the leaf restated here)| over `families` = {name: params} on a grid of distances: what ties this
    module's restatement to the leaf the kernel calls (WeightFunction.cdf_param_grad_vec; no GPU)."""
    import loco_hd_amd as lh

    x = np.concatenate([np.linspace(0.0, 14.0, 113), [np.inf]])
    worst = 0.0
    for name, params in families.items():
        got = lh.WeightFunction(name, params).cdf_param_grad_vec(x)
        worst = max(worst, float(np.max(np.abs((got - cdf_param_grad(name, params, x)) * np.asarray(params)[None, :]))))
    return worst
