"""Dense neighbour sensitivities under minimum-image periodic boundaries from their definition (test infrastructure, CPU, NumPy only).

The chosen-vector forms of tests/min_image_util.py's min_image_box / min_image_cell in the arithmetic include/loco_hd_hip.h prescribes
(the first strict minimum in SHIFTS27 order), the model sensitivity -- tests/dense_sensitivity_util.from_dmxs (longdouble) on the
min_image_matrix rows, with disp looked up per slot --, the model gradient from disp, and a central-difference helper.

Measured (tests/test_min_image_sensitivity_model.py): the model's gradient against central differences (h = 1e-4) of the model's own
score deviates by at most FD_MEASURED over its cases; 4 x that is FD_BOUND, the bound of the GPU test's difference quotients (the factor
covers the library's f64 against the model's long double), the convention of tests/periodic_sensitivity_util.py.
"""
from __future__ import annotations

import itertools
from collections import namedtuple

import numpy as np

import dense_sensitivity_util as du
from integral_form import LD
from min_image_util import SHIFTS27, min_image_matrix, norm3
from periodic_cell_util import CELLS
from periodic_sensitivity_util import H_STEP

MSens = namedtuple("MSens", "scores count_a idx_a dist_a g_a disp_a count_b idx_b dist_b g_b disp_b")
FD_MEASURED = 1.33e-9  # largest |model gradient - central difference| of tests/test_min_image_sensitivity_model.py (the 4-term hyper_exp case)
FD_BOUND = 4 * FD_MEASURED


def is_diagonal(m):
    m = np.asarray(m, dtype=np.float64)
    return np.count_nonzero(m - np.diag(np.diagonal(m))) == 0


def min_image_box_vec(d, box):
    """d [..., 3] displacements, box (Lx, Ly, Lz): w = d - L rint(d / L) per axis."""
    box = np.asarray(box, dtype=np.float64)
    return d - box * np.rint(d / box)


def min_image_cell_vec(d, reduced, inverse):
    """d [..., 3]; reduced / inverse from lchd_cell_reduce: the first of the 27 candidates, in SHIFTS27 order, with the smallest
    (wx wx + wy wy) + wz wz -- an update on strict < only."""
    R, I = np.asarray(reduced, dtype=np.float64), np.asarray(inverse, dtype=np.float64)
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    f = [(dx * I[0, k] + dy * I[1, k]) + dz * I[2, k] for k in range(3)]
    f = [fk - np.rint(fk) for fk in f]
    v = [(f[0] * R[0, c] + f[1] * R[1, c]) + f[2] * R[2, c] for c in range(3)]
    best = np.full(d.shape[:-1], np.inf)
    chosen = np.zeros(d.shape)
    for i, j, k in SHIFTS27:
        w = np.stack([v[c] + ((float(i) * R[0, c] + float(j) * R[1, c]) + float(k) * R[2, c]) for c in range(3)], axis=-1)
        d2 = (w[..., 0] * w[..., 0] + w[..., 1] * w[..., 1]) + w[..., 2] * w[..., 2]
        better = d2 < best
        best = np.where(better, d2, best)
        chosen = np.where(better[..., None], w, chosen)
    return chosen


def disp_matrix(x, box=None, cell=None, reduce=None):
    """[n][n][3]: entry (r, i) = the displacement from atom r to the nearest image of atom i = -w with d = x[r] - x[i]; an open
    structure (neither box nor cell): w = d.  `reduce` is loco_hd_amd.api.cell_reduce (needed for a cell)."""
    x = np.asarray(x, dtype=np.float64)
    d = x[:, None, :] - x[None, :, :]
    if box is not None:
        return -min_image_box_vec(d, box)
    if cell is None:
        return -d
    reduced, inverse = reduce(cell)
    if is_diagonal(reduced):
        return -min_image_box_vec(d, np.diagonal(reduced))
    return -min_image_cell_vec(d, reduced, inverse)


def rows_matrix(x, box=None, cell=None, reduce=None):
    """The rows the call scores: min_image_matrix, or for an open structure the rows of from_coords."""
    if box is None and cell is None:
        return du.coords_rows(x)
    return min_image_matrix(np.asarray(x, dtype=np.float64), box=box, cell=cell, reduce=reduce)


def brute_disp(x, cell, span=3):
    """(disp [n][n][3], unique [n][n]): the nearest image by brute force over the shifts -span .. span of the caller's cell applied to
    the displacement moved to within half a cell, and whether it is the only one at that distance (to 1e-9)."""
    x, cell = np.asarray(x, dtype=np.float64), np.asarray(cell, dtype=np.float64)
    d = x[None, :, :] - x[:, None, :]  # member - row atom
    d = d - np.rint(d @ np.linalg.inv(cell)) @ cell
    cands = np.stack([d + np.asarray(s, dtype=np.float64) @ cell for s in itertools.product(range(-span, span + 1), repeat=3)])
    norms = norm3(cands)
    pick = np.argmin(norms, axis=0)
    best = np.take_along_axis(norms, pick[None], 0)[0]
    unique = (norms <= best + 1e-9).sum(axis=0) == 1
    return np.take_along_axis(cands, pick[None, ..., None], 0)[0], unique


def sensitivity(cat_a, xyz_a, per_a, cat_b, xyz_b, per_b, n_categories, wf, sd=("Hellinger", [2.0]), category_weights=None, width=None,
                reduce=None):
    """The MSens tuple LoCoHD.sensitivity_from_coords_periodic returns; per_x: None (open), ("box", L) or ("cell", M)."""
    kw = [{} if per is None else {per[0]: np.asarray(per[1], dtype=np.float64)} for per in (per_a, per_b)]
    rows = [rows_matrix(x, reduce=reduce, **k) for x, k in ((xyz_a, kw[0]), (xyz_b, kw[1]))]
    s = du.from_dmxs(cat_a, rows[0], cat_b, rows[1], n_categories, wf, sd, category_weights, width)
    disp = []
    for x, k, idx in ((xyz_a, kw[0], s.idx_a), (xyz_b, kw[1], s.idx_b)):
        full = disp_matrix(x, reduce=reduce, **k)
        real = idx >= 0
        at = np.where(real, idx, 0)
        disp.append(np.where(real[..., None], full[np.arange(len(idx))[:, None], at], 0.0))
    return MSens(s.scores, s.count_a, s.idx_a, s.dist_a, s.g_a, disp[0], s.count_b, s.idx_b, s.dist_b, s.g_b, disp[1])


def scores(cat_a, xyz_a, per_a, cat_b, xyz_b, per_b, n_categories, wf, sd=("Hellinger", [2.0]), reduce=None):
    return sensitivity(cat_a, xyz_a, per_a, cat_b, xyz_b, per_b, n_categories, wf, sd, reduce=reduce).scores


def gradient(ms, pair_weights=None):
    """(grad_a, grad_b), longdouble sums term by term over the rows of an MSens: member += v g disp / d, row atom -= the same; slot 0,
    members at d == 0 and non-finite g are skipped."""
    n = len(ms.scores)
    v = np.ones(n) if pair_weights is None else np.asarray(pair_weights, dtype=np.float64)
    out = []
    for cnt, idx, dist, g, disp in ((ms.count_a, ms.idx_a, ms.dist_a, ms.g_a, ms.disp_a), (ms.count_b, ms.idx_b, ms.dist_b, ms.g_b, ms.disp_b)):
        grad = np.zeros((n, 3), dtype=LD)
        for r in range(n):
            for k in range(1, int(cnt[r])):
                if dist[r, k] > 0.0 and np.isfinite(g[r, k]):
                    step = LD(v[r]) * LD(g[r, k]) / LD(dist[r, k]) * disp[r, k].astype(LD)
                    grad[idx[r, k]] += step
                    grad[r] -= step
        out.append(grad.astype(np.float64))
    return out[0], out[1]


def central_difference(xyz_a, xyz_b, side, atom, score_fn, pair_weights=None, step=H_STEP):
    """d sum_r v_r S_r / d x[atom] of side `side` (0 / 1) by central differences of score_fn(xyz_a, xyz_b) -> scores [n]."""
    v = np.ones(len(xyz_a)) if pair_weights is None else np.asarray(pair_weights, dtype=np.float64)
    out = np.zeros(3)
    for d in range(3):
        val = []
        for sign in (+1.0, -1.0):
            moved = [np.array(xyz_a, dtype=np.float64), np.array(xyz_b, dtype=np.float64)]
            moved[side][atom, d] += sign * step
            val.append(float(np.dot(v, np.asarray(score_fn(moved[0], moved[1]), dtype=np.float64))))
        out[d] = (val[0] - val[1]) / (2 * step)
    return out


def quiet_atoms(side, xyz_a, per_a, xyz_b, per_b, reduce, how_many, margin=0.05, gap=4 * H_STEP):
    """Atoms of side `side` (0 / 1) at which the score is smooth over a step of H_STEP: every minimum-image vector of the atom is unique
    by `margin` (no image tie, no half-cell separation; an open side has none), and no distance the atom's move changes -- its own
    row, and its column in every other row -- comes within `gap` of another event of the same row pair (no change of order)."""
    xyz, per = ((xyz_a, per_a), (xyz_b, per_b))[side]
    x = np.asarray(xyz, dtype=np.float64)
    n = len(x)
    ok = np.ones(n, dtype=bool)
    if per is not None:
        cell = np.diag(per[1]) if per[0] == "box" else np.asarray(per[1])
        d = x[None, :, :] - x[:, None, :]
        d = d - np.rint(d @ np.linalg.inv(cell)) @ cell
        cands = np.stack([norm3(d + np.asarray(s, dtype=np.float64) @ cell) for s in itertools.product(range(-2, 3), repeat=3)])
        two = np.sort(cands, axis=0)[:2]
        clear = (two[1] - two[0] > margin) | np.eye(n, dtype=bool)
        ok &= clear.all(axis=1) & clear.all(axis=0)
    rows = [rows_matrix(xx, reduce=reduce, **({} if pp is None else {pp[0]: np.asarray(pp[1], dtype=np.float64)}))
            for xx, pp in ((xyz_a, per_a), (xyz_b, per_b))]
    for i in np.flatnonzero(ok):
        for r in range(n):
            events = np.concatenate([rows[0][r], rows[1][r]])
            moved = np.zeros(2 * n, dtype=bool)
            moved[side * n: side * n + n] = (np.arange(n) != i) if r == i else (np.arange(n) == i)  # (entry (i, i) stays 0)
            diff = np.abs(events[moved][:, None] - events[None, :])
            diff[np.arange(moved.sum()), np.flatnonzero(moved)] = np.inf
            if diff.min() <= gap:
                ok[i] = False
                break
    return [int(i) for i in np.flatnonzero(ok)][:how_many]


# ---- the gradient cases the CPU and GPU tests share ----------------------------------------------------------------------------------
GRAD_WF = ("hyper_exp", [1.0, 0.5, 0.2, 0.05])
GRAD_N = 24
GRAD_PERIODS = {"open": None, "box": ("box", np.asarray([12.0, 10.5, 13.25])), "skewed": ("cell", CELLS["skewed"] * 0.55),
                "dodecahedron": ("cell", CELLS["dodecahedron"] * 0.55)}
GRAD_MIXES = [("skewed", "box"), ("dodecahedron", "open")]


def structure(seed, n, per, n_cat=4, spread=(-1.0, 2.0)):
    """(cat, xyz): n atoms spread over three cells a side, unwrapped (an open side: inside a cube of the box's size)."""
    rng = np.random.default_rng(seed)
    cell = np.diag(GRAD_PERIODS["box"][1]) if per is None else (np.diag(per[1]) if per[0] == "box" else np.asarray(per[1]))
    u = rng.uniform(0.0, 1.0, (n, 3)) if per is None else rng.uniform(spread[0], spread[1], (n, 3))
    return rng.integers(0, n_cat, n), u @ cell


def gradient_case(mix, reduce):
    """(cat_a, xyz_a, per_a, cat_b, xyz_b, per_b, row weights in [0.5, 1], [(side, atom)] where the score is smooth over H_STEP)."""
    per_a, per_b = GRAD_PERIODS[mix[0]], GRAD_PERIODS[mix[1]]
    ca, xa = structure(61, GRAD_N, per_a)
    cb, xb = structure(62, GRAD_N, per_b)
    v = np.random.default_rng(6).uniform(0.5, 1.0, GRAD_N)
    picks = [(0, i) for i in quiet_atoms(0, xa, per_a, xb, per_b, reduce, 2)] + [(1, i) for i in quiet_atoms(1, xa, per_a, xb, per_b, reduce, 1)]
    return ca, xa, per_a, cb, xb, per_b, v, picks
