"""Neighbour sensitivities under periodic boundaries from their definition (test infrastructure, CPU, NumPy only).

The periodic image cloud of a structure is built on the host by the contract of include/loco_hd_hip.h ("periodic boundaries"), as
image_cloud / image_cloud_cell of tests/test_gpu_periodic.py / tests/test_gpu_periodic_cell.py do, and additionally every slot's source
atom (`origin`) and image code (`code` = c0 + 3 c1 + 9 c2; c: 0 original, 1 plus, 2 minus).  tests/sensitivity_util.from_primitives
(longdouble) runs on those arrays as on any open structure; its lists index the image cloud and are mapped back here:
idx -> origin[idx], image = code[idx], disp = x_img[idx] - x_img[anchor].  The gradient is accumulated from those alone.

Measured (tests/test_periodic_sensitivity_model.py): the model's gradient against central differences (h = 1e-4) of the model's own
periodic score deviates by at most 2.7e-11 over its cases; 4 x that is FD_BOUND, the bound of the GPU test's difference quotients.
"""
from __future__ import annotations

import itertools
from collections import namedtuple

import numpy as np

import sensitivity_util as su
from integral_form import LD
from periodic_cell_util import CELLS, widths

PSens = namedtuple("PSens", "scores count_a idx_a image_a dist_a g_a disp_a count_b idx_b image_b dist_b g_b disp_b")
COEF = (0.0, 1.0, -1.0)  # per-axis choice 0 original, 1 plus, 2 minus
CODES = [(c0, c1, c2) for c2 in range(3) for c1 in range(3) for c0 in range(3)][1:]  # ascending image code c0 + 3 c1 + 9 c2
UNI = ("uniform", [3.0, 10.0])
CATS7 = [f"c{k}" for k in range(7)]
THR = 10.0
BOX32 = (32.0, 32.0, 32.0)
THIN = (12.0, 40.0, 40.0)
H_STEP = 1e-4
FD_MEASURED = 2.7e-11  # largest |model gradient - central difference| of tests/test_periodic_sensitivity_model.py
FD_BOUND = 4 * FD_MEASURED
PERIODS = {"box": ("box", BOX32), "thin": ("box", THIN), "skewed": ("cell", CELLS["skewed"]), "dodecahedron": ("cell", CELLS["dodecahedron"]),
           "open": None}


# ---- the contract -----------------------------------------------------------------------------------------------------------------
def wrap_box(x, box):
    box = np.asarray(box, dtype=np.float64)
    w = x - np.floor(x / box) * box
    return np.where(w == box, 0.0, w)


def shift(cell, c0, c1, c2):
    """t = i a + j b + k c per component as (i a[d] + j b[d]) + k c[d]."""
    return (COEF[c0] * cell[0] + COEF[c1] * cell[1]) + COEF[c2] * cell[2]


def frac(x, cell):
    return np.asarray(x) @ np.linalg.inv(cell)


def wrap_cell(x, cell):
    f = np.floor(frac(x, cell))
    return x - ((f[:, :1] * cell[0] + f[:, 1:2] * cell[1]) + f[:, 2:] * cell[2])


def _ghosts(w, plus, minus, image_of):
    xyz, origin, code = [], [], []
    for i in range(len(w)):
        ok = [(True, plus[i, k], minus[i, k]) for k in range(3)]
        for c0, c1, c2 in CODES:
            if ok[0][c0] and ok[1][c1] and ok[2][c2]:
                xyz.append(image_of(i, c0, c1, c2))
                origin.append(i)
                code.append(c0 + 3 * c1 + 9 * c2)
    return (np.concatenate([w, np.asarray(xyz, dtype=np.float64).reshape(-1, 3)]), np.concatenate([np.arange(len(w)), origin]).astype(np.int32),
            np.concatenate([np.zeros(len(w)), code]).astype(np.int8))


def image_cloud(w, box, reach):
    """(xyz, origin, code) of the image cloud of the WRAPPED atoms w in an orthorhombic box: the originals, then per atom its ghosts in
    ascending image code; w + L exists iff w < reach, w - L iff w >= L - reach."""
    box = np.asarray(box, dtype=np.float64)
    return _ghosts(w, w < reach, w >= box - reach, lambda i, *c: [(w[i, k], w[i, k] + box[k], w[i, k] - box[k])[c[k]] for k in range(3)])


def image_cloud_cell(p, cell, reach):
    """The same in a triclinic cell (rows a, b, c): along axis k, p + a_k exists iff g_k w_k < reach, p - a_k iff (1 - g_k) w_k <= reach."""
    g, w = frac(p, cell), widths(cell)
    return _ghosts(p, g * w < reach, (1.0 - g) * w <= reach, lambda i, c0, c1, c2: p[i] + shift(cell, c0, c1, c2))


def images(x, per, reach, wrapped=None):
    """(xyz, origin, code) of what a pass searches for a structure: per = None (open: the structure itself), ("box", L) or ("cell", M).
    wrapped: the wrapped originals to build from (a device's own, for bit-exact comparisons in a cell) instead of wrapping x here."""
    x = np.asarray(x, dtype=np.float64)
    if per is None:
        return x, np.arange(len(x), dtype=np.int32), np.zeros(len(x), dtype=np.int8)
    if per[0] == "box":
        return image_cloud(wrap_box(x, per[1]) if wrapped is None else wrapped, per[1], reach)
    return image_cloud_cell(wrap_cell(x, per[1]) if wrapped is None else wrapped, per[1], reach)


def image_of(w, per, origin, code):
    """The coordinates of image `code` of wrapped atom `origin`, by the contract's expression."""
    c = (int(code) % 3, int(code) // 3 % 3, int(code) // 9)
    if code == 0:
        return w[origin]
    if per[0] == "box":
        return np.asarray([(w[origin, k], w[origin, k] + per[1][k], w[origin, k] - per[1][k])[c[k]] for k in range(3)])
    return w[origin] + shift(np.asarray(per[1]), *c)


# ---- the model ----------------------------------------------------------------------------------------------------------------------
def from_primitives(a, per_a, b, per_b, pairs, thr, n_categories, wf=UNI, sd=("Hellinger", [2.0]), category_weights=None, accept_same=True,
                    width=None, wrapped=(None, None)):
    """The PSens tuple LoCoHD.sensitivity_from_primitives_periodic returns; a / b: (xyz, cat, tag)."""
    img = [images(s[0], per, thr, w) for s, per, w in ((a, per_a, wrapped[0]), (b, per_b, wrapped[1]))]
    lab = [(np.asarray(s[1])[o], np.asarray(s[2])[o]) for s, (_, o, _) in zip((a, b), img)]
    s = su.from_primitives(lab[0][0], img[0][0], lab[0][1], lab[1][0], img[1][0], lab[1][1], pairs, thr, n_categories, wf, sd, category_weights,
                           accept_same, width)
    sides = []
    for (xyz, origin, code), cnt, idx, dist, g in ((img[0], s.count_a, s.idx_a, s.dist_a, s.g_a), (img[1], s.count_b, s.idx_b, s.dist_b, s.g_b)):
        real = idx >= 0
        at = np.where(real, idx, 0)
        disp = np.where(real[..., None], xyz[at] - xyz[at[:, :1]], 0.0)
        disp[:, 0] = 0.0
        sides.append((cnt, np.where(real, origin[at], -1).astype(np.int32), np.where(real, code[at], 0).astype(np.int8), dist, g, disp))
    return PSens(s.scores, *sides[0], *sides[1])


def scores(a, per_a, b, per_b, pairs, thr, n_categories, wf=UNI, sd=("Hellinger", [2.0])):
    return from_primitives(a, per_a, b, per_b, pairs, thr, n_categories, wf, sd).scores


def gradient(ps, n_a, n_b, pair_weights=None):
    """(grad_a, grad_b), longdouble sums over the rows of a PSens: source atom += v g disp / d, anchor -= the same; d == 0 skipped."""
    v = np.ones(len(ps.scores)) if pair_weights is None else np.asarray(pair_weights, dtype=np.float64)
    out = []
    for n, cnt, idx, dist, g, disp in ((n_a, ps.count_a, ps.idx_a, ps.dist_a, ps.g_a, ps.disp_a), (n_b, ps.count_b, ps.idx_b, ps.dist_b, ps.g_b, ps.disp_b)):
        grad = np.zeros((n, 3), dtype=LD)
        for p in range(len(cnt)):
            for k in range(1, int(cnt[p])):
                if dist[p, k] > 0.0:
                    step = LD(v[p]) * LD(g[p, k]) / LD(dist[p, k]) * disp[p, k].astype(LD)
                    grad[idx[p, k]] += step
                    grad[idx[p, 0]] -= step
        out.append(grad.astype(np.float64))
    return out[0], out[1]


def central_difference(a, per_a, b, per_b, pairs, thr, n_categories, side, atom, score_fn, pair_weights=None, step=H_STEP):
    """d sum_p v_p S_p / d x[atom] of side `side` (0 / 1) by central differences of score_fn(a, per_a, b, per_b, pairs, thr)."""
    v = np.ones(len(pairs)) if pair_weights is None else np.asarray(pair_weights, dtype=np.float64)
    out = np.zeros(3)
    for d in range(3):
        val = []
        for sign in (+1.0, -1.0):
            moved = [(np.array(s[0], dtype=np.float64), s[1], s[2]) for s in (a, b)]
            moved[side][0][atom, d] += sign * step
            val.append(float(np.dot(v, score_fn(moved[0], per_a, moved[1], per_b, pairs, thr))))
        out[d] = (val[0] - val[1]) / (2 * step)
    return out


# ---- the cases the CPU and GPU tests share --------------------------------------------------------------------------------------------
def side(seed, n, per, n_cat=7, n_tag=3):
    """(xyz, cat, tag): n atoms uniform in the side's box / cell (an open side: in a 32^3 cube)."""
    rng = np.random.default_rng(seed)
    u = rng.uniform(0.0, 1.0, (n, 3))
    xyz = u * np.asarray(BOX32) if per is None else (u * np.asarray(per[1]) if per[0] == "box" else u @ np.asarray(per[1]))
    return xyz, rng.integers(0, n_cat, n).astype(np.int32), rng.integers(0, n_tag, n).astype(np.int32)


RANDOM_SIDES = {"box/box": ("box", "box"), "box/open": ("box", "open"), "open/cell": ("open", "skewed"), "cell/cell": ("dodecahedron", "dodecahedron")}
SEED_A, SEED_B, SEED_PAIRS, SEED_THIN = 701, 702, 17, 5
N_RANDOM, N_THIN = 300, 120


def random_case(name):
    """(a, per_a, b, per_b, pairs) of one of the four random cases: about 300 atoms a side, 30 pairs."""
    pa, pb = (PERIODS[k] for k in RANDOM_SIDES[name])
    rng = np.random.default_rng(SEED_PAIRS)
    return side(SEED_A, N_RANDOM, pa), pa, side(SEED_B, N_RANDOM, pb), pb, [(int(i), int(j)) for i, j in rng.integers(0, N_RANDOM, (30, 2))]


def fd_atoms(case):
    """Three (side, atom) of a random case: anchors of its pairs with a nonzero gradient, the first within the threshold of a face."""
    a, per_a, b, per_b, pairs = random_case(case)
    ps = from_primitives(a, per_a, b, per_b, pairs, THR, 7)
    grads = gradient(ps, len(a[0]), len(b[0]))
    side = 0 if per_a is not None else 1
    s, per = ((a, per_a), (b, per_b))[side]
    w = images(s[0], per, THR)[0][: len(s[0])]
    g = frac(w, np.diag(per[1]) if per[0] == "box" else per[1])
    near = np.min(np.minimum(g, 1.0 - g) * (np.asarray(per[1]) if per[0] == "box" else widths(per[1])), axis=1) < THR
    moving = np.flatnonzero(np.abs(grads[side]).sum(1) > 0)
    rim = [int(i) for i in moving if near[i]]
    assert rim, "no moving atom near a face"
    picks = [(side, rim[0])] + [(side, int(i)) for i in moving if int(i) != rim[0]][:1]
    other = np.flatnonzero(np.abs(grads[1 - side]).sum(1) > 0)
    return picks + [(1 - side, int(other[0]))], grads


def thin_case():
    """The thin box (12, 40, 40): every atom with 2 <= x < 10 has both images along x."""
    per = PERIODS["thin"]
    rng = np.random.default_rng(SEED_THIN + 1)
    return side(SEED_THIN, N_THIN, per), per, side(SEED_THIN + 7, N_THIN, per), per, [(int(i), int(j)) for i, j in rng.integers(0, N_THIN, (12, 2))]


def twice(ps):
    """[(pair, side, source atom)] where one source atom sits in one list under two different image codes."""
    found = []
    for s, (cnt, idx, image) in enumerate(((ps.count_a, ps.idx_a, ps.image_a), (ps.count_b, ps.idx_b, ps.image_b))):
        for p in range(len(cnt)):
            seen = {}
            for k in range(int(cnt[p])):
                seen.setdefault(int(idx[p, k]), set()).add(int(image[p, k]))
            found += [(p, s, i) for i, codes in sorted(seen.items()) if len(codes) > 1]
    return found


def lattice_case():
    """3 x 3 x 3 lattice of spacing 4 that fills the box 12^3, both sides identical: ties at every distance, between home atoms and ghosts too."""
    i = np.arange(27)
    xyz = np.stack([i % 3, (i // 3) % 3, i // 9], 1) * 4.0
    s = (xyz, (i % 7).astype(np.int32), np.zeros(27, dtype=np.int32))
    per = ("box", (12.0, 12.0, 12.0))
    return s, per, s, per, [(0, 0), (13, 13), (26, 26), (5, 5)]


def tie_order_ok(ps):
    """Among exact ties of a list (slot 0 aside): home atoms before ghosts, then source index, then image code."""
    ties = 0
    for cnt, idx, image, dist in ((ps.count_a, ps.idx_a, ps.image_a, ps.dist_a), (ps.count_b, ps.idx_b, ps.image_b, ps.dist_b)):
        for p in range(len(cnt)):
            keys = [(dist[p, k], image[p, k] != 0, idx[p, k], image[p, k]) for k in range(1, int(cnt[p]))]
            assert keys == sorted(keys)
            for (d0, g0, *_), (d1, g1, *_) in itertools.pairwise(keys):
                ties += d0 == d1 and g0 != g1
    return ties


def tie_groups_cancel(ps, tol):
    """Identical sides: the members of both lists at one distance enter one at a time (side A first), so g_a and g_b do not cancel slot
    by slot where a side has several members at that distance; over the whole group they do: H is 0 in front of it and behind it."""
    worst = 0.0
    for p in range(len(ps.scores)):
        na, nb = int(ps.count_a[p]), int(ps.count_b[p])
        for d in np.unique(ps.dist_a[p, 1:na]):
            total = ps.g_a[p, 1:na][ps.dist_a[p, 1:na] == d].sum() + ps.g_b[p, 1:nb][ps.dist_b[p, 1:nb] == d].sum()
            worst = max(worst, abs(float(total)))
    assert worst <= tol, worst
    return worst
