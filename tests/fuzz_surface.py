"""The draw and the CPU references of the whole-surface fuzz (tests/test_gpu_fuzz_surface.py; checked on their own, without a device, by
tests/test_fuzz_surface_draw.py).  No device and no product scoring code is touched here.

draw(seed) is a plain function of the seed.  The driver follows a fixed rotation of the seed (SLOTS), and so do the axes whose
combinations the default 40 seeds must reach: the boundary, the cell kind of from_primitives, the threshold equal to the width
(one from_primitives visit in eight, on a period that shares no factor with the boundaries'), category counts at the byte boundary,
the old category counts and the number of structures of an ensemble.  Everything else is drawn from the seed's own generator, each
axis on its own.  Weight functions and statistical distances keep the ranges of tests/test_gpu_fuzz.py (the reference's generator
is cited there).

expected(case, oracle) scores the case with the CPU oracle through code that shares no periodic arithmetic with the library:

    open cases            the oracle's own driver (sampled rows of the stably sorted distance rows for ensembles and ragged rows)
    periodic prims        image_cloud(): every atom wrapped into the cell by whole lattice vectors, then its images at the shifts
                          -1 .. 1, home images first (anchor indices stay), tags and categories copied; the oracle's OPEN
                          from_primitives on that cloud
    periodic dense rows   min_image_util.brute_rows (brute force over the shifts of the caller's unreduced cell) on at most 24 sampled
                          rows per structure, rows 0 and n - 1 always, scored by dense_rows_util.oracle_rows
    ensembles             the same per structure pair; excluded entries are +inf in the rows before they are scored

integral_check(case, oracle) feeds the same clouds / rows to tests/integral_form.py, a differently shaped computation of the score.
"""
import itertools

import numpy as np

from dense_rows_util import oracle_rows
from min_image_util import brute_rows, norm3
from periodic_cell_util import CELLS, widths
from test_gpu_fuzz import draw_sd, draw_wf

DRIVERS = ["prims", "prims_batch", "coords", "dmxs", "dmxs_ragged", "coords_ensemble", "dmxs_ensemble"]
# The driver of seed s is SLOTS[s % 9] (9 shares no factor with the seed classes of the environment hooks, s % 2 and s % 4);
# from_primitives, the driver with the most axes of its own, has every third seed, as it has three draws in five in test_gpu_fuzz.py.
SLOTS = ["prims", "prims_batch", "coords", "prims", "dmxs", "coords_ensemble", "prims", "dmxs_ragged", "dmxs_ensemble"]
PRIMS_BOUNDARIES = ["open", "box", "cell", "mixed", "cell"]  # by the visit v = s // 3: five long, so that it meets the period of 8 below everywhere
PRIMS_BIG_CATS = [254, 257, 255, 300, 256]                   # on even visits: 16-bit ids meet a cell (v = 2) and a box (v = 6) image cloud
BOUNDARIES = {"prims": ["open", "box", "cell", "mixed"], "coords": ["open", "box", "cell", "mixed"], "coords_ensemble": ["open", "box", "cell"]}
SESSION_DRIVERS = ("prims", "prims_batch", "coords", "coords_ensemble")  # what DeviceSession offers
DICT_DRIVERS = tuple(d for d in DRIVERS if d != "prims_batch")           # from_primitives_batch takes a single weight function
ENSEMBLES = ("coords_ensemble", "dmxs_ensemble")
OLD_CATS = [2, 3, 5, 7, 10, 13, 20, 25, 31, 40]
BIG_CATS = [254, 255, 256, 257, 300]  # the byte and 16-bit category boundary
CELL_KINDS = ["skewed", "dodecahedron", "diagonal"]
MAX_ROWS = 24
STREAM = 434000  # the generator of seed s is default_rng(STREAM + s); chosen so that the default seeds cover what test_fuzz_surface_draw.py lists


# ---- geometry ---------------------------------------------------------------------------------------------------------------------
def is_orthorhombic(per):
    cell = cell_of(per)
    return np.count_nonzero(cell - np.diag(np.diagonal(cell))) == 0


def cell_of(per):
    """The 3 x 3 cell of a side's boundary ("box", L) / ("cell", M)."""
    return np.diag(per[1]) if per[0] == "box" else np.asarray(per[1], dtype=np.float64)


def reach_of(per):
    """The largest legal threshold of a side: the smallest edge / perpendicular width, the very number the library validates against."""
    return float(np.min(per[1])) if per[0] == "box" else float(np.min(widths(per[1])))


def draw_box(rng):
    side = rng.uniform(14.0, 34.0)
    return ("box", side * np.asarray([1.0, 0.9, 1.1]))


def draw_cell(rng, kind=None):
    kind = str(rng.choice(CELL_KINDS)) if kind is None else kind
    if kind == "diagonal":  # an orthorhombic box passed as a cell
        return ("cell", np.diag(draw_box(rng)[1])), kind
    return ("cell", np.array(CELLS[kind])), kind


def draw_sides(rng, boundary, kind=None):
    """(side A, side B, name of the cell kind or None) for a two-sided call; `kind`: the cell kind where the caller rotates it."""
    if boundary == "open":
        return None, None, None
    if boundary == "box":
        box = draw_box(rng)
        return box, box, None
    if boundary == "cell":
        cell, kind = draw_cell(rng, kind)
        return cell, cell, kind
    cell, kind = draw_cell(rng, kind)  # mixed sides
    return (draw_box(rng), cell, kind) if rng.random() < 0.5 else (cell, None, kind)


def cloud_in(rng, n, cell, unwrapped, lattice):
    x = rng.uniform(-2.0, 2.0, (n, 3)) @ cell if unwrapped else rng.uniform(0.0, 1.0, (n, 3)) @ cell
    return np.round(x) if lattice else x  # (a rounded coordinate may leave the cell by less than one unit)


def rule_accepts(rule, t0, t1):
    """tag_pairing_rule.rs:49-75 for the anchor's tag t0 and a point's tag t1 (None: the constructor's default, accept_same)."""
    if rule is None:
        return t0 == t1
    if "accept_same" in rule:
        return (t0 == t1) == rule["accept_same"]
    hit = (t0, t1) in rule["tag_pairs"] or (not rule["ordered"] and (t1, t0) in rule["tag_pairs"])
    return hit == rule["accepted_pairs"]


def plant_neighbour(rng, x, tags, rule, anchor, cell, unwrapped):
    """Put the anchor just inside the face g0 = 0 of its cell and one atom the tag rule accepts just inside the opposite face: the
    anchor then sees that atom's image 0.06 |a| away (|a| < 3.3 widths in every cell drawn, the threshold is >= 0.2 widths), which
    the open call on the same input does not.  Without it a one-pair case with a short threshold could be a legitimately open one."""
    others = [j for j in range(len(x)) if j != anchor and rule_accepts(rule, tags[anchor], tags[j])]
    if not others:
        return
    j = others[int(rng.integers(len(others)))]
    u, v = rng.uniform(0.3, 0.7, 2)
    lift = (lambda: rng.integers(-2, 3, 3).astype(float)) if unwrapped else (lambda: np.zeros(3))
    x[anchor] = (np.asarray([0.03, u, v]) + lift()) @ cell
    x[j] = (np.asarray([0.97, u + 0.01, v - 0.01]) + lift()) @ cell


# ---- the draw ---------------------------------------------------------------------------------------------------------------------
def draw(seed):
    seed = int(seed)
    slot, j = seed % len(SLOTS), seed // len(SLOTS)
    driver = SLOTS[slot]
    v = seed // 3 if driver == "prims" else j  # the driver's visit
    rng = np.random.default_rng(STREAM + seed)
    bounds = PRIMS_BOUNDARIES if driver == "prims" else BOUNDARIES.get(driver, ["open"])
    case = {"seed": seed, "driver": driver, "boundary": bounds[(v + slot) % len(bounds)] if driver != "prims" else bounds[v % len(bounds)]}
    case["det"] = bool(rng.random() < 0.5)
    case["entry"] = "session" if driver in SESSION_DRIVERS and rng.random() < 0.5 else "host"
    if driver == "prims":
        ncat = PRIMS_BIG_CATS[(v // 2) % len(PRIMS_BIG_CATS)] if v % 2 == 0 else OLD_CATS[(3 * seed) % len(OLD_CATS)]
    else:  # every other visit of a driver at the byte boundary, the old counts in rotation
        ncat = BIG_CATS[(seed // 2) % len(BIG_CATS)] if v % 2 == 1 else OLD_CATS[(3 * seed) % len(OLD_CATS)]
    case["ncat"], case["cats"] = ncat, [f"t{i}" for i in range(ncat)]
    case["weights"] = None if rng.random() < 0.6 else rng.uniform(0.2, 3.0, ncat).tolist()
    case["multi"] = bool(driver in DICT_DRIVERS and rng.random() < 0.45)
    if case["multi"]:
        case["wfs"] = {f"k{i}": draw_wf(rng) for i in range(int(rng.integers(2, 5)))}
    else:
        case["wfs"] = draw_wf(rng)
    case["sd"] = draw_sd(rng)
    case["lattice"] = bool(rng.random() < 0.3)  # lattice coordinates: many exact distance ties
    case["unwrapped"] = bool(rng.random() < 0.5)

    def names(n):
        seq = rng.choice(case["cats"], n).tolist()
        seq[int(rng.integers(n))] = case["cats"][-1]  # the highest category id occurs
        return seq

    def keys(n):
        return [f"k{int(i)}" for i in rng.integers(0, len(case["wfs"]), n)] if case["multi"] else None

    def open_cloud(n, box):
        x = rng.uniform(-box, box, (n, 3))
        return np.round(x) if case["lattice"] else x

    if driver in ("prims", "prims_batch"):
        tag_kind = int(rng.integers(0, 4))
        case["rule"] = [{"accept_same": True}, {"accept_same": False},
                        {"tag_pairs": {(f"r{a}", f"r{b}") for a in range(0, 20) for b in range(0, 100, 7)},
                         "accepted_pairs": bool(rng.integers(0, 2)), "ordered": bool(rng.integers(0, 2))}, None][tag_kind]

        def tags(n):  # accept_same=True with distinct tags would empty most environments; use uniform tags instead
            return [""] * n if tag_kind == 0 else [f"r{i // 4}" for i in range(n)]

    if driver == "prims":
        na, nb = int(rng.integers(20, 400)), int(rng.integers(20, 400))
        npairs = int(rng.integers(1, 300))
        case["sa"], case["sb"], case["tags_a"], case["tags_b"] = names(na), names(nb), tags(na), tags(nb)
        case["pairs"] = [(int(a), int(b)) for a, b in zip(rng.integers(0, na, npairs), rng.integers(0, nb, npairs))]
        case["keys"] = keys(npairs)
        per_a, per_b, case["cell_kind"] = draw_sides(rng, case["boundary"], CELL_KINDS[(v // 2) % len(CELL_KINDS)])
        case["per_a"], case["per_b"] = per_a, per_b
        if case["boundary"] == "open":
            box = float(rng.uniform(6.0, 40.0))
            case["xa"], case["xb"] = open_cloud(na, box), open_cloud(nb, box)
            case["thr"] = float("inf") if rng.random() < 0.1 else float(rng.uniform(0.3, 1.5) * box)
            case["at_width"] = False
        else:
            reach = min(reach_of(p) for p in (per_a, per_b) if p is not None)
            # one visit in eight: the width itself, the largest legal reach.  Eight and the five boundaries of PRIMS_BOUNDARIES share no
            # factor, so the width meets every boundary in turn (v = 1 a box, v = 9 a cell -- a dodecahedron -- v = 17 a cell, v = 33 mixed sides)
            case["at_width"] = v % 8 == 1
            case["thr"] = reach if case["at_width"] else float(rng.uniform(0.2, 1.0) * reach)
            if case["thr"] > reach:  # (0.2, 1.0] x the smallest width
                case["thr"] = reach
            # At a threshold equal to a box edge every anchor has an image of ITSELF at the threshold exactly (in a skewed cell the
            # lattice vectors are longer than the widths); which side of it a rounded sum falls on is pinned only while both sides
            # round the same coordinates, so an ORTHORHOMBIC side of such a case keeps its atoms inside the box, where wrapping changes
            # nothing.  A triclinic side at its width is drawn wrapped or unwrapped, on or off the lattice, like any other.
            xs, case["inside"] = [], []
            for n, per, tg, col in ((na, per_a, case["tags_a"], 0), (nb, per_b, case["tags_b"], 1)):
                cell = cell_of(per if per is not None else (per_a or per_b))  # an open side fills the other side's cell
                inside = bool(case["at_width"] and per is not None and is_orthorhombic(per))
                case["inside"].append(inside)
                x = cloud_in(rng, n, cell, case["unwrapped"] and not inside, case["lattice"] and not inside)
                if per is not None:
                    plant_neighbour(rng, x, tg, case["rule"], case["pairs"][0][col], cell, case["unwrapped"] and not inside)
                xs.append(x)
            case["xa"], case["xb"] = xs
    elif driver == "prims_batch":
        m = int(rng.integers(3, 6))
        box = float(rng.uniform(6.0, 30.0))
        sizes = [int(rng.integers(20, 150)) for _ in range(m)]
        case["structs"] = [(names(n), tags(n), open_cloud(n, box)) for n in sizes]
        case["thr"] = float(rng.uniform(0.3, 1.5) * box)

        def some(a, b, k):
            return [(int(p), int(q)) for p, q in zip(rng.integers(0, sizes[a], k), rng.integers(0, sizes[b], k))]
        # as in test_from_primitives_batch_matches_single_calls: plain jobs, a reversed one, a structure against itself, a short and
        # an empty one
        case["jobs"] = [(0, 1, some(0, 1, int(rng.integers(1, 80)))), (0, 2, some(0, 2, int(rng.integers(1, 80)))),
                        (m - 1, 0, some(m - 1, 0, int(rng.integers(1, 60)))), (1, 1, [(i, i) for i in range(0, sizes[1], 3)]),
                        (m - 1, 1, some(m - 1, 1, 3)), (2, m - 1, [])]
    elif driver in ("coords", "dmxs", "dmxs_ragged"):
        na, nb = int(rng.integers(20, 400)), int(rng.integers(20, 400))
        n = min(na, nb) if driver != "dmxs_ragged" else min(na, nb, 64)  # (a ragged row costs the reference one oracle call)
        case["n"] = n
        if driver == "coords":
            per_a, per_b, case["cell_kind"] = draw_sides(rng, case["boundary"])
            case["per_a"], case["per_b"] = per_a, per_b
            case["sa"], case["sb"], case["keys"] = names(n), names(n), keys(n)
            if case["boundary"] == "open":
                box = float(rng.uniform(6.0, 40.0))
                case["xa"], case["xb"] = open_cloud(n, box), open_cloud(n, box)
            else:
                ca, cb = (cell_of(p if p is not None else (per_a or per_b)) for p in (per_a, per_b))
                case["xa"], case["xb"] = (cloud_in(rng, n, c, case["unwrapped"], case["lattice"]) for c in (ca, cb))
        else:
            box = float(rng.uniform(6.0, 40.0))
            xa, xb = open_cloud(na, box), open_cloud(nb, box)
            case["sa"], case["sb"], case["keys"] = names(na), names(nb), keys(n)
            da, db = norm3(xa[:n, None, :] - xa[None, :, :]), norm3(xb[:n, None, :] - xb[None, :, :])  # n rows over the whole side
            if driver == "dmxs":
                case["da"], case["db"] = da, db
            else:  # rows of different lengths (each sorted with a prefix of its sequence), some entries +inf
                rows = []
                for mat, width in ((da, na), (db, nb)):
                    side = []
                    for r in range(n):
                        row = mat[r, :int(rng.integers(r + 1, width + 1))].copy()  # (a row holds its own atom, at distance 0)
                        far = rng.random(len(row)) < 0.05
                        far[r] = False
                        row[far] = np.inf
                        side.append(row)
                    full = int(rng.integers(n))
                    side[full] = mat[full].copy()  # one row of full length: the padded width
                    rows.append(side)
                case["rows_a"], case["rows_b"] = rows
    else:  # the two ensembles
        m, n = 2 + (v + (slot == 8)) % 4, int(rng.integers(30, 201))  # M = 2 .. 5 in rotation
        case["m"], case["n"] = m, n
        case["seq"], case["keys"] = names(n), keys(n)
        case["block"] = bool(rng.random() < 1.0 / 3.0)  # LCHD_ENSEMBLE_BLOCK=2
        case["spairs"] = None
        if rng.random() < 0.5:  # an explicit list with an (i, i) pair and a reversed pair
            extra = [(int(a), int(b)) for a, b in rng.integers(0, m, (int(rng.integers(0, 4)), 2))]
            case["spairs"] = [(1, 1), (m - 1, 0), (0, m - 1)] + extra
        case["excluded"] = None
        if rng.random() < 0.5:  # both orders
            ex = [(r, c) for r in range(0, n, 7) for c in (r + 1, r + 2) if c < n]
            case["excluded"] = ex + [(c, r) for r, c in ex]
        case["per"], case["cell_kind"] = None, None
        if driver == "coords_ensemble" and case["boundary"] != "open":
            if case["boundary"] == "box":
                case["per"] = draw_box(rng)
                cells = [cell_of(case["per"])] * m
            else:
                (_, cell), case["cell_kind"] = draw_cell(rng)
                if rng.random() < 0.5:  # one cell per structure (NPT)
                    cells = [cell * s for s in rng.uniform(0.95, 1.1, m)]
                    case["per"] = ("cell", np.stack(cells))
                else:
                    cells, case["per"] = [cell] * m, ("cell", cell)
            frac = rng.uniform(-2.0, 2.0, (n, 3)) if case["unwrapped"] else rng.uniform(0.0, 1.0, (n, 3))
            xs = np.stack([(frac + rng.normal(0.0, 0.02, (n, 3))) @ cells[k] for k in range(m)])
        else:
            side = (n / 0.05) ** (1 / 3)
            base = rng.uniform(0.0, side, (n, 3))
            xs = np.stack([base + rng.normal(0.0, 1.0, (n, 3)) for _ in range(m)])
        if case["lattice"]:
            xs = np.round(xs)
        if driver == "coords_ensemble":
            case["xs"] = xs
        else:  # square matrices; the excluded entries are +inf in what the caller passes (from_dmxs_ensemble has no list of them)
            mats = np.stack([norm3(x[:, None, :] - x[None, :, :]) for x in xs])
            for r, c in case["excluded"] or []:
                mats[:, r, c] = np.inf
            case["dmxs"] = mats
    return case


def is_periodic(case):
    return case["boundary"] != "open"


def open_twin(case):
    """The same input with every periodic keyword dropped."""
    twin = dict(case)
    twin["boundary"] = "open"
    for k in ("per_a", "per_b", "per"):
        if k in twin:
            twin[k] = None
    return twin


def structure_pairs(case):
    m = case["m"]
    return case["spairs"] if case["spairs"] is not None else [(i, k) for i in range(m) for k in range(i + 1, m)]


def sampled_rows(case, n):
    """At most MAX_ROWS rows, 0 and n - 1 always (a function of the seed).  A sampled row costs the reference a 343-shift brute force
    over n atoms per structure and one oracle call per structure pair, so long rows and many pairs are sampled more thinly: at most
    12 rows beyond 150 atoms, and about 96 row pairs per ensemble, never fewer than 4 rows."""
    k = MAX_ROWS if n <= 150 else MAX_ROWS // 2
    if case["driver"] in ENSEMBLES:
        k = max(4, min(k, 96 // len(structure_pairs(case))))
    if n <= k:
        return list(range(n))
    rng = np.random.default_rng(77000 + case["seed"])
    return sorted(set(rng.integers(0, n, k - 2).tolist()) | {0, n - 1})


# ---- the references ---------------------------------------------------------------------------------------------------------------
def build(mod, case, **kw):
    """The LoCoHD instance of the case from `mod` (the oracle or the library: the same constructor)."""
    wf = {k: mod.WeightFunction(*v) for k, v in case["wfs"].items()} if case["multi"] else mod.WeightFunction(*case["wfs"])
    rule = case.get("rule")
    return mod.LoCoHD(case["cats"], wf, None if rule is None else mod.TagPairingRule(rule), category_weights=case["weights"],
                      statistical_distance=mod.StatisticalDistance(*case["sd"]), **kw)


def image_cloud(x, per, span=1):
    """(coordinates, atom index) of the periodic images of x at the shifts -span .. span: every atom moved into the cell by whole
    lattice vectors first, the home images first.  An open side (per None) is its own cloud."""
    x = np.asarray(x, dtype=np.float64)
    if per is None:
        return x, np.arange(len(x))
    cell = cell_of(per)
    p = x - np.floor(x @ np.linalg.inv(cell)) @ cell
    shifts = [s for s in itertools.product(range(-span, span + 1), repeat=3) if s != (0, 0, 0)]
    pts = [p] + [p + ((s[0] * cell[0] + s[1] * cell[1]) + s[2] * cell[2]) for s in shifts]
    return np.concatenate(pts), np.tile(np.arange(len(x)), len(pts))


def prim_list(mod, seq, tags, x, atom=None):
    atom = np.arange(len(x)) if atom is None else atom
    return [mod.PrimitiveAtom(seq[a], tags[a], c) for a, c in zip(atom, x)]


def anchor_pairs(case):
    return [(a, b, k) for (a, b), k in zip(case["pairs"], case["keys"])] if case["multi"] else case["pairs"]


def dense_rows(x, rows, per):
    """Reference rows of one structure: plain distances, or the nearest images by brute force."""
    if per is None:
        return [norm3(x[r] - x) for r in rows]
    return brute_rows(x, rows, cell_of(per))


def ensemble_rows(case, rows):
    """rows_of[k]: the sampled reference rows of structure k, excluded entries +inf."""
    out = []
    for k in range(case["m"]):
        if case["driver"] == "dmxs_ensemble":
            rs = [case["dmxs"][k][r].copy() for r in rows]
        else:
            per = case["per"]
            if per is not None and np.ndim(per[1]) == 3:
                per = ("cell", per[1][k])
            rs = [np.array(r) for r in dense_rows(case["xs"][k], rows, per)]
            lookup = {r: i for i, r in enumerate(rows)}
            for r, c in case["excluded"] or []:
                if r in lookup:
                    rs[lookup[r]][c] = np.inf
        out.append(rs)
    return out


def expected(case, oracle):
    """(scores, rows): the oracle's scores of the case; rows = the sampled row indices the scores belong to, or None for all."""
    lo = build(oracle, case)
    drv = case["driver"]
    if drv == "prims":
        (ca, ia), (cb, ib) = image_cloud(case["xa"], case["per_a"]), image_cloud(case["xb"], case["per_b"])
        pa, pb = prim_list(oracle, case["sa"], case["tags_a"], ca, ia), prim_list(oracle, case["sb"], case["tags_b"], cb, ib)
        return np.asarray(lo.from_primitives(pa, pb, anchor_pairs(case), case["thr"])), None
    if drv == "prims_batch":
        ps = [prim_list(oracle, *s) for s in case["structs"]]
        return [np.asarray(lo.from_primitives(ps[a], ps[b], pairs, case["thr"])) if pairs else np.zeros(0) for a, b, pairs in case["jobs"]], None
    if drv == "coords":
        if not is_periodic(case):
            return np.asarray(lo.from_coords(case["sa"], case["sb"], case["xa"], case["xb"], case["keys"])), None
        rows = sampled_rows(case, case["n"])
        keys = None if case["keys"] is None else [case["keys"][r] for r in rows]
        return oracle_rows(lo, case["sa"], case["sb"], dense_rows(case["xa"], rows, case["per_a"]), dense_rows(case["xb"], rows, case["per_b"]), keys), rows
    if drv == "dmxs":
        return np.asarray(lo.from_dmxs(case["sa"], case["sb"], case["da"], case["db"], case["keys"])), None
    if drv == "dmxs_ragged":
        return oracle_rows(lo, case["sa"], case["sb"], case["rows_a"], case["rows_b"], case["keys"]), None
    rows = sampled_rows(case, case["n"])
    keys = None if case["keys"] is None else [case["keys"][r] for r in rows]
    rows_of = ensemble_rows(case, rows)
    return np.stack([oracle_rows(lo, case["seq"], case["seq"], rows_of[i], rows_of[k], keys) for i, k in structure_pairs(case)]), rows


# ---- the same references through the integral form ----------------------------------------------------------------------------------
def integral_check(case, oracle, n_items=8):
    """(integral form, oracle) on up to n_items anchor pairs / rows of the case, both fed the reference clouds / rows of expected()."""
    import integral_form as iform

    index = {c: i for i, c in enumerate(case["cats"])}
    wf_of = (lambda key: case["wfs"][key]) if case["multi"] else (lambda key: case["wfs"])
    want, rows = expected(case, oracle)
    rng = np.random.default_rng(88000 + case["seed"])
    mine, theirs = [], []

    def score(cat_a, dist_a, cat_b, dist_b, key):
        return iform.score(cat_a, dist_a, cat_b, dist_b, case["ncat"], wf_of(key), case["sd"], case["weights"])

    if case["driver"] == "prims":
        clouds = []
        for x, per, seq, tags in ((case["xa"], case["per_a"], case["sa"], case["tags_a"]), (case["xb"], case["per_b"], case["sb"], case["tags_b"])):
            pts, atom = image_cloud(x, per)
            clouds.append((pts, np.asarray([index[seq[a]] for a in atom]), [tags[a] for a in atom]))
        thr2 = case["thr"] * case["thr"]
        for p in rng.choice(len(case["pairs"]), min(n_items, len(case["pairs"])), replace=False):
            env = []
            for (pts, cat, tags), anchor in zip(clouds, case["pairs"][p]):
                d = pts - pts[anchor]
                d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
                keep = np.asarray([q == anchor or rule_accepts(case["rule"], tags[anchor], tags[q]) for q in range(len(pts))]) & (d2 < thr2)
                env += [cat[keep], np.sqrt(d2[keep])]
            mine.append(score(*env, case["keys"][p] if case["multi"] else None))
            theirs.append(want[p])
        return np.asarray(mine), np.asarray(theirs)
    if case["driver"] == "coords":
        rows = list(range(case["n"])) if rows is None else rows
        pick = rng.choice(len(rows), min(n_items, len(rows)), replace=False)
        ra, rb = dense_rows(case["xa"], [rows[k] for k in pick], case["per_a"]), dense_rows(case["xb"], [rows[k] for k in pick], case["per_b"])
        ca, cb = np.asarray([index[s] for s in case["sa"]]), np.asarray([index[s] for s in case["sb"]])
        for k, a, b in zip(pick, ra, rb):
            mine.append(score(ca, a, cb, b, case["keys"][rows[k]] if case["multi"] else None))
            theirs.append(want[k])
        return np.asarray(mine), np.asarray(theirs)
    assert case["driver"] in ENSEMBLES
    rows_of = ensemble_rows(case, rows)
    cat = np.asarray([index[s] for s in case["seq"]])
    pairs = structure_pairs(case)
    for _ in range(n_items):
        p, k = int(rng.integers(len(pairs))), int(rng.integers(len(rows)))
        i, q = pairs[p]
        mine.append(score(cat, rows_of[i][k], cat, rows_of[q][k], case["keys"][rows[k]] if case["multi"] else None))
        theirs.append(want[p, k])
    return np.asarray(mine), np.asarray(theirs)
