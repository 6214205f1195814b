"""The pair-family axes of the whole-surface fuzz and their CPU references (tests/test_gpu_fuzz_pairs.py; checked on their own, without a
device, by tests/test_fuzz_pairs_draw.py): score attribution by category, neighbour sensitivities / coordinate gradients, and
cross-scoring / nearest.  No device and no product code is touched here.

pair_axes(case) adds, to a case of fuzz_surface.draw, what the three families need on top of it.  It is a plain function of case["seed"]
(the case is drawn again from the seed, so an open twin has the axes of its periodic original) and draws from a generator of its own,
default_rng(STREAM + seed); fuzz_surface.draw and fuzz_profiles.profile_axes are not touched.

    driver              attribution                       sensitivity / gradient                cross / nearest
    prims               attribution_from_primitives       sensitivity_from_primitives           cross_from_primitives (host: open sides)
    prims_batch         attribution_from_primitives       sensitivity_from_primitives           one call per structure of B (host); one call
                        per job                           per job                               over the batch (session, global indices)
    coords              attribution_from_coords           --                                    --
    dmxs                attribution_from_dmxs             --                                    --
    dmxs_ragged         ValueError                        --                                    --
    ensembles           --                                --                                    --

ax["fit"][family] is the case the family accepts, made from the case as drawn by changing only what the family refuses;
ax["changed"][family] lists every change:

    more than 64 categories (attribution, sensitivity)   ids folded to W = W_ROTATION[visit % 5]: id -> id % W, the highest drawn id to
                                                         W - 1 (so the highest folded id occurs); weights = the first W drawn weights
    a non-Hellinger distance (attribution)               ("Hellinger", [e]), e from E_ROTATION by the visit (one of them drawn here)
    a periodic side (sensitivity; cross on the host)     fuzz_surface.open_twin: neither host call takes a box or a cell.  The session
                                                         cross / nearest calls take the periodic case as drawn, as image clouds.

Cross axes (by rotations of the driver's visit, of lengths 3, 7, 9 and 11: no factor shared with the 5 boundaries or the 8 of at_width):
anchors_a = Na entries of the A column of the drawn pairs, anchors_b = Nb entries of the B column -- repeats kept, and one planted where
none was drawn, so that nearest meets exact ties -- k clipped to Nb, tile_rows, and with a dictionary one key for the whole call.
ax["cross"]["groups"] lists, per structure of side B, (structure or None, local anchors, their columns in anchors_b).

References:
    attribution   attribution_util.attribution on the environments of fuzz_profiles.Env of the fitted case (image clouds + rule_accepts,
                  dense_rows / brute_rows, the matrices), the categories renumbered to those present as radial_reference does
    sensitivity   sensitivity_util.sensitivity on indexed_environment() below: the anchor first, then ascending (distance, index), the
                  distances in integral_form's arithmetic, membership by fuzz_surface.rule_accepts; gradients by sensitivity_util.gradient
    cross         the oracle's open from_primitives on the explicit Na x Nb pair list, on the reference clouds of fuzz_surface.expected
"""
import numpy as np

import attribution_util as au
import fuzz_profiles as fp
import fuzz_surface as fs
import sensitivity_util as su
from integral_form import _sqdist

STREAM = 5_207_000  # the generator of seed s is default_rng(STREAM + s): apart from 434000 + s, 2605000 + s, 77000 + s and 88000 + s;
#                     chosen so that the default seeds cover what test_fuzz_pairs_draw.py lists
W_ROTATION = [64, 63, 33, 32, 2]                    # the folded category count, by visit % 5
NA_ROTATION = [1, 5, 12]
NB_ROTATION = [1, 63, 64, 65, 80, 64, 65]           # the widths next to the wavefront of k_nearest_rows
K_ROTATION = [1, 2, 64, 63, 8, 64, 2, 63, 8]        # clipped to Nb
TILE_ROTATION = [0, 1, 5, "Na", 5, 0, "Na", 1, 5, 0, 1]
MAX_CATEGORIES = 64
ATTRIBUTION_DRIVERS = ("prims", "prims_batch", "coords", "dmxs")
PAIR_DRIVERS = ("prims", "prims_batch")  # sensitivity and cross
FAMILIES = ("attribution", "sensitivity", "cross")
RAGGED_ATTRIBUTION = "attribution_from_dmxs takes rectangular distance matrices (rows of equal length)"
TOO_MANY = "64 categories"
PERIODIC_SENSITIVITY = "periodic boxes and cells are not supported"


def visit_of(seed):
    slot, j = seed % len(fs.SLOTS), seed // len(fs.SLOTS)
    return seed // 3 if fs.SLOTS[slot] == "prims" else j + slot


# ---- fitting ----------------------------------------------------------------------------------------------------------------------
def fold(case, width):
    """The case with its category ids folded to `width`: id -> id % width, the highest drawn id to width - 1."""
    top = case["ncat"] - 1
    name = {f"t{i}": f"t{width - 1 if i == top else i % width}" for i in range(case["ncat"])}
    out = dict(case, ncat=width, cats=[f"t{i}" for i in range(width)], weights=None if case["weights"] is None else case["weights"][:width])
    for k in ("sa", "sb"):
        if k in out:
            out[k] = [name[s] for s in case[k]]
    if "structs" in out:
        out["structs"] = [([name[s] for s in seq], tags, x) for seq, tags, x in case["structs"]]
    return out


def refusals(case):
    """family -> the reasons the case AS DRAWN is refused by the family's host calls (empty: it runs unfitted)."""
    drv = case["driver"]
    out = {}
    if drv in ATTRIBUTION_DRIVERS:
        out["attribution"] = [TOO_MANY] * (case["ncat"] > MAX_CATEGORIES) + [case["sd"][0]] * (case["sd"][0] != "Hellinger")
    if drv in PAIR_DRIVERS:
        out["sensitivity"] = [PERIODIC_SENSITIVITY] * fs.is_periodic(case) + [TOO_MANY] * (case["ncat"] > MAX_CATEGORIES)
        out["cross"] = []  # (the host call has no periodic keyword to refuse: it is given the open twin)
    return out


# ---- the axes ---------------------------------------------------------------------------------------------------------------------
def _entries(rng, n_have, n_want):
    """n_want positions in a list of n_have: distinct ones first, repeats once the list is used up."""
    if n_want <= n_have:
        return rng.choice(n_have, n_want, replace=False)
    return np.concatenate([rng.permutation(n_have), rng.integers(0, n_have, n_want - n_have)])


def pair_axes(case):
    seed = int(case["seed"])
    case = fs.draw(seed)  # (an open twin gets the axes of the case it was made from)
    drv = case["driver"]
    v = visit_of(seed)
    rng = np.random.default_rng(STREAM + seed)
    ax = {"seed": seed, "visit": v, "ragged": drv == "dmxs_ragged", "fit": {}, "changed": {}, "refused": refusals(case)}
    ax["runs"] = {"attribution": drv in ATTRIBUTION_DRIVERS, "sensitivity": drv in PAIR_DRIVERS, "cross": drv in PAIR_DRIVERS}
    # the pairs / rows of the references
    if drv == "prims":
        ax["sample"] = fp._pick(rng, len(case["pairs"]))
    elif drv == "prims_batch":
        ax["sample"] = [fp._pick(rng, len(pairs)) for _, _, pairs in case["jobs"]]
    elif drv in ("coords", "dmxs"):
        ax["sample"] = fs.sampled_rows(case, case["n"])
    else:
        ax["sample"] = []
    e_drawn = float(rng.uniform(1.0, 5.0))
    width = W_ROTATION[v % len(W_ROTATION)]
    exponent = [2.0, e_drawn, 1.0][v % 3]
    wide = case["ncat"] > MAX_CATEGORIES
    for family in FAMILIES:
        if not ax["runs"][family]:
            continue
        fit, changed = case, []
        if wide and family != "cross":
            fit = fold(fit, width)
            changed.append(f"{case['ncat']} categories folded to {width}")
        if family == "attribution" and case["sd"][0] != "Hellinger":
            fit = dict(fit, sd=("Hellinger", [exponent]))
            changed.append(f"{case['sd'][0]} replaced by Hellinger, exponent {exponent}")
        if family in ("sensitivity", "cross") and fs.is_periodic(case):
            fit = fs.open_twin(fit)
            changed.append("periodic sides opened" + (" (host call; the session call takes image clouds)" if family == "cross" else ""))
        ax["fit"][family], ax["changed"][family] = fit, changed
    if drv not in PAIR_DRIVERS:
        return ax
    # pair weights of the gradient, one per sampled pair
    n_sampled = len(ax["sample"]) if drv == "prims" else sum(len(s) for s in ax["sample"])
    ax["pair_weights"] = rng.uniform(0.5, 2.0, n_sampled)
    # the cross axes
    na, nb = NA_ROTATION[v % len(NA_ROTATION)], NB_ROTATION[v % len(NB_ROTATION)]
    k = min(K_ROTATION[v % len(K_ROTATION)], nb)
    tile = TILE_ROTATION[v % len(TILE_ROTATION)]
    if drv == "prims":
        cols = np.asarray(case["pairs"], dtype=np.int64).reshape(-1, 2)
        anchors_a = cols[_entries(rng, len(cols), na), 0]
        local_b = cols[_entries(rng, len(cols), nb), 1]
        struct_b = np.zeros(nb, dtype=np.int64)
        offsets = np.zeros(1, dtype=np.int64)
    else:
        anchors_a = np.asarray(case["jobs"][0][2], dtype=np.int64).reshape(-1, 2)[:, 0]
        anchors_a = anchors_a[_entries(rng, len(anchors_a), na)]
        pool = np.asarray([(b, q) for _, b, pairs in case["jobs"] for _, q in pairs], dtype=np.int64)  # (structure, atom) of every B anchor
        pool = pool[_entries(rng, len(pool), nb)]
        struct_b, local_b = pool[:, 0], pool[:, 1]
        offsets = np.concatenate([[0], np.cumsum([len(s[0]) for s in case["structs"]])]).astype(np.int64)
    if nb >= 2 and len(set(zip(struct_b.tolist(), local_b.tolist()))) == nb:  # no repeat was drawn: plant one (an exact tie for nearest)
        struct_b[-1], local_b[-1] = struct_b[0], local_b[0]
    groups = [(None if drv == "prims" else int(s), local_b[struct_b == s].tolist(), np.flatnonzero(struct_b == s).tolist())
              for s in sorted(set(struct_b.tolist()))]
    ax["cross"] = {"anchors_a": anchors_a.tolist(), "anchors_b": (offsets[struct_b] + local_b).tolist(), "groups": groups, "na": na, "nb": nb, "k": k,
                   "tile_rows": na if tile == "Na" else tile, "tile_name": tile,
                   "key": sorted(case["wfs"])[int(rng.integers(len(case["wfs"])))] if case["multi"] else None}
    return ax


# ---- attribution ------------------------------------------------------------------------------------------------------------------
def attribution_reference(case, ax, swap_sides=False):
    """(rows (len(items), C), items): attribution_util.attribution of every sampled pair / row of the FITTED case `case`, in the order of
    fuzz_profiles.Env(case, sample).items.  swap_sides: the mutation check of test_fuzz_pairs_draw.py, never the reference."""
    assert case["sd"][0] == "Hellinger" and case["ncat"] <= MAX_CATEGORIES
    w = None if case["weights"] is None else np.asarray(case["weights"])
    items = fp.Env(case, ax["sample"]).items
    out = np.zeros((len(items), case["ncat"]))
    for i, (_, key, (ca, da), (cb, db)) in enumerate(items):
        if swap_sides:
            ca, da, cb, db = cb, db, ca, da
        present, inverse = np.unique(np.concatenate([ca, cb]), return_inverse=True)
        out[i, present] = au.attribution(inverse[:len(ca)], da, inverse[len(ca):], db, len(present), fp._wf(case, key), case["sd"][1][0],
                                         None if w is None else w[present])
    return out, items


def sampled_scores(case, ax, oracle):
    """fuzz_surface.expected() of `case` on the sampled items (what attribution rows sum to, what sensitivity scores are)."""
    return fp.oracle_scores(case, ax, oracle)


# ---- sensitivity ------------------------------------------------------------------------------------------------------------------
def indexed_environment(cloud, anchor, thr, rule):
    """(idx, cat, dist) of the environment of `anchor` in an open cloud (points, categories, tags): the anchor first, then ascending
    (distance, index); distances in integral_form's arithmetic, membership by fuzz_surface.rule_accepts."""
    pts, cat, tags = cloud
    d2 = _sqdist(pts[anchor], pts)
    thr2 = np.float64(thr) * np.float64(thr) if np.isfinite(thr) else np.inf
    near = np.flatnonzero(d2 < thr2)
    idx = np.asarray([q for q in near if q == anchor or fs.rule_accepts(rule, tags[anchor], tags[q])], dtype=np.int64)
    d = np.sqrt(d2[idx])
    order = np.lexsort((idx, d, idx != anchor))
    return idx[order], cat[idx[order]], d[order]


def sensitivity_pairs(case, ax):
    """[(job or None, structure a, structure b, pair index, (i, j), key)] of the sampled pairs of the fitted (open) case."""
    if case["driver"] == "prims":
        return [(None, 0, 1, p, case["pairs"][p], case["keys"][p] if case["multi"] else None) for p in ax["sample"]]
    return [(j, a, b, p, pairs[p], None) for j, (a, b, pairs) in enumerate(case["jobs"]) for p in ax["sample"][j]]


def sensitivity_clouds(case):
    if case["driver"] == "prims":
        assert case["per_a"] is None and case["per_b"] is None
        return [fp._prim_cloud(case, case["xa"], None, case["sa"], case["tags_a"]), fp._prim_cloud(case, case["xb"], None, case["sb"], case["tags_b"])]
    return [fp._prim_cloud(case, x, None, seq, tags) for seq, tags, x in case["structs"]]


def sensitivity_reference(case, ax, swap_sides=False, rule="as drawn"):
    """A sensitivity_util.Sens over sensitivity_pairs(case, ax) (g as float64; indices local to the pair's structures) as wide as the
    longest environment.  swap_sides / rule: the mutation checks, never the reference."""
    clouds = sensitivity_clouds(case)
    rule = case["rule"] if rule == "as drawn" else rule
    rows = []
    for _, a, b, _, (i, j), key in sensitivity_pairs(case, ax):
        ia, ca, da = indexed_environment(clouds[a], i, case["thr"], rule)
        ib, cb, db = indexed_environment(clouds[b], j, case["thr"], rule)
        if swap_sides:
            s, gb, ga = su.sensitivity(cb, db, ca, da, case["ncat"], fp._wf(case, key), case["sd"], case["weights"])
        else:
            s, ga, gb = su.sensitivity(ca, da, cb, db, case["ncat"], fp._wf(case, key), case["sd"], case["weights"])
        rows.append((s, ia, da, ga, ib, db, gb))
    n, k = len(rows), max([max(len(r[1]), len(r[4])) for r in rows], default=1)
    out = su.Sens(np.zeros(n), np.zeros(n, np.int32), np.full((n, k), -1, np.int32), np.zeros((n, k)), np.zeros((n, k)), np.zeros(n, np.int32),
                  np.full((n, k), -1, np.int32), np.zeros((n, k)), np.zeros((n, k)))
    for p, (s, ia, da, ga, ib, db, gb) in enumerate(rows):
        out.scores[p] = s
        out.count_a[p], out.count_b[p] = len(ia), len(ib)
        out.idx_a[p, : len(ia)], out.dist_a[p, : len(ia)], out.g_a[p, : len(ia)] = ia, da, ga.astype(np.float64)
        out.idx_b[p, : len(ib)], out.dist_b[p, : len(ib)], out.g_b[p, : len(ib)] = ib, db, gb.astype(np.float64)
    return out


def densities(case, ax, sens):
    """(w(d) of side A, of side B) at every slot of a Sens over sensitivity_pairs: the longdouble density the bound of g scales with."""
    keys = [key for *_, key in sensitivity_pairs(case, ax)]
    out = []
    for dist in (sens.dist_a, sens.dist_b):
        out.append(np.asarray([np.asarray(su.pdf(*fp._wf(case, key), row), dtype=np.float64) for key, row in zip(keys, dist)]).reshape(dist.shape))
    return out


def gradient_reference(case, ax, sens):
    """(grad_a, grad_b, sum |v g| per side) of a prims case, or per job [(job, grad_a, grad_b, sum |v g|)] of a batch: the sampled pairs
    with ax["pair_weights"] through sensitivity_util.gradient."""
    pairs = sensitivity_pairs(case, ax)
    v = ax["pair_weights"]

    def size(rows):
        return float(sum(np.sum(np.abs(v[r] * sens.g_a[r])) + np.sum(np.abs(v[r] * sens.g_b[r])) for r in rows))

    if case["driver"] == "prims":
        ga, gb = su.gradient(sens, case["xa"], case["xb"], v)
        return ga, gb, size(range(len(pairs)))
    out = []
    for j, (a, b, _) in enumerate(case["jobs"]):
        rows = [r for r, pr in enumerate(pairs) if pr[0] == j]
        if rows:
            part = su.Sens(*[np.asarray(f)[rows] for f in sens])
            ga, gb = su.gradient(part, case["structs"][a][2], case["structs"][b][2], v[rows])
            out.append((j, ga, gb, size(rows)))
    return out


# ---- cross ------------------------------------------------------------------------------------------------------------------------
def cross_reference(case, ax, oracle, swap_sides=False, rule="as drawn"):
    """The (Na, Nb) matrix of the oracle's open from_primitives on the explicit pair list, on the reference clouds of
    fuzz_surface.expected (image clouds for periodic sides of `case`, the anchors their home images)."""
    cx = ax["cross"]
    if rule != "as drawn":
        case = dict(case, rule=rule)
    lo = fs.build(oracle, case)
    out = np.zeros((cx["na"], cx["nb"]))

    def prims(seq, tags, x, per):
        pts, atom = fs.image_cloud(x, per)
        return fs.prim_list(oracle, seq, tags, pts, atom)

    if case["driver"] == "prims":
        pa, pb = prims(case["sa"], case["tags_a"], case["xa"], case["per_a"]), prims(case["sb"], case["tags_b"], case["xb"], case["per_b"])
        sides = {None: pb}
    else:
        pa = prims(*case["structs"][0], None)
        sides = {s: prims(*case["structs"][s], None) for s, _, _ in cx["groups"]}
    key = () if cx["key"] is None else (cx["key"],)
    for s, local, cols in cx["groups"]:
        if swap_sides:
            pairs = [(int(j), int(i)) + key for i in cx["anchors_a"] for j in local]
            got = lo.from_primitives(sides[s], pa, pairs, case["thr"])
        else:
            pairs = [(int(i), int(j)) + key for i in cx["anchors_a"] for j in local]
            got = lo.from_primitives(pa, sides[s], pairs, case["thr"])
        out[:, cols] = np.asarray(got).reshape(cx["na"], len(local))
    return out
