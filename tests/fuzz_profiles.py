"""The profile axes of the whole-surface fuzz and their CPU references (tests/test_gpu_fuzz_profiles.py; checked on their own, without a
device, by tests/test_fuzz_profiles_draw.py).  No device and no product code is touched here.

profile_axes(case) adds, to a case of fuzz_surface.draw, what a radial / composition profile call needs on top of it: the edges (bin
count by a rotation of the driver's visit, one of five edge kinds) and the pairs / rows whose reference is computed.  It is a plain
function of case["seed"] (the case is drawn again from the seed, so an open twin has the axes of its periodic original) and draws from a
generator of its own, default_rng(STREAM + seed); fuzz_surface.draw is not touched.

    driver              radial                                         composition
    prims               radial_from_primitives                         composition_from_primitives per side (anchors: the A / B column)
    prims_batch         radial_from_primitives per job                 --
    coords              radial_from_coords                             composition_from_coords per side
    dmxs                radial_from_dmxs                               composition_from_dmx per side
    dmxs_ragged         ValueError                                     ValueError
    coords_ensemble     --                                             composition_from_coords on structures 0 and M - 1 (own cell)
    dmxs_ensemble       --                                             composition_from_dmx on matrices 0 and M - 1 (the case holds no
                                                                       coordinates; the excluded entries are +inf in the rows)

The references build every environment as fuzz_surface.integral_check does (image_cloud + rule_accepts, dense_rows / brute_rows, the
matrices themselves) and score it with radial_util.profile (longdouble) / composition_util.profile.  radial_util.profile gets the
environment's categories renumbered to those that occur in it: a category that occurs on neither side adds 0 to every statistical
distance and nothing to a normalisation, and a (points x 300) longdouble table per side would cost seconds per pair.

Edge kinds (R: the threshold; the diameter of the clouds for an infinite one; the largest finite entry of the reference rows for a dense
driver):
    cover      e_0 = 0, e_K = +inf, inner edges uniform over (0, R): a row sums to the pair's score
    on_points  cover, with at least half of the inner edges copied as float64 values from distances that occur: from the anchors of a
               drawn pair to the atoms (images) of their own sides, or the entries of a drawn row pair; on a lattice whole shells
    window     e_0 > 0 and a finite e_K, all inside (0, R)
    below      every edge below 1e-3, under the smallest positive distance of the clouds drawn here: no breakpoint in any bin, bin k
               is H(anchors) * (F(e_{k+1}) - F(e_k)) -- exactly 0.0 where the weight function has no support there
    beyond     every edge >= R, +inf last: bin k is H(whole environments) * (F(e_{k+1}) - F(e_k)), the last bin the rest of the tail
"""
import numpy as np

import composition_util as cu
import fuzz_surface as fs
import radial_util as ru

STREAM = 2_605_000  # the generator of seed s is default_rng(STREAM + s): apart from fuzz_surface's 434000 + s, 77000 + s and 88000 + s;
#                     chosen so that the default seeds cover what test_fuzz_profiles_draw.py lists
K_ROTATION = [1, 2, 9, 63, 64, 2, 63]  # by the driver's visit: seven long, no factor shared with the 5 boundaries, the 10 category widths or the 8 of at_width
EDGE_KINDS = ["cover", "on_points", "window", "below", "beyond"]
RADIAL_DRIVERS = ("prims", "prims_batch", "coords", "dmxs")
COMPOSITION_DRIVERS = ("prims", "coords", "dmxs") + fs.ENSEMBLES
MAX_PAIRS, SAMPLED_PAIRS = 40, 24
BELOW = 1e-3
RAGGED_RADIAL = "radial_from_dmxs takes rectangular distance matrices (rows of equal length)"
RAGGED_COMPOSITION = "composition_from_dmx takes a rectangular distance matrix (rows of equal length)"


# ---- the reference environments ---------------------------------------------------------------------------------------------------
def _prim_cloud(case, x, per, seq, tags):
    index = {c: i for i, c in enumerate(case["cats"])}
    pts, atom = fs.image_cloud(x, per)
    return pts, np.asarray([index[seq[a]] for a in atom]), [tags[a] for a in atom]


def _sq(pts, anchor):
    d = pts - pts[anchor]
    return d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]


def _env(cloud, anchor, thr, rule):
    """(categories, distances) of the environment of `anchor` in an image cloud: fuzz_surface.integral_check's."""
    pts, cat, tags = cloud
    d2 = _sq(pts, anchor)
    near = np.flatnonzero(d2 < thr * thr)
    keep = np.asarray([q for q in near if q == anchor or fs.rule_accepts(rule, tags[anchor], tags[q])], dtype=np.int64)
    return cat[keep], np.sqrt(d2[keep])


def _pick(rng, n):
    """Every pair of a list of at most MAX_PAIRS, otherwise SAMPLED_PAIRS of them, the first and the last always."""
    if n <= MAX_PAIRS:
        return list(range(n))
    return sorted(set(rng.choice(n, SAMPLED_PAIRS - 2, replace=False).tolist()) | {0, n - 1})


def _per_of(case, k):
    per = case["per"]
    return ("cell", per[1][k]) if per is not None and np.ndim(per[1]) == 3 else per


class Env:
    """What the references are computed from: items[i] = (where, key, side A, side B) with a side = (categories, distances) or None;
    `where` = the pair index (prims), (job, pair index), the row, or (structure, row)."""

    def __init__(self, case, sample):
        drv = case["driver"]
        index = {c: i for i, c in enumerate(case["cats"])}
        self.items = []
        self.reach = 0.0   # the largest finite distance of the environments (R of the dense drivers)

        def key_of(k):
            return case["keys"][k] if case.get("keys") is not None else None

        if drv == "prims":
            self.clouds = [_prim_cloud(case, case["xa"], case["per_a"], case["sa"], case["tags_a"]),
                           _prim_cloud(case, case["xb"], case["per_b"], case["sb"], case["tags_b"])]
            for p in sample:
                a, b = case["pairs"][p]
                self.items.append((p, key_of(p), _env(self.clouds[0], a, case["thr"], case["rule"]), _env(self.clouds[1], b, case["thr"], case["rule"])))
        elif drv == "prims_batch":
            self.clouds = [_prim_cloud(case, x, None, seq, tags) for seq, tags, x in case["structs"]]
            for j, (a, b, pairs) in enumerate(case["jobs"]):
                for p in sample[j]:
                    self.items.append(((j, p), None, _env(self.clouds[a], pairs[p][0], case["thr"], case["rule"]),
                                       _env(self.clouds[b], pairs[p][1], case["thr"], case["rule"])))
        elif drv == "coords":
            ca, cb = np.asarray([index[s] for s in case["sa"]]), np.asarray([index[s] for s in case["sb"]])
            ra, rb = fs.dense_rows(case["xa"], sample, case["per_a"]), fs.dense_rows(case["xb"], sample, case["per_b"])
            self.items = [(r, key_of(r), (ca, np.asarray(a)), (cb, np.asarray(b))) for r, a, b in zip(sample, ra, rb)]
        elif drv == "dmxs":
            ca, cb = np.asarray([index[s] for s in case["sa"]]), np.asarray([index[s] for s in case["sb"]])
            self.items = [(r, key_of(r), (ca, case["da"][r]), (cb, case["db"][r])) for r in sample]
        elif drv in fs.ENSEMBLES:
            cat = np.asarray([index[s] for s in case["seq"]])
            for k in (0, case["m"] - 1):
                rows = [case["dmxs"][k][r] for r in sample] if drv == "dmxs_ensemble" else fs.dense_rows(case["xs"][k], sample, _per_of(case, k))
                self.items += [((k, r), key_of(r), (cat, np.asarray(row)), None) for r, row in zip(sample, rows)]
        for it in self.items:
            for side in it[2:]:
                if side is not None:
                    d = side[1][np.isfinite(side[1])]
                    self.reach = max(self.reach, float(np.max(d, initial=0.0)))


def _diameter(x):
    d = x[:, None, :] - x[None, :, :]
    return float(np.sqrt(np.max(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])))


# ---- the axes ---------------------------------------------------------------------------------------------------------------------
def _distinct(rng, start, n, lo, hi):
    """n distinct float64 values, ascending: those of `start`, the rest uniform over (lo, hi); a value drawn twice is drawn again."""
    vals = set(float(v) for v in start)
    while len(vals) < n:
        v = float(rng.uniform(lo, hi))
        if lo < v < hi:
            vals.add(v)
    return sorted(vals)


def profile_axes(case):
    seed = int(case["seed"])
    case = fs.draw(seed)  # (an open twin gets the axes of the case it was made from)
    drv = case["driver"]
    slot, j = seed % len(fs.SLOTS), seed // len(fs.SLOTS)
    v = seed // 3 if drv == "prims" else j + slot
    rng = np.random.default_rng(STREAM + seed)
    ax = {"seed": seed, "radial": drv in RADIAL_DRIVERS, "composition": drv in COMPOSITION_DRIVERS, "ragged": drv == "dmxs_ragged"}
    k_bins = K_ROTATION[v % len(K_ROTATION)]
    kind = EDGE_KINDS[int(rng.integers(len(EDGE_KINDS)))]
    # the pairs / rows of the references
    if drv == "prims":
        ax["sample"] = _pick(rng, len(case["pairs"]))
    elif drv == "prims_batch":
        ax["sample"] = [_pick(rng, len(pairs)) for _, _, pairs in case["jobs"]]
    elif drv == "dmxs_ragged":
        ax["sample"] = []
    else:
        ax["sample"] = fs.sampled_rows(case, case["n"])
    if not (ax["radial"] or ax["ragged"]):
        ax["k"], ax["kind"], ax["edges"] = None, None, None
        return ax
    # R
    if ax["ragged"]:
        big, env = float(max(np.max(r[np.isfinite(r)]) for r in case["rows_a"] + case["rows_b"])), None
    else:
        env = environments(case, ax)
        if drv in ("prims", "prims_batch"):
            big = case["thr"] if np.isfinite(case["thr"]) else max(_diameter(case["xa"]), _diameter(case["xb"]))
        else:
            big = env.reach
    ax["R"] = big
    if ax["ragged"]:
        kind = "cover"
    on = []
    if kind == "on_points":  # distances that occur, as the float64 values the reference environments hold
        pool = set()
        for _ in range(4):
            if drv == "prims":
                a, b = case["pairs"][int(rng.integers(len(case["pairs"])))]
                ds = [np.sqrt(_sq(env.clouds[0][0], a)), np.sqrt(_sq(env.clouds[1][0], b))]
            elif drv == "prims_batch":
                sa, sb, pairs = case["jobs"][int(rng.integers(0, 5))]  # (the last job is empty)
                a, b = pairs[int(rng.integers(len(pairs)))]
                ds = [np.sqrt(_sq(env.clouds[sa][0], a)), np.sqrt(_sq(env.clouds[sb][0], b))]
            else:
                it = env.items[int(rng.integers(len(env.items)))]
                ds = [it[2][1], it[3][1]]
            for d in ds:
                pool |= set(d[(d > 0.0) & (d < big)].tolist())
            if len(pool) >= k_bins - 1:
                break
        pool = np.asarray(sorted(pool))
        need = k_bins // 2  # at least half of the k_bins - 1 inner edges
        take = min(len(pool), int(rng.integers(need, k_bins))) if k_bins > 1 else 0
        on = rng.choice(pool, take, replace=False).tolist() if take else []
    if kind in ("cover", "on_points"):
        edges = _distinct(rng, [0.0] + on, k_bins, 0.0, big) + [np.inf]
    elif kind == "window":
        edges = _distinct(rng, [], k_bins + 1, 0.0, big)
    elif kind == "below":
        edges = _distinct(rng, [0.0] if rng.random() < 0.5 else [], k_bins + 1, 0.0, BELOW)
    else:
        edges = _distinct(rng, [big] if rng.random() < 0.5 else [], k_bins, big, 2.0 * big) + [np.inf]
    ax["k"], ax["kind"], ax["edges"], ax["on"] = k_bins, kind, np.asarray(edges, dtype=np.float64), sorted(on)
    return ax


_ENV_CACHE = {}


def environments(case, ax):
    """The reference environments of the sampled pairs / rows (kept for the last few cases: a periodic case and its open twin differ)."""
    key = (case["seed"], case["boundary"])
    if key not in _ENV_CACHE:
        if len(_ENV_CACHE) >= 4:
            _ENV_CACHE.clear()
        _ENV_CACHE[key] = Env(case, ax["sample"])
    return _ENV_CACHE[key]


# ---- the references ---------------------------------------------------------------------------------------------------------------
def _wf(case, key):
    return case["wfs"][key] if case["multi"] else case["wfs"]


def radial_reference(case, ax):
    """Rows (len(items), K): radial_util.profile of every sampled pair / row, in the order of environments(case, ax).items."""
    w = None if case["weights"] is None else np.asarray(case["weights"])
    out = []
    for _, key, (ca, da), (cb, db) in environments(case, ax).items:
        present, inverse = np.unique(np.concatenate([ca, cb]), return_inverse=True)
        out.append(ru.profile(inverse[:len(ca)], da, inverse[len(ca):], db, len(present), _wf(case, key), ax["edges"], case["sd"],
                              None if w is None else w[present]))
    return np.asarray(out).reshape(len(out), len(ax["edges"]) - 1)


def oracle_scores(case, ax, oracle):
    """fuzz_surface.expected() on the items of the references (the scores that cover / on_points rows sum to)."""
    want, rows = fs.expected(case, oracle)
    drv = case["driver"]
    if drv == "prims_batch":
        return np.asarray([want[j][p] for j, s in enumerate(ax["sample"]) for p in s])
    if rows is not None:
        assert rows == ax["sample"]
        return np.asarray(want)
    return np.asarray(want)[ax["sample"]]


def composition_reference(case, ax, oracle):
    """[table of side A, table of side B or None]: composition_util.profile of every sampled environment, (len(items), C) each; the
    CDF is the oracle's WeightFunction.integral_vec."""
    w = np.ones(case["ncat"]) if case["weights"] is None else np.asarray(case["weights"])
    cdfs = {}

    def cdf_of(key):
        if key not in cdfs:
            wf = oracle.WeightFunction(*_wf(case, key))
            cdfs[key] = lambda x, wf=wf: np.asarray(wf.integral_vec(np.asarray(x, dtype=np.float64).tolist()))
        return cdfs[key]

    items = environments(case, ax).items
    tables = []
    for side in (2, 3):
        if any(it[side] is None for it in items):
            tables.append(None)
            continue
        tables.append(np.stack([cu.profile(it[side][1], it[side][0], w, cdf_of(it[1])) for it in items]))
    return tables


def tv_check(case, ax, oracle, tables, n_items=2):
    """(reference, oracle) of composition_util.tv_identity on two sampled environments: all categories up to 40 of them, otherwise
    those of the environment and the highest id."""
    items = environments(case, ax).items
    rng = np.random.default_rng(STREAM + 500_000_000 + case["seed"])
    w = np.ones(case["ncat"]) if case["weights"] is None else np.asarray(case["weights"])
    mine, theirs = [], []
    for i in rng.choice(len(items), min(n_items, len(items)), replace=False):
        _, key, (cat, dist) = items[i][:3]
        order = np.argsort(dist, kind="stable")  # from_anchors takes a sorted environment (which point at distance 0 leads is immaterial)
        cat, dist = cat[order], np.asarray(dist)[order]
        ids = np.arange(case["ncat"]) if case["ncat"] <= 40 else np.unique(np.concatenate([cat, [case["ncat"] - 1]]))
        names = [case["cats"][c] for c in ids]
        wf = {k: oracle.WeightFunction(*s) for k, s in case["wfs"].items()} if case["multi"] else oracle.WeightFunction(*case["wfs"])
        theirs.append(cu.tv_identity(oracle, names, w[ids].tolist(), wf, [case["cats"][c] for c in cat], np.asarray(dist).tolist(), key))
        mine.append(tables[0][i][ids])
        rest = np.setdiff1d(np.arange(case["ncat"]), ids)
        assert np.all(tables[0][i][rest] == 0.0)  # a category outside the environment has no share
    return mine, theirs


def spans(case, ax, oracle):
    """F(inf) - F(0) of every item's weight function: what a composition row sums to."""
    out = []
    for it in environments(case, ax).items:
        f0, finf = oracle.WeightFunction(*_wf(case, it[1])).integral_vec([0.0, np.inf])
        out.append(finf - f0)
    return np.asarray(out)
