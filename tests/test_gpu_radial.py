"""Radial score profiles on the device against identities of the CPU oracle and the numpy restatement they pin.

Expected values never come from the library:
  uniform identity   under uniform[a, b], bin_k = (e'_{k+1} - e'_k) / (b - a) * oracle_score(uniform[e'_k, e'_{k+1}]), e' clipped to [a, b]
  restatement        tests/radial_util.py (longdouble, from the definition), which tests/test_radial_model.py pins to the oracle to 1e-12
  row sums           the oracle's / the library's scoring call of the same name
Bound: the project's parity bound, 1e-11 absolute, unless a test states another (row sums against the deterministic-mode score: 1e-13,
two f64 summation orders of a few hundred terms of size <= 1)."""
import numpy as np
import pytest

import radial_util as ru
from min_image_util import brute_rows

pytestmark = pytest.mark.gpu

TOL = 1e-11
INF = float("inf")
CATS7 = [f"c{k}" for k in range(7)]
UNI = ("uniform", [3.0, 10.0])
FAMILIES = {"hyper_exp": [1.0, 0.5, 0.2, 0.05], "dagum": [4.0, 6.0, 1.5], "kumaraswamy": [2.0, 11.0, 2.0, 3.0]}
DISTANCES = {
    "hellinger2": ("Hellinger", [2.0]),
    "hellinger1": ("Hellinger", [1.0]),
    "hellinger3.5": ("Hellinger", [3.5]),
    "ks": ("Kolmogorov-Smirnov", []),
    "kl": ("Kullback-Leibler", [1e-3]),
    "renyi": ("Renyi", [2.5, 1e-3]),
}
EDGES = [0.0, 2.0, 3.0, 4.5, 6.0, 7.25, 9.0, 10.0, 12.0, INF]


def _lh():
    import loco_hd_amd as lh

    return lh


def _atoms(mod, types, tags, xyz):
    return [mod.PrimitiveAtom(t, g, list(c)) for t, g, c in zip(types, tags, xyz)]


class Cloud:
    def __init__(self, seed, n, edge, cats, n_tags=4):
        rng = np.random.default_rng(seed)
        self.xyz = rng.uniform(0.0, edge, (n, 3))
        self.cat_ids = rng.integers(0, len(cats), n)
        self.types = [cats[k] for k in self.cat_ids]
        self.tag_ids = rng.integers(0, n_tags, n)
        self.tags = [f"t{k}" for k in self.tag_ids]
        self.atoms = _atoms(_lh(), self.types, self.tags, self.xyz)


@pytest.fixture(scope="module")
def two_clouds():
    return Cloud(101, 300, 20.0, CATS7), Cloud(102, 300, 20.0, CATS7)


@pytest.fixture(scope="module")
def pairs40():
    rng = np.random.default_rng(9)
    return [(int(i), int(j)) for i, j in rng.integers(0, 300, (40, 2))]


def _check(got, want, what, tol=TOL):
    got = np.asarray(got)
    err = float(np.max(np.abs(got - want)))
    print(f"{what}: max |device - expected| = {err:.3g}")
    assert np.isfinite(got).all()
    assert err <= tol, what


def _restated(a, b, pairs, thr, wf, edges=EDGES, sd=("Hellinger", [2.0]), weights=None, accept_same=True):
    return ru.from_primitives(a.cat_ids, a.xyz, a.tag_ids, b.cat_ids, b.xyz, b.tag_ids, pairs, thr, len(CATS7), wf, edges, sd, weights, accept_same)


# ---- thresholded parity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dist", sorted(DISTANCES))
def test_uniform_identity(oracle, two_clouds, pairs40, dist):
    lh, (a, b) = _lh(), two_clouds
    sd = DISTANCES[dist]
    got = lh.LoCoHD(CATS7, lh.WeightFunction(*UNI), statistical_distance=lh.StatisticalDistance(*sd)).radial_from_primitives(
        a.atoms, b.atoms, pairs40, 8.0, EDGES)
    assert got.shape == (40, len(EDGES) - 1)
    pa, pb = _atoms(oracle, a.types, a.tags, a.xyz), _atoms(oracle, b.types, b.tags, b.xyz)
    want = np.zeros_like(got)
    for k in range(len(EDGES) - 1):
        lo, hi = min(max(EDGES[k], 3.0), 10.0), min(max(EDGES[k + 1], 3.0), 10.0)
        if hi > lo:
            sub = oracle.LoCoHD(CATS7, oracle.WeightFunction("uniform", [lo, hi]), statistical_distance=oracle.StatisticalDistance(*sd))
            want[:, k] = (hi - lo) / 7.0 * np.asarray(sub.from_primitives(pa, pb, pairs40, 8.0))
        else:
            assert np.all(got[:, k] == 0.0)
    _check(got, want, f"uniform identity, {dist}")


@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("dist", ["hellinger2", "ks", "kl"])
def test_other_families_against_the_restatement(two_clouds, pairs40, family, dist):
    lh, (a, b) = _lh(), two_clouds
    wf, sd = (family, FAMILIES[family]), DISTANCES[dist]
    got = lh.LoCoHD(CATS7, lh.WeightFunction(*wf), statistical_distance=lh.StatisticalDistance(*sd)).radial_from_primitives(
        a.atoms, b.atoms, pairs40, 7.0, EDGES)
    _check(got, _restated(a, b, pairs40, 7.0, wf, sd=sd), f"{family}, {dist}")


@pytest.mark.parametrize("accept_same", [True, False])
@pytest.mark.parametrize("dist", ["hellinger2", "hellinger1"])
def test_category_weights_and_tag_rules(two_clouds, pairs40, accept_same, dist):
    lh, (a, b) = _lh(), two_clouds
    weights = np.random.default_rng(3).uniform(0.3, 3.0, 7)
    sd = DISTANCES[dist]
    l = lh.LoCoHD(CATS7, lh.WeightFunction(*UNI), lh.TagPairingRule({"accept_same": accept_same}), category_weights=list(weights),
                  statistical_distance=lh.StatisticalDistance(*sd))
    got = l.radial_from_primitives(a.atoms, b.atoms, pairs40, 9.0, EDGES)
    _check(got, _restated(a, b, pairs40, 9.0, UNI, sd=sd, weights=weights, accept_same=accept_same), f"weights, accept_same={accept_same}, {dist}")


def test_weight_function_dictionary_with_per_pair_keys(two_clouds, pairs40):
    lh, (a, b) = _lh(), two_clouds
    specs = {"u": UNI, "h": ("hyper_exp", FAMILIES["hyper_exp"]), "d": ("dagum", FAMILIES["dagum"])}
    keys = [("u", "h", "d")[p % 3] for p in range(len(pairs40))]
    l = lh.LoCoHD(CATS7, {k: lh.WeightFunction(*v) for k, v in specs.items()})
    got = l.radial_from_primitives(a.atoms, b.atoms, [(i, j, k) for (i, j), k in zip(pairs40, keys)], 8.0, EDGES)
    _check(got, _restated(a, b, pairs40, 8.0, [specs[k] for k in keys]), "dictionary, per-pair keys")


# ---- edges and sums -------------------------------------------------------------------------------------------------------------------
def test_one_bin_and_64_bins_and_row_sums(two_clouds, pairs40):
    lh, (a, b) = _lh(), two_clouds
    l = lh.LoCoHD(CATS7, lh.WeightFunction(*UNI), deterministic=True)
    score = np.asarray(l.from_primitives(a.atoms, b.atoms, pairs40, 8.0))
    one = l.radial_from_primitives(a.atoms, b.atoms, pairs40, 8.0, [0.0, INF])
    assert one.shape == (40, 1)
    _check(one[:, 0], score, "K = 1 against the deterministic-mode score", 1e-13)
    e64 = list(np.linspace(0.0, 11.0, 64)) + [INF]
    fine = l.radial_from_primitives(a.atoms, b.atoms, pairs40, 8.0, e64)
    assert fine.shape == (40, 64)
    _check(fine, _restated(a, b, pairs40, 8.0, UNI, edges=e64), "K = 64")
    _check(fine.sum(1), score, "row sums of K = 64", 1e-13)
    _check(l.radial_from_primitives(a.atoms, b.atoms, pairs40, 8.0, EDGES).sum(1), score, "row sums of K = 9", 1e-13)


def test_edges_outside_the_support_and_dropped_tail(two_clouds, pairs40):
    lh, (a, b) = _lh(), two_clouds
    l = lh.LoCoHD(CATS7, lh.WeightFunction(*UNI))
    below = l.radial_from_primitives(a.atoms, b.atoms, pairs40, 8.0, [0.0, 1.0, 2.0, 3.0])
    assert below.shape == (40, 3) and np.all(below == 0.0) and not np.any(np.signbit(below))
    # a finite last edge below the threshold: the mass beyond it, the tail included, is dropped
    cut = [0.0, 4.0, 6.5]
    got = l.radial_from_primitives(a.atoms, b.atoms, pairs40, 8.0, cut)
    _check(got, _restated(a, b, pairs40, 8.0, UNI, edges=cut), "finite last edge")
    full = l.radial_from_primitives(a.atoms, b.atoms, pairs40, 8.0, cut + [INF])
    assert np.all(full[:, 2] > 0.0)  # (every pair has mass beyond 6.5: the tail alone is (1 - F(8)) H > 0 unless H = 0)
    _check(got, full[:, :2], "the first bins do not depend on what follows", 1e-15)


# ---- ties -----------------------------------------------------------------------------------------------------------------------------
def test_lattice_with_edges_on_lattice_distances():
    lh = _lh()
    rng = np.random.default_rng(77)
    g = np.stack(np.meshgrid(*[np.arange(6.0)] * 3, indexing="ij"), -1).reshape(-1, 3) * 1.5  # 216 points, spacing 1.5
    ca, cb = rng.integers(0, 7, len(g)), rng.integers(0, 7, len(g))
    pa = _atoms(lh, [CATS7[k] for k in ca], ["x"] * len(g), g)
    pb = _atoms(lh, [CATS7[k] for k in cb], ["x"] * len(g), g)
    pairs = [(int(i), int(j)) for i, j in rng.integers(0, len(g), (30, 2))]
    edges = [0.0, 1.5, 3.0, 1.5 * np.sqrt(5.0), 4.5, 6.0, INF]  # lattice distances: whole shells of tied points sit ON an edge
    for wf in (UNI, ("hyper_exp", FAMILIES["hyper_exp"])):
        for det in (False, True):
            got = lh.LoCoHD(CATS7, lh.WeightFunction(*wf), deterministic=det).radial_from_primitives(pa, pb, pairs, 6.1, edges)
            want = ru.from_primitives(ca, g, None, cb, g, None, pairs, 6.1, 7, wf, edges)
            _check(got, want, f"lattice, {wf[0]}, deterministic={det}")


# ---- environment sizes (dense rows) ---------------------------------------------------------------------------------------------------
SIZES = [1, 2, 63, 64, 65, 128, 129, 600]


@pytest.mark.parametrize("n_a,n_b", list(zip(SIZES, SIZES[::-1])) + [(64, 64), (600, 600)])
@pytest.mark.parametrize("dist", ["hellinger2", "ks"])
def test_row_sizes(oracle, n_a, n_b, dist):
    lh = _lh()
    rng = np.random.default_rng(n_a * 1000 + n_b)
    rows = 5
    sd = DISTANCES[dist]

    def side(n):
        m = np.round(rng.uniform(0.0, 12.0, (rows, n)), 2)
        m[rng.uniform(size=m.shape) < 0.1] = INF
        m[np.arange(rows), np.arange(rows) % n] = 0.0
        return m, rng.integers(0, 7, n)

    (ma, ca), (mb, cb) = side(n_a), side(n_b)
    sa, sb = [CATS7[k] for k in ca], [CATS7[k] for k in cb]
    wf = ("hyper_exp", FAMILIES["hyper_exp"])
    got = lh.LoCoHD(CATS7, lh.WeightFunction(*wf), statistical_distance=lh.StatisticalDistance(*sd)).radial_from_dmxs(sa, sb, ma, mb, EDGES)
    _check(got, ru.from_rows(ca, ma, cb, mb, 7, wf, EDGES, sd), f"rows of {n_a} / {n_b} points, {dist}")
    want = oracle.LoCoHD(CATS7, oracle.WeightFunction(*wf), statistical_distance=oracle.StatisticalDistance(*sd)).from_dmxs(sa, sb, ma, mb)
    _check(got.sum(1), np.asarray(want), "row sums against the oracle's from_dmxs")


# ---- overflow -------------------------------------------------------------------------------------------------------------------------
def test_overflowing_blob_repeats_the_pass():
    lh = _lh()
    rng = np.random.default_rng(13)
    blob = rng.normal(0.0, 1.0, (700, 3)) * 0.8 + 20.0  # 700 atoms well inside one threshold: more than a 512-point slot
    sparse = rng.uniform(0.0, 40.0, (150, 3))
    xyz = np.vstack([blob, sparse])
    cat = rng.integers(0, 7, len(xyz))
    atoms = _atoms(lh, [CATS7[k] for k in cat], ["x"] * len(xyz), xyz)
    pairs = [(0, 5), (3, 720), (701, 702), (710, 10), (849, 848), (700, 700)]
    got = lh.LoCoHD(CATS7, lh.WeightFunction(*UNI)).radial_from_primitives(atoms, atoms, pairs, 7.0, EDGES)
    _check(got, ru.from_primitives(cat, xyz, None, cat, xyz, None, pairs, 7.0, 7, UNI, EDGES), "700-atom blob, small environments included")


# ---- categories -----------------------------------------------------------------------------------------------------------------------
def test_300_categories_and_the_limit():
    lh = _lh()
    rng = np.random.default_rng(17)
    cats = [f"k{k}" for k in range(300)]
    n = 300
    xyz_a, xyz_b = rng.uniform(0.0, 20.0, (n, 3)), rng.uniform(0.0, 20.0, (n, 3))
    ca, cb = rng.integers(0, 300, n), rng.integers(0, 300, n)
    ca[:2], cb[:2] = [299, 256], [255, 299]  # ids on both sides of the one-byte limit
    pa, pb = _atoms(lh, [cats[k] for k in ca], ["x"] * n, xyz_a), _atoms(lh, [cats[k] for k in cb], ["x"] * n, xyz_b)
    pairs = [(0, 0), (1, 1)] + [(int(i), int(j)) for i, j in rng.integers(0, n, (10, 2))]
    for sd in (("Hellinger", [2.0]), ("Kolmogorov-Smirnov", [])):
        got = lh.LoCoHD(cats, lh.WeightFunction(*UNI), statistical_distance=lh.StatisticalDistance(*sd)).radial_from_primitives(pa, pb, pairs, 8.0, EDGES)
        _check(got, ru.from_primitives(ca, xyz_a, None, cb, xyz_b, None, pairs, 8.0, 300, UNI, EDGES, sd), f"300 categories, {sd[0]}")
    cats513 = [f"k{k}" for k in range(513)]
    with pytest.raises(NotImplementedError, match="512 categories"):
        lh.LoCoHD(cats513, lh.WeightFunction(*UNI)).radial_from_primitives(pa[:5], pb[:5], [(0, 0)], 8.0, EDGES)


@pytest.mark.parametrize("n_cat", [64, 65, 255, 256, 257])
def test_category_counts_at_the_kernel_switches(n_cat):
    """64 / 65: four pairs per workgroup against one (one-byte ids); 255 / 256 / 257: the one-byte against the 16-bit store.  The
    highest id sits on an anchor and on an atom that is no anchor but inside an anchor's environment, on both sides."""
    lh = _lh()
    rng = np.random.default_rng(1000 + n_cat)
    cats = [f"k{k}" for k in range(n_cat)]
    n, thr = 120, 7.0
    pairs = [(int(i), int(j)) for i, j in rng.integers(0, n, (12, 2))]
    sides = []
    for col in (0, 1):
        xyz, cat = rng.uniform(0.0, 14.0, (n, 3)), rng.integers(0, n_cat, n)
        anchors = {p[col] for p in pairs}
        first = pairs[0][col]
        near = [int(q) for q in np.argsort(np.linalg.norm(xyz - xyz[first], axis=1)) if q not in anchors][0]
        assert np.linalg.norm(xyz[near] - xyz[first]) < thr
        cat[first] = cat[near] = n_cat - 1
        sides.append((xyz, cat, _atoms(lh, [cats[k] for k in cat], ["x"] * n, xyz)))
    (xa, ca, pa), (xb, cb, pb) = sides
    weights = rng.uniform(0.3, 3.0, n_cat)
    for dist in ("hellinger2", "ks"):
        for w in (None, weights):
            l = lh.LoCoHD(cats, lh.WeightFunction(*UNI), category_weights=None if w is None else list(w),
                          statistical_distance=lh.StatisticalDistance(*DISTANCES[dist]))
            got = l.radial_from_primitives(pa, pb, pairs, thr, EDGES)
            want = ru.from_primitives(ca, xa, None, cb, xb, None, pairs, thr, n_cat, UNI, EDGES, DISTANCES[dist], w)
            _check(got, want, f"{n_cat} categories, {dist}, {'weighted' if w is not None else 'unit weights'}")


def test_63_bins_and_one_bin_too_many(two_clouds, pairs40):
    lh, (a, b) = _lh(), two_clouds
    l = lh.LoCoHD(CATS7, lh.WeightFunction(*UNI))
    e63 = list(np.linspace(0.0, 11.0, 63)) + [INF]
    got = l.radial_from_primitives(a.atoms, b.atoms, pairs40, 8.0, e63)
    assert got.shape == (40, 63)
    _check(got, _restated(a, b, pairs40, 8.0, UNI, edges=e63), "K = 63")
    with pytest.raises(ValueError):
        l.radial_from_primitives(a.atoms, b.atoms, pairs40, 8.0, list(np.linspace(0.0, 11.0, 65)) + [INF])  # K = 65


# ---- dense and device-resident calls --------------------------------------------------------------------------------------------------
def test_from_coords_open_and_in_a_cell():
    lh = _lh()
    rng = np.random.default_rng(19)
    n = 90
    xa, xb = rng.uniform(0.0, 14.0, (n, 3)), rng.uniform(0.0, 14.0, (n, 3))
    ca, cb = rng.integers(0, 7, n), rng.integers(0, 7, n)
    sa, sb = [CATS7[k] for k in ca], [CATS7[k] for k in cb]
    l = lh.LoCoHD(CATS7, lh.WeightFunction(*UNI))

    def open_rows(x):
        d = x[:, None, :] - x[None, :, :]
        return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])

    _check(l.radial_from_coords(sa, sb, xa, xb, EDGES), ru.from_rows(ca, open_rows(xa), cb, open_rows(xb), 7, UNI, EDGES), "from_coords, open")
    cell = np.asarray([[14.0, 0.0, 0.0], [3.0, 13.0, 0.0], [-2.0, 4.0, 15.0]])
    rows_a = np.asarray(brute_rows(xa, range(n), cell))
    _check(l.radial_from_coords(sa, sb, xa, xb, EDGES, cell_a=cell), ru.from_rows(ca, rows_a, cb, open_rows(xb), 7, UNI, EDGES), "from_coords, cell_a")


def test_device_session_image_cloud_batch_and_coords(two_clouds):
    lh, (a, b) = _lh(), two_clouds
    from loco_hd_amd.device import DeviceSession

    rng = np.random.default_rng(23)
    l = lh.LoCoHD(CATS7, lh.WeightFunction(*UNI))
    sess = DeviceSession(l)
    try:
        torch = sess.torch
        tag = {f"t{k}": k for k in range(4)}
        pk = [(c.xyz, c.cat_ids.astype(np.int32), np.asarray([tag[t] for t in c.tags], dtype=np.int32)) for c in (a, b)]
        # a batch of the two structures: pair (i of structure 0, j of structure 1) through global indices
        batch, offs = sess.upload_batch(pk)
        pairs = rng.integers(0, 300, (50, 2))
        anc = torch.from_numpy(pairs + np.asarray([offs[0], offs[1]])).cuda()
        got = sess.radial(batch, batch, anc, 8.0, EDGES)
        assert tuple(got.shape) == (50, len(EDGES) - 1)
        _check(got.cpu().numpy(), _restated(a, b, pairs, 8.0, UNI), "DeviceSession.radial on a batch")
        # an image cloud of structure a in a box of its own edge against the open structure b
        box = np.asarray([20.0, 20.0, 20.0])
        ca_, cb_ = sess.upload(*pk[0]), sess.upload(*pk[1])
        img = sess.periodic_images(ca_, box, 8.0)
        out = torch.full((50, len(EDGES) - 1), -1.0, dtype=torch.float64, device="cuda")
        assert sess.radial(img, cb_, torch.from_numpy(pairs).cuda(), 8.0, EDGES, out=out) is out
        shifts = np.stack(np.meshgrid(*[np.arange(-1.0, 2.0)] * 3, indexing="ij"), -1).reshape(-1, 3) * box
        order = np.argsort(np.abs(shifts).sum(1) > 0, kind="stable")  # the originals first: anchor index i is atom i
        xyz_img = (a.xyz[None, :, :] + shifts[order][:, None, :]).reshape(-1, 3)
        want = ru.from_primitives(np.tile(a.cat_ids, 27), xyz_img, np.tile(a.tag_ids, 27), b.cat_ids, b.xyz, b.tag_ids, pairs, 8.0, 7, UNI, EDGES)
        _check(out.cpu().numpy(), want, "DeviceSession.radial on an image cloud")
        # dense rows of two device clouds
        small = [(c.xyz[:70], c.cat_ids[:70].astype(np.int32), None) for c in (a, b)]
        da, db = sess.upload(*small[0]), sess.upload(*small[1])
        got = sess.radial_coords(da, db, EDGES).cpu().numpy()

        def open_rows(x):
            d = x[:, None, :] - x[None, :, :]
            return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])

        _check(got, ru.from_rows(small[0][1], open_rows(small[0][0]), small[1][1], open_rows(small[1][0]), 7, UNI, EDGES), "radial_coords on device clouds")
    finally:
        sess.close()


# ---- determinism and non-interference -------------------------------------------------------------------------------------------------
def test_deterministic_rows_are_a_function_of_the_pair(two_clouds, pairs40):
    lh, (a, b) = _lh(), two_clouds
    l = lh.LoCoHD(CATS7, lh.WeightFunction(*UNI), deterministic=True)
    base = l.radial_from_primitives(a.atoms, b.atoms, pairs40, 8.0, EDGES)
    alone = np.vstack([l.radial_from_primitives(a.atoms, b.atoms, [p], 8.0, EDGES) for p in pairs40[:6]])
    assert np.array_equal(alone, base[:6])
    perm = np.random.default_rng(1).permutation(len(pairs40))
    assert np.array_equal(l.radial_from_primitives(a.atoms, b.atoms, [pairs40[k] for k in perm], 8.0, EDGES), base[perm])
    rng = np.random.default_rng(2)
    larger = pairs40 + [(int(i), int(j)) for i, j in rng.integers(0, 300, (500, 2))]
    assert np.array_equal(l.radial_from_primitives(a.atoms, b.atoms, larger, 8.0, EDGES)[:40], base)
    fresh = lh.LoCoHD(CATS7, lh.WeightFunction(*UNI), deterministic=True)
    assert np.array_equal(fresh.radial_from_primitives(a.atoms, b.atoms, pairs40, 8.0, EDGES), base)


@pytest.mark.parametrize("det", [False, True])
def test_scores_and_the_sweep_record_are_left_alone(two_clouds, det):
    lh, (a, b) = _lh(), two_clouds
    from loco_hd_amd.device import DeviceSession

    rng = np.random.default_rng(29)
    sess = DeviceSession(lh.LoCoHD(CATS7, lh.WeightFunction(*UNI), deterministic=det))
    try:
        torch = sess.torch
        tag = {f"t{k}": k for k in range(4)}
        ca, cb = [sess.upload(c.xyz, c.cat_ids.astype(np.int32), np.asarray([tag[t] for t in c.tags], dtype=np.int32)) for c in (a, b)]
        anc = torch.from_numpy(rng.integers(0, 300, (6000, 2))).cuda()
        for _ in range(2):  # (the second call runs with the hints of the first)
            before = sess.from_primitives(ca, cb, anc, 8.0).clone()
        rec = sess.last_sweep()
        assert rec is not None
        sess.radial(ca, cb, anc[:500], 8.0, EDGES)
        assert sess.last_sweep() == rec
        after = sess.from_primitives(ca, cb, anc, 8.0)
        assert torch.equal(before, after)
        assert sess.last_sweep() == rec
    finally:
        sess.close()


# ---- errors ---------------------------------------------------------------------------------------------------------------------------
def test_errors(two_clouds):
    lh, (a, b) = _lh(), two_clouds
    from loco_hd_amd import _native as N

    l = lh.LoCoHD(CATS7, lh.WeightFunction(*UNI))
    with pytest.raises(N.PanicException):
        l.radial_from_primitives(a.atoms, b.atoms, [(0, 300)], 8.0, EDGES)
    odd = a.atoms[:10] + [lh.PrimitiveAtom("not-in-the-map", "t0", list(a.xyz[0] + 0.5))]
    with pytest.raises(ValueError):
        l.radial_from_primitives(odd, b.atoms, [(0, 0)], 8.0, EDGES)
    with pytest.raises(ValueError, match="one device"):
        lh.LoCoHD(CATS7, lh.WeightFunction(*UNI), devices=[0]).radial_from_primitives(a.atoms, b.atoms, [(0, 0)], 8.0, EDGES)
