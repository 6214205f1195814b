"""Score attribution by category on the device against the numpy restatement (tests/attribution_util.py, longdouble, from the definition;
tests/test_attribution_model.py pins it to the oracle to 1e-12) and, directly, against the CPU oracle: every row sums to the oracle's
score of the pair, and under exponent 1 every column is half a two-category oracle score.

Expected values never come from the library.  Bound: the project's parity bound, 1e-11 absolute, unless a test states another."""
import numpy as np
import pytest

import attribution_util as au
from min_image_util import brute_rows

pytestmark = pytest.mark.gpu

TOL = 1e-11
INF = float("inf")
TILE = 384  # kSweepTile (loco_hd_amd/csrc/lchd_device.h): merged events per tile of the kernel
CATS7 = [f"c{k}" for k in range(7)]
UNI = ("uniform", [3.0, 10.0])
FAMILIES = {"hyper_exp": [1.0, 0.5, 0.2, 0.05], "dagum": [4.0, 6.0, 1.5], "kumaraswamy": [2.0, 11.0, 2.0, 3.0]}
OTHER_DISTANCES = {"ks": ("Kolmogorov-Smirnov", []), "kl": ("Kullback-Leibler", [1e-3]), "renyi": ("Renyi", [2.5, 1e-3])}


def _lh():
    import loco_hd_amd as lh

    return lh


def _atoms(mod, types, tags, xyz):
    return [mod.PrimitiveAtom(t, g, list(c)) for t, g, c in zip(types, tags, xyz)]


class Cloud:
    def __init__(self, seed, n, edge, cats, n_tags=4, n_used=None):
        """n_used: only the first n_used categories occur, and every one of them does."""
        rng = np.random.default_rng(seed)
        self.xyz = rng.uniform(0.0, edge, (n, 3))
        self.cat_ids = rng.integers(0, len(cats) if n_used is None else n_used, n)
        if n_used is not None:
            self.cat_ids[:n_used] = np.arange(n_used)
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
    err = float(np.max(np.abs(got - want))) if got.size else 0.0
    print(f"{what}: max |device - expected| = {err:.3g}")
    assert got.shape == np.asarray(want).shape, what
    assert np.isfinite(got).all()
    assert err <= tol, what


def _restated(a, b, pairs, thr, wf, e=2.0, weights=None, accept_same=True, n_cat=7):
    return au.from_primitives(a.cat_ids, a.xyz, a.tag_ids, b.cat_ids, b.xyz, b.tag_ids, pairs, thr, n_cat, wf, e, weights, accept_same)


def _oracle_scores(oracle, cats, a, b, pairs, thr, wf, e=2.0, weights=None, accept_same=True):
    """wf: one (name, params), or a dictionary of them with `pairs` carrying the keys."""
    w = {k: oracle.WeightFunction(*v) for k, v in wf.items()} if isinstance(wf, dict) else oracle.WeightFunction(*wf)
    l = oracle.LoCoHD(cats, w, oracle.TagPairingRule({"accept_same": accept_same}), category_weights=None if weights is None else list(weights),
                      statistical_distance=oracle.StatisticalDistance("Hellinger", [e]))
    return np.asarray(l.from_primitives(_atoms(oracle, a.types, a.tags, a.xyz), _atoms(oracle, b.types, b.tags, b.xyz), pairs, thr))


# ---- thresholded parity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("e", [2.0, 1.0, 3.5])
def test_exponents_under_uniform(oracle, two_clouds, pairs40, e):
    lh, (a, b) = _lh(), two_clouds
    got = lh.LoCoHD(CATS7, lh.WeightFunction(*UNI), statistical_distance=lh.StatisticalDistance("Hellinger", [e])).attribution_from_primitives(
        a.atoms, b.atoms, pairs40, 8.0)
    _check(got, _restated(a, b, pairs40, 8.0, UNI, e), f"uniform, exponent {e}")
    _check(got.sum(1), _oracle_scores(oracle, CATS7, a, b, pairs40, 8.0, UNI, e), f"row sums against the oracle, exponent {e}")


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_other_families(oracle, two_clouds, pairs40, family):
    lh, (a, b) = _lh(), two_clouds
    wf = (family, FAMILIES[family])
    got = lh.LoCoHD(CATS7, lh.WeightFunction(*wf)).attribution_from_primitives(a.atoms, b.atoms, pairs40, 8.0)
    _check(got, _restated(a, b, pairs40, 8.0, wf), family)
    _check(got.sum(1), _oracle_scores(oracle, CATS7, a, b, pairs40, 8.0, wf), f"row sums against the oracle, {family}")


@pytest.mark.parametrize("accept_same", [True, False])
@pytest.mark.parametrize("e", [2.0, 3.5])
def test_category_weights_and_tag_rules(oracle, two_clouds, pairs40, accept_same, e):
    lh, (a, b) = _lh(), two_clouds
    weights = np.random.default_rng(3).uniform(0.3, 3.0, 7)
    l = lh.LoCoHD(CATS7, lh.WeightFunction(*UNI), lh.TagPairingRule({"accept_same": accept_same}), category_weights=list(weights),
                  statistical_distance=lh.StatisticalDistance("Hellinger", [e]))
    got = l.attribution_from_primitives(a.atoms, b.atoms, pairs40, 8.0)
    _check(got, _restated(a, b, pairs40, 8.0, UNI, e, weights, accept_same), f"weights, accept_same={accept_same}, exponent {e}")
    _check(got.sum(1), _oracle_scores(oracle, CATS7, a, b, pairs40, 8.0, UNI, e, weights, accept_same), "row sums against the oracle")


def test_weight_function_dictionary_with_per_pair_keys(oracle, two_clouds, pairs40):
    lh, (a, b) = _lh(), two_clouds
    specs = {"u": UNI, "h": ("hyper_exp", FAMILIES["hyper_exp"]), "d": ("dagum", FAMILIES["dagum"])}
    keys = [("u", "h", "d")[p % 3] for p in range(len(pairs40))]
    keyed = [(i, j, k) for (i, j), k in zip(pairs40, keys)]
    got = lh.LoCoHD(CATS7, {k: lh.WeightFunction(*v) for k, v in specs.items()}).attribution_from_primitives(a.atoms, b.atoms, keyed, 8.0)
    _check(got, _restated(a, b, pairs40, 8.0, [specs[k] for k in keys]), "dictionary, per-pair keys")
    _check(got.sum(1), _oracle_scores(oracle, CATS7, a, b, keyed, 8.0, specs), "row sums against the oracle, dictionary")


def test_exponent_1_columns_are_two_category_oracle_scores(oracle, two_clouds, pairs40):
    """Two-category total variation is |a_c - b_c|: column c is 1/2 of the oracle's score with every other category relabelled "rest"."""
    lh, (a, b) = _lh(), two_clouds
    got = lh.LoCoHD(CATS7, lh.WeightFunction(*UNI), statistical_distance=lh.StatisticalDistance("Hellinger", [1.0])).attribution_from_primitives(
        a.atoms, b.atoms, pairs40, 8.0)
    l2 = oracle.LoCoHD(["c", "rest"], oracle.WeightFunction(*UNI), statistical_distance=oracle.StatisticalDistance("Hellinger", [1.0]))
    want = np.zeros_like(got)
    for c in range(7):
        pa = _atoms(oracle, ["c" if k == c else "rest" for k in a.cat_ids], a.tags, a.xyz)
        pb = _atoms(oracle, ["c" if k == c else "rest" for k in b.cat_ids], b.tags, b.xyz)
        want[:, c] = 0.5 * np.asarray(l2.from_primitives(pa, pb, pairs40, 8.0))
    _check(got, want, "exponent 1 against the two-category projection")


# ---- properties -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("e,weighted", [(2.0, False), (2.0, True), (3.5, False)])
def test_identical_environments_give_exact_zeros_and_sides_swap(two_clouds, pairs40, e, weighted):
    lh, (a, b) = _lh(), two_clouds
    weights = list(np.random.default_rng(3).uniform(0.3, 3.0, 7)) if weighted else None
    l = lh.LoCoHD(CATS7, lh.WeightFunction(*UNI), category_weights=weights, statistical_distance=lh.StatisticalDistance("Hellinger", [e]))
    same = l.attribution_from_primitives(a.atoms, a.atoms, [(i, i) for i, _ in pairs40], 8.0)
    assert same.shape == (40, 7) and np.all(same == 0.0)
    ab = l.attribution_from_primitives(a.atoms, b.atoms, pairs40, 8.0)
    ba = l.attribution_from_primitives(b.atoms, a.atoms, [(j, i) for i, j in pairs40], 8.0)
    assert np.all(ab >= 0.0) and np.any(ab > 0.0)
    _check(ba, ab, "swapped sides", 1e-13)


# ---- environment sizes (dense rows) ---------------------------------------------------------------------------------------------------
EVENTS = [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 3]  # non-anchor events of a side


@pytest.mark.parametrize("ev_a,ev_b", list(zip(EVENTS, EVENTS[::-1])))
@pytest.mark.parametrize("e", [2.0, 3.5])
def test_row_sizes(oracle, ev_a, ev_b, e):
    lh = _lh()
    rng = np.random.default_rng(ev_a * 1000 + ev_b)
    rows = 4

    def side(n):
        m = np.round(rng.uniform(0.0, 12.0, (rows, n)), 2)  # two decimals: ties within and across the sides
        m[rng.uniform(size=m.shape) < 0.1] = INF
        m[np.arange(rows), np.arange(rows) % n] = 0.0
        return m, rng.integers(0, 7, n)

    (ma, ca), (mb, cb) = side(ev_a + 1), side(ev_b + 1)
    sa, sb = [CATS7[k] for k in ca], [CATS7[k] for k in cb]
    wf = ("hyper_exp", FAMILIES["hyper_exp"])
    got = lh.LoCoHD(CATS7, lh.WeightFunction(*wf), statistical_distance=lh.StatisticalDistance("Hellinger", [e])).attribution_from_dmxs(sa, sb, ma, mb)
    _check(got, au.from_rows(ca, ma, cb, mb, 7, wf, e), f"rows of {ev_a} / {ev_b} events, exponent {e}")
    want = oracle.LoCoHD(CATS7, oracle.WeightFunction(*wf), statistical_distance=oracle.StatisticalDistance("Hellinger", [e])).from_dmxs(sa, sb, ma, mb)
    _check(got.sum(1), np.asarray(want), "row sums against the oracle's from_dmxs")


# ---- categories -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cat,all_present", [(1, True), (2, True), (2, False), (63, True), (63, False), (64, True), (64, False)])
def test_category_counts(oracle, n_cat, all_present):
    """63 / 64: the largest accumulator blocks (fewer pairs per workgroup).  all_present False: the upper half of the categories (of two:
    the second) occurs in neither cloud, and those columns are exactly 0."""
    lh = _lh()
    cats = [f"k{k}" for k in range(n_cat)]
    n_used = n_cat if all_present else max(1, n_cat // 2)
    a, b = Cloud(500 + n_cat, 200, 14.0, cats, n_used=n_used), Cloud(600 + n_cat, 200, 14.0, cats, n_used=n_used)
    assert len(set(a.cat_ids)) == len(set(b.cat_ids)) == n_used
    rng = np.random.default_rng(n_cat)
    pairs = [(int(i), int(j)) for i, j in rng.integers(0, 200, (12, 2))]
    weights = rng.uniform(0.3, 3.0, n_cat)
    for e, w in ((2.0, None), (2.0, weights), (3.5, None)):
        l = lh.LoCoHD(cats, lh.WeightFunction(*UNI), category_weights=None if w is None else list(w),
                      statistical_distance=lh.StatisticalDistance("Hellinger", [e]))
        got = l.attribution_from_primitives(a.atoms, b.atoms, pairs, 7.0)
        what = f"{n_cat} categories ({n_used} used), exponent {e}, {'weighted' if w is not None else 'unit weights'}"
        _check(got, _restated(a, b, pairs, 7.0, UNI, e, w, n_cat=n_cat), what)
        _check(got.sum(1), _oracle_scores(oracle, cats, a, b, pairs, 7.0, UNI, e, w), "row sums against the oracle, " + what)
        assert np.all(got[:, n_used:] == 0.0)
        if n_used > 1:  # (one category in use: both PMFs are (1, 0, ...) at every radius)
            assert np.any(got > 0.0)


# Pairs (wavefronts) per workgroup: the most of 4, 2, 1 whose dynamic LDS fits 150 KiB = 153 600 bytes.  A wavefront takes
# 7680 + C * (260 + 512 * columns) bytes rounded up to 16 (loco_hd_amd/csrc/lchd_pair_columns.h; columns: the f64 columns [C][64] of the
# mode), so 4 fit up to 38 400 bytes and 2 up to 76 800:
#   1 column  (exponent 2):       7680 + 772 C   <= 38 400  <=>  C <= 39   (39: 37 788, 40: 38 560);  C = 64 is 57 088 <= 76 800: never 1
#   2 columns (other exponents):  7680 + 1284 C  <= 38 400  <=>  C <= 23   (23: 37 212, 24: 38 496)
#                                                <= 76 800  <=>  C <= 53   (53: 75 732, 54: 77 016)
WAVE_SEAMS = [(2.0, False, 39), (2.0, False, 40), (2.0, True, 39), (2.0, True, 40), (3.5, False, 23), (3.5, False, 24), (3.5, False, 53), (3.5, False, 54)]


@pytest.mark.parametrize("e,weighted,n_cat", WAVE_SEAMS)
def test_both_sides_of_every_pairs_per_workgroup_switch(oracle, e, weighted, n_cat):
    """9 pairs (more than one workgroup at any width) of environments of about 40 points."""
    lh = _lh()
    cats = [f"k{k}" for k in range(n_cat)]
    a, b = Cloud(700 + n_cat, 120, 14.0, cats), Cloud(800 + n_cat, 120, 14.0, cats)
    rng = np.random.default_rng(n_cat)
    pairs = [(int(i), int(j)) for i, j in rng.integers(0, 120, (9, 2))]
    w = rng.uniform(0.3, 3.0, n_cat) if weighted else None
    l = lh.LoCoHD(cats, lh.WeightFunction(*UNI), category_weights=None if w is None else list(w), statistical_distance=lh.StatisticalDistance("Hellinger", [e]))
    got = l.attribution_from_primitives(a.atoms, b.atoms, pairs, 6.0)
    what = f"{n_cat} categories, exponent {e}, {'weighted' if weighted else 'unit weights'}"
    _check(got, _restated(a, b, pairs, 6.0, UNI, e, w, n_cat=n_cat), what)
    _check(got.sum(1), _oracle_scores(oracle, cats, a, b, pairs, 6.0, UNI, e, w), "row sums against the oracle, " + what)
    assert np.any(got > 0.0)


def test_second_trip_of_the_pair_loop_repeats_the_first():
    """8192 workgroups of 4 pairs cover 32 768 pairs; with 5 more the first wavefronts take a second pair.  The list is 7 pairs repeated:
    every repetition's rows are the bytes of the first occurrence's."""
    lh = _lh()
    a, b = Cloud(31, 20, 7.0, CATS7), Cloud(32, 20, 7.0, CATS7)
    short = [(int(i), int(j)) for i, j in np.random.default_rng(33).integers(0, 20, (7, 2))]
    n = 8192 * 4 + 5
    got = lh.LoCoHD(CATS7, lh.WeightFunction(*UNI)).attribution_from_primitives(a.atoms, b.atoms, (short * (n // 7 + 1))[:n], 6.0)
    assert got.shape == (n, 7) and np.isfinite(got).all() and np.any(got[:7] > 0.0)
    first = np.tile(got[:7], (n // 7 + 1, 1))[:n]
    assert np.array_equal(got.view(np.uint8), first.view(np.uint8))


def test_65_categories_are_refused():
    lh = _lh()
    cats = [f"k{k}" for k in range(65)]
    a = Cloud(7, 30, 8.0, cats)
    l = lh.LoCoHD(cats, lh.WeightFunction(*UNI))
    with pytest.raises(NotImplementedError, match="64 categories"):
        l.attribution_from_primitives(a.atoms, a.atoms, [(0, 1)], 6.0)
    with pytest.raises(NotImplementedError, match="64 categories"):
        l.attribution_from_coords(a.types, a.types, a.xyz, a.xyz)
    assert len(l.from_primitives(a.atoms, a.atoms, [(0, 1)], 6.0)) == 1  # the scoring call is untouched


# ---- the other distances ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dist", sorted(OTHER_DISTANCES))
def test_other_distances_are_refused_by_all_five_entry_points(two_clouds, dist):
    lh, (a, b) = _lh(), two_clouds
    from loco_hd_amd.device import DeviceSession

    name = OTHER_DISTANCES[dist][0]
    l = lh.LoCoHD(CATS7, lh.WeightFunction(*UNI), statistical_distance=lh.StatisticalDistance(*OTHER_DISTANCES[dist]))
    xa, xb, sa, sb = a.xyz[:40], b.xyz[:40], a.types[:40], b.types[:40]
    dmx = np.linalg.norm(xa[:, None, :] - xa[None, :, :], axis=-1)
    with pytest.raises(NotImplementedError, match=name):
        l.attribution_from_primitives(a.atoms, b.atoms, [(0, 1)], 8.0)
    with pytest.raises(NotImplementedError, match=name):
        l.attribution_from_coords(sa, sb, xa, xb)
    with pytest.raises(NotImplementedError, match=name):
        l.attribution_from_dmxs(sa, sa, dmx, dmx)
    sess = DeviceSession(l)
    try:
        torch = sess.torch
        ca, cb = [sess.upload(c.xyz[:40], c.cat_ids[:40].astype(np.int32), c.tag_ids[:40].astype(np.int32)) for c in (a, b)]
        anc = torch.tensor([[0, 1], [2, 3]], dtype=torch.int64, device="cuda")
        with pytest.raises(NotImplementedError, match=name):
            sess.attribution(ca, cb, anc, 8.0)
        with pytest.raises(NotImplementedError, match=name):
            sess.attribution_coords(ca, cb)
        assert sess.from_primitives(ca, cb, anc, 8.0).shape[0] == 2
    finally:
        sess.close()
    assert len(l.from_primitives(a.atoms, b.atoms, [(0, 1), (5, 7)], 8.0)) == 2  # the same object still scores
    assert len(l.from_coords(sa, sb, xa, xb)) == 40


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
    for e in (2.0, 3.5):
        got = lh.LoCoHD(CATS7, lh.WeightFunction(*UNI), statistical_distance=lh.StatisticalDistance("Hellinger", [e])).attribution_from_primitives(
            atoms, atoms, pairs, 7.0)
        _check(got, au.from_primitives(cat, xyz, None, cat, xyz, None, pairs, 7.0, 7, UNI, e), f"700-atom blob, exponent {e}")


# ---- dense and device-resident calls --------------------------------------------------------------------------------------------------
def test_from_coords_open_and_in_a_cell():
    lh = _lh()
    rng = np.random.default_rng(19)
    n = 90
    xa, xb = rng.uniform(0.0, 14.0, (n, 3)), rng.uniform(0.0, 14.0, (n, 3))
    ca, cb = rng.integers(0, 7, n), rng.integers(0, 7, n)
    sa, sb = [CATS7[k] for k in ca], [CATS7[k] for k in cb]
    l = lh.LoCoHD(CATS7, lh.WeightFunction(*UNI))
    _check(l.attribution_from_coords(sa, sb, xa, xb), au.from_rows(ca, au.open_rows(xa), cb, au.open_rows(xb), 7, UNI), "from_coords, open")
    cell = np.asarray([[14.0, 0.0, 0.0], [3.0, 13.0, 0.0], [-2.0, 4.0, 15.0]])
    rows_a = np.asarray(brute_rows(xa, range(n), cell))
    _check(l.attribution_from_coords(sa, sb, xa, xb, cell_a=cell), au.from_rows(ca, rows_a, cb, au.open_rows(xb), 7, UNI), "from_coords, cell_a")


def test_device_session_image_cloud_batch_coords_and_out(two_clouds):
    lh, (a, b) = _lh(), two_clouds
    from loco_hd_amd.device import DeviceSession

    rng = np.random.default_rng(23)
    sess = DeviceSession(lh.LoCoHD(CATS7, lh.WeightFunction(*UNI)))
    try:
        torch = sess.torch
        pk = [(c.xyz, c.cat_ids.astype(np.int32), c.tag_ids.astype(np.int32)) for c in (a, b)]
        batch, offs = sess.upload_batch(pk)
        pairs = rng.integers(0, 300, (50, 2))
        got = sess.attribution(batch, batch, torch.from_numpy(pairs + np.asarray([offs[0], offs[1]])).cuda(), 8.0)
        assert tuple(got.shape) == (50, 7)
        _check(got.cpu().numpy(), _restated(a, b, pairs, 8.0, UNI), "DeviceSession.attribution on a batch")
        # an image cloud of structure a in a box of its own edge against the open structure b; a caller-supplied `out`
        box = np.asarray([20.0, 20.0, 20.0])
        ca_, cb_ = sess.upload(*pk[0]), sess.upload(*pk[1])
        img = sess.periodic_images(ca_, box, 8.0)
        out = torch.full((50, 7), -1.0, dtype=torch.float64, device="cuda")
        assert sess.attribution(img, cb_, torch.from_numpy(pairs).cuda(), 8.0, out=out) is out
        shifts = np.stack(np.meshgrid(*[np.arange(-1.0, 2.0)] * 3, indexing="ij"), -1).reshape(-1, 3) * box
        order = np.argsort(np.abs(shifts).sum(1) > 0, kind="stable")  # the originals first: anchor index i is atom i
        xyz_img = (a.xyz[None, :, :] + shifts[order][:, None, :]).reshape(-1, 3)
        want = au.from_primitives(np.tile(a.cat_ids, 27), xyz_img, np.tile(a.tag_ids, 27), b.cat_ids, b.xyz, b.tag_ids, pairs, 8.0, 7, UNI)
        _check(out.cpu().numpy(), want, "DeviceSession.attribution on an image cloud, into `out`")
        # dense rows of two device clouds, into `out`
        small = [(c.xyz[:70], c.cat_ids[:70].astype(np.int32), None) for c in (a, b)]
        da, db = sess.upload(*small[0]), sess.upload(*small[1])
        out2 = torch.full((70, 7), -1.0, dtype=torch.float64, device="cuda")
        assert sess.attribution_coords(da, db, out=out2) is out2
        want = au.from_rows(small[0][1], au.open_rows(small[0][0]), small[1][1], au.open_rows(small[1][0]), 7, UNI)
        _check(out2.cpu().numpy(), want, "attribution_coords on device clouds, into `out`")
        _check(sess.attribution_coords(da, db).cpu().numpy(), want, "attribution_coords on device clouds")
    finally:
        sess.close()


# ---- determinism and non-interference -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("e", [2.0, 3.5])
def test_deterministic_rows_are_a_function_of_the_pair(two_clouds, pairs40, e):
    lh, (a, b) = _lh(), two_clouds
    l = lh.LoCoHD(CATS7, lh.WeightFunction(*UNI), statistical_distance=lh.StatisticalDistance("Hellinger", [e]), deterministic=True)
    base = l.attribution_from_primitives(a.atoms, b.atoms, pairs40, 8.0)
    alone = np.vstack([l.attribution_from_primitives(a.atoms, b.atoms, [p], 8.0) for p in pairs40[:6]])
    assert np.array_equal(alone, base[:6])
    assert np.array_equal(l.attribution_from_primitives(a.atoms, b.atoms, pairs40[::-1], 8.0), base[::-1])


def test_scores_and_the_sweep_record_are_left_alone(two_clouds):
    lh, (a, b) = _lh(), two_clouds
    from loco_hd_amd.device import DeviceSession

    rng = np.random.default_rng(29)
    sess = DeviceSession(lh.LoCoHD(CATS7, lh.WeightFunction(*UNI), deterministic=True))
    try:
        torch = sess.torch
        ca, cb = [sess.upload(c.xyz, c.cat_ids.astype(np.int32), c.tag_ids.astype(np.int32)) for c in (a, b)]
        anc = torch.from_numpy(rng.integers(0, 300, (6000, 2))).cuda()
        for _ in range(2):  # (the second call runs with the hints of the first)
            before = sess.from_primitives(ca, cb, anc, 8.0).clone()
        rec = sess.last_sweep()
        assert rec is not None
        sess.attribution(ca, cb, anc[:500], 8.0)
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
    from loco_hd_amd.device import DeviceSession

    l = lh.LoCoHD(CATS7, lh.WeightFunction(*UNI))
    with pytest.raises(N.PanicException):
        l.attribution_from_primitives(a.atoms, b.atoms, [(0, 300)], 8.0)
    odd = a.atoms[:10] + [lh.PrimitiveAtom("not-in-the-map", "t0", list(a.xyz[0] + 0.5))]
    with pytest.raises(ValueError):
        l.attribution_from_primitives(odd, b.atoms, [(0, 0)], 8.0)
    d = lh.LoCoHD(CATS7, {"u": lh.WeightFunction(*UNI), "h": lh.WeightFunction("hyper_exp", FAMILIES["hyper_exp"])})
    with pytest.raises(ValueError):
        d.attribution_from_primitives(a.atoms, b.atoms, [(0, 1, "no-such-key")], 8.0)
    sess = DeviceSession(d)
    try:
        torch = sess.torch
        ca, cb = [sess.upload(c.xyz, c.cat_ids.astype(np.int32), c.tag_ids.astype(np.int32)) for c in (a, b)]
        anc = torch.tensor([[0, 1], [2, 3], [4, 5]], dtype=torch.int64, device="cuda")
        wf = torch.tensor([0, 2, 1], dtype=torch.int32, device="cuda")  # index 2 is outside a dictionary of two
        out = torch.zeros((3, 7), dtype=torch.float64, device="cuda")
        with pytest.raises(ValueError):
            sess.attribution(ca, cb, anc, 8.0, out=out, wf_index=wf)
        got = out.cpu().numpy()
        assert np.isnan(got[1]).all() and np.isfinite(got[[0, 2]]).all()  # the row is NaN, as a radial row is
    finally:
        sess.close()
