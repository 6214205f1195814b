"""Category-weight gradients on the device against the numpy restatement (tests/category_gradient_util.py, longdouble, from the
definition; tests/test_category_gradient_model.py pins it to finite differences of the CPU oracle) and, once, against those finite
differences directly.

Expected values never come from the library.  Bound: the project's parity bound, 1e-11 absolute, on the log-weight form w_c * G[p][c],
whose terms are bounded like a score's (|d_c| / H <= sqrt 2, ln(1 / eps) about 7)."""
import numpy as np
import pytest

import category_gradient_util as cg
from attribution_util import open_rows
from min_image_util import brute_rows

pytestmark = pytest.mark.gpu

TOL = 1e-11
INF = float("inf")
TILE = 384  # kSweepTile (loco_hd_amd/csrc/lchd_device.h): merged events per tile of the kernel
CATS7 = [f"c{k}" for k in range(7)]
UNI = ("uniform", [3.0, 10.0])
FAMILIES = {"uniform": [3.0, 10.0], "hyper_exp": [1.0, 0.5, 0.2, 0.05], "dagum": [4.0, 6.0, 1.5], "kumaraswamy": [2.0, 11.0, 2.0, 3.0]}
H2, KL = ("Hellinger", 2.0), ("Kullback-Leibler", 1e-3)
DISTANCES = {"h2": H2, "h1": ("Hellinger", 1.0), "h3.5": ("Hellinger", 3.5), "kl": KL}
WEIGHTS = np.random.default_rng(3).uniform(0.3, 3.0, 7)


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


def _locohd(distance=H2, wf=UNI, weights=None, cats=CATS7, **kw):
    lh = _lh()
    w = {k: lh.WeightFunction(*v) for k, v in wf.items()} if isinstance(wf, dict) else lh.WeightFunction(*wf)
    return lh.LoCoHD(cats, w, category_weights=None if weights is None else list(weights),
                     statistical_distance=lh.StatisticalDistance(distance[0], [distance[1]]), **kw)


def _check(got, want_log, weights, what, tol=TOL):
    """got: G from the library; want_log: w * G from the restatement (longdouble)."""
    got = np.asarray(got)
    assert got.shape == np.asarray(want_log).shape, what
    assert np.isfinite(got).all(), what
    w = np.ones(got.shape[1]) if weights is None else np.asarray(weights)
    err = float(np.max(np.abs(got.astype(np.longdouble) * w[None, :] - want_log))) if got.size else 0.0
    print(f"{what}: max |w (device - expected)| = {err:.3g}")
    assert err <= tol, what


def _restated(a, b, pairs, thr, wf, distance=H2, weights=None, accept_same=True, n_cat=7):
    return cg.from_primitives(a.cat_ids, a.xyz, a.tag_ids, b.cat_ids, b.xyz, b.tag_ids, pairs, thr, n_cat, wf, distance, weights, accept_same)


# ---- thresholded parity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("dist", sorted(DISTANCES))
def test_distances_with_unit_and_drawn_weights(two_clouds, pairs40, dist, weighted):
    (a, b), distance = two_clouds, DISTANCES[dist]
    weights = WEIGHTS if weighted else None
    got = _locohd(distance, weights=weights).category_gradient_from_primitives(a.atoms, b.atoms, pairs40, 8.0)
    _check(got, _restated(a, b, pairs40, 8.0, UNI, distance, weights), weights, f"{dist}, weighted={weighted}")
    euler = float(np.max(np.abs((got * (1.0 if weights is None else weights)).sum(1))))
    print(f"max |sum_c w_c G_c| = {euler:.3g}")
    assert euler <= TOL and np.any(np.abs(got) > 1e-4)


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_weight_function_families(two_clouds, pairs40, family):
    a, b = two_clouds
    wf = (family, FAMILIES[family])
    got = _locohd(wf=wf, weights=WEIGHTS).category_gradient_from_primitives(a.atoms, b.atoms, pairs40, 8.0)
    _check(got, _restated(a, b, pairs40, 8.0, wf, H2, WEIGHTS), WEIGHTS, family)


def test_weight_function_dictionary_with_per_pair_keys(two_clouds, pairs40):
    a, b = two_clouds
    specs = {"u": UNI, "h": ("hyper_exp", FAMILIES["hyper_exp"]), "d": ("dagum", FAMILIES["dagum"])}
    keys = [("u", "h", "d")[p % 3] for p in range(len(pairs40))]
    keyed = [(i, j, k) for (i, j), k in zip(pairs40, keys)]
    got = _locohd(KL, wf=specs, weights=WEIGHTS).category_gradient_from_primitives(a.atoms, b.atoms, keyed, 8.0)
    _check(got, _restated(a, b, pairs40, 8.0, [specs[k] for k in keys], KL, WEIGHTS), WEIGHTS, "dictionary, per-pair keys")


@pytest.mark.parametrize("accept_same", [True, False])
def test_tag_rules(two_clouds, pairs40, accept_same):
    lh, (a, b) = _lh(), two_clouds
    l = _locohd(weights=WEIGHTS, tag_pairing_rule=lh.TagPairingRule({"accept_same": accept_same}))
    got = l.category_gradient_from_primitives(a.atoms, b.atoms, pairs40, 8.0)
    _check(got, _restated(a, b, pairs40, 8.0, UNI, H2, WEIGHTS, accept_same), WEIGHTS, f"accept_same={accept_same}")


def test_meaning_against_finite_differences_of_the_oracle(oracle, two_clouds, pairs40):
    """No model in between: G against Richardson-extrapolated central differences of the oracle's scores (bound: cg.FD_BOUND)."""
    (a, b), pairs = two_clouds, pairs40[:10]
    pa, pb = _atoms(oracle, a.types, a.tags, a.xyz), _atoms(oracle, b.types, b.tags, b.xyz)

    def score_of(w):
        return oracle.LoCoHD(CATS7, oracle.WeightFunction(*UNI), category_weights=list(w)).from_primitives(pa, pb, pairs, 8.0)

    want = np.stack([cg.richardson(score_of, WEIGHTS, c)[0] for c in range(7)], 1)
    got = _locohd(weights=WEIGHTS).category_gradient_from_primitives(a.atoms, b.atoms, pairs, 8.0)
    err = float(np.max(np.abs(got - want)))
    print(f"max |device - oracle finite difference| = {err:.3g}")
    assert err <= cg.FD_BOUND


# ---- merged event counts (dense rows) -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("merged", [20, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
@pytest.mark.parametrize("dist", ["h2", "h3.5", "kl"])
def test_tile_seams_ties_and_points_beyond_the_support(merged, dist):
    """Rows of merged // 2 and merged - merged // 2 non-anchor events: fewer than 64 (lanes without events) and the tile seams.  Two
    decimals: ties within and across the sides; distances up to 12 under uniform [3, 10] and +inf entries: points beyond the support."""
    distance = DISTANCES[dist]
    rng = np.random.default_rng(merged)
    rows = 4

    def side(n):
        m = np.round(rng.uniform(0.0, 12.0, (rows, n)), 2)
        m[rng.uniform(size=m.shape) < 0.1] = INF
        m[np.arange(rows), np.arange(rows) % n] = 0.0
        return m, rng.integers(0, 7, n)

    (ma, ca), (mb, cb) = side(merged // 2 + 1), side(merged - merged // 2 + 1)
    got = _locohd(distance, weights=WEIGHTS).category_gradient_from_dmxs([CATS7[k] for k in ca], [CATS7[k] for k in cb], ma, mb)
    _check(got, cg.from_rows(ca, ma, cb, mb, 7, UNI, distance, WEIGHTS), WEIGHTS, f"{merged} merged events, {dist}")


def test_exact_ties_at_one_distance():
    """Every non-anchor point of both sides at distance 5: one piece up to it, one behind it."""
    rng = np.random.default_rng(2)
    ma, mb = np.full((3, 30), 5.0), np.full((3, 26), 5.0)
    ma[np.arange(3), np.arange(3)] = 0.0
    mb[np.arange(3), np.arange(3)] = 0.0
    ca, cb = rng.integers(0, 7, 30), rng.integers(0, 7, 26)
    for distance in (H2, KL):
        got = _locohd(distance, weights=WEIGHTS).category_gradient_from_dmxs([CATS7[k] for k in ca], [CATS7[k] for k in cb], ma, mb)
        _check(got, cg.from_rows(ca, ma, cb, mb, 7, UNI, distance, WEIGHTS), WEIGHTS, f"all tied, {distance[0]}")
        assert np.any(got != 0.0)


# ---- categories -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cat,n_used", [(1, 1), (7, 4), (64, 64), (64, 32)])
def test_category_counts_and_unused_categories(n_cat, n_used):
    """One category: exact zeros.  n_used < n_cat: the upper categories occur in neither cloud, and their columns are exactly 0.  64: the
    largest accumulator blocks (one pair per workgroup where the term columns are staged)."""
    cats = [f"k{k}" for k in range(n_cat)]
    a, b = Cloud(500 + n_cat, 200, 14.0, cats, n_used=n_used), Cloud(600 + n_cat, 200, 14.0, cats, n_used=n_used)
    rng = np.random.default_rng(n_cat)
    pairs = [(int(i), int(j)) for i, j in rng.integers(0, 200, (12, 2))]
    weights = rng.uniform(0.3, 3.0, n_cat)
    for name, distance in sorted(DISTANCES.items()):
        if name == "h1":
            continue
        got = _locohd(distance, weights=weights, cats=cats).category_gradient_from_primitives(a.atoms, b.atoms, pairs, 7.0)
        _check(got, _restated(a, b, pairs, 7.0, UNI, distance, weights, n_cat=n_cat), weights, f"{n_cat} categories ({n_used} used), {name}")
        assert np.all(got[:, n_used:] == 0.0)
        assert np.all(got == 0.0) if n_cat == 1 else np.any(got != 0.0)


# Pairs (wavefronts) per workgroup: the most of 4, 2, 1 whose dynamic LDS fits 150 KiB = 153 600 bytes.  A wavefront takes
# 7680 + C * (260 + 512 * columns) bytes rounded up to 16 (loco_hd_amd/csrc/lchd_pair_columns.h; columns: the f64 columns [C][64] of the
# mode), so 4 fit up to 38 400 bytes and 2 up to 76 800:
#   1 column  (Hellinger 2):                   7680 + 772 C   <= 38 400  <=>  C <= 39   (39: 37 788, 40: 38 560);  C = 64 is 57 088: never 1
#   3 columns (other exponents, Kullback-L.):  7680 + 1796 C  <= 38 400  <=>  C <= 17   (17: 38 212, 18: 40 008)
#                                                             <= 76 800  <=>  C <= 38   (38: 75 928, 39: 77 724)
WAVE_SEAMS = [("h2", 39), ("h2", 40)] + [(d, c) for d in ("h3.5", "kl") for c in (17, 18, 38, 39)]


@pytest.mark.parametrize("dist,n_cat", WAVE_SEAMS)
def test_both_sides_of_every_pairs_per_workgroup_switch(dist, n_cat):
    """9 pairs (more than one workgroup at any width) of environments of about 40 points."""
    cats = [f"k{k}" for k in range(n_cat)]
    a, b = Cloud(700 + n_cat, 120, 14.0, cats), Cloud(800 + n_cat, 120, 14.0, cats)
    rng = np.random.default_rng(n_cat)
    pairs = [(int(i), int(j)) for i, j in rng.integers(0, 120, (9, 2))]
    weights = rng.uniform(0.3, 3.0, n_cat)
    got = _locohd(DISTANCES[dist], weights=weights, cats=cats).category_gradient_from_primitives(a.atoms, b.atoms, pairs, 6.0)
    _check(got, _restated(a, b, pairs, 6.0, UNI, DISTANCES[dist], weights, n_cat=n_cat), weights, f"{n_cat} categories, {dist}")
    assert np.any(got != 0.0)


def test_second_trip_of_the_pair_loop_repeats_the_first():
    """8192 workgroups of 4 pairs cover 32 768 pairs; with 5 more the first wavefronts take a second pair.  The list is 7 pairs repeated:
    every repetition's rows are the bytes of the first occurrence's."""
    a, b = Cloud(31, 20, 7.0, CATS7), Cloud(32, 20, 7.0, CATS7)
    short = [(int(i), int(j)) for i, j in np.random.default_rng(33).integers(0, 20, (7, 2))]
    n = 8192 * 4 + 5
    got = _locohd(H2, weights=WEIGHTS).category_gradient_from_primitives(a.atoms, b.atoms, (short * (n // 7 + 1))[:n], 6.0)
    assert got.shape == (n, 7) and np.isfinite(got).all() and np.any(got[:7] != 0.0)
    first = np.tile(got[:7], (n // 7 + 1, 1))[:n]
    assert np.array_equal(got.view(np.uint8), first.view(np.uint8))


def test_a_category_on_one_side_only(two_clouds, pairs40):
    a, b = two_clouds
    only_a = Cloud(103, 300, 20.0, CATS7, n_used=6)  # category 6 occurs in cloud b alone
    for distance in (H2, ("Hellinger", 3.5), KL):
        got = _locohd(distance, weights=WEIGHTS).category_gradient_from_primitives(only_a.atoms, b.atoms, pairs40, 8.0)
        _check(got, _restated(only_a, b, pairs40, 8.0, UNI, distance, WEIGHTS), WEIGHTS, f"category 6 on side B only, {distance}")
        assert np.any(got[:, 6] != 0.0)


@pytest.mark.parametrize("dist", ["h2", "h1", "h3.5"])
def test_identical_environments_give_exact_zero_rows(two_clouds, pairs40, dist):
    a, _ = two_clouds
    got = _locohd(DISTANCES[dist], weights=WEIGHTS).category_gradient_from_primitives(a.atoms, a.atoms, [(i, i) for i, _ in pairs40], 8.0)
    assert got.shape == (40, 7) and np.all(got == 0.0)


# ---- dense calls ----------------------------------------------------------------------------------------------------------------------
def test_from_coords_open_in_a_box_and_in_a_triclinic_cell():
    rng = np.random.default_rng(19)
    n = 40
    xa, xb = rng.uniform(0.0, 14.0, (n, 3)), rng.uniform(0.0, 14.0, (n, 3))
    ca, cb = rng.integers(0, 7, n), rng.integers(0, 7, n)
    sa, sb = [CATS7[k] for k in ca], [CATS7[k] for k in cb]
    box = np.asarray([14.0, 15.0, 16.0])
    cell = np.asarray([[14.0, 0.0, 0.0], [3.0, 13.0, 0.0], [-2.0, 4.0, 15.0]])
    for distance in (H2, KL):
        l = _locohd(distance, weights=WEIGHTS)
        want = cg.from_rows(ca, open_rows(xa), cb, open_rows(xb), 7, UNI, distance, WEIGHTS)
        _check(l.category_gradient_from_coords(sa, sb, xa, xb), want, WEIGHTS, f"from_coords, open, {distance[0]}")
        rows_box = np.asarray(brute_rows(xa, range(n), np.diag(box)))
        want = cg.from_rows(ca, rows_box, cb, open_rows(xb), 7, UNI, distance, WEIGHTS)
        _check(l.category_gradient_from_coords(sa, sb, xa, xb, box_a=box), want, WEIGHTS, f"from_coords, box_a, {distance[0]}")
        rows_cell = np.asarray(brute_rows(xb, range(n), cell))
        want = cg.from_rows(ca, open_rows(xa), cb, rows_cell, 7, UNI, distance, WEIGHTS)
        _check(l.category_gradient_from_coords(sa, sb, xa, xb, cell_b=cell), want, WEIGHTS, f"from_coords, cell_b, {distance[0]}")


def test_from_dmxs_with_infinite_entries():
    rng = np.random.default_rng(31)
    ma, mb = rng.uniform(0.5, 11.0, (9, 50)), rng.uniform(0.5, 11.0, (9, 43))
    ma[rng.uniform(size=ma.shape) < 0.3] = INF
    mb[rng.uniform(size=mb.shape) < 0.3] = INF
    ma[np.arange(9), np.arange(9)] = 0.0
    mb[np.arange(9), np.arange(9)] = 0.0
    ca, cb = rng.integers(0, 7, 50), rng.integers(0, 7, 43)
    for distance in (H2, ("Hellinger", 3.5), KL):
        got = _locohd(distance, weights=WEIGHTS).category_gradient_from_dmxs([CATS7[k] for k in ca], [CATS7[k] for k in cb], ma, mb)
        _check(got, cg.from_rows(ca, ma, cb, mb, 7, UNI, distance, WEIGHTS), WEIGHTS, f"from_dmxs with +inf, {distance}")


# ---- device-resident calls ------------------------------------------------------------------------------------------------------------
def test_device_session_batch_image_cloud_coords_and_set_category_weights(two_clouds):
    lh, (a, b) = _lh(), two_clouds
    from loco_hd_amd.device import DeviceSession

    rng = np.random.default_rng(23)
    l = _locohd(weights=WEIGHTS, deterministic=True)
    sess = DeviceSession(l)
    try:
        torch = sess.torch
        pk = [(c.xyz, c.cat_ids.astype(np.int32), c.tag_ids.astype(np.int32)) for c in (a, b)]
        batch, offs = sess.upload_batch(pk)
        pairs = rng.integers(0, 300, (50, 2))
        got = sess.category_gradient(batch, batch, torch.from_numpy(pairs + np.asarray([offs[0], offs[1]])).cuda(), 8.0)
        assert tuple(got.shape) == (50, 7)
        want = _restated(a, b, pairs, 8.0, UNI, H2, WEIGHTS)
        _check(got.cpu().numpy(), want, WEIGHTS, "DeviceSession.category_gradient on a batch")
        host = l.category_gradient_from_primitives(a.atoms, b.atoms, [(int(i), int(j)) for i, j in pairs], 8.0)
        assert np.array_equal(got.cpu().numpy(), host)  # the same stored pairs: the same bits
        # an image cloud of structure a in a box of its own edge against the open structure b; a caller-supplied `out`
        box = np.asarray([20.0, 20.0, 20.0])
        ca_, cb_ = sess.upload(*pk[0]), sess.upload(*pk[1])
        img = sess.periodic_images(ca_, box, 8.0)
        out = torch.full((50, 7), -1.0, dtype=torch.float64, device="cuda")
        assert sess.category_gradient(img, cb_, torch.from_numpy(pairs).cuda(), 8.0, out=out) is out
        host = l.category_gradient_from_primitives(a.atoms, b.atoms, [(int(i), int(j)) for i, j in pairs], 8.0, box_a=box)
        shifts = np.stack(np.meshgrid(*[np.arange(-1.0, 2.0)] * 3, indexing="ij"), -1).reshape(-1, 3) * box
        order = np.argsort(np.abs(shifts).sum(1) > 0, kind="stable")  # the originals first: anchor index i is atom i
        xyz_img = (a.xyz[None, :, :] + shifts[order][:, None, :]).reshape(-1, 3)
        want = cg.from_primitives(np.tile(a.cat_ids, 27), xyz_img, np.tile(a.tag_ids, 27), b.cat_ids, b.xyz, b.tag_ids, pairs, 8.0, 7, UNI, H2,
                                  WEIGHTS)
        _check(out.cpu().numpy(), want, WEIGHTS, "DeviceSession.category_gradient on an image cloud, into `out`")
        _check(host, want, WEIGHTS, "category_gradient_from_primitives with box_a")
        assert float(np.max(np.abs(out.cpu().numpy() - host))) <= 1e-13
        # dense rows of two device clouds
        small = [(c.xyz[:40], c.cat_ids[:40].astype(np.int32), None) for c in (a, b)]
        da, db = sess.upload(*small[0]), sess.upload(*small[1])
        want = cg.from_rows(small[0][1], open_rows(small[0][0]), small[1][1], open_rows(small[1][0]), 7, UNI, H2, WEIGHTS)
        _check(sess.category_gradient_coords(da, db).cpu().numpy(), want, WEIGHTS, "category_gradient_coords on device clouds")
        # other weights: validated as the constructor validates them, then in force for gradients and scores; the clouds stay
        for bad in ([1.0] * 6, [1.0] * 6 + [0.0], [1.0] * 6 + [-2.0]):
            with pytest.raises(ValueError):
                sess.set_category_weights(bad)
        w2 = np.random.default_rng(4).uniform(0.3, 3.0, 7)
        sess.set_category_weights(w2)
        got2 = sess.category_gradient(ca_, cb_, torch.from_numpy(pairs).cuda(), 8.0)
        _check(got2.cpu().numpy(), _restated(a, b, pairs, 8.0, UNI, H2, w2), w2, "after set_category_weights")
        assert l.category_weights == list(WEIGHTS)
    finally:
        sess.close()


# ---- determinism and non-interference -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dist", ["h2", "h3.5", "kl"])
def test_two_calls_give_identical_bits(two_clouds, pairs40, dist):
    a, b = two_clouds
    l = _locohd(DISTANCES[dist], weights=WEIGHTS, deterministic=True)
    base = l.category_gradient_from_primitives(a.atoms, b.atoms, pairs40, 8.0)
    assert np.array_equal(l.category_gradient_from_primitives(a.atoms, b.atoms, pairs40, 8.0), base)
    assert np.array_equal(l.category_gradient_from_primitives(a.atoms, b.atoms, pairs40[::-1], 8.0), base[::-1])
    assert np.array_equal(np.vstack([l.category_gradient_from_primitives(a.atoms, b.atoms, [p], 8.0) for p in pairs40[:4]]), base[:4])


def test_scores_and_the_sweep_record_are_left_alone(two_clouds):
    (a, b) = two_clouds
    from loco_hd_amd.device import DeviceSession

    rng = np.random.default_rng(29)
    sess = DeviceSession(_locohd(weights=WEIGHTS, deterministic=True))
    try:
        torch = sess.torch
        ca, cb = [sess.upload(c.xyz, c.cat_ids.astype(np.int32), c.tag_ids.astype(np.int32)) for c in (a, b)]
        anc = torch.from_numpy(rng.integers(0, 300, (6000, 2))).cuda()
        for _ in range(2):  # (the second call runs with the hints of the first)
            before = sess.from_primitives(ca, cb, anc, 8.0).clone()
        rec = sess.last_sweep()
        assert rec is not None
        sess.category_gradient(ca, cb, anc[:500], 8.0)
        assert sess.last_sweep() == rec
        after = sess.from_primitives(ca, cb, anc, 8.0)
        assert torch.equal(before, after)
        assert sess.last_sweep() == rec
    finally:
        sess.close()


# ---- errors ---------------------------------------------------------------------------------------------------------------------------
def test_errors_are_the_attribution_calls(two_clouds):
    lh, (a, b) = _lh(), two_clouds
    from loco_hd_amd import _native as N
    from loco_hd_amd.device import DeviceSession

    l = _locohd()
    with pytest.raises(N.PanicException):
        l.category_gradient_from_primitives(a.atoms, b.atoms, [(0, 300)], 8.0)
    odd = a.atoms[:10] + [lh.PrimitiveAtom("not-in-the-map", "t0", list(a.xyz[0] + 0.5))]
    with pytest.raises(ValueError):
        l.category_gradient_from_primitives(odd, b.atoms, [(0, 0)], 8.0)
    d = _locohd(wf={"u": UNI, "h": ("hyper_exp", FAMILIES["hyper_exp"])})
    with pytest.raises(ValueError):
        d.category_gradient_from_primitives(a.atoms, b.atoms, [(0, 1, "no-such-key")], 8.0)
    sess = DeviceSession(d)
    try:
        torch = sess.torch
        ca, cb = [sess.upload(c.xyz, c.cat_ids.astype(np.int32), c.tag_ids.astype(np.int32)) for c in (a, b)]
        anc = torch.tensor([[0, 1], [2, 3], [4, 5]], dtype=torch.int64, device="cuda")
        wf = torch.tensor([0, 2, 1], dtype=torch.int32, device="cuda")  # index 2 is outside a dictionary of two
        out = torch.zeros((3, 7), dtype=torch.float64, device="cuda")
        with pytest.raises(ValueError):
            sess.category_gradient(ca, cb, anc, 8.0, out=out, wf_index=wf)
        got = out.cpu().numpy()
        assert np.isnan(got[1]).all() and np.isfinite(got[[0, 2]]).all()  # the row is NaN, as an attribution row is
        # an anchor outside its structure: the attribution call's error, and its NaN row
        far = torch.tensor([[0, 1], [2, 300], [4, 5]], dtype=torch.int64, device="cuda")
        rows = {}
        for name in ("attribution", "category_gradient"):
            rows[name] = torch.zeros((3, 7), dtype=torch.float64, device="cuda")
            with pytest.raises(N.PanicException):
                getattr(sess, name)(ca, cb, far, 8.0, out=rows[name])
        assert np.array_equal(np.isnan(rows["attribution"].cpu().numpy()), np.isnan(rows["category_gradient"].cpu().numpy()))
    finally:
        sess.close()
