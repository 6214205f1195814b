"""Neighbour sensitivities on the device against the numpy restatement (tests/sensitivity_util.py, longdouble, from the definition;
tests/test_sensitivity_model.py pins it to the score model by difference quotients).

Expected values never come from the library.  idx, dist and count must match the model exactly; scores must match from_primitives of the
same call within 1e-11 (the bound tests/test_gpu_attribution.py puts on row sums); g is bounded by TOL_G, 16 x the largest deviation
from the model measured over this file's cases on an MI355X."""
import numpy as np
import pytest

import sensitivity_util as su

pytestmark = pytest.mark.gpu

TOL = 1e-11
TOL_G = 16 * 3.61e-16  # measured: 3.61e-16 (64 categories, category weights, Kullback-Leibler), DESIGN.md section 5
TILE = 384  # kSweepTile (loco_hd_amd/csrc/lchd_device.h)
MAX_POINTS = 65535  # kRadialMaxPoints
UNI = ("uniform", [3.0, 10.0])
FAMILIES = {"hyper_exp": [1.0, 0.5, 0.2, 0.05], "dagum": [4.0, 6.0, 1.5], "kumaraswamy": [2.0, 11.0, 2.0, 3.0]}
DISTANCES = {"h2": ("Hellinger", [2.0]), "h3.5": ("Hellinger", [3.5]), "ks": ("Kolmogorov-Smirnov", []), "kl": ("Kullback-Leibler", [1e-3]),
             "renyi": ("Renyi", [2.5, 1e-3])}
WORST = {"g": 0.0}


def _lh():
    import loco_hd_amd as lh

    return lh


class Cloud:
    def __init__(self, xyz, cat_ids, tag_ids, cats):
        lh = _lh()
        self.xyz, self.cat_ids, self.tag_ids = np.asarray(xyz, dtype=np.float64), np.asarray(cat_ids), np.asarray(tag_ids)
        self.atoms = [lh.PrimitiveAtom(cats[c], f"t{t}", list(x)) for c, t, x in zip(self.cat_ids, self.tag_ids, self.xyz)]


def _random_cloud(seed, n, edge, cats, n_tags=3):
    rng = np.random.default_rng(seed)
    return Cloud(rng.uniform(0.0, edge, (n, 3)), rng.integers(0, len(cats), n), rng.integers(0, n_tags, n), cats)


def _ball_cloud(seed, n_near, cats, radius=6.0, n_far=5):
    """Atom 0 at the origin with exactly n_near neighbours inside `radius`; n_far atoms far away (each alone in its environment)."""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n_near, 3))
    v *= (radius * rng.uniform(0.05, 0.999, n_near) ** (1 / 3) / np.linalg.norm(v, axis=1))[:, None]
    far = 100.0 + 50.0 * np.arange(1, n_far + 1)[:, None] * np.ones((1, 3))
    xyz = np.vstack([np.zeros((1, 3)), v, far])
    return Cloud(xyz, rng.integers(0, len(cats), len(xyz)), np.zeros(len(xyz), dtype=int), cats)


def _compare(got, want, scores_ref, what):
    for name in ("count_a", "count_b", "idx_a", "idx_b", "dist_a", "dist_b"):
        assert np.array_equal(getattr(got, name), getattr(want, name)), f"{what}: {name}"
    err_s = float(np.max(np.abs(got.scores - np.asarray(scores_ref)))) if len(got.scores) else 0.0
    err_m = float(np.max(np.abs(got.scores - want.scores))) if len(got.scores) else 0.0
    err_g = max(float(np.max(np.abs(got.g_a - want.g_a), initial=0.0)), float(np.max(np.abs(got.g_b - want.g_b), initial=0.0)))
    WORST["g"] = max(WORST["g"], err_g)
    print(f"{what}: max |g - model| = {err_g:.3g}, |scores - from_primitives| = {err_s:.3g}, |scores - model| = {err_m:.3g}  (worst g so far {WORST['g']:.3g})")
    assert np.isfinite(got.g_a).all() and np.isfinite(got.g_b).all()
    assert err_s <= TOL and err_m <= TOL, what
    assert err_g <= TOL_G, what


def _run(cats, a, b, pairs, thr, wf=UNI, sd=DISTANCES["h2"], weights=None, accept_same=True, what=""):
    lh = _lh()
    l = lh.LoCoHD(cats, lh.WeightFunction(*wf), lh.TagPairingRule({"accept_same": accept_same}),
                  category_weights=None if weights is None else list(weights), statistical_distance=lh.StatisticalDistance(*sd))
    got = l.sensitivity_from_primitives(a.atoms, b.atoms, pairs, thr)
    want = su.from_primitives(a.cat_ids, a.xyz, a.tag_ids, b.cat_ids, b.xyz, b.tag_ids, pairs, thr, len(cats), wf, sd, weights, accept_same)
    _compare(got, want, l.from_primitives(a.atoms, b.atoms, pairs, thr), what)
    return got


CATS7 = [f"c{k}" for k in range(7)]


@pytest.fixture(scope="module")
def two_clouds():
    return _random_cloud(201, 300, 20.0, CATS7), _random_cloud(202, 300, 20.0, CATS7)


@pytest.fixture(scope="module")
def pairs30():
    rng = np.random.default_rng(11)
    return [(int(i), int(j)) for i, j in rng.integers(0, 300, (30, 2))]


@pytest.mark.parametrize("dist", sorted(DISTANCES))
def test_every_statistical_distance(two_clouds, pairs30, dist):
    a, b = two_clouds
    _run(CATS7, a, b, pairs30, 8.0, sd=DISTANCES[dist], what=f"uniform, {dist}")


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_other_weight_functions(two_clouds, pairs30, family):
    a, b = two_clouds
    _run(CATS7, a, b, pairs30, 8.0, wf=(family, FAMILIES[family]), what=family)


@pytest.mark.parametrize("accept_same", [True, False])
def test_tag_rules_and_category_weights(two_clouds, pairs30, accept_same):
    a, b = two_clouds
    weights = np.random.default_rng(3).uniform(0.3, 3.0, 7)
    _run(CATS7, a, b, pairs30, 8.0, weights=weights, accept_same=accept_same, sd=DISTANCES["h3.5"], what=f"weights, accept_same={accept_same}")


def test_two_weight_functions_by_key(two_clouds, pairs30):
    lh, (a, b) = _lh(), two_clouds
    specs = {"u": UNI, "h": ("hyper_exp", FAMILIES["hyper_exp"])}
    keys = [("u", "h")[p % 2] for p in range(len(pairs30))]
    keyed = [(i, j, k) for (i, j), k in zip(pairs30, keys)]
    l = lh.LoCoHD(CATS7, {k: lh.WeightFunction(*v) for k, v in specs.items()})
    got = l.sensitivity_from_primitives(a.atoms, b.atoms, keyed, 8.0)
    want = su.from_primitives(a.cat_ids, a.xyz, a.tag_ids, b.cat_ids, b.xyz, b.tag_ids, pairs30, 8.0, 7, [specs[k] for k in keys])
    _compare(got, want, l.from_primitives(a.atoms, b.atoms, keyed, 8.0), "dictionary, per-pair keys")


def test_repeated_anchors_one_object_and_width(two_clouds):
    a, _ = two_clouds
    pairs = [(5, 9), (5, 9), (9, 5), (5, 5), (17, 9), (5, 17)]
    got = _run(CATS7, a, a, pairs, 8.0, what="repeated anchors, both sides one list")
    assert np.array_equal(got.g_a[0], got.g_a[1]) and np.array_equal(got.idx_b[0], got.idx_b[1])
    assert got.idx_a.shape[1] == max(got.count_a.max(), got.count_b.max())  # rows as wide as the longest environment
    assert np.all(got.g_a[3] + got.g_b[3] == 0.0) and got.scores[3] == 0.0  # (5, 5): every member ties with itself on the other side


# merged non-anchor events of the pair (0, 0): n_a + n_b
@pytest.mark.parametrize("n_a,n_b", [(0, 0), (1, 0), (0, 1), (40, 23), (32, 32), (33, 32), (TILE // 2, TILE // 2 - 1), (TILE // 2, TILE // 2),
                                     (TILE // 2 + 1, TILE // 2), (TILE + 5, TILE + 6)])
def test_environment_sizes(n_a, n_b):
    a, b = _ball_cloud(300 + n_a, n_a, CATS7), _ball_cloud(400 + n_b, n_b, CATS7)
    fa, fb = len(a.xyz) - 1, len(b.xyz) - 1  # far atoms: alone in their environments
    pairs = [(0, 0), (fa, 0), (0, fb), (fa, fb)]  # the full environments, one side empty of neighbours, both anchors alone
    got = _run(CATS7, a, b, pairs, 6.5, wf=("hyper_exp", FAMILIES["hyper_exp"]), what=f"{n_a} + {n_b} events")
    assert got.count_a[0] == n_a + 1 and got.count_b[0] == n_b + 1 and got.count_a[3] == got.count_b[3] == 1
    assert np.all(got.g_a[3] == 0.0) and np.all(got.idx_a[3, 1:] == -1)


@pytest.mark.parametrize("n_cat", [1, 2, 20, 64])
def test_category_counts(n_cat):
    cats = [f"k{k}" for k in range(n_cat)]
    a, b = _random_cloud(500 + n_cat, 200, 14.0, cats), _random_cloud(600 + n_cat, 200, 14.0, cats)
    rng = np.random.default_rng(n_cat)
    pairs = [(int(i), int(j)) for i, j in rng.integers(0, 200, (10, 2))]
    _run(cats, a, b, pairs, 7.0, what=f"{n_cat} categories")
    _run(cats, a, b, pairs, 7.0, weights=rng.uniform(0.3, 3.0, n_cat), sd=DISTANCES["kl"], what=f"{n_cat} categories, weighted, KL")


def test_65_categories_are_refused():
    lh = _lh()
    cats = [f"k{k}" for k in range(65)]
    a = _random_cloud(7, 30, 8.0, cats)
    with pytest.raises(NotImplementedError, match="64 categories"):
        lh.LoCoHD(cats, lh.WeightFunction(*UNI)).sensitivity_from_primitives(a.atoms, a.atoms, [(0, 1)], 6.0)


def test_exact_ties_come_out_in_distance_then_index_order():
    """A lattice: many members at exactly equal distances, within a list and across the two."""
    g = np.stack(np.meshgrid(*[np.arange(5.0)] * 3, indexing="ij"), -1).reshape(-1, 3) * 2.0
    rng = np.random.default_rng(5)
    a = Cloud(g, rng.integers(0, 7, len(g)), np.zeros(len(g), dtype=int), CATS7)
    b = Cloud(g[::-1].copy(), rng.integers(0, 7, len(g)), np.zeros(len(g), dtype=int), CATS7)
    pairs = [(62, 62), (0, 124), (31, 7), (62, 0)]
    got = _run(CATS7, a, b, pairs, 5.0, wf=("hyper_exp", FAMILIES["hyper_exp"]), what="lattice ties")
    for idx, dist, cnt in ((got.idx_a, got.dist_a, got.count_a), (got.idx_b, got.dist_b, got.count_b)):
        for p in range(len(pairs)):
            rest = list(zip(dist[p, 1:cnt[p]], idx[p, 1:cnt[p]]))
            assert rest == sorted(rest) and len(set(dist[p, 1:cnt[p]])) < cnt[p] - 1 and dist[p, 0] == 0.0


def test_largest_environment_and_one_over_it():
    lh = _lh()
    cats = ["x", "y"]
    a, b = _ball_cloud(31, MAX_POINTS - 1, cats, n_far=1), _ball_cloud(32, 700, cats, n_far=1)
    got = _run(cats, a, b, [(0, 0)], 6.5, what=f"{MAX_POINTS} points against 701")
    assert got.count_a[0] == MAX_POINTS and got.idx_a.shape[1] == MAX_POINTS
    over = _ball_cloud(33, MAX_POINTS, cats, n_far=1)
    with pytest.raises(NotImplementedError, match="at most 65535"):
        lh.LoCoHD(cats, lh.WeightFunction(*UNI)).sensitivity_from_primitives(over.atoms, b.atoms, [(0, 0)], 6.5)


def test_width_too_small_and_bad_key_row(two_clouds, pairs30):
    lh, (a, b) = _lh(), two_clouds
    from loco_hd_amd.device import DeviceSession

    l = lh.LoCoHD(CATS7, lh.WeightFunction(*UNI))
    with pytest.raises(ValueError, match="row width 4 is too small"):
        l.sensitivity_from_primitives(a.atoms, b.atoms, pairs30, 8.0, width=4)
    with pytest.raises(lh.PanicException):
        l.sensitivity_from_primitives(a.atoms, b.atoms, [(0, 300)], 8.0)
    d = lh.LoCoHD(CATS7, {"u": lh.WeightFunction(*UNI), "h": lh.WeightFunction("hyper_exp", FAMILIES["hyper_exp"])})
    sess = DeviceSession(d)
    try:
        torch = sess.torch
        ca, cb = [sess.upload(c.xyz, c.cat_ids.astype(np.int32), c.tag_ids.astype(np.int32)) for c in (a, b)]
        anc = torch.tensor([[0, 1], [2, 3], [4, 5]], dtype=torch.int64, device="cuda")
        wf = torch.tensor([0, 2, 1], dtype=torch.int32, device="cuda")  # index 2 is outside a dictionary of two
        full = sess.sensitivity(ca, cb, anc, 8.0)
        out = type(full)(*[torch.zeros_like(t) for t in full])
        with pytest.raises(ValueError):
            sess.sensitivity(ca, cb, anc, 8.0, out=out, wf_index=wf)
        assert torch.isnan(out.scores[1]) and torch.isnan(out.g_a[1]).all() and out.count_a[1] == 0  # the row is NaN, as a radial row is
        assert torch.isfinite(out.scores[[0, 2]]).all()
    finally:
        sess.close()


def test_device_session_gradient_autograd_and_streams(two_clouds):
    lh = _lh()
    from loco_hd_amd.autograd import locohd_scores
    from loco_hd_amd.device import DeviceSession

    rng = np.random.default_rng(41)
    cats = CATS7
    a, b = _random_cloud(71, 40, 9.0, cats), _random_cloud(72, 40, 9.0, cats)
    pairs = rng.integers(0, 40, (25, 2))
    l = lh.LoCoHD(cats, lh.WeightFunction(*UNI))
    host = l.sensitivity_from_primitives(a.atoms, b.atoms, [tuple(map(int, p)) for p in pairs], 8.0)
    v = rng.uniform(0.5, 2.0, len(pairs))
    s_host, ga_host, gb_host = l.gradient_from_primitives(a.atoms, b.atoms, [tuple(map(int, p)) for p in pairs], 8.0, pair_weights=v)
    want = su.from_primitives(a.cat_ids, a.xyz, a.tag_ids, b.cat_ids, b.xyz, b.tag_ids, pairs, 8.0, 7, UNI)
    ga_model, gb_model = su.gradient(want, a.xyz, b.xyz, v)
    # an atom's sum has at most 25 pairs x 100 members terms v g (x_m - x_anchor) / d with |v| <= 2 and a unit direction: each within
    # 2 TOL_G of the model's, plus the float64 rounding of the sum itself
    bound = 25 * 100 * 2 * TOL_G + 1e-13
    assert np.max(np.abs(ga_host - ga_model)) <= bound and np.max(np.abs(gb_host - gb_model)) <= bound
    assert np.max(np.abs(ga_host.sum(0))) <= 1e-12 and np.max(np.abs(gb_host.sum(0))) <= 1e-12  # translation invariance
    sess = DeviceSession(l)
    try:
        torch = sess.torch
        ca, cb = [sess.upload(c.xyz, c.cat_ids.astype(np.int32), c.tag_ids.astype(np.int32)) for c in (a, b)]
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):  # the anchors are produced on the stream the session then runs on
            sess.use_current_stream()
            big = torch.randn(2048, 2048, device="cuda")
            for _ in range(3):
                big = big @ big * 1e-3
            anc = (torch.from_numpy(pairs).cuda() + (big[0, 0] * 0).long()).contiguous()
            dev = sess.sensitivity(ca, cb, anc, 8.0)
            for name in dev._fields:
                assert np.array_equal(getattr(dev, name).cpu().numpy(), getattr(host, name)), name
            xa, xb = torch.from_numpy(a.xyz).cuda(), torch.from_numpy(b.xyz).cuda()
            s_dev, ga_dev, gb_dev = sess.gradient(ca, cb, anc, 8.0, xa, xb, pair_weights=torch.from_numpy(v).cuda())
            assert np.array_equal(s_dev.cpu().numpy(), s_host)
            assert np.max(np.abs(ga_dev.cpu().numpy() - ga_host)) <= 1e-13 and np.max(np.abs(gb_dev.cpu().numpy() - gb_host)) <= 1e-13
            # backward of the autograd function against the host gradient
            x = xa.clone().requires_grad_(True)
            scores = locohd_scores(sess, cb, x, a.cat_ids.astype(np.int32), a.tag_ids.astype(np.int32), anc, 8.0)
            assert np.array_equal(scores.detach().cpu().numpy(), s_host)
            (scores * torch.from_numpy(v).cuda()).sum().backward()
            assert np.max(np.abs(x.grad.cpu().numpy() - ga_host)) <= 1e-13
        torch.cuda.synchronize()
    finally:
        torch.cuda.current_stream().synchronize()
        sess.use_current_stream()
        sess.close()
