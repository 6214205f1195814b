"""Weight-function gradients on the device against the numpy restatement (tests/weight_gradient_util.py, longdouble, from the definition;
tests/test_weight_gradient_model.py pins it to finite differences of the CPU oracle).

Expected values never come from the library.  Bound: the same restatement run in float64 deviates from the longdouble one by at most
FLOAT64_DEVIATION on theta_k * grad[p][k] over the cases of this module (measured on the CPU: test_float64_restatement_deviation prints
and asserts it); that is within 1e-12, so the bound is the project's parity bound, 1e-11 absolute on theta_k * grad[p][k].  Scores are
held to 1e-11 of the CPU oracle."""
import numpy as np
import pytest

import weight_gradient_util as wg
from attribution_util import open_rows

TOL = wg.PARITY  # 1e-11
FLOAT64_DEVIATION = 1e-12
TILE = 384  # kSweepTile (loco_hd_amd/csrc/lchd_device.h): merged events per tile of the kernel
CATS7 = [f"c{k}" for k in range(7)]
UNI = ("uniform", [3.0, 10.0])
FAMILIES = {"uniform": [3.0, 10.0], "hyper_exp": [1.0, 0.5, 0.2, 0.05], "dagum": [4.0, 6.0, 1.5], "kumaraswamy": [2.0, 11.0, 2.0, 3.0]}
DISTANCES = {"h2": ("Hellinger", [2.0]), "h3.5": ("Hellinger", [3.5]), "ks": ("Kolmogorov-Smirnov", []), "kl": ("Kullback-Leibler", [1e-3]),
             "renyi": ("Renyi", [2.5, 1e-3])}
gpu = pytest.mark.gpu


def _lh():
    import loco_hd_amd as lh

    return lh


class Cloud:
    def __init__(self, seed, n, edge, cats=CATS7, n_tags=4):
        rng = np.random.default_rng(seed)
        self.xyz = rng.uniform(0.0, edge, (n, 3))
        self.cat_ids = rng.integers(0, len(cats), n)
        self.types = [cats[k] for k in self.cat_ids]
        self.tag_ids = rng.integers(0, n_tags, n)
        self.tags = [f"t{k}" for k in self.tag_ids]

    def atoms(self, mod):
        return [mod.PrimitiveAtom(t, g, list(c)) for t, g, c in zip(self.types, self.tags, self.xyz)]


@pytest.fixture(scope="module", autouse=True)
def library_leaf():
    """Every conclusion of this module is about the restated leaf; it carries over to the library only where the library's host leaf
    (the function the kernel calls) is that leaf: 1e-13 on theta_k * G_k, a few ulp of values of size <= 1."""
    worst = wg.library_leaf_deviation(FAMILIES)
    print(f"max |theta (library leaf - restated leaf)| = {worst:.3g}")
    assert worst <= 1e-13


@pytest.fixture(scope="module")
def two_clouds():
    return Cloud(101, 300, 20.0), Cloud(102, 300, 20.0)


@pytest.fixture(scope="module")
def pairs40():
    rng = np.random.default_rng(9)
    return [(int(i), int(j)) for i, j in rng.integers(0, 300, (40, 2))]


def _locohd(sd=DISTANCES["h2"], wf=UNI, mod=None, **kw):
    lh = _lh() if mod is None else mod
    w = {k: lh.WeightFunction(*v) for k, v in wf.items()} if isinstance(wf, dict) else lh.WeightFunction(*wf)
    return lh.LoCoHD(CATS7, w, statistical_distance=lh.StatisticalDistance(sd[0], sd[1]), **kw)


def _theta(wfs, width):
    """[P][width]: the parameters of every row's function, 1 in the padding."""
    t = np.ones((len(wfs), width))
    for p, f in enumerate(wfs):
        t[p, :len(f[1])] = f[1]
    return t


def _check(got, want, wfs, what, tol=TOL):
    """got: a WeightGradient from the library; want: (scores, grad) of the restatement (longdouble); wfs: the function of every row."""
    grad = np.asarray(got.grad)
    assert grad.shape == want[1].shape and np.asarray(got.scores).shape == (len(wfs),), what
    assert np.isfinite(grad).all(), what
    err = float(np.max(np.abs((grad.astype(np.longdouble) - want[1]) * _theta(wfs, grad.shape[1])))) if grad.size else 0.0
    serr = float(np.max(np.abs(np.asarray(got.scores).astype(np.longdouble) - want[0]))) if grad.size else 0.0
    print(f"{what}: max |theta (device - expected)| = {err:.3g}, max |score - expected| = {serr:.3g}")
    assert err <= tol and serr <= tol, what
    for p, f in enumerate(wfs):  # the padding columns are exact zeros
        assert np.all(grad[p, len(f[1]):] == 0.0) and not np.any(np.signbit(grad[p, len(f[1]):])), what


def _restated(a, b, pairs, thr, wf, sd, dtype=wg.LD):
    return wg.from_primitives(a.cat_ids, a.xyz, a.tag_ids, b.cat_ids, b.xyz, b.tag_ids, pairs, thr, 7, wf, sd, dtype=dtype)


# ---- the bound ------------------------------------------------------------------------------------------------------------------------
def test_float64_restatement_deviation(two_clouds, pairs40):
    """CPU: how far the restatement in float64 is from the restatement in longdouble, on theta_k * grad[p][k]: measured 4.8e-15 at most
    over the twenty thresholded cases (the rounding of a sum of a few hundred terms of size <= 1), far inside 1e-12."""
    a, b = two_clouds
    worst = 0.0
    for family, params in FAMILIES.items():
        for sd in DISTANCES.values():
            ld = _restated(a, b, pairs40, 8.0, (family, params), sd)[1]
            f64 = _restated(a, b, pairs40, 8.0, (family, params), sd, np.float64)[1]
            worst = max(worst, float(np.max(np.abs((ld - f64) * np.asarray(params)[None, :]))))
    print(f"max |theta (float64 - longdouble)| = {worst:.3g}")
    assert worst <= FLOAT64_DEVIATION


# ---- thresholded parity ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dist", sorted(DISTANCES))
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_families_and_distances(two_clouds, pairs40, oracle, family, dist):
    (a, b), sd, wf = two_clouds, DISTANCES[dist], (family, FAMILIES[family])
    lh = _lh()
    got = _locohd(sd, wf).weight_gradient_from_primitives(a.atoms(lh), b.atoms(lh), pairs40, 8.0)
    assert isinstance(got, lh.WeightGradient) and got.grad.dtype == np.float64 and got.grad.shape == (40, len(wf[1]))
    _check(got, _restated(a, b, pairs40, 8.0, wf, sd), [wf] * 40, f"{family}, {dist}")
    want = np.asarray(_locohd(sd, wf, oracle).from_primitives(a.atoms(oracle), b.atoms(oracle), pairs40, 8.0))
    assert float(np.max(np.abs(got.scores - want))) <= 1e-11
    assert np.any(np.abs(got.grad) > 1e-4)
    if family == "hyper_exp":
        assert float(np.max(np.abs((got.grad[:, :2] * np.asarray(wf[1][:2])).sum(1)))) <= TOL


@gpu
def test_dictionary_with_per_anchor_keys(two_clouds, pairs40):
    a, b = two_clouds
    lh = _lh()
    specs = {"u": UNI, "d": ("dagum", FAMILIES["dagum"]), "k": ("kumaraswamy", FAMILIES["kumaraswamy"])}  # n_params 2, 3, 4
    keys = [("u", "d", "k")[p % 3] for p in range(40)]
    keyed = [(i, j, k) for (i, j), k in zip(pairs40, keys)]
    sd = DISTANCES["kl"]
    got = _locohd(sd, specs).weight_gradient_from_primitives(a.atoms(lh), b.atoms(lh), keyed, 8.0)
    assert got.grad.shape == (40, 4)
    wfs = [specs[k] for k in keys]
    _check(got, _restated(a, b, pairs40, 8.0, wfs, sd), wfs, "dictionary, per-anchor keys")


@gpu
def test_support_beyond_the_threshold(two_clouds, pairs40, oracle):
    """uniform [12, 15] with threshold 10: no member moves F, the row is exact zeros and the score the distance of the whole environments."""
    a, b = two_clouds
    lh = _lh()
    wf = ("uniform", [12.0, 15.0])
    got = _locohd(wf=wf).weight_gradient_from_primitives(a.atoms(lh), b.atoms(lh), pairs40, 10.0)
    assert np.all(got.grad == 0.0)
    want = np.asarray(_locohd(wf=wf, mod=oracle).from_primitives(a.atoms(oracle), b.atoms(oracle), pairs40, 10.0))
    assert float(np.max(np.abs(got.scores - want))) <= 1e-11 and np.all(got.scores > 0.0)


@gpu
def test_bits_repeat_and_do_not_depend_on_the_other_pairs(two_clouds, pairs40):
    a, b = two_clouds
    lh = _lh()
    l = _locohd(DISTANCES["h3.5"], ("kumaraswamy", FAMILIES["kumaraswamy"]))
    pa, pb = a.atoms(lh), b.atoms(lh)
    one, two = (l.weight_gradient_from_primitives(pa, pb, pairs40, 8.0) for _ in range(2))
    assert one.grad.tobytes() == two.grad.tobytes() and one.scores.tobytes() == two.scores.tobytes()
    more = l.weight_gradient_from_primitives(pa, pb, [(7, 7), (250, 3)] + pairs40[:10] + [(1, 299)], 8.0)
    assert more.grad[2:12].tobytes() == one.grad[:10].tobytes() and more.scores[2:12].tobytes() == one.scores[:10].tobytes()


# ---- dense rows ------------------------------------------------------------------------------------------------------------------------
def _dense_case(n, seed):
    rng = np.random.default_rng(seed)
    xa, xb = rng.uniform(0.0, 14.0, (n, 3)), rng.uniform(0.0, 14.0, (n, 3))
    ca, cb = rng.integers(0, 7, n), rng.integers(0, 7, n)
    return xa, xb, ca, cb, [CATS7[k] for k in ca], [CATS7[k] for k in cb]


@gpu
@pytest.mark.parametrize("n", [40, 200])
@pytest.mark.parametrize("family", ["uniform", "dagum"])
def test_dense_rows_from_coords_and_from_dmxs(n, family):
    wf, sd = (family, FAMILIES[family]), DISTANCES["h2"]
    xa, xb, ca, cb, sa, sb = _dense_case(n, 50 + n)
    ma, mb = open_rows(xa), open_rows(xb)
    want = wg.from_rows(ca, ma, cb, mb, 7, wf, sd)
    l = _locohd(sd, wf)
    _check(l.weight_gradient_from_coords(sa, sb, xa, xb), want, [wf] * n, f"from_coords {n}, {family}")
    _check(l.weight_gradient_from_dmxs(sa, sb, ma, mb), want, [wf] * n, f"from_dmxs {n}, {family}")


@gpu
@pytest.mark.parametrize("events", [63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_tile_and_lane_seams(events):
    """Pairs with exactly `events` merged non-anchor events: split between the sides, and with side B empty beyond its anchor."""
    rng = np.random.default_rng(events)
    wf, sd = ("kumaraswamy", FAMILIES["kumaraswamy"]), DISTANCES["h2"]
    l = _locohd(sd, wf)
    for m_b in (events // 3, 0):
        m_a = events - m_b
        ma = np.concatenate([np.zeros((3, 1)), rng.uniform(0.1, 12.0, (3, m_a))], axis=1)
        mb = np.concatenate([np.zeros((3, 1)), rng.uniform(0.1, 12.0, (3, m_b))], axis=1)
        ca, cb = rng.integers(0, 7, 1 + m_a), rng.integers(0, 7, 1 + m_b)
        got = l.weight_gradient_from_dmxs([CATS7[k] for k in ca], [CATS7[k] for k in cb], ma, mb)
        _check(got, wg.from_rows(ca, ma, cb, mb, 7, wf, sd), [wf] * 3, f"{m_a} + {m_b} events")


@gpu
def test_lone_anchors_identical_environments_and_ties():
    wf, sd = ("uniform", [0.0, 10.0]), DISTANCES["h2"]
    l = _locohd(sd, wf)
    # a lone anchor on both sides: the boundary terms only, -G(0) H_first = (1 / 10, 0) * H
    got = l.weight_gradient_from_dmxs(["c0"], ["c1"], np.zeros((2, 1)), np.zeros((2, 1)))
    _check(got, wg.from_rows([0], np.zeros((2, 1)), [1], np.zeros((2, 1)), 7, wf, sd), [wf] * 2, "lone anchors")
    assert np.all(got.scores == 1.0) and np.all(got.grad[:, 0] == 0.1) and np.all(got.grad[:, 1] == 0.0)
    # two identical environments under Hellinger: exact zeros and a score of 0
    rng = np.random.default_rng(12)
    m = np.concatenate([np.zeros((2, 1)), rng.uniform(0.1, 12.0, (2, 90))], axis=1)
    c = rng.integers(0, 7, 91)
    s = [CATS7[k] for k in c]
    got = l.weight_gradient_from_dmxs(s, s, m, m)
    assert np.all(got.grad == 0.0) and np.all(got.scores == 0.0)
    # exact ties: duplicated points within a side and equal distances across the sides
    ma = np.concatenate([np.zeros((2, 1)), np.round(rng.uniform(0.1, 12.0, (2, 70)), 0)], axis=1)
    mb = np.concatenate([np.zeros((2, 1)), np.round(rng.uniform(0.1, 12.0, (2, 50)), 0)], axis=1)
    ca, cb = rng.integers(0, 7, 71), rng.integers(0, 7, 51)
    for f in (wf, ("hyper_exp", FAMILIES["hyper_exp"])):
        got = _locohd(sd, f).weight_gradient_from_dmxs([CATS7[k] for k in ca], [CATS7[k] for k in cb], ma, mb)
        _check(got, wg.from_rows(ca, ma, cb, mb, 7, f, sd), [f] * 2, f"ties, {f[0]}")


# ---- error rows ------------------------------------------------------------------------------------------------------------------------
@gpu
def test_bad_category_and_bad_wf_index(two_clouds):
    from loco_hd_amd.device import DeviceSession

    a, b = two_clouds
    lh = _lh()
    pa, pb = a.atoms(lh), b.atoms(lh)
    pa[5] = lh.PrimitiveAtom("not-a-category", pa[5].tag, pa[5].coordinates)
    l = _locohd()
    with pytest.raises(Exception) as info:
        l.weight_gradient_from_primitives(pa, pb, [(5, 5), (9, 9)], 8.0)
    with pytest.raises(type(info.value)):
        l.sensitivity_from_primitives(pa, pb, [(5, 5), (9, 9)], 8.0)
    d = _locohd(wf={"u": UNI, "h": ("hyper_exp", FAMILIES["hyper_exp"])})
    sess = DeviceSession(d)
    try:
        torch = sess.torch
        ca, cb = [sess.upload(c.xyz, c.cat_ids.astype(np.int32), c.tag_ids.astype(np.int32)) for c in (a, b)]
        anc = torch.tensor([[0, 1], [2, 3], [4, 5]], dtype=torch.int64, device="cuda")
        wf = torch.tensor([0, 2, 1], dtype=torch.int32, device="cuda")  # index 2 is outside a dictionary of two
        out = torch.zeros(3 * 5, dtype=torch.float64, device="cuda")
        with pytest.raises(Exception) as bad:
            sess.weight_gradient(ca, cb, anc, 8.0, out=out, wf_index=wf)
        with pytest.raises(type(bad.value)):
            sess.sensitivity(ca, cb, anc, 8.0, wf_index=wf)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        scores, grad = got[:3], got[3:].reshape(3, 4)
        assert np.isnan(scores[1]) and np.isnan(grad[1]).all()
        assert np.isfinite(scores[[0, 2]]).all() and np.isfinite(grad[[0, 2]]).all() and np.all(grad[0, 2:] == 0.0)
    finally:
        sess.close()
