"""Dense ensembles (LoCoHD.from_coords_ensemble / from_dmxs_ensemble, DeviceSession.from_coords_ensemble; lchd_ensemble.hip):
M structures of one topology scored all-vs-all -- python_codes/ensembles/compare_ensembles.py:277-296 of the reference, where every
pair i < j is one from_dmxs call -- with each structure's dense rows sorted once.  Row r of structure pair (i, j) must equal
from_coords(seq, seq, X[i], X[j])[r] (1e-12; bit for bit in deterministic mode) and the CPU oracle on sampled rows (1e-11)."""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TIGHT = 1e-11
SAME = 1e-12
NAMES = [f"c{i}" for i in range(300)]


@pytest.fixture(scope="module")
def lh():
    import loco_hd_amd

    return loco_hd_amd


def ensemble(rng, m, n, n_cat, jitter=1.0):
    """m conformations of one n-point topology: a common cloud plus per-structure displacements."""
    side = (n / 0.05) ** (1 / 3)
    base = rng.uniform(0.0, side, (n, 3))
    seq = [NAMES[k] for k in rng.integers(0, n_cat, n)]
    return seq, np.stack([base + rng.normal(0.0, jitter, (n, 3)) for _ in range(m)])


def dist_matrix(x):
    d = x[:, None, :] - x[None, :, :]
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])  # utils.rs:1-8 order


def oracle_rows(lo, seq, rows_a, rows_b, keys=None):
    """stat_dist_integral on the stably sorted rows (utils.rs:25-39), one from_anchors call per row pair."""
    out = []
    for k, (ra, rb) in enumerate(zip(rows_a, rows_b)):
        ra, rb = np.asarray(ra, dtype=float) + 0.0, np.asarray(rb, dtype=float) + 0.0
        oa, ob = np.argsort(ra, kind="stable"), np.argsort(rb, kind="stable")
        args = ([seq[i] for i in oa], [seq[i] for i in ob], ra[oa].tolist(), rb[ob].tolist())
        out.append(lo.from_anchors(*args) if keys is None else lo.from_anchors(*args, keys[k]))
    return np.asarray(out)


def all_pairs(m):
    return [(i, j) for i in range(m) for j in range(i + 1, m)]


@pytest.mark.parametrize("n", [37, 300, 1024, 1500, 3000])
def test_default_pairs_match_from_coords_and_oracle(lh, oracle, n):
    rng = np.random.default_rng(500 + n)
    m, n_cat, wf = 5, 10, ("uniform", [3.0, 10.0])
    seq, xs = ensemble(rng, m, n, n_cat)
    lchd = lh.LoCoHD(NAMES[:n_cat], lh.WeightFunction(*wf))
    got = lchd.from_coords_ensemble(seq, xs)
    assert got.shape == (m * (m - 1) // 2, n) and got.dtype == np.float64
    lo = oracle.LoCoHD(NAMES[:n_cat], oracle.WeightFunction(*wf))
    rows = sorted(set(rng.integers(0, n, 6).tolist()) | {0, n - 1})
    for p, (i, j) in enumerate(all_pairs(m)):
        want = np.asarray(lchd.from_coords(seq, seq, xs[i], xs[j]))
        assert np.max(np.abs(got[p] - want)) < SAME
        if p in (0, 9):
            da, db = dist_matrix(xs[i]), dist_matrix(xs[j])
            ref = oracle_rows(lo, seq, [da[r] for r in rows], [db[r] for r in rows])
            assert np.max(np.abs(got[p][rows] - ref)) < TIGHT


def test_explicit_pairs_self_reversed_and_repeated(lh):
    rng = np.random.default_rng(11)
    m, n, n_cat, wf = 5, 300, 10, ("uniform", [3.0, 10.0])
    seq, xs = ensemble(rng, m, n, n_cat)
    lchd = lh.LoCoHD(NAMES[:n_cat], lh.WeightFunction(*wf))
    base = lchd.from_coords_ensemble(seq, xs)
    index = {pq: k for k, pq in enumerate(all_pairs(m))}
    pairs = [(2, 2), (3, 1), (1, 3), (0, 4), (0, 4), (4, 0), (1, 1)]
    got = lchd.from_coords_ensemble(seq, list(xs), structure_pairs=pairs)
    assert got.shape == (len(pairs), n)
    for k, (i, j) in enumerate(pairs):
        if i == j:
            assert np.max(np.abs(got[k])) < SAME  # a structure against itself
        elif i < j:
            assert np.max(np.abs(got[k] - base[index[(i, j)]])) < SAME
        else:
            assert np.max(np.abs(got[k] - np.asarray(lchd.from_coords(seq, seq, xs[i], xs[j])))) < SAME


def test_homo_residue_exclusions_match_from_dmxs(lh, oracle):
    """The script's ban (compare_ensembles.py:234-263): contacts between atoms of the same residue set to +inf, both orders."""
    rng = np.random.default_rng(23)
    m, n, n_cat, wf = 4, 240, 10, ("uniform", [3.0, 10.0])
    seq, xs = ensemble(rng, m, n, n_cat)
    resi = np.repeat(np.arange(n // 4), 4)
    excl = [(a, b) for a, b in itertools.permutations(range(n), 2) if resi[a] == resi[b]]
    dmxs = []
    for x in xs:
        d = dist_matrix(x)
        for a, b in excl:
            d[a, b] = np.inf
        dmxs.append(d)
    lchd = lh.LoCoHD(NAMES[:n_cat], lh.WeightFunction(*wf))
    got = lchd.from_coords_ensemble(seq, xs, excluded_pairs=excl)
    lo = oracle.LoCoHD(NAMES[:n_cat], oracle.WeightFunction(*wf))
    rows = [0, 1, 77, n - 1]
    for p, (i, j) in enumerate(all_pairs(m)):
        want = np.asarray(lchd.from_dmxs(seq, seq, dmxs[i], dmxs[j]))
        assert np.max(np.abs(got[p] - want)) < SAME
        ref = oracle_rows(lo, seq, [dmxs[i][r] for r in rows], [dmxs[j][r] for r in rows])
        assert np.max(np.abs(got[p][rows] - ref)) < TIGHT
    # the same matrices through from_dmxs_ensemble: the same rows are sorted, so the same bits (deterministic mode: ties included)
    det = lh.LoCoHD(NAMES[:n_cat], lh.WeightFunction(*wf), deterministic=True)
    assert np.array_equal(det.from_dmxs_ensemble(seq, dmxs), det.from_coords_ensemble(seq, xs, excluded_pairs=excl))


def lattice_ensemble(rng, m, g, n_cat):
    """m copies of a g^3 integer lattice, every point twice (ties at every distance), each copy shifted by an integer vector and
    with a few points moved by whole lattice steps: exact ties in every row of every structure."""
    pts = np.repeat(np.array(list(itertools.product(range(g), repeat=3)), dtype=float), 2, axis=0)
    seq = [NAMES[k] for k in rng.integers(0, n_cat, len(pts))]
    xs = []
    for _ in range(m):
        x = pts + rng.integers(-3, 4, 3)
        mv = rng.choice(len(pts), 6, replace=False)
        x[mv] += rng.integers(-1, 2, (6, 3))
        xs.append(x)
    return seq, np.stack(xs)


def test_deterministic_bits_equal_per_pair_calls_and_blocking(lh, monkeypatch):
    rng = np.random.default_rng(31)
    m, n_cat, wf = 5, 6, ("hyper_exp", [1.0, 0.3])
    seq, xs = lattice_ensemble(rng, m, 5, n_cat)
    det = lh.LoCoHD(NAMES[:n_cat], lh.WeightFunction(*wf), deterministic=True)
    got = det.from_coords_ensemble(seq, xs)
    for p, (i, j) in enumerate(all_pairs(m)):
        assert np.array_equal(got[p], np.asarray(det.from_coords(seq, seq, xs[i], xs[j])))
    monkeypatch.setenv("LCHD_ENSEMBLE_BLOCK", "2")  # one structure per block: five blocks, rows rebuilt per block pair
    blocked = lh.LoCoHD(NAMES[:n_cat], lh.WeightFunction(*wf), deterministic=True)
    assert np.array_equal(blocked.from_coords_ensemble(seq, xs), got)
    pairs = [(4, 0), (1, 1), (3, 2), (0, 4)]
    again = blocked.from_coords_ensemble(seq, xs, structure_pairs=pairs)
    for k, (i, j) in enumerate(pairs):
        assert np.array_equal(again[k], np.asarray(det.from_coords(seq, seq, xs[i], xs[j])))


def test_blocked_default_mode_matches(lh, monkeypatch):
    rng = np.random.default_rng(37)
    seq, xs = ensemble(rng, 6, 500, 10)
    wf = ("uniform", [3.0, 10.0])
    want = lh.LoCoHD(NAMES[:10], lh.WeightFunction(*wf)).from_coords_ensemble(seq, xs)
    monkeypatch.setenv("LCHD_ENSEMBLE_BLOCK", "3")  # odd cap: two slots, six blocks
    got = lh.LoCoHD(NAMES[:10], lh.WeightFunction(*wf)).from_coords_ensemble(seq, xs)
    assert np.max(np.abs(got - want)) < SAME


CONFIGS = {
    "w_func_dict": dict(n_cat=8, n=200),
    "category_weights": dict(n_cat=8, n=200),
    "kolmogorov_smirnov": dict(n_cat=8, n=200),
    "hellinger_e3": dict(n_cat=8, n=200),
    "categories_300": dict(n_cat=300, n=300),
}


@pytest.mark.parametrize("case", list(CONFIGS))
def test_configurations_match_oracle(lh, oracle, case):
    rng = np.random.default_rng(100 + list(CONFIGS).index(case))
    n_cat, n, m = CONFIGS[case]["n_cat"], CONFIGS[case]["n"], 3
    seq, xs = ensemble(rng, m, n, n_cat)
    cats = NAMES[:n_cat]
    kw, okw, keys = {}, {}, None
    wf, owf = lh.WeightFunction("uniform", [3.0, 10.0]), oracle.WeightFunction("uniform", [3.0, 10.0])
    if case == "w_func_dict":
        wf = {"a": wf, "b": lh.WeightFunction("hyper_exp", [1.0, 0.2])}
        owf = {"a": owf, "b": oracle.WeightFunction("hyper_exp", [1.0, 0.2])}
        keys = [("a", "b")[k] for k in rng.integers(0, 2, n)]
    elif case == "category_weights":
        w = rng.uniform(0.5, 2.0, n_cat).tolist()
        kw, okw = dict(category_weights=w), dict(category_weights=w)
    elif case == "kolmogorov_smirnov":
        kw = dict(statistical_distance=lh.StatisticalDistance("Kolmogorov-Smirnov", []))
        okw = dict(statistical_distance=oracle.StatisticalDistance("Kolmogorov-Smirnov", []))
    elif case == "hellinger_e3":
        kw = dict(statistical_distance=lh.StatisticalDistance("Hellinger", [3.0]))
        okw = dict(statistical_distance=oracle.StatisticalDistance("Hellinger", [3.0]))
    lchd = lh.LoCoHD(cats, wf, **kw)
    lo = oracle.LoCoHD(cats, owf, **okw)
    got = lchd.from_coords_ensemble(seq, xs, w_func_keys=keys)
    rows = [0, 5, n // 2, n - 1]
    for p, (i, j) in enumerate(all_pairs(m)):
        da, db = dist_matrix(xs[i]), dist_matrix(xs[j])
        ref = oracle_rows(lo, seq, [da[r] for r in rows], [db[r] for r in rows], None if keys is None else [keys[r] for r in rows])
        assert np.max(np.abs(got[p][rows] - ref)) < TIGHT
        assert np.max(np.abs(got[p] - np.asarray(lchd.from_coords(seq, seq, xs[i], xs[j], w_func_keys=keys)))) < SAME


def test_device_session_frames_buffer_matches_host_entry(lh):
    import torch

    from loco_hd_amd.device import DeviceSession

    rng = np.random.default_rng(41)
    m, n, n_cat = 6, 400, 10
    seq, xs = ensemble(rng, m, n, n_cat)
    det = lh.LoCoHD(NAMES[:n_cat], lh.WeightFunction("uniform", [3.0, 10.0]), deterministic=True)
    want = det.from_coords_ensemble(seq, xs)
    sess = DeviceSession(det)
    try:
        cat = det._cats(seq)
        tmpl = sess.upload(xs[0], cat)
        buf = sess.frames_buffer(tmpl, m)
        sess.load_frames(buf, xs)
        got = sess.from_coords_ensemble(buf).cpu().numpy()
        assert np.array_equal(got, want)
        batch, _ = sess.upload_batch([(x, cat) for x in xs])
        pairs = torch.tensor([[5, 0], [2, 2]], dtype=torch.int32, device=torch.device("cuda", sess.device))
        two = sess.from_coords_ensemble(batch, pairs=pairs).cpu().numpy()
        assert np.array_equal(two[0], np.asarray(det.from_coords(seq, seq, xs[5], xs[0])))
        assert np.all(two[1] == 0.0)
    finally:
        sess.close()


def test_errors(lh):
    from loco_hd_amd import _native as N
    from loco_hd_amd.device import DeviceSession

    rng = np.random.default_rng(43)
    seq, xs = ensemble(rng, 3, 50, 4)
    lchd = lh.LoCoHD(NAMES[:4], lh.WeightFunction("uniform", [3.0, 10.0]))
    with pytest.raises(ValueError, match="Expected matrices with the same length"):
        lchd.from_coords_ensemble(seq, [xs[0], xs[1][:40]])
    with pytest.raises(ValueError, match="structure"):
        lchd.from_coords_ensemble(seq, xs, structure_pairs=[(0, 3)])
    with pytest.raises(ValueError):
        lchd.from_coords_ensemble(seq, xs, excluded_pairs=[(0, 50)])
    with pytest.raises(ValueError):  # the diagonal banned: the row no longer starts at distance 0 (src/locohd.rs:74-77)
        lchd.from_coords_ensemble(seq, xs, excluded_pairs=[(3, 3)])
    with pytest.raises(ValueError, match="w_func"):
        lchd.from_coords_ensemble(seq, xs, w_func_keys=["a"] * 50)
    # the C entry itself rejects an out-of-range pair and a cloud that is not a regular batch
    cfg, keep = lchd._config()
    cs = lchd._cats(seq)
    out = np.empty((1, 50))
    bad = np.asarray([[0, 7]], dtype=np.int32)
    x = np.ascontiguousarray(xs)
    assert N.lib().lchd_ensemble_from_coords(lchd._context(), N.C.byref(cfg), N.ip(cs), 50, N.dp(x), 3, N.ip(bad), 1, None, None, None,
                                             N.dp(out)) == N.EVALUE
    sess = DeviceSession(lchd)
    try:
        irregular, _ = sess.upload_batch([(xs[0], cs), (xs[1][:40], cs[:40])])
        with pytest.raises(ValueError, match="regular batch"):
            sess.from_coords_ensemble(irregular)
        single = sess.upload(xs[0], cs)
        with pytest.raises(ValueError, match="regular batch"):
            sess.from_coords_ensemble(single)
    finally:
        sess.close()
    # rows beyond the dense limits: more than 65535 points with more than 255 categories
    wide = lh.LoCoHD(NAMES[:300], lh.WeightFunction("uniform", [3.0, 10.0]))
    big = rng.uniform(0.0, 100.0, (2, 70000, 3))
    with pytest.raises(NotImplementedError, match="65535"):
        wide.from_coords_ensemble([NAMES[k % 300] for k in range(70000)], big)
