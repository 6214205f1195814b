"""Dense-row neighbour sensitivities on the device against the numpy restatement (tests/dense_sensitivity_util.py on
tests/sensitivity_util.py, longdouble; tests/test_dense_sensitivity_model.py pins it to the score model by central differences).

Expected values never come from the library.  idx and count must match the model exactly and dist must be the input entry bit for bit;
scores must match the scoring call of the same name within 1e-11; g is bounded by the TOL_G of tests/test_gpu_sensitivity.py -- the sweep
kernel is the same (largest deviation measured over this file's cases on an MI355X: DESIGN.md section 5, "Dense sensitivities")."""
import numpy as np
import pytest

import dense_sensitivity_util as du
from test_gpu_sensitivity import DISTANCES, TOL, TOL_G

pytestmark = pytest.mark.gpu

UNI = ("uniform", [3.0, 10.0])
HYP = ("hyper_exp", [1.0, 0.5, 0.2, 0.05])
CATS3 = ["c0", "c1", "c2"]
WORST = {"g": 0.0}


def _lh():
    import loco_hd_amd as lh

    return lh


def _capacity():
    from loco_hd_amd import _native as N

    return N.SENSITIVITY_ROWS_LDS_POINTS


def _matrix(rng, rows, cols, hi=12.0):
    m = rng.uniform(0.2, hi, (rows, cols))
    m[np.arange(rows), rng.integers(0, cols, rows)] = 0.0  # every row holds its 0, in any column
    return m


def _compare(got, want, scores_ref, what, tol_g=TOL_G):
    for name in ("count_a", "count_b", "idx_a", "idx_b"):
        assert np.array_equal(getattr(got, name), getattr(want, name)), f"{what}: {name}"
    for name in ("dist_a", "dist_b"):
        assert np.array_equal(getattr(got, name).view(np.uint64), getattr(want, name).view(np.uint64)), f"{what}: {name}"
    err_s = float(np.max(np.abs(got.scores - np.asarray(scores_ref))))
    err_m = float(np.max(np.abs(got.scores - want.scores)))
    err_g = max(float(np.max(np.abs(got.g_a - want.g_a))), float(np.max(np.abs(got.g_b - want.g_b))))
    WORST["g"] = max(WORST["g"], err_g)
    print(f"{what}: max |g - model| = {err_g:.3g}, |scores - scoring call| = {err_s:.3g}, |scores - model| = {err_m:.3g}  (worst g so far {WORST['g']:.3g})")
    assert np.isfinite(got.g_a).all() and np.isfinite(got.g_b).all()
    assert err_s <= TOL and err_m <= TOL, what
    assert err_g <= tol_g, what


def _run_dmxs(cats, seq_a, dmx_a, seq_b, dmx_b, wf=UNI, sd=DISTANCES["h2"], weights=None, what=""):
    lh = _lh()
    l = lh.LoCoHD(cats, lh.WeightFunction(*wf), category_weights=None if weights is None else list(weights),
                  statistical_distance=lh.StatisticalDistance(*sd))
    names_a, names_b = [cats[c] for c in seq_a], [cats[c] for c in seq_b]
    got = l.sensitivity_from_dmxs(names_a, names_b, dmx_a, dmx_b)
    want = du.from_dmxs(seq_a, dmx_a, seq_b, dmx_b, len(cats), wf, sd, weights)
    _compare(got, want, l.from_dmxs(names_a, names_b, dmx_a, dmx_b), what)
    return got


def _case(seed, rows, cols_a, cols_b, n_cat):
    rng = np.random.default_rng(seed)
    return rng.integers(0, n_cat, cols_a), _matrix(rng, rows, cols_a), rng.integers(0, n_cat, cols_b), _matrix(rng, rows, cols_b)


# around the wave width and kSweepTile = 384 (the tile of k_sensitivity)
@pytest.mark.parametrize("cols", [(1, 1), (1, 65), (2, 64), (63, 385), (384, 384), (769, 130)], ids=lambda c: f"{c[0]}x{c[1]}")
def test_row_lengths(cols):
    sa, ma, sb, mb = _case(300 + cols[0], 3, cols[0], cols[1], 3)
    got = _run_dmxs(CATS3, sa, ma, sb, mb, what=f"cols {cols}")
    assert got.idx_a.shape == (3, max(cols)) and got.count_a.tolist() == [cols[0]] * 3 and got.count_b.tolist() == [cols[1]] * 3


@pytest.mark.parametrize("dist", sorted(DISTANCES))
def test_every_statistical_distance(dist):
    sa, ma, sb, mb = _case(17, 3, 63, 385, 3)
    _run_dmxs(CATS3, sa, ma, sb, mb, sd=DISTANCES[dist], what=f"63 x 385, {dist}")


def test_category_weights_and_a_dictionary_with_row_keys():
    lh = _lh()
    sa, ma, sb, mb = _case(23, 3, 64, 65, 3)
    weights = np.random.default_rng(3).uniform(0.3, 3.0, 3)
    _run_dmxs(CATS3, sa, ma, sb, mb, weights=weights, sd=DISTANCES["h3.5"], what="64 x 65, category weights")
    wfs = {"u": UNI, "h": HYP}
    keys = ["h", "u", "h"]
    l = lh.LoCoHD(CATS3, {k: lh.WeightFunction(*v) for k, v in wfs.items()})
    names_a, names_b = [CATS3[c] for c in sa], [CATS3[c] for c in sb]
    got = l.sensitivity_from_dmxs(names_a, names_b, ma, mb, keys)
    want = du.from_dmxs(sa, ma, sb, mb, 3, [wfs[k] for k in keys])
    _compare(got, want, l.from_dmxs(names_a, names_b, ma, mb, keys), "64 x 65, two weight functions by key")


def _seam_lengths():
    cap = _capacity()
    return sorted({cap - 1, cap, cap + 1} | ({2049} if cap != 2048 else set()))


@pytest.mark.parametrize("cols", _seam_lengths())
def test_the_builders_lds_seam(cols):
    """Rows of capacity - 1 and capacity points are sorted in LDS, capacity + 1 in place in the list block (2049: the seam of
    k_env_indexed, whose in-place sort the builder shares)."""
    sa, ma, sb, mb = _case(cols, 2, cols, cols, 2)
    _run_dmxs(["c0", "c1"], sa, ma, sb, mb, what=f"seam, {cols} columns")


def _lattice():
    """27 atoms on the integer lattice {0, 1, 2}^3 and atom 13's twin at index 27; side B is the same lattice in another category order."""
    g = np.arange(3.0)
    xyz = np.asarray([[x, y, z] for x in g for y in g for z in g] + [[1.0, 1.0, 1.0]])
    rng = np.random.default_rng(5)
    return xyz, rng.integers(0, 3, 28), rng.integers(0, 3, 28)


def test_ties_come_out_in_distance_column_order():
    lh = _lh()
    xyz, ca, cb = _lattice()
    l = lh.LoCoHD(CATS3, lh.WeightFunction(*HYP))
    names_a, names_b = [CATS3[c] for c in ca], [CATS3[c] for c in cb]
    got = l.sensitivity_from_coords(names_a, names_b, xyz, xyz)
    rows = du.coords_rows(xyz)
    want = du.from_dmxs(ca, rows, cb, rows, 3, HYP)
    _compare(got, want, l.from_coords(names_a, names_b, xyz, xyz), "lattice with a twin")
    for r in range(28):
        members = list(zip(got.dist_a[r], got.idx_a[r]))
        assert members == sorted(members) and len(set(got.dist_a[r])) <= 10  # 28 members at 10 distances at most: ties, in column order
    assert got.idx_a[27, 0] == 13 and got.idx_a[27, 1] == 27 and got.idx_a[13, :2].tolist() == [13, 27]  # the lower-indexed twin leads
    assert got.dist_a[27, 1] == 0.0 and np.isfinite(got.g_a[27, 1]) and np.isfinite(got.g_a[13, 1])
    v = np.random.default_rng(6).uniform(0.5, 2.0, 28)
    s, ga, gb = l.gradient_from_coords(names_a, names_b, xyz, xyz, pair_weights=v)
    ga_model, gb_model = du.gradient_coords(want, xyz, xyz, v)
    bound = 28 * 28 * 2 * TOL_G + 1e-13
    assert np.isfinite(ga).all() and np.isfinite(gb).all()  # the zero-distance twins are skipped, not divided by
    assert np.max(np.abs(ga - ga_model)) <= bound and np.max(np.abs(gb - gb_model)) <= bound


def test_deterministic_mode_repeats_bit_for_bit():
    lh = _lh()
    xyz, ca, cb = _lattice()
    l = lh.LoCoHD(CATS3, lh.WeightFunction(*HYP), deterministic=True)
    names_a, names_b = [CATS3[c] for c in ca], [CATS3[c] for c in cb]
    first = l.sensitivity_from_coords(names_a, names_b, xyz, xyz)
    for _ in range(4):
        again = l.sensitivity_from_coords(names_a, names_b, xyz, xyz)
        for name, x, y in zip(first._fields, first, again):
            assert x.tobytes() == y.tobytes(), name
    plain = lh.LoCoHD(CATS3, lh.WeightFunction(*HYP)).sensitivity_from_coords(names_a, names_b, xyz, xyz)
    for name, x, y in zip(first._fields, first, plain):  # every element has one writer: the lists and g do not depend on the mode
        if name != "scores":
            assert x.tobytes() == y.tobytes(), name


@pytest.fixture(scope="module")
def two_structures():
    rng = np.random.default_rng(77)
    n = 40
    return (rng.uniform(0.0, 9.0, (n, 3)), rng.integers(0, 3, n)), (rng.uniform(0.0, 9.0, (n, 3)), rng.integers(0, 3, n))


def test_from_coords_against_from_dmxs(two_structures):
    lh = _lh()
    (xa, ca), (xb, cb) = two_structures
    l = lh.LoCoHD(CATS3, lh.WeightFunction(*UNI))
    names_a, names_b = [CATS3[c] for c in ca], [CATS3[c] for c in cb]
    ra, rb = du.coords_rows(xa), du.coords_rows(xb)
    by_coords = l.sensitivity_from_coords(names_a, names_b, xa, xb)
    by_rows = l.sensitivity_from_dmxs(names_a, names_b, ra, rb)
    for name in ("count_a", "count_b", "idx_a", "idx_b", "dist_a", "dist_b"):
        assert getattr(by_coords, name).tobytes() == getattr(by_rows, name).tobytes(), name
    assert np.array_equal(by_coords.idx_a[:, 0], np.arange(40))
    for name in ("g_a", "g_b", "scores"):
        assert np.max(np.abs(getattr(by_coords, name) - getattr(by_rows, name))) <= 1e-13, name
    _compare(by_coords, du.from_dmxs(ca, ra, cb, rb, 3, UNI), l.from_coords(names_a, names_b, xa, xb), "from_coords, n = 40")


def test_gradients_host_session_autograd_and_streams(two_structures):
    lh = _lh()
    from loco_hd_amd.autograd import locohd_scores_dense
    from loco_hd_amd.device import DeviceSession

    (xa, ca), (xb, cb) = two_structures
    n = len(xa)
    l = lh.LoCoHD(CATS3, lh.WeightFunction(*HYP))
    names_a, names_b = [CATS3[c] for c in ca], [CATS3[c] for c in cb]
    v = np.random.default_rng(8).uniform(0.5, 2.0, n)
    host = l.sensitivity_from_coords(names_a, names_b, xa, xb)
    s_host, ga_host, gb_host = l.gradient_from_coords(names_a, names_b, xa, xb, pair_weights=v)
    assert np.array_equal(s_host, host.scores)
    want = du.from_dmxs(ca, du.coords_rows(xa), cb, du.coords_rows(xb), 3, HYP)
    ga_model, gb_model = du.gradient_coords(want, xa, xb, v)
    # an atom's sum has at most 40 rows x 40 members terms v g (x_m - x_r) / d with |v| <= 2 and a unit direction: each within 2 TOL_G of
    # the model's, plus the float64 rounding of the dense product itself
    bound = n * n * 2 * TOL_G + 1e-13
    err = max(float(np.max(np.abs(ga_host - ga_model))), float(np.max(np.abs(gb_host - gb_model))))
    print(f"gradient_from_coords, n = {n}: max |grad - model| = {err:.3g} (bound {bound:.3g}), |sum grad| = {np.max(np.abs(ga_host.sum(0))):.3g}")
    assert err <= bound and np.any(ga_host != 0)
    assert np.max(np.abs(ga_host.sum(0))) <= 1e-12 and np.max(np.abs(gb_host.sum(0))) <= 1e-12  # translation invariance
    sess = DeviceSession(l)
    try:
        torch = sess.torch
        cl_a, cl_b = sess.upload(xa, ca.astype(np.int32)), sess.upload(xb, cb.astype(np.int32))
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):  # the coordinates are produced on the stream the session then runs on
            sess.use_current_stream()
            big = torch.randn(1024, 1024, device="cuda")
            for _ in range(3):
                big = big @ big * 1e-3
            ta = (torch.from_numpy(xa).cuda() + big[0, 0].double() * 0).contiguous()
            tb, tv = torch.from_numpy(xb).cuda(), torch.from_numpy(v).cuda()
            dev = sess.sensitivity_coords(cl_a, cl_b)
            for name in dev._fields:
                assert np.array_equal(getattr(dev, name).cpu().numpy(), getattr(host, name)), name
            s_dev, ga_dev, gb_dev = sess.gradient_coords(cl_a, cl_b, ta, tb, pair_weights=tv)
            assert np.array_equal(s_dev.cpu().numpy(), s_host)
            assert np.max(np.abs(ga_dev.cpu().numpy() - ga_host)) <= 1e-13 and np.max(np.abs(gb_dev.cpu().numpy() - gb_host)) <= 1e-13
            x = ta.clone().requires_grad_(True)
            scores = locohd_scores_dense(sess, cl_b, x, ca.astype(np.int32))
            assert np.array_equal(scores.detach().cpu().numpy(), s_host)
            (scores * tv).sum().backward()
            assert np.max(np.abs(x.grad.cpu().numpy() - ga_host)) <= 1e-13
            wide = sess.sensitivity_coords(cl_a, cl_b, width=n + 3)  # a wider row: padded with -1 / 0
            assert wide.idx_a.shape == (n, n + 3) and bool((wide.idx_a[:, n:] == -1).all()) and bool((wide.g_b[:, n:] == 0).all())
            assert np.array_equal(wide.g_a[:, :n].cpu().numpy(), host.g_a)
        torch.cuda.synchronize()
    finally:
        torch.cuda.current_stream().synchronize()
        sess.use_current_stream()
        sess.close()


def test_gradient_from_dmxs_is_the_scatter_of_g():
    lh = _lh()
    sa, ma, sb, mb = _case(91, 4, 30, 45, 3)
    l = lh.LoCoHD(CATS3, lh.WeightFunction(*HYP))
    names_a, names_b = [CATS3[c] for c in sa], [CATS3[c] for c in sb]
    v = np.asarray([0.5, 2.0, 1.0, 1.5])
    s, G_a, G_b = l.gradient_from_dmxs(names_a, names_b, ma, mb, pair_weights=v)
    want = du.from_dmxs(sa, ma, sb, mb, 3, HYP)
    W_a, W_b = du.gradient_dmx(want, 30, 45, v)
    assert G_a.shape == (4, 30) and G_b.shape == (4, 45)
    assert np.max(np.abs(G_a - W_a)) <= 2 * TOL_G and np.max(np.abs(G_b - W_b)) <= 2 * TOL_G  # |v| <= 2
    assert np.max(np.abs(s - l.from_dmxs(names_a, names_b, ma, mb))) <= TOL
    assert np.all(G_a[ma == 0.0] == 0.0) and np.all(G_b[mb == 0.0] == 0.0) and np.count_nonzero(G_a) > 60  # the slot-0 columns


def _raised(call):
    try:
        call()
    except Exception as exc:  # noqa: BLE001 -- the test compares whatever the two calls raise
        return type(exc), str(exc)
    return None, ""


def test_errors_with_a_device():
    lh = _lh()
    sa, ma, sb, mb = _case(55, 3, 20, 33, 3)
    l = lh.LoCoHD(CATS3, lh.WeightFunction(*UNI))
    names_a, names_b = [CATS3[c] for c in sa], [CATS3[c] for c in sb]
    with pytest.raises(ValueError, match="33"):
        l.sensitivity_from_dmxs(names_a, names_b, ma, mb, width=32)
    assert l.sensitivity_from_dmxs(names_a, names_b, ma, mb, width=40).g_a.shape == (3, 40)
    bad = ma.copy()
    bad[1, 7] = np.nan
    scoring = _raised(lambda: l.from_dmxs(names_a, names_b, bad, mb))
    assert scoring[0] is not None and _raised(lambda: l.sensitivity_from_dmxs(names_a, names_b, bad, mb)) == scoring
    strangers = list(names_a)
    strangers[5] = "not-a-category"
    attribution = _raised(lambda: l.attribution_from_dmxs(strangers, names_b, ma, mb))
    assert attribution[0] is not None and _raised(lambda: l.sensitivity_from_dmxs(strangers, names_b, ma, mb)) == attribution
    assert np.isfinite(l.sensitivity_from_dmxs(names_a, names_b, ma, mb).scores).all()  # the context is clean afterwards


def test_no_cross_talk_with_the_thresholded_call():
    """Both calls keep their lists in one grow-only block: a thresholded call must return the bytes it returned before a dense call."""
    lh = _lh()
    rng = np.random.default_rng(12)
    xyz, cat = rng.uniform(0.0, 14.0, (150, 3)), rng.integers(0, 3, 150)
    atoms = [lh.PrimitiveAtom(CATS3[c], "t", list(x)) for c, x in zip(cat, xyz)]
    pairs = [(int(i), int(j)) for i, j in rng.integers(0, 150, (12, 2))]
    l = lh.LoCoHD(CATS3, lh.WeightFunction(*UNI))
    before = l.sensitivity_from_primitives(atoms, atoms[::-1], pairs, 7.0)
    sa, ma, sb, mb = _case(13, 5, 300, 70, 3)
    l.sensitivity_from_dmxs([CATS3[c] for c in sa], [CATS3[c] for c in sb], ma, mb)
    after = l.sensitivity_from_primitives(atoms, atoms[::-1], pairs, 7.0)
    for name, x, y in zip(before._fields, before, after):
        assert x.tobytes() == y.tobytes(), name
