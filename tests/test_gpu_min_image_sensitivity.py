"""Dense minimum-image sensitivities and gradients on the device (LoCoHD.sensitivity_from_coords_periodic / gradient_from_coords_periodic,
DeviceSession.sensitivity_coords_periodic / gradient_coords_periodic, autograd.locohd_scores_dense_periodic; k_sens_min_image_disp of
loco_hd_amd/csrc/lchd_sensitivity.hip behind k_rows_indexed and k_sensitivity) against the numpy model of
tests/min_image_sensitivity_util.py (tests/test_min_image_sensitivity_model.py pins it to its own score by central differences).

Expected values never come from the library.  idx and count must match the model exactly, dist and disp bit for bit, dist must be
norm3(disp) bit for bit; scores must match from_coords(..., box / cell) within 1e-11; g is bounded by the TOL_G of
tests/test_gpu_sensitivity.py (the sweep kernel is the same).  A gradient sums at most 2 n n terms g disp / d with |disp / d| <= 1, so
it is within n n 2 TOL_G + 1e-13 of the model's for row weights of at most 1."""
import numpy as np
import pytest

import min_image_sensitivity_util as mu
from min_image_util import norm3
from periodic_cell_util import CELLS
from periodic_sensitivity_util import H_STEP
from test_gpu_sensitivity import DISTANCES, TOL, TOL_G

pytestmark = pytest.mark.gpu

UNI = ("uniform", [3.0, 10.0])
HYP = ("hyper_exp", [1.0, 0.5, 0.2, 0.05])
CATS = [f"c{k}" for k in range(4)]
SCALE = 0.55  # the cells shrunk so that a structure of ~100 atoms fills the weight functions' supports
BOX = np.asarray([12.0, 10.5, 13.25])
BOX2 = np.asarray([9.75, 14.0, 11.5])
SKEWED = CELLS["skewed"] * SCALE
DODECA = CELLS["dodecahedron"] * SCALE
UNREDUCED = np.asarray([SKEWED[0] + 2.0 * SKEWED[1], SKEWED[1] - SKEWED[2], SKEWED[2]])
PERIODS = {"open": None, "box": ("box", BOX), "box2": ("box", BOX2), "skewed": ("cell", SKEWED), "dodecahedron": ("cell", DODECA),
           "unreduced": ("cell", UNREDUCED)}
MIXES = [("box", "box2"), ("box", "open"), ("open", "skewed"), ("skewed", "dodecahedron"), ("dodecahedron", "dodecahedron"),
         ("unreduced", "box")]


def reduce(cell):
    from loco_hd_amd.api import cell_reduce

    return cell_reduce(cell)


def _lh():
    import loco_hd_amd as lh

    return lh


def kw(per_a, per_b):
    out = {}
    for side, per in (("a", per_a), ("b", per_b)):
        if per is not None:
            out[f"{per[0]}_{side}"] = per[1]
    return out


def cell_of(per):
    return np.diag(BOX) if per is None else (np.diag(per[1]) if per[0] == "box" else np.asarray(per[1]))


def structure(seed, n, per, n_cat=4, spread=(-1.0, 2.0)):
    """(cat, xyz): n atoms spread over three cells a side, unwrapped (an open side: inside a box-sized cube)."""
    rng = np.random.default_rng(seed)
    u = rng.uniform(0.0, 1.0, (n, 3)) if per is None else rng.uniform(spread[0], spread[1], (n, 3))
    return rng.integers(0, n_cat, n), u @ cell_of(per)


def build(wf=UNI, sd=DISTANCES["h2"], weights=None, cats=CATS, **more):
    lh = _lh()
    w = {k: lh.WeightFunction(*v) for k, v in wf.items()} if isinstance(wf, dict) else lh.WeightFunction(*wf)
    return lh.LoCoHD(cats, w, category_weights=None if weights is None else list(weights), statistical_distance=lh.StatisticalDistance(*sd),
                     **more)


def names(cat, cats=CATS):
    return [cats[c] for c in cat]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def compare(got, want, scores_ref, what):
    for name in ("count_a", "count_b", "idx_a", "idx_b"):
        assert np.array_equal(getattr(got, name), getattr(want, name)), f"{what}: {name}"
    for name in ("dist_a", "dist_b", "disp_a", "disp_b"):
        assert np.array_equal(bits(getattr(got, name)), bits(getattr(want, name))), f"{what}: {name}"
    assert np.array_equal(bits(norm3(got.disp_a)), bits(got.dist_a)) and np.array_equal(bits(norm3(got.disp_b)), bits(got.dist_b)), what
    err_s = float(np.max(np.abs(got.scores - np.asarray(scores_ref))))
    err_m = float(np.max(np.abs(got.scores - want.scores)))
    err_g = max(float(np.max(np.abs(got.g_a - want.g_a))), float(np.max(np.abs(got.g_b - want.g_b))))
    print(f"{what}: max |g - model| = {err_g:.3g}, |scores - from_coords| = {err_s:.3g}, |scores - model| = {err_m:.3g}")
    assert err_s <= TOL and err_m <= TOL, what
    assert err_g <= TOL_G, what


def on_session(lchd, ca, xa, cb, xb, fn):
    from loco_hd_amd.device import DeviceSession

    sess = DeviceSession(lchd)
    try:
        a, b = sess.upload(xa, lchd._cats(names(ca))), sess.upload(xb, lchd._cats(names(cb)))
        return fn(sess, a, b)
    finally:
        sess.close()


def to_numpy(t):
    return type(t)(*[x.cpu().numpy() for x in t])


MODELS = {}


def shared_model(n, mix, wf=UNI):
    """One model (width n) per (n, side mix), shared by the tests that need it."""
    key = (n, mix, str(wf))
    if key not in MODELS:
        per_a, per_b = PERIODS[mix[0]], PERIODS[mix[1]]
        ca, xa = structure(100 + n, n, per_a)
        cb, xb = structure(200 + n, n, per_b)
        MODELS[key] = (ca, xa, cb, xb, per_a, per_b, mu.sensitivity(ca, xa, per_a, cb, xb, per_b, 4, wf, reduce=reduce))
    return MODELS[key]


def widen(ms, width):
    """The model's rows padded to `width` slots: idx -1, everything else 0."""
    n, k = ms.idx_a.shape
    pad = lambda a, fill: np.concatenate([a, np.full((n, width - k) + a.shape[2:], fill, dtype=a.dtype)], axis=1)  # noqa: E731
    return mu.MSens(ms.scores, ms.count_a, pad(ms.idx_a, -1), pad(ms.dist_a, 0.0), pad(ms.g_a, 0.0), pad(ms.disp_a, 0.0), ms.count_b,
                    pad(ms.idx_b, -1), pad(ms.dist_b, 0.0), pad(ms.g_b, 0.0), pad(ms.disp_b, 0.0))


# n: one quad, rows ending inside a lane's quad (width n + 3 and odd n), one block and more than one wavefront of quads
@pytest.mark.parametrize("extra", [0, 3], ids=["width-n", "width-n+3"])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 64, 65, 130])
def test_row_lengths_widths_and_both_paths(n, extra):
    ca, xa, cb, xb, per_a, per_b, want = shared_model(n, ("box", "skewed"))
    want = widen(want, n + extra)
    lchd = build()
    ref = lchd.from_coords(names(ca), names(cb), xa, xb, **kw(per_a, per_b))
    host = lchd.sensitivity_from_coords_periodic(names(ca), names(cb), xa, xb, width=n + extra if extra else None, **kw(per_a, per_b))
    assert host.disp_a.shape == (n, n + extra, 3)
    compare(host, want, ref, f"host, n = {n}, width n + {extra}")
    dev = on_session(lchd, ca, xa, cb, xb, lambda s, a, b: to_numpy(s.sensitivity_coords_periodic(a, b, width=n + extra, **kw(per_a, per_b))))
    compare(dev, want, ref, f"session, n = {n}, width n + {extra}")
    for x, y in zip(host, dev):
        assert np.array_equal(x, y, equal_nan=True)


@pytest.mark.parametrize("mix", MIXES, ids=lambda m: f"{m[0]}/{m[1]}")
def test_side_mixes(mix):
    n = 65
    ca, xa, cb, xb, per_a, per_b, want = shared_model(n, mix, HYP)
    lchd = build(HYP)
    ref = lchd.from_coords(names(ca), names(cb), xa, xb, **kw(per_a, per_b))
    compare(lchd.sensitivity_from_coords_periodic(names(ca), names(cb), xa, xb, **kw(per_a, per_b)), want, ref, f"host, {mix}")
    dev = on_session(lchd, ca, xa, cb, xb, lambda s, a, b: to_numpy(s.sensitivity_coords_periodic(a, b, **kw(per_a, per_b))))
    compare(dev, want, ref, f"session, {mix}")


def test_open_open_is_the_open_call_plus_disp():
    n = 65
    ca, xa = structure(1, n, None)
    cb, xb = structure(2, n, None)
    lchd = build()
    plain = lchd.sensitivity_from_coords(names(ca), names(cb), xa, xb)
    got = lchd.sensitivity_from_coords_periodic(names(ca), names(cb), xa, xb)
    for name in plain._fields:
        assert np.array_equal(getattr(plain, name), getattr(got, name)), name
    for x, idx, disp in ((xa, got.idx_a, got.disp_a), (xb, got.idx_b, got.disp_b)):
        assert np.array_equal(disp, x[idx] - x[:, None, :])
    compare(got, mu.sensitivity(ca, xa, None, cb, xb, None, 4, UNI), lchd.from_coords(names(ca), names(cb), xa, xb), "open/open")


def test_whole_lattice_vectors_change_nothing():
    """Coordinates on a grid of 1/64 in a box whose edges are odd multiples of 1/64 (no two atoms exactly half an edge apart): a shift
    by whole edges is exact, and so is every step of the prescribed arithmetic but the quotient d / L, which rint maps to the same
    integer -- the outputs are identical."""
    n = 64
    rng = np.random.default_rng(5)
    box = np.asarray([16.0, 12.0, 20.0]) + 1.0 / 64.0
    ca, cb = rng.integers(0, 4, n), rng.integers(0, 4, n)
    xa, xb = rng.integers(0, 768, (n, 3)) / 64.0, rng.integers(0, 768, (n, 3)) / 64.0
    lchd = build()
    base = lchd.sensitivity_from_coords_periodic(names(ca), names(cb), xa, xb, box_a=box, cell_b=np.diag(box))
    sa, sb = rng.integers(-3, 4, (n, 3)) * box, rng.integers(-3, 4, (n, 3)) * box
    moved = lchd.sensitivity_from_coords_periodic(names(ca), names(cb), xa + sa, xb + sb, box_a=box, cell_b=np.diag(box))
    for name, x, y in zip(base._fields, base, moved):
        assert np.array_equal(bits(x) if x.dtype == np.float64 else x, bits(y) if y.dtype == np.float64 else y), name
    assert np.abs(base.disp_a).max() <= box.max() / 2


@pytest.mark.parametrize("geo", ["box", "dodecahedron"])
def test_tie_rule(geo):
    """Two atoms exactly half a cell apart along one axis / lattice vector (two images at the same distance) and an atom a whole
    lattice vector from the row atom (distance 0 beyond slot 0): disp follows the prescribed arithmetic bit for bit."""
    n = 33
    per = ("box", np.asarray([16.0, 12.0, 20.0])) if geo == "box" else ("cell", np.asarray(CELLS["dodecahedron"]) * 0.5)
    cell = cell_of(per)
    ca, xa = structure(31, n, per)
    cb, xb = structure(32, n, per)
    xa[0] = [1.5, 2.25, 3.0]
    xa[1] = xa[0] + 0.5 * cell[0]
    xa[2] = xa[0] + cell[1]
    xb[n - 1] = [0.5, 0.75, 1.0]
    xb[n - 2] = xb[n - 1] - 0.5 * cell[2]
    xb[n - 3] = xb[n - 1] + cell[0] - cell[2]
    want = mu.sensitivity(ca, xa, per, cb, xb, per, 4, UNI, reduce=reduce)
    if geo == "box":  # (every number is a dyadic fraction: the lattice vector cancels exactly)
        assert (want.dist_a[0, 1:] == 0.0).any() and (want.dist_b[n - 1, 1:] == 0.0).any()
    lchd = build()
    ref = lchd.from_coords(names(ca), names(cb), xa, xb, **kw(per, per))
    compare(lchd.sensitivity_from_coords_periodic(names(ca), names(cb), xa, xb, **kw(per, per)), want, ref, f"ties, {geo}, host")
    dev = on_session(lchd, ca, xa, cb, xb, lambda s, a, b: to_numpy(s.sensitivity_coords_periodic(a, b, **kw(per, per))))
    compare(dev, want, ref, f"ties, {geo}, session")
    if geo == "box":
        half = np.flatnonzero(want.idx_a[0] == 1)[0]
        assert np.array_equal(dev.disp_a[0, half], [8.0, 0.0, 0.0])  # rint(-0.5) = -0: no wrap


@pytest.mark.parametrize("dist", sorted(DISTANCES))
def test_every_statistical_distance(dist):
    n = 33
    per_a, per_b = PERIODS["dodecahedron"], PERIODS["box"]
    ca, xa = structure(41, n, per_a)
    cb, xb = structure(42, n, per_b)
    lchd = build(sd=DISTANCES[dist])
    want = mu.sensitivity(ca, xa, per_a, cb, xb, per_b, 4, UNI, DISTANCES[dist], reduce=reduce)
    compare(lchd.sensitivity_from_coords_periodic(names(ca), names(cb), xa, xb, **kw(per_a, per_b)), want,
            lchd.from_coords(names(ca), names(cb), xa, xb, **kw(per_a, per_b)), dist)


def test_category_weights_and_a_dictionary_with_row_keys():
    n = 33
    per_a, per_b = PERIODS["skewed"], PERIODS["box"]
    ca, xa = structure(51, n, per_a)
    cb, xb = structure(52, n, per_b)
    weights = np.random.default_rng(3).uniform(0.3, 3.0, 4)
    wfs = {"u": UNI, "h": HYP}
    keys = [("h", "u")[r % 2] for r in range(n)]
    lchd = build(wfs, DISTANCES["h3.5"], weights)
    want = mu.sensitivity(ca, xa, per_a, cb, xb, per_b, 4, [wfs[k] for k in keys], DISTANCES["h3.5"], weights, reduce=reduce)
    compare(lchd.sensitivity_from_coords_periodic(names(ca), names(cb), xa, xb, keys, **kw(per_a, per_b)), want,
            lchd.from_coords(names(ca), names(cb), xa, xb, keys, **kw(per_a, per_b)), "category weights, two weight functions by key")


def test_deterministic_mode_repeats_bit_for_bit():
    ca, xa, cb, xb, per_a, per_b, want = shared_model(65, ("skewed", "dodecahedron"), HYP)
    lchd = build(HYP, deterministic=True)
    first = lchd.sensitivity_from_coords_periodic(names(ca), names(cb), xa, xb, **kw(per_a, per_b))
    second = lchd.sensitivity_from_coords_periodic(names(ca), names(cb), xa, xb, **kw(per_a, per_b))
    for name, x, y in zip(first._fields, first, second):
        assert np.array_equal(bits(x) if x.dtype == np.float64 else x, bits(y) if y.dtype == np.float64 else y), name
    compare(first, want, lchd.from_coords(names(ca), names(cb), xa, xb, **kw(per_a, per_b)), "deterministic")


@pytest.mark.parametrize("mix", mu.GRAD_MIXES, ids=lambda m: f"{m[0]}/{m[1]}")
def test_gradients_host_session_autograd_model_and_differences(mix):
    import torch

    from loco_hd_amd.autograd import locohd_scores_dense_periodic

    ca, xa, per_a, cb, xb, per_b, v, picks = mu.gradient_case(mix, reduce)  # (shared with the model test that measures FD_MEASURED)
    n = len(xa)
    assert mu.GRAD_WF == HYP
    want = mu.gradient(mu.sensitivity(ca, xa, per_a, cb, xb, per_b, 4, HYP, reduce=reduce), v)
    bound = n * n * 2 * TOL_G + 1e-13
    lchd = build(HYP)
    scores, ga, gb = lchd.gradient_from_coords_periodic(names(ca), names(cb), xa, xb, pair_weights=v, **kw(per_a, per_b))
    ref = np.asarray(lchd.from_coords(names(ca), names(cb), xa, xb, **kw(per_a, per_b)))
    assert np.max(np.abs(scores - ref)) <= TOL

    def session(s, a, b):
        dev = torch.device("cuda", s.device)
        sc, da, db = s.gradient_coords_periodic(a, b, pair_weights=torch.as_tensor(v, device=dev), **kw(per_a, per_b))
        x = torch.tensor(xa, dtype=torch.float64, device=dev, requires_grad=True)
        ka = {per_a[0]: per_a[1]}
        kb = {} if per_b is None else {f"ref_{per_b[0]}": per_b[1]}
        out = locohd_scores_dense_periodic(s, b, x, lchd._cats(names(ca)), **ka, **kb)
        (out * torch.as_tensor(v, device=dev)).sum().backward()
        return sc.cpu().numpy(), da.cpu().numpy(), db.cpu().numpy(), out.detach().cpu().numpy(), x.grad.cpu().numpy()

    sc, da, db, auto_scores, auto_grad = on_session(lchd, ca, xa, cb, xb, session)
    for what, got, side in (("host A", ga, 0), ("host B", gb, 1), ("session A", da, 0), ("session B", db, 1), ("autograd A", auto_grad, 0)):
        err = float(np.max(np.abs(got - want[side])))
        print(f"{mix} {what}: max |gradient - model| = {err:.3g} (bound {bound:.3g})")
        assert err <= bound, what
    assert np.array_equal(sc, scores) and np.array_equal(auto_scores, scores)

    # central differences of the scoring call itself, at atoms where the score is smooth over the step
    fn = lambda a, b: lchd.from_coords(names(ca), names(cb), a, b, **kw(per_a, per_b))  # noqa: E731
    assert len(picks) == 3
    for side, atom in picks:
        fd = mu.central_difference(xa, xb, side, atom, fn, v, H_STEP)
        err = float(np.max(np.abs(fd - (ga, gb)[side][atom])))
        print(f"{mix} side {side} atom {atom}: |central difference - gradient| = {err:.3g} (FD_BOUND {mu.FD_BOUND:.3g})")
        assert err <= mu.FD_BOUND

    # a rigid translation of side A changes nothing, so the gradient of side A sums to 0
    moved = np.asarray(lchd.from_coords(names(ca), names(cb), xa + np.asarray([0.125, -0.25, 0.0625]), xb, **kw(per_a, per_b)))
    _, ga1, _ = lchd.gradient_from_coords_periodic(names(ca), names(cb), xa, xb, **kw(per_a, per_b))
    print(f"{mix} translation: |scores moved - scores| = {np.max(np.abs(moved - ref)):.3g}, |sum grad_a| = {np.max(np.abs(ga1.sum(axis=0))):.3g}")
    assert np.max(np.abs(moved - ref)) <= mu.FD_BOUND and np.max(np.abs(ga1.sum(axis=0))) <= mu.FD_BOUND


def test_errors_with_a_device():
    from loco_hd_amd.device import DeviceSession

    n = 20
    ca, xa = structure(71, n, PERIODS["box"], spread=(0.0, 1.0))
    lchd = build()
    with pytest.raises(ValueError, match=f"holds {n} points"):
        lchd.sensitivity_from_coords_periodic(names(ca), names(ca), xa, xa, width=n - 1, box_a=BOX)
    nan = np.array(xa)
    nan[3, 1] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        lchd.sensitivity_from_coords_periodic(names(ca), names(ca), xa, nan, box_a=BOX, box_b=BOX)
    sess = DeviceSession(lchd)
    try:
        cat = lchd._cats(names(ca))
        a = sess.upload(xa, cat)
        with pytest.raises(ValueError, match=f"holds {n} points"):
            sess.sensitivity_coords_periodic(a, a, width=n - 1, box_a=BOX)
        images = sess.periodic_images(a, BOX, 5.0)
        with pytest.raises((ValueError, NotImplementedError), match="image cloud"):
            sess.sensitivity_coords_periodic(images, images, box_a=BOX)
        batch, _ = sess.upload_batch([(xa, cat), (xa, cat)])
        with pytest.raises(ValueError, match="batches"):
            sess.sensitivity_coords_periodic(batch, batch, box_a=BOX)
        with pytest.raises(ValueError, match="both given"):
            sess.sensitivity_coords_periodic(a, a, box_a=BOX, cell_a=np.diag(BOX))
        # the context is usable after every refusal
        got = to_numpy(sess.sensitivity_coords_periodic(a, a, box_a=BOX, box_b=BOX))
        assert np.all(got.scores == 0.0) and np.array_equal(bits(norm3(got.disp_a)), bits(got.dist_a))
    finally:
        sess.close()


def test_a_thresholded_call_before_and_after_is_unaffected():
    lh = _lh()
    n = 65
    ca, xa, cb, xb, per_a, per_b, _ = shared_model(n, ("box", "skewed"))
    lchd = build(deterministic=True)
    pa = [lh.PrimitiveAtom(CATS[c], "", x) for c, x in zip(ca, xa)]
    pb = [lh.PrimitiveAtom(CATS[c], "", x) for c, x in zip(cb, xb)]
    pairs = [(i, i) for i in range(n)]
    before = lchd.sensitivity_from_primitives(pa, pb, pairs, 8.0)
    lchd.sensitivity_from_coords_periodic(names(ca), names(cb), xa, xb, **kw(per_a, per_b))
    after = lchd.sensitivity_from_primitives(pa, pb, pairs, 8.0)
    for name, x, y in zip(before._fields, before, after):
        assert np.array_equal(x, y, equal_nan=True), name
