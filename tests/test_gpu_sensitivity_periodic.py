"""Neighbour sensitivities and gradients under periodic boundaries on the device against the numpy restatement
(tests/periodic_sensitivity_util.py: the image cloud by the header's contract with every slot's origin and code, tests/sensitivity_util.py
in longdouble on it; tests/test_periodic_sensitivity_model.py pins it to its own periodic score by difference quotients).

Expected values never come from the library.  count, idx and image must match the model exactly; scores, dist and disp within TOL = 1e-11
and g within TOL_G, the bounds of tests/test_gpu_sensitivity.py.  Difference quotients of from_primitives(box_a=...) are bounded by
periodic_sensitivity_util.FD_BOUND = 4 x 2.7e-11, four times what the model test measures at the same atoms and step.

On identical sides with several members at one distance g_a and g_b cancel over the group of tied members, not slot by slot: tied
members enter one at a time, side A first (periodic_sensitivity_util.tie_groups_cancel)."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import periodic_sensitivity_util as pu
from test_gpu_sensitivity import TOL_G

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
TOL = 1e-11
KL = ("Kullback-Leibler", [1e-3])
H2 = ("Hellinger", [2.0])


def _lh():
    import loco_hd_amd as lh

    return lh


def _lchd(sd=H2, weights=None, accept_same=True, cats=pu.CATS7):
    lh = _lh()
    return lh.LoCoHD(cats, lh.WeightFunction(*pu.UNI), lh.TagPairingRule({"accept_same": accept_same}),
                     category_weights=None if weights is None else list(weights), statistical_distance=lh.StatisticalDistance(*sd))


def _atoms(s, cats=pu.CATS7):
    lh = _lh()
    return [lh.PrimitiveAtom(cats[c], f"t{t}", list(x)) for x, c, t in zip(*s)]


def _kw(per_a, per_b):
    kw = {}
    for side, per in (("a", per_a), ("b", per_b)):
        if per is not None:
            kw[f"{per[0]}_{side}"] = np.asarray(per[1], dtype=np.float64)
    return kw


def _compare(got, want, what, scores_ref=None):
    for name in ("count_a", "count_b", "idx_a", "idx_b", "image_a", "image_b"):
        assert np.array_equal(np.asarray(getattr(got, name)), getattr(want, name)), f"{what}: {name}"
    err = {name: float(np.max(np.abs(np.asarray(getattr(got, name)) - getattr(want, name)), initial=0.0))
           for name in ("scores", "dist_a", "dist_b", "disp_a", "disp_b", "g_a", "g_b")}
    if scores_ref is not None:
        err["scores vs from_primitives"] = float(np.max(np.abs(np.asarray(got.scores) - np.asarray(scores_ref)), initial=0.0))
    print(f"{what}: " + ", ".join(f"{k} {v:.3g}" for k, v in err.items()))
    assert np.isfinite(np.asarray(got.g_a)).all() and np.isfinite(np.asarray(got.g_b)).all()
    for name, e in err.items():
        assert e <= (TOL_G if name in ("g_a", "g_b") else TOL), (what, name, e)


class Rig:
    """A session with the two structures of a case and what stands for each in a pass (the structure itself, or its image cloud)."""

    def __init__(self, lchd, a, per_a, b, per_b, reach=pu.THR):
        from loco_hd_amd.device import DeviceSession

        self.sess = DeviceSession(lchd, interner={})
        self.torch = self.sess.torch
        self.src = [self.sess.upload(*s) for s in (a, b)]
        self.per, self.n = [per_a, per_b], [len(a[0]), len(b[0])]
        self.cl = [self.images(cl, per, reach) for cl, per in zip(self.src, self.per)]

    def images(self, cl, per, reach):
        if per is None:
            return cl
        return self.sess.periodic_images(cl, per[1], reach) if per[0] == "box" else self.sess.periodic_images(cl, reach=reach, cell=per[1])

    def anchors(self, pairs):
        return self.torch.from_numpy(np.ascontiguousarray(pairs, dtype=np.int64).reshape(-1, 2)).cuda()

    def close(self):
        self.sess.close()


def _np(t):
    return type(t)(*[x.cpu().numpy() for x in t])


# ---- 1, 2: the origin map ------------------------------------------------------------------------------------------------------------
ONE = (np.zeros((1, 3)), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32))


def test_origin_map_of_the_smallest_clouds():
    box8 = ("box", (8.0, 8.0, 8.0))
    for s, per, reach, codes in ((ONE, box8, 8.0, list(range(27))), ((np.full((1, 3), 4.0), ONE[1], ONE[2]), box8, 3.0, [0]),
                                 (ONE, pu.PERIODS["skewed"], 4.0, [0, 1, 3, 4, 9, 10, 12, 13])):
        rig = Rig(_lchd(), s, per, s, per, reach)
        try:
            origin, code = rig.sess.image_origin(rig.cl[0])
            assert origin.dtype == np.int32 and code.dtype == np.int8
            assert origin.tolist() == [0] * len(codes) and code.tolist() == codes
            with pytest.raises(ValueError):
                rig.sess.image_origin(rig.src[0])  # not an image cloud
        finally:
            rig.close()


@pytest.mark.parametrize("kind", ["box", "skewed"])
def test_origin_map_around_the_scan_span(kind):
    from loco_hd_amd import _native as N

    span = int(N.lib().lchd_images_scan_span())
    per = pu.PERIODS[kind]
    reach = 10.0 if kind == "box" else 6.0
    for n in (span - 1, span, span + 1, 2 * span + 1):
        s = pu.side(900 + n, n, per)
        rig = Rig(_lchd(), s, per, s, per, reach)
        try:
            origin, code = rig.sess.image_origin(rig.cl[0])
            got = rig.sess.coords_of(rig.cl[0], len(origin))
            w = got[:n] if kind != "box" else pu.wrap_box(s[0], per[1])
            xyz, want_origin, want_code = pu.images(s[0], per, reach, wrapped=w)
            assert np.array_equal(origin, want_origin) and np.array_equal(code, want_code), (kind, n)
            assert len(origin) > n and np.array_equal(got, xyz)
            for o in range(len(origin)):  # the slot holds the image (origin, code) of the contract, bit for bit
                assert np.array_equal(got[o], pu.image_of(w, per, origin[o], code[o])), (kind, n, o)
            assert int(N.lib().lchd_cloud_home_size(rig.cl[0])) == n == int(N.lib().lchd_cloud_home_size(rig.src[0]))
        finally:
            rig.close()


# ---- 3: random clouds ----------------------------------------------------------------------------------------------------------------
WEIGHTS = np.random.default_rng(3).uniform(0.3, 3.0, 7)
RANDOM = [(case, sd, accept_same, weights) for case in sorted(pu.RANDOM_SIDES) for sd, accept_same, weights in
          ((H2, case != "box/open", None), (KL, True, WEIGHTS if case == "open/cell" else None))]


@pytest.mark.parametrize("case, sd, accept_same, weights", RANDOM, ids=[f"{c}-{s[0][:2]}-{a}-{'w' if w is not None else 'u'}" for c, s, a, w in RANDOM])
def test_random_clouds(case, sd, accept_same, weights):
    a, per_a, b, per_b, pairs = pu.random_case(case)
    l = _lchd(sd, weights, accept_same)
    got = l.sensitivity_from_primitives_periodic(_atoms(a), _atoms(b), pairs, pu.THR, **_kw(per_a, per_b))
    want = pu.from_primitives(a, per_a, b, per_b, pairs, pu.THR, 7, pu.UNI, sd, weights, accept_same)
    assert got.idx_a.shape[1] == max(want.count_a.max(), want.count_b.max())
    _compare(got, want, f"{case}, {sd[0]}", l.from_primitives(_atoms(a), _atoms(b), pairs, pu.THR, **_kw(per_a, per_b)))
    for per, image in ((per_a, got.image_a), (per_b, got.image_b)):
        assert bool(np.any(image != 0)) == (per is not None)


# ---- 4: an atom that enters through two images ----------------------------------------------------------------------------------------
def test_thin_box_atom_under_two_codes_contributes_twice():
    lh = _lh()
    a, per_a, b, per_b, pairs = pu.thin_case()
    l = _lchd()
    got = l.sensitivity_from_primitives_periodic(_atoms(a), _atoms(b), pairs, pu.THR, **_kw(per_a, per_b))
    want = pu.from_primitives(a, per_a, b, per_b, pairs, pu.THR, 7)
    _compare(got, want, "thin box")
    p, s, atom = pu.twice(want)[0]
    idx, image, g, dist = ((got.idx_a, got.image_a, got.g_a, got.dist_a), (got.idx_b, got.image_b, got.g_b, got.dist_b))[s]
    slots = np.flatnonzero(idx[p] == atom)
    assert len(slots) == 2 and image[p, slots[0]] != image[p, slots[1]]
    # the atom's gradient holds both terms: without the second slot's g it is short of exactly that slot's term
    full = lh.LoCoHD._assemble_gradient_periodic(got, len(a[0]), len(b[0]))[s]
    cut_g = g.copy()
    cut_g[p, slots[1]] = 0.0
    cut = lh.LoCoHD._assemble_gradient_periodic(got._replace(**{("g_a", "g_b")[s]: cut_g}), len(a[0]), len(b[0]))[s]
    disp = (got.disp_a, got.disp_b)[s]
    term = g[p, slots[1]] / dist[p, slots[1]] * disp[p, slots[1]]
    assert np.max(np.abs((full[atom] - cut[atom]) - term)) <= 1e-15
    _, ga, gb = l.gradient_from_primitives_periodic(_atoms(a), _atoms(b), pairs, pu.THR, **_kw(per_a, per_b))
    assert np.array_equal((ga, gb)[s], full)
    model = pu.gradient(want, len(a[0]), len(b[0]))[s]
    assert np.max(np.abs(full - model)) <= len(pairs) * idx.shape[1] * 2 * TOL_G + 1e-13


# ---- 5: ties ------------------------------------------------------------------------------------------------------------------------------
def test_lattice_that_fills_its_box_ties_in_home_source_code_order():
    a, per_a, b, per_b, pairs = pu.lattice_case()
    got = _lchd().sensitivity_from_primitives_periodic(_atoms(a), _atoms(b), pairs, pu.THR, **_kw(per_a, per_b))
    want = pu.from_primitives(a, per_a, b, per_b, pairs, pu.THR, 7)
    _compare(got, want, "lattice")
    assert pu.tie_order_ok(got) > 0
    assert np.all(got.scores == 0.0) and np.any(got.g_a != 0.0)
    assert np.array_equal(got.idx_a, got.idx_b) and np.array_equal(got.image_a, got.image_b) and np.array_equal(got.disp_a, got.disp_b)
    pu.tie_groups_cancel(got, TOL_G)


# ---- 6: unwrapped input -----------------------------------------------------------------------------------------------------------------
def test_unwrapped_input_gives_the_same_bits():
    rng = np.random.default_rng(23)
    n, box = 200, ("box", (32.0, 32.0, 32.0))
    sides = []
    for _ in range(2):
        xyz = rng.integers(0, 32 * 1024, (n, 3)) / 1024.0  # multiples of 2^-10 in a power-of-two box: wrapping is exact
        sides.append((xyz, rng.integers(0, 7, n).astype(np.int32), rng.integers(0, 3, n).astype(np.int32)))
    moved = [(s[0] + rng.integers(-2, 3, (n, 3)) * 32.0, s[1], s[2]) for s in sides]
    assert np.any(moved[0][0] != sides[0][0]) and np.array_equal(pu.wrap_box(moved[0][0], box[1]), sides[0][0])
    pairs = [(int(i), int(j)) for i, j in rng.integers(0, n, (20, 2))]
    l, kw = _lchd(), _kw(box, box)
    want = l.sensitivity_from_primitives_periodic(_atoms(sides[0]), _atoms(sides[1]), pairs, pu.THR, **kw)
    got = l.sensitivity_from_primitives_periodic(_atoms(moved[0]), _atoms(moved[1]), pairs, pu.THR, **kw)
    for name in got._fields:
        assert np.array_equal(getattr(got, name), getattr(want, name)), name
    assert np.any(got.image_a != 0)
    g0 = l.gradient_from_primitives_periodic(_atoms(sides[0]), _atoms(sides[1]), pairs, pu.THR, **kw)
    g1 = l.gradient_from_primitives_periodic(_atoms(moved[0]), _atoms(moved[1]), pairs, pu.THR, **kw)
    assert all(np.array_equal(x, y) for x, y in zip(g0, g1))


# ---- 7: no periodic side at all ---------------------------------------------------------------------------------------------------------
def test_open_sides_through_the_new_call():
    a, b = pu.side(41, 150, None), pu.side(42, 150, None)
    a, b = (a[0] * 0.5, a[1], a[2]), (b[0] * 0.5, b[1], b[2])
    pairs = [(int(i), int(j)) for i, j in np.random.default_rng(4).integers(0, 150, (20, 2))]
    l = _lchd()
    old = l.sensitivity_from_primitives(_atoms(a), _atoms(b), pairs, 8.0)
    new = l.sensitivity_from_primitives_periodic(_atoms(a), _atoms(b), pairs, 8.0)
    for name in old._fields:
        assert np.array_equal(getattr(new, name), getattr(old, name)), name
    for s, idx, image, disp in ((a, new.idx_a, new.image_a, new.disp_a), (b, new.idx_b, new.image_b, new.disp_b)):
        at = np.where(idx >= 0, idx, idx[:, :1])
        assert not image.any() and np.array_equal(disp, s[0][at] - s[0][at[:, :1]])
    _compare(new, pu.from_primitives(a, None, b, None, pairs, 8.0, 7), "open / open")


# ---- 8: gradients -----------------------------------------------------------------------------------------------------------------------
def test_gradient_against_the_model_and_difference_quotients():
    a, per_a, b, per_b, pairs = pu.random_case("box/box")
    l, kw = _lchd(), _kw(per_a, per_b)
    v = np.random.default_rng(8).uniform(0.5, 2.0, len(pairs))
    want = pu.from_primitives(a, per_a, b, per_b, pairs, pu.THR, 7)
    scores, ga, gb = l.gradient_from_primitives_periodic(_atoms(a), _atoms(b), pairs, pu.THR, pair_weights=v, **kw)
    ma, mb = pu.gradient(want, len(a[0]), len(b[0]), v)
    # an atom's sum has at most pairs x width terms v g disp / d with |v| <= 2 and a unit direction: each within 2 TOL_G of the model's,
    # plus the float64 rounding of the sum itself
    bound = len(pairs) * want.idx_a.shape[1] * 2 * TOL_G + 1e-13
    err = max(float(np.max(np.abs(ga - ma))), float(np.max(np.abs(gb - mb))))
    print(f"gradient: max |host - model| = {err:.3g} (bound {bound:.3g}), column sums {np.abs(ga.sum(0)).max():.3g} {np.abs(gb.sum(0)).max():.3g}")
    assert err <= bound and np.max(np.abs(scores - want.scores)) <= TOL
    assert np.max(np.abs(ga.sum(0))) <= 1e-12 and np.max(np.abs(gb.sum(0))) <= 1e-12 and np.any(ga != 0) and np.any(gb != 0)
    # central differences of the scoring call itself, at the atoms and step of the model test (unit pair weights, as measured there)
    picks, _ = pu.fd_atoms("box/box")
    _, ua, ub = l.gradient_from_primitives_periodic(_atoms(a), _atoms(b), pairs, pu.THR, **kw)

    def library_scores(sa, pa, sb, pb, prs, thr):
        return np.asarray(l.from_primitives(_atoms(sa), _atoms(sb), prs, thr, **_kw(pa, pb)))

    worst = 0.0
    for side, atom in picks:
        q = pu.central_difference(a, per_a, b, per_b, pairs, pu.THR, 7, side, atom, library_scores)
        worst = max(worst, float(np.max(np.abs(q - (ua, ub)[side][atom]))))
    print(f"gradient: max |host - central difference of from_primitives| = {worst:.3g} at {picks} (bound {pu.FD_BOUND:.3g})")
    assert worst <= pu.FD_BOUND


# ---- 9: the session -----------------------------------------------------------------------------------------------------------------------
def _close(got, want, what, tol=1e-13):
    for name in want._fields:
        x, y = np.asarray(getattr(got, name)), np.asarray(getattr(want, name))
        assert x.shape == y.shape and x.dtype == y.dtype, (what, name)
        if x.dtype.kind == "i":
            assert np.array_equal(x, y), (what, name)
        else:
            assert float(np.max(np.abs(x - y), initial=0.0)) <= tol, (what, name)


@pytest.mark.parametrize("case", ["box/open", "cell/cell"])
def test_session_calls_against_the_host_call(case):
    a, per_a, b, per_b, pairs = pu.random_case(case)
    l, kw = _lchd(), _kw(per_a, per_b)
    host = l.sensitivity_from_primitives_periodic(_atoms(a), _atoms(b), pairs, pu.THR, **kw)
    v = np.random.default_rng(9).uniform(0.5, 2.0, len(pairs))
    s_host, ga_host, gb_host = l.gradient_from_primitives_periodic(_atoms(a), _atoms(b), pairs, pu.THR, pair_weights=v, **kw)
    rig = Rig(l, a, per_a, b, per_b)
    try:
        torch, anc = rig.torch, rig.anchors(pairs)
        dev = rig.sess.sensitivity_images(rig.cl[0], rig.cl[1], anc, pu.THR)
        assert dev.image_a.dtype == torch.int8 and tuple(dev.disp_a.shape) == tuple(dev.idx_a.shape) + (3,)
        _close(_np(dev), host, case)
        s_dev, ga, gb = rig.sess.gradient_images(rig.cl[0], rig.cl[1], anc, pu.THR, pair_weights=torch.from_numpy(v).cuda())
        assert tuple(ga.shape) == (len(a[0]), 3) and tuple(gb.shape) == (len(b[0]), 3)
        assert np.max(np.abs(s_dev.cpu().numpy() - s_host)) <= 1e-13
        assert np.max(np.abs(ga.cpu().numpy() - ga_host)) <= 1e-13 and np.max(np.abs(gb.cpu().numpy() - gb_host)) <= 1e-13
        # out= of another width: the error names the width the pairs take
        k = int(dev.idx_a.shape[1])
        narrow = type(dev)(*[t[:, : k - 1].contiguous() if t.dim() >= 2 else t.clone() for t in dev])
        with pytest.raises(ValueError, match=f"row width {k - 1} is too small.*holds {k} points"):
            rig.sess.sensitivity_images(rig.cl[0], rig.cl[1], anc, pu.THR, out=narrow)
        again = rig.sess.sensitivity_images(rig.cl[0], rig.cl[1], anc, pu.THR, out=type(dev)(*[torch.zeros_like(t) for t in dev]))
        _close(_np(again), _np(dev), "out=", 0.0)
    finally:
        rig.close()


def test_updated_images_get_a_fresh_origin_map():
    a, per_a, b, per_b, pairs = pu.random_case("box/box")
    moved = a[0].copy()
    moved[0] = (31.5, 16.0, 16.0)
    a = (moved, a[1], a[2])
    across = moved.copy()
    across[0] = (32.5, 16.0, 16.0)  # over the +x face: wraps to 0.5, its -x images go, +x images come
    pairs = [(0, 0), (1, 0)] + pairs[:10] + [(int(i), 3) for i in np.flatnonzero(np.linalg.norm(pu.wrap_box(across, per_a[1]) - (0.5, 16.0, 16.0), axis=1) < 8.0)[:4]]
    l = _lchd()
    rig, fresh = Rig(l, a, per_a, b, per_b), Rig(l, (across, a[1], a[2]), per_a, b, per_b)
    try:
        anc = rig.anchors(pairs)
        before = _np(rig.sess.sensitivity_images(rig.cl[0], rig.cl[1], anc, pu.THR))  # (builds the origin map of the first coordinates)
        rig.sess.set_coords(rig.src[0], across)
        rig.sess.update_images(rig.cl[0], rig.src[0], per_a[1])
        after = _np(rig.sess.sensitivity_images(rig.cl[0], rig.cl[1], anc, pu.THR))
        want = _np(fresh.sess.sensitivity_images(fresh.cl[0], fresh.cl[1], fresh.anchors(pairs), pu.THR))
        _close(after, want, "after update_images", 0.0)
        assert not np.array_equal(before.image_a, after.image_a)
        o1, c1 = rig.sess.image_origin(rig.cl[0])
        o2, c2 = fresh.sess.image_origin(fresh.cl[0])
        assert np.array_equal(o1, o2) and np.array_equal(c1, c2)
        _compare(after, pu.from_primitives((across, a[1], a[2]), per_a, b, per_b, pairs, pu.THR, 7), "after update_images")
    finally:
        rig.close()
        fresh.close()


def test_ragged_batch_with_a_box_per_structure_names_global_atoms():
    from loco_hd_amd.device import DeviceSession

    boxes = [(32.0, 32.0, 32.0), (24.0, 28.0, 36.0), (40.0, 22.0, 30.0)]
    structs = [pu.side(60 + k, n, ("box", bx)) for k, (n, bx) in enumerate(zip((90, 140, 61), boxes))]
    ref = pu.side(77, 120, pu.PERIODS["box"])
    l = _lchd()
    sess = DeviceSession(l, interner={})
    try:
        torch = sess.torch
        batch, offs = sess.upload_batch(structs)
        images = sess.periodic_images(batch, np.asarray(boxes), pu.THR)
        cref = sess.upload(*ref)
        iref = sess.periodic_images(cref, pu.BOX32, pu.THR)
        rng = np.random.default_rng(6)
        local = [[(int(i), int(j)) for i, j in zip(rng.integers(0, len(s[0]), 8), rng.integers(0, 120, 8))] for s in structs]
        glob = np.asarray([(offs[k] + i, j) for k, prs in enumerate(local) for i, j in prs], dtype=np.int64)
        dev = _np(sess.sensitivity_images(images, iref, torch.from_numpy(glob).cuda(), pu.THR))
        origin, code = sess.image_origin(images)
        assert np.array_equal(origin[: offs[-1]], np.arange(offs[-1])) and origin.max() == offs[-1] - 1 and not code[: offs[-1]].any()
        width = dev.idx_a.shape[1]
        for k, (s, prs) in enumerate(zip(structs, local)):
            want = pu.from_primitives(s, ("box", boxes[k]), ref, pu.PERIODS["box"], prs, pu.THR, 7, width=width)
            rows = dev.__class__(*[np.asarray(t)[8 * k: 8 * k + 8] for t in dev])
            shifted = want._replace(idx_a=np.where(want.idx_a >= 0, want.idx_a + offs[k], -1).astype(np.int32))
            _compare(rows, shifted, f"batch structure {k}")
        _, ga, gb = sess.gradient_images(images, iref, torch.from_numpy(glob).cuda(), pu.THR)
        assert tuple(ga.shape) == (int(offs[-1]), 3) and tuple(gb.shape) == (120, 3)
    finally:
        sess.close()


# ---- 10: autograd ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["box/box", "cell/cell"])
def test_autograd_backward_is_side_a_of_the_host_gradient(case):
    from loco_hd_amd.autograd import locohd_scores_periodic

    a, per_a, b, per_b, pairs = pu.random_case(case)
    l, kw = _lchd(), _kw(per_a, per_b)
    v = np.random.default_rng(10).uniform(0.5, 2.0, len(pairs))
    s_host, ga_host, _ = l.gradient_from_primitives_periodic(_atoms(a), _atoms(b), pairs, pu.THR, pair_weights=v, **kw)
    rig = Rig(l, a, None, b, per_b)  # the movable side is uploaded by the function itself
    try:
        torch = rig.torch
        held = len(rig.sess._clouds)
        x = torch.from_numpy(a[0]).cuda().requires_grad_(True)
        scores = locohd_scores_periodic(rig.sess, rig.cl[1], x, a[1], a[2], rig.anchors(pairs), pu.THR, **{per_a[0]: per_a[1]})
        assert np.max(np.abs(scores.detach().cpu().numpy() - s_host)) <= 1e-13
        (scores * torch.from_numpy(v).cuda()).sum().backward()
        assert np.max(np.abs(x.grad.cpu().numpy() - ga_host)) <= 1e-13 and np.any(ga_host != 0)
        assert len(rig.sess._clouds) == held
    finally:
        rig.close()


# ---- 11: a C client ---------------------------------------------------------------------------------------------------------------------------
def test_c_client_of_the_periodic_sensitivity_entry_points(tmp_path):
    if shutil.which("gcc") is None:
        pytest.fail("gcc is needed to build the C client")
    exe = tmp_path / "cabi_sensitivity_periodic"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", str(ROOT / "include"),
                           str(ROOT / "tests" / "cabi_sensitivity_periodic.c"), "-o", str(exe), "-L", str(ROOT / "loco_hd_amd"), "-lloco_hd_hip",
                           "-lm", f"-Wl,-rpath,{ROOT / 'loco_hd_amd'}"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    assert "cabi sensitivity periodic ok" in out.stdout
