"""The native periodic gradient calls and the strain derivative on the device, bit for bit against the model (tests/strain_native_util.py).

The expected value is built as in tests/test_gpu_gradient_native.py: the contribution rule of include/loco_hd_hip.h ("under periodic
boundaries, and the strain derivative") applied in numpy float64 to the outputs of the periodic sensitivity call of the same arguments,
then the Python-integer accumulator.  grad_a, grad_b, strain_a and strain_b must equal it in every bit (uint64 views), the scores must
equal the sensitivity call's.

Shapes.  Thresholded: environments of 1, 2, 64, 65 and 129 points (the anchor alone, one member, one slot per lane, one over, two
strides and one: the last is wider than the 128 slots a call starts with, so its tile is repeated before it is added), pair counts 1, 2,
3 and half the strain grid's wavefronts plus one (every wavefront of a side loops twice, the first a third time).  Dense: the six side
mixes of tests/test_gpu_min_image_sensitivity.py at n = 1, 2, 63, 64, 65, 130.
"""
import numpy as np
import pytest

import gradient_native_util as gn
import periodic_sensitivity_util as psu
import strain_native_util as sn
from test_gpu_min_image_sensitivity import MIXES, PERIODS, kw, names, structure

pytestmark = pytest.mark.gpu

CATS = [f"c{k}" for k in range(4)]
UNI = ("uniform", [3.0, 10.0])
MESSAGE = r"gradient contribution not finite or >= 2\^63 \(pair weights\?\)"
BIG = np.asarray([40.0, 44.0, 48.0])


def _lh():
    import loco_hd_amd as lh

    return lh


def _locohd(cats=CATS):
    lh = _lh()
    return lh.LoCoHD(cats, lh.WeightFunction(*UNI))


class Session:
    def __init__(self, l, det=False):
        from loco_hd_amd.device import DeviceSession

        self.s = DeviceSession(l)
        self.s.set_deterministic(det)

    def __enter__(self):
        return self.s

    def __exit__(self, *exc):
        self.s.close()


def _np(t):
    return type(t)(*[x.cpu().numpy() for x in t])


def _same_bits(got, want, what):
    got, want = np.asarray(got.cpu().numpy() if hasattr(got, "cpu") else got), np.asarray(want)
    assert got.shape == want.shape, what
    assert np.array_equal(gn.bits(got), gn.bits(want)), f"{what}: max |difference| = {np.nanmax(np.abs(got - want))}"


def _ball(seed, n_near, radius=6.0):
    """Atom 0 at the origin -- a corner of the box, so its neighbours arrive through images -- with exactly n_near neighbours inside
    `radius`, and atom n_near + 1 in the middle of BIG, alone within the threshold."""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n_near, 3))
    v *= (radius * rng.uniform(0.05, 0.999, n_near) ** (1 / 3) / np.linalg.norm(v, axis=1))[:, None]
    xyz = np.vstack([np.zeros((1, 3)), v, BIG[None, :] / 2])
    return xyz, rng.integers(0, len(CATS), len(xyz)).astype(np.int32)


def _periodic(sess, cloud, per, thr):
    if per is None:
        return cloud
    return sess.periodic_images(cloud, per[1], thr) if per[0] == "box" else sess.periodic_images(cloud, None, thr, cell=per[1])


def _check_images(sess, a, b, n_a, n_b, pairs, thr, weights=None, tiles=(0,), what=""):
    """native_gradient_images, with and without strain, for every tile size against the model on the session's own lists."""
    torch = sess.torch
    anc = torch.tensor(np.asarray(pairs, dtype=np.int64).reshape(-1, 2), device="cuda")
    sens = _np(sess.sensitivity_images(a, b, anc, thr))
    want = sn.result(sens, n_a, n_b, weights)
    assert want[4] == 0
    w = None if weights is None else torch.tensor(np.asarray(weights, dtype=np.float64), device="cuda")
    for tile in tiles:
        got = sess.native_gradient_images(a, b, anc, thr, pair_weights=w, tile_pairs=tile, strain=True)
        assert type(got).__name__ == "NativeGradient"
        _same_bits(got.scores, sens.scores, f"{what}: scores, tile_pairs {tile}")
        for name, exp in zip(("grad_a", "grad_b", "strain_a", "strain_b"), want):
            _same_bits(getattr(got, name), exp, f"{what}: {name}, tile_pairs {tile}")
        plain = sess.native_gradient_images(a, b, anc, thr, pair_weights=w, tile_pairs=tile)
        assert len(plain) == 3
        for x, y, name in zip(plain, got, ("scores", "grad_a", "grad_b")):
            _same_bits(x, y.cpu().numpy(), f"{what}: {name} without strain, tile_pairs {tile}")
    return sens, want


# ---- thresholded ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 2, 64, 65, 129])
def test_environment_lengths_in_a_box(count):
    (xa, ca), (xb, cb) = _ball(900 + count, count - 1), _ball(950, 9)
    la, lb = len(xa) - 1, len(xb) - 1
    pairs = [(0, 0), (la, 0), (0, lb), (la, lb), (min(1, la), 1)]
    v = np.random.default_rng(count).uniform(0.5, 2.0, len(pairs))
    per = ("box", BIG)
    with Session(_locohd()) as sess:
        a, b = _periodic(sess, sess.upload(xa, ca), per, 6.5), _periodic(sess, sess.upload(xb, cb), per, 6.5)
        sens, want = _check_images(sess, a, b, len(xa), len(xb), pairs, 6.5, v, tiles=(0, 2), what=f"{count} points")
        assert sens.count_a[0] == count and sens.count_a[1] == 1 and sens.count_b[2] == 1
        if count >= 64:
            assert np.any(sens.image_a[0] != 0) and np.any(want[2] != 0.0)  # members through images; a strain on side A


@pytest.mark.parametrize("n_pairs", [1, 2, 3, "grid"])
def test_pair_counts_up_to_more_than_the_strain_grid(n_pairs):
    from loco_hd_amd import _native as N

    if n_pairs == "grid":
        n_pairs = int(N.lib().lchd_gradient_strain_waves()) // 2 * 2 + 1  # per side: every wavefront twice, the first three times
    (xa, ca), (xb, cb) = _ball(31, 5), _ball(32, 4)
    rng = np.random.default_rng(n_pairs)
    pairs = np.stack([rng.integers(0, len(xa), n_pairs), rng.integers(0, len(xb), n_pairs)], axis=1)
    v = rng.uniform(-1.0, 2.0, n_pairs)
    per = ("box", BIG)
    with Session(_locohd()) as sess:
        a, b = _periodic(sess, sess.upload(xa, ca), per, 6.5), _periodic(sess, sess.upload(xb, cb), per, 6.5)
        _, want = _check_images(sess, a, b, len(xa), len(xb), pairs, 6.5, v, tiles=(0,), what=f"{n_pairs} pairs")
        assert n_pairs < 1000 or (np.any(want[2] != 0.0) and np.any(want[3] != 0.0))


SIDES = {"box/box": ("box", "box"), "cell/cell": ("skewed", "dodecahedron"), "image/plain": ("box", "open")}


@pytest.fixture(scope="module")
def sixty():
    out = {}
    for name, (ka, kb) in SIDES.items():
        pa, pb = psu.PERIODS[ka], psu.PERIODS[kb]
        rng = np.random.default_rng(17)
        out[name] = (psu.side(701, 60, pa), pa, psu.side(702, 60, pb), pb, rng.integers(0, 60, (14, 2)), rng.uniform(0.5, 2.0, 14))
    return out


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("name", sorted(SIDES))
def test_sides_tiles_modes_and_runs(sixty, name, det):
    """Box both sides, cell both sides, an image cloud against a plain cloud: identical bits of all four outputs for tile_pairs 1, 7, the
    whole list and 0, in default and deterministic mode (each against the same model of the session's lists), and on a second run."""
    a, pa, b, pb, pairs, v = sixty[name]
    with Session(_locohd(psu.CATS7), det) as sess:
        ca, cb = _periodic(sess, sess.upload(a[0], a[1], a[2]), pa, psu.THR), _periodic(sess, sess.upload(b[0], b[1], b[2]), pb, psu.THR)
        sens, want = _check_images(sess, ca, cb, 60, 60, pairs, psu.THR, v, tiles=(1, 7, len(pairs), 0), what=f"{name}, det={det}")
        _check_images(sess, ca, cb, 60, 60, pairs, psu.THR, v, tiles=(0,), what=f"{name}, det={det}, second run")
        assert np.any(want[2] != 0.0) and np.any(want[3] != 0.0)
        assert np.any(sens.image_a != 0)
        for w in want[2:4]:
            assert np.array_equal(gn.bits(w), gn.bits(w.T))


def test_host_call_box_against_open(sixty):
    lh = _lh()
    a, pa, b, pb, pairs, v = sixty["image/plain"]
    l = _locohd(psu.CATS7)
    atoms = [[lh.PrimitiveAtom(psu.CATS7[c], f"t{t}", list(x)) for x, c, t in zip(*s)] for s in (a, b)]
    plist = [tuple(map(int, p)) for p in pairs]
    sens = l.sensitivity_from_primitives_periodic(atoms[0], atoms[1], plist, psu.THR, box_a=pa[1])
    want = sn.result(sens, 60, 60, v)
    for tile in (0, 5):
        got = l.native_gradient_from_primitives_periodic(atoms[0], atoms[1], plist, psu.THR, pair_weights=v, tile_pairs=tile, box_a=pa[1],
                                                         strain=True)
        _same_bits(got.scores, sens.scores, "host call: scores")
        for name, exp in zip(("grad_a", "grad_b", "strain_a", "strain_b"), want):
            _same_bits(getattr(got, name), exp, f"host call: {name}, tile_pairs {tile}")
        assert got.strain_a.shape == (3, 3) and got.strain_a.dtype == np.float64
    three = l.native_gradient_from_primitives_periodic(atoms[0], atoms[1], plist, psu.THR, pair_weights=v, box_a=pa[1])
    assert isinstance(three, tuple) and len(three) == 3
    for x, y in zip(three, got):
        _same_bits(x, y, "host call without strain")
    # against the host assembly of the same lists: a sum in another order, not a bit pattern
    _, ha, hb = l.gradient_from_primitives_periodic(atoms[0], atoms[1], plist, psu.THR, pair_weights=v, box_a=pa[1])
    assert max(np.max(np.abs(ha - got.grad_a)), np.max(np.abs(hb - got.grad_b))) <= 1e-13
    # ... and W against the long double sum of the same lists: a float64 term carries three roundings, the exact sum one more
    wa, wb = sn.strain_longdouble(sens, v)
    for got_w, ref, side in ((got.strain_a, wa, "a"), (got.strain_b, wb, "b")):
        idx, dist, g = (getattr(sens, f"{f}_{side}") for f in ("idx", "dist", "g"))
        use = (idx >= 0) & (dist > 0.0) & np.isfinite(g)
        use[:, 0] = False
        scale = float(np.sum(np.abs(v[:, None] * g * dist)[use]))  # sum |coef| |disp|^2
        assert np.max(np.abs(got_w - ref.astype(np.float64))) <= 4 * np.finfo(float).eps * scale


# ---- dense ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 130])
@pytest.mark.parametrize("mix", MIXES, ids=lambda m: f"{m[0]}/{m[1]}")
def test_dense_side_mixes_and_row_lengths(mix, n):
    per_a, per_b = PERIODS[mix[0]], PERIODS[mix[1]]
    ca, xa = structure(100 + n, n, per_a)
    cb, xb = structure(200 + n, n, per_b)
    v = np.random.default_rng(n).uniform(-1.0, 2.0, n)
    l = _locohd()
    with Session(l) as sess:
        torch = sess.torch
        a, b = sess.upload(xa, l._cats(names(ca))), sess.upload(xb, l._cats(names(cb)))
        sens = _np(sess.sensitivity_coords_periodic(a, b, **kw(per_a, per_b)))
        want = sn.result(sens, n, n, v, dense=True)
        assert want[4] == 0
        got = sess.native_gradient_coords_periodic(a, b, pair_weights=torch.tensor(v, device="cuda"), strain=True, **kw(per_a, per_b))
        _same_bits(got.scores, sens.scores, f"dense {mix}, n = {n}: scores")
        for name, exp in zip(("grad_a", "grad_b", "strain_a", "strain_b"), want):
            _same_bits(getattr(got, name), exp, f"dense {mix}, n = {n}: {name}")
        plain = sess.native_gradient_coords_periodic(a, b, pair_weights=torch.tensor(v, device="cuda"), **kw(per_a, per_b))
        for x, y in zip(plain, got):
            _same_bits(x, y.cpu().numpy(), f"dense {mix}, n = {n}: without strain")
        assert n < 3 or (np.any(want[0] != 0.0) and np.any(want[2] != 0.0))


def test_open_dense_pair_is_the_open_native_call():
    n = 65
    ca, xa = structure(11, n, None)
    cb, xb = structure(12, n, None)
    v = np.random.default_rng(2).uniform(0.5, 2.0, n)
    l = _locohd()
    sens = l.sensitivity_from_coords_periodic(names(ca), names(cb), xa, xb)
    for x, idx, dist, disp in ((xa, sens.idx_a, sens.dist_a, sens.disp_a), (xb, sens.idx_b, sens.dist_b, sens.disp_b)):
        assert np.all(idx >= 0)
        diff = x[idx] - x[:, None, :]
        # disp == x[m] - x[r]: in every bit on every slot the rule uses (dist > 0); a row's own atom, at distance 0, has the displacement
        # -0.0 from the sensitivity kernel where numpy's x - x is +0.0 -- equal values, and no term is built from that slot
        assert np.array_equal(disp, diff)
        used = dist > 0.0
        assert used.sum() == n * (n - 1)
        assert np.array_equal(gn.bits(disp[used]), gn.bits(diff[used]))
    open_call = l.native_gradient_from_coords(names(ca), names(cb), xa, xb, pair_weights=v)
    three = l.native_gradient_from_coords_periodic(names(ca), names(cb), xa, xb, pair_weights=v)
    five = l.native_gradient_from_coords_periodic(names(ca), names(cb), xa, xb, pair_weights=v, strain=True)
    for x, y, z, name in zip(open_call, three, five, ("scores", "grad_a", "grad_b")):
        _same_bits(y, x, f"open consistency: {name}")
        _same_bits(z, x, f"open consistency with strain: {name}")
    want = sn.result(sens, n, n, v, dense=True)
    _same_bits(five.strain_a, want[2], "open strain_a")
    _same_bits(five.strain_b, want[3], "open strain_b")


# ---- failure paths ----------------------------------------------------------------------------------------------------------------------
def test_out_of_range_weight_fails_behind_valid_scores_and_leaves_clean_accumulators(sixty):
    a, pa, b, pb, pairs, v = sixty["box/box"]
    with Session(_locohd(psu.CATS7)) as sess:
        torch = sess.torch
        ca, cb = _periodic(sess, sess.upload(a[0], a[1], a[2]), pa, psu.THR), _periodic(sess, sess.upload(b[0], b[1], b[2]), pb, psu.THR)
        anc = torch.tensor(pairs, dtype=torch.int64, device="cuda")
        sens = _np(sess.sensitivity_images(ca, cb, anc, psu.THR))
        huge = v.copy()
        huge[4] = 2.0 ** 70
        assert sn.result(sens, 60, 60, huge)[4] == 1
        out = tuple(torch.zeros(s, dtype=torch.float64, device="cuda") for s in ((14,), (60, 3), (60, 3), (3, 3), (3, 3)))
        with pytest.raises(ValueError, match=MESSAGE):
            sess.native_gradient_images(ca, cb, anc, psu.THR, pair_weights=torch.tensor(huge, device="cuda"), strain=True, out=out)
        _same_bits(out[0], sens.scores, "scores of the failed call")
        _check_images(sess, ca, cb, 60, 60, pairs, psu.THR, v, tiles=(0, 5), what="after an out-of-range call")
        with pytest.raises(ValueError, match="tile_pairs = -2 is negative"):
            sess.native_gradient_images(ca, cb, anc, psu.THR, tile_pairs=-2)
        with pytest.raises(ValueError, match="pair_weights has 3 entries"):
            sess.native_gradient_images(ca, cb, anc, psu.THR, pair_weights=torch.ones(3, device="cuda"))
        with pytest.raises(ValueError, match="out holds 3 tensors"):
            sess.native_gradient_images(ca, cb, anc, psu.THR, strain=True, out=out[:3])
        with pytest.raises(ValueError, match="box_a and cell_a were both given"):
            sess.native_gradient_coords_periodic(ca, cb, box_a=[30.0, 30.0, 30.0], cell_a=np.eye(3) * 30.0)


def test_strain_on_a_batch_is_unsupported_and_gradients_still_work():
    rng = np.random.default_rng(5)
    parts = [(rng.uniform(0.0, 9.0, (n, 3)), rng.integers(0, 4, n).astype(np.int32)) for n in (30, 37)]
    xb, cb = rng.uniform(0.0, 9.0, (40, 3)), rng.integers(0, 4, 40).astype(np.int32)
    with Session(_locohd()) as sess:
        torch = sess.torch
        batch, offs = sess.upload_batch(parts)
        b = sess.upload(xb, cb)
        pairs = [(int(offs[k % 2] + rng.integers(0, (30, 37)[k % 2])), int(rng.integers(0, 40))) for k in range(10)]
        anc = torch.tensor(pairs, dtype=torch.int64, device="cuda")
        with pytest.raises(NotImplementedError, match="a strain derivative belongs to one box or cell"):
            sess.native_gradient_images(batch, b, anc, 7.0, strain=True)
        sens = _np(sess.sensitivity_images(batch, b, anc, 7.0))
        want = sn.result(sens, 67, 40)
        scores, ga, gb = sess.native_gradient_images(batch, b, anc, 7.0)
        _same_bits(scores, sens.scores, "batch: scores")
        _same_bits(ga, want[0], "batch: grad_a")
        _same_bits(gb, want[1], "batch: grad_b")


# ---- autograd ---------------------------------------------------------------------------------------------------------------------------
def test_autograd_native_backward(sixty):
    from loco_hd_amd.autograd import locohd_scores_dense_periodic, locohd_scores_periodic

    a, pa, b, pb, pairs, v = sixty["box/box"]
    with Session(_locohd(psu.CATS7)) as sess:
        torch = sess.torch
        cb = _periodic(sess, sess.upload(b[0], b[1], b[2]), pb, psu.THR)
        anc = torch.tensor(pairs, dtype=torch.int64, device="cuda")
        w = torch.tensor(v, device="cuda")
        grads = []
        for native in (True, True, False):
            x = torch.tensor(a[0], device="cuda", requires_grad=True)
            scores = locohd_scores_periodic(sess, cb, x, a[1], a[2], anc, psu.THR, box=pa[1], native=native)
            (scores * w).sum().backward()
            grads.append((scores.detach().cpu().numpy(), x.grad.cpu().numpy()))
        _same_bits(grads[1][0], grads[0][0], "two native forward passes")
        _same_bits(grads[1][1], grads[0][1], "two native backward passes")
        _same_bits(grads[2][0], grads[0][0], "native and default scores")
        assert np.any(grads[0][1] != 0.0)
        assert np.max(np.abs(grads[2][1] - grads[0][1])) <= 1e-13  # (the bound of the open form's test: index_add_ has torch's order)

    n = 24
    per_a, per_b = PERIODS["box"], PERIODS["skewed"]
    ca, xa = structure(61, n, per_a)
    cc, xc = structure(62, n, per_b)
    l = _locohd()
    with Session(l) as sess:
        torch = sess.torch
        ref = sess.upload(xc, l._cats(names(cc)))
        w = torch.tensor(np.linspace(0.5, 2.0, n), device="cuda")
        grads = []
        for native in (True, True, False):
            x = torch.tensor(xa, device="cuda", requires_grad=True)
            scores = locohd_scores_dense_periodic(sess, ref, x, l._cats(names(ca)), box=per_a[1], ref_cell=per_b[1], native=native)
            (scores * w).sum().backward()
            grads.append((scores.detach().cpu().numpy(), x.grad.cpu().numpy()))
        _same_bits(grads[1][1], grads[0][1], "two dense native backward passes")
        _same_bits(grads[2][0], grads[0][0], "dense native and default scores")
        assert np.any(grads[0][1] != 0.0)
        assert np.max(np.abs(grads[2][1] - grads[0][1])) <= 1e-13
