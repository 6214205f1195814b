"""The native gradient calls on the device, bit for bit against the model (tests/gradient_native_util.py).

The expected value is always built the same way: the contribution rule of include/loco_hd_hip.h ("native coordinate gradients") applied,
in numpy float64, to the outputs of the existing sensitivity call on the same inputs, then the Python-integer accumulator.  grad_a and
grad_b must equal it in every bit, and the scores must equal the sensitivity call's in every bit.

One case of the list cannot be built through the public calls: a pair that is unusable (NaN score) inside a call that succeeds.  Every
environment holds its anchor, non-finite coordinates are refused when a cloud is created, and the conditions that give a NaN row (a
weight-function index outside the dictionary, a type outside the category map) fail the sensitivity call itself.  The tests below take
what exists: an anchor alone in its environment (nothing contributes, the score is the sensitivity call's), a member at distance 0, and
a weight-function index outside the dictionary (the call fails as the sensitivity call does, that pair's score is NaN, and the next call
on the session is correct).

Accuracy (test_host_call_and_accuracy_on_forty_atoms, test_dense_host_call_and_accuracy): max |gradient - longdouble assembly of the
same lists| measured on an MI355X, native / host: 1.39e-17 / 2.78e-17 (40 atoms, 12 pairs), 2.78e-17 / 1.67e-16 (dense n = 24).
"""
import numpy as np
import pytest

import dense_sensitivity_util as dsu
import gradient_native_util as gn
import sensitivity_util as su

pytestmark = pytest.mark.gpu

CATS = [f"c{k}" for k in range(5)]
UNI = ("uniform", [3.0, 10.0])
MESSAGE = r"gradient contribution not finite or >= 2\^63 \(pair weights\?\)"


def _lh():
    import loco_hd_amd as lh

    return lh


def _locohd(wf=None):
    lh = _lh()
    return lh.LoCoHD(CATS, lh.WeightFunction(*UNI) if wf is None else wf)


class Session:
    """A DeviceSession that closes itself; `det`: deterministic mode."""

    def __init__(self, l, det=False):
        from loco_hd_amd.device import DeviceSession

        self.s = DeviceSession(l)
        self.s.set_deterministic(det)

    def __enter__(self):
        return self.s

    def __exit__(self, *exc):
        self.s.close()


def _cloud(seed, n, edge):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.0, edge, (n, 3)), rng.integers(0, len(CATS), n).astype(np.int32)


def _ball(seed, n_near, radius=6.0, n_far=6):
    """Atom 0 at the origin with exactly n_near neighbours inside `radius`, then n_far atoms far away, each alone within `radius`."""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n_near, 3))
    v *= (radius * rng.uniform(0.05, 0.999, n_near) ** (1 / 3) / np.linalg.norm(v, axis=1))[:, None]
    far = 100.0 + 50.0 * np.arange(1, n_far + 1)[:, None] * np.ones((1, 3))
    xyz = np.vstack([np.zeros((1, 3)), v, far])
    return xyz, rng.integers(0, len(CATS), len(xyz)).astype(np.int32)


def _np(sens):
    return type(sens)(*[t.cpu().numpy() for t in sens])


def _same_bits(got, want, what):
    assert np.array_equal(gn.bits(got), gn.bits(want)), f"{what}: max |difference| = {np.nanmax(np.abs(np.asarray(got) - np.asarray(want)))}"


def _check(sess, ca, cb, xa, xb, pairs, thr, weights=None, tiles=(0,), what=""):
    """native_gradient for every tile size against the model on the session's own sensitivity lists; returns (sens, model grads)."""
    torch = sess.torch
    anc = torch.tensor(np.asarray(pairs, dtype=np.int64).reshape(-1, 2), device="cuda")
    sens = _np(sess.sensitivity(ca, cb, anc, thr))
    want_a, want_b, flag = gn.gradient(sens, xa, xb, weights)
    assert flag == 0
    w = None if weights is None else torch.tensor(np.asarray(weights, dtype=np.float64), device="cuda")
    for tile in tiles:
        scores, ga, gb = sess.native_gradient(ca, cb, anc, thr, pair_weights=w, tile_pairs=tile)
        _same_bits(scores.cpu().numpy(), sens.scores, f"{what}: scores, tile_pairs {tile}")
        _same_bits(ga.cpu().numpy(), want_a, f"{what}: grad_a, tile_pairs {tile}")
        _same_bits(gb.cpu().numpy(), want_b, f"{what}: grad_b, tile_pairs {tile}")
    return sens, want_a, want_b


@pytest.fixture(scope="module")
def forty():
    (xa, ca), (xb, cb) = _cloud(71, 40, 9.0), _cloud(72, 40, 9.0)
    rng = np.random.default_rng(5)
    return xa, ca, xb, cb, rng.integers(0, 40, (12, 2)), rng.uniform(0.5, 2.0, 12)


@pytest.mark.parametrize("det", [False, True])
def test_forty_atoms_twelve_pairs_with_weights(forty, det):
    xa, ca, xb, cb, pairs, v = forty
    with Session(_locohd(), det) as sess:
        a, b = sess.upload(xa, ca), sess.upload(xb, cb)
        sens, want_a, want_b = _check(sess, a, b, xa, xb, pairs, 10.0, v, what=f"40 atoms, det={det}")
        assert np.any(want_a != 0.0) and np.any(want_b != 0.0)
        _check(sess, a, b, xa, xb, pairs, 10.0, None, what=f"40 atoms without weights, det={det}")


def test_host_call_and_accuracy_on_forty_atoms(forty):
    lh = _lh()
    xa, ca, xb, cb, pairs, v = forty
    l = _locohd()
    atoms = [[lh.PrimitiveAtom(CATS[c], "t", list(x)) for c, x in zip(cc, xx)] for cc, xx in ((ca, xa), (cb, xb))]
    plist = [tuple(map(int, p)) for p in pairs]
    sens = l.sensitivity_from_primitives(atoms[0], atoms[1], plist, 10.0)
    want_a, want_b, _ = gn.gradient(sens, xa, xb, v)
    for tile in (0, 5):
        scores, ga, gb = l.native_gradient_from_primitives(atoms[0], atoms[1], plist, 10.0, pair_weights=v, tile_pairs=tile)
        _same_bits(scores, sens.scores, "host call: scores")
        _same_bits(ga, want_a, "host call: grad_a")
        _same_bits(gb, want_b, "host call: grad_b")
    _, ha, hb = l.gradient_from_primitives(atoms[0], atoms[1], plist, 10.0, pair_weights=v)
    ref_a, ref_b = su.gradient(sens, xa, xb, v)  # the longdouble assembly of the same lists
    dev_native = max(np.max(np.abs(ga - ref_a)), np.max(np.abs(gb - ref_b)))
    dev_host = max(np.max(np.abs(ha - ref_a)), np.max(np.abs(hb - ref_b)))
    print(f"thresholded, 40 atoms: max |native - longdouble| = {dev_native:.3g}, max |gradient_from_primitives - longdouble| = {dev_host:.3g}")
    assert dev_native <= dev_host


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("members", [64, 65, 200])
def test_tile_invariance_long_environments_and_the_repeat_before_accumulate(members, det):
    """Environments of `members` points (the anchor included) on side A: 64 is one slot per lane, 65 and 200 are several, none of the
    row widths is a multiple of 64.  The long pair comes sixth: with members = 200 the first tiles of tile_pairs 1 and 5 run at the
    starting width of 128, and the tile that holds the long pair is repeated at the width it takes before anything of it is added.  A
    context starts a call at the width its last call ended with, so every tile size gets a session of its own."""
    (xa, ca), (xb, cb) = _ball(300 + members, members - 1), _ball(400, 30)
    fa = len(xa) - 1
    pairs = [(fa, 0), (fa - 1, 1), (fa - 2, 0), (fa - 3, 2), (fa, 3), (0, 0), (1, 1), (0, len(xb) - 1), (2, 0)]
    v = np.random.default_rng(members).uniform(0.5, 2.0, len(pairs))
    results = []
    for tile in (1, 5, 0):
        with Session(_locohd(), det) as sess:
            a, b = sess.upload(xa, ca), sess.upload(xb, cb)
            sens, want_a, want_b = _check(sess, a, b, xa, xb, pairs, 6.5, v, tiles=(tile,), what=f"{members} members, det={det}")
            assert sens.count_a[5] == members and sens.idx_a.shape[1] == members
            results.append((want_a, want_b))
    for want_a, want_b in results[1:]:
        _same_bits(want_a, results[0][0], "tile invariance of the lists")
        _same_bits(want_b, results[0][1], "tile invariance of the lists")


@pytest.mark.parametrize("det", [False, True])
def test_three_thousand_pairs_on_one_anchor(det):
    """Every pair has anchor 0 on side A, whose 25 members are hot atoms: 3 000 wave-reduced sums on one row of limbs, 3 000 adds on each
    member's."""
    (xa, ca), (xb, cb) = _ball(11, 25), _cloud(12, 60, 16.0)
    pairs = [(0, k % 60) for k in range(3000)]
    v = np.random.default_rng(3).uniform(-1.0, 1.0, 3000)
    with Session(_locohd(), det) as sess:
        a, b = sess.upload(xa, ca), sess.upload(xb, cb)
        _check(sess, a, b, xa, xb, pairs, 6.5, v, tiles=(0, 700), what=f"3000 pairs on one anchor, det={det}")


@pytest.mark.parametrize("det", [False, True])
def test_opposite_weights_cancel_to_plus_zero_and_extreme_weights(forty, det):
    xa, ca, xb, cb, pairs, v = forty
    with Session(_locohd(), det) as sess:
        torch = sess.torch
        a, b = sess.upload(xa, ca), sess.upload(xb, cb)
        twice = np.concatenate([pairs, pairs])
        anc = torch.tensor(twice, dtype=torch.int64, device="cuda")
        w = torch.tensor(np.concatenate([v, -v]), device="cuda")
        _, ga, gb = sess.native_gradient(a, b, anc, 10.0, pair_weights=w, tile_pairs=7)
        assert np.all(gn.bits(ga.cpu().numpy()) == 0) and np.all(gn.bits(gb.cpu().numpy()) == 0)  # +0.0 in every element
        big = np.where(np.arange(12) % 2 == 0, 2.0 ** 40, 2.0 ** -40)
        _check(sess, a, b, xa, xb, pairs, 10.0, big, tiles=(0, 5), what=f"weights 2^40 and 2^-40, det={det}")


@pytest.mark.parametrize("det", [False, True])
def test_coincident_member_and_anchor_alone(det):
    xa, ca = _ball(21, 20)
    xa[7] = xa[0]  # a member at distance 0 from anchor 0: a g but no direction
    xb, cb = _ball(22, 15)
    fa, fb = len(xa) - 1, len(xb) - 1
    pairs = [(0, 0), (fa, 0), (0, fb), (fa, fb), (7, 1)]
    with Session(_locohd(), det) as sess:
        a, b = sess.upload(xa, ca), sess.upload(xb, cb)
        sens, want_a, _ = _check(sess, a, b, xa, xb, pairs, 6.5, [1.0, 2.0, 3.0, 4.0, 5.0], tiles=(0, 2), what="distance 0, lone anchors")
        assert sens.dist_a[0, 1] == 0.0 and {int(sens.idx_a[0, 0]), int(sens.idx_a[0, 1])} == {0, 7}
        assert sens.count_a[3] == 1 and sens.count_b[3] == 1 and np.all(want_a[fa] == 0.0)


@pytest.mark.parametrize("det", [False, True])
def test_batch_cloud_with_global_indices(det):
    (x0, c0), (x1, c1), (xb, cb) = _cloud(31, 30, 8.0), _cloud(32, 37, 8.0), _cloud(33, 40, 8.0)
    with Session(_locohd(), det) as sess:
        batch, offs = sess.upload_batch([(x0, c0), (x1, c1)])
        b = sess.upload(xb, cb)
        rng = np.random.default_rng(9)
        pairs = [(int(offs[k % 2] + rng.integers(0, (30, 37)[k % 2])), int(rng.integers(0, 40))) for k in range(14)]
        xa = np.vstack([x0, x1])
        sens, want_a, _ = _check(sess, batch, b, xa, xb, pairs, 7.0, rng.uniform(0.5, 2.0, 14), tiles=(0, 3), what=f"batch, det={det}")
        assert sens.idx_a.max() >= 30 and np.any(want_a[30:] != 0.0)  # the second structure's atoms under their global indices


def test_out_of_range_weight_and_bad_key_leave_clean_accumulators(forty):
    lh = _lh()
    xa, ca, xb, cb, pairs, v = forty
    l = lh.LoCoHD(CATS, {"u": lh.WeightFunction(*UNI), "h": lh.WeightFunction("hyper_exp", [1.0, 0.5, 0.2, 0.05])})
    with Session(l) as sess:
        torch = sess.torch
        a, b = sess.upload(xa, ca), sess.upload(xb, cb)
        anc = torch.tensor(pairs, dtype=torch.int64, device="cuda")
        wf = torch.zeros(12, dtype=torch.int32, device="cuda")
        sens = _np(sess.sensitivity(a, b, anc, 10.0, wf_index=wf))
        want_a, want_b, _ = gn.gradient(sens, xa, xb, v)
        huge = v.copy()
        huge[4] = 2.0 ** 70
        assert gn.gradient(sens, xa, xb, huge)[2] == 1
        out = tuple(torch.zeros(s, dtype=torch.float64, device="cuda") for s in ((12,), (40, 3), (40, 3)))
        with pytest.raises(ValueError, match=MESSAGE):
            sess.native_gradient(a, b, anc, 10.0, pair_weights=torch.tensor(huge, device="cuda"), wf_index=wf, out=out)
        _same_bits(out[0].cpu().numpy(), sens.scores, "scores of the failed call")
        for tile in (0, 5):
            _, ga, gb = sess.native_gradient(a, b, anc, 10.0, pair_weights=torch.tensor(v, device="cuda"), wf_index=wf, tile_pairs=tile)
            _same_bits(ga.cpu().numpy(), want_a, "grad_a after an out-of-range call")
            _same_bits(gb.cpu().numpy(), want_b, "grad_b after an out-of-range call")
        bad = wf.clone()
        bad[9] = 2  # outside a dictionary of two: the second tile of five fails, behind a first tile that was added
        with pytest.raises(ValueError):
            sess.native_gradient(a, b, anc, 10.0, pair_weights=torch.tensor(v, device="cuda"), wf_index=bad, tile_pairs=5, out=out)
        assert torch.isnan(out[0][9])
        _, ga, gb = sess.native_gradient(a, b, anc, 10.0, pair_weights=torch.tensor(v, device="cuda"), wf_index=wf)
        _same_bits(ga.cpu().numpy(), want_a, "grad_a after an abandoned call")
        _same_bits(gb.cpu().numpy(), want_b, "grad_b after an abandoned call")
        with pytest.raises(ValueError, match="tile_pairs = -2 is negative"):
            sess.native_gradient(a, b, anc, 10.0, tile_pairs=-2)
        with pytest.raises(ValueError, match="pair_weights has 3 entries"):
            sess.native_gradient(a, b, anc, 10.0, pair_weights=torch.ones(3, device="cuda"))


# ---- dense rows ---------------------------------------------------------------------------------------------------------------------
def _dense_check(sess, xa, ca, xb, cb, weights=None, wf_index=None, what=""):
    torch = sess.torch
    a, b = sess.upload(xa, ca), sess.upload(xb, cb)
    wf = None if wf_index is None else torch.tensor(np.asarray(wf_index, dtype=np.int32), device="cuda")
    sens = _np(sess.sensitivity_coords(a, b, wf_index=wf))
    want_a, want_b, flag = gn.gradient(sens, xa, xb, weights, dense=True)
    assert flag == 0
    w = None if weights is None else torch.tensor(np.asarray(weights, dtype=np.float64), device="cuda")
    scores, ga, gb = sess.native_gradient_coords(a, b, pair_weights=w, wf_index=wf)
    _same_bits(scores.cpu().numpy(), sens.scores, f"{what}: scores")
    _same_bits(ga.cpu().numpy(), want_a, f"{what}: grad_a")
    _same_bits(gb.cpu().numpy(), want_b, f"{what}: grad_b")
    return sens, want_a, want_b


@pytest.mark.parametrize("n", [24, 65, 130])
def test_dense_rows(n):
    (xa, ca), (xb, cb) = _cloud(500 + n, n, 12.0), _cloud(600 + n, n, 12.0)
    v = np.random.default_rng(n).uniform(-1.0, 2.0, n)
    with Session(_locohd()) as sess:
        _dense_check(sess, xa, ca, xb, cb, None, what=f"dense n={n}")
        _, want_a, _ = _dense_check(sess, xa, ca, xb, cb, v, what=f"dense n={n}, weights")
        assert np.any(want_a != 0.0)


def test_dense_coincident_atoms_and_row_keys():
    lh = _lh()
    (xa, ca), (xb, cb) = _cloud(41, 24, 10.0), _cloud(42, 24, 10.0)
    xa[9] = xa[2]  # slot 0 of row 9 is atom 2: the anchor of the row is still atom 9
    l = lh.LoCoHD(CATS, {"u": lh.WeightFunction(*UNI), "h": lh.WeightFunction("hyper_exp", [1.0, 0.5, 0.2, 0.05])})
    with Session(l) as sess:
        sens, want_a, _ = _dense_check(sess, xa, ca, xb, cb, np.linspace(0.5, 2.0, 24), wf_index=[r % 2 for r in range(24)],
                                       what="dense, coincident atoms, per-row keys")
        assert sens.idx_a[9, 0] == 2 and sens.idx_a[9, 1] == 9
        assert sens.dist_a[9, 1] == 0.0 and np.any(want_a[9] != 0.0)


def test_dense_host_call_and_accuracy():
    (xa, ca), (xb, cb) = _cloud(51, 24, 10.0), _cloud(52, 24, 10.0)
    seq_a, seq_b = [CATS[c] for c in ca], [CATS[c] for c in cb]
    v = np.random.default_rng(8).uniform(0.5, 2.0, 24)
    l = _locohd()
    sens = l.sensitivity_from_coords(seq_a, seq_b, xa, xb)
    want_a, want_b, _ = gn.gradient(sens, xa, xb, v, dense=True)
    scores, ga, gb = l.native_gradient_from_coords(seq_a, seq_b, xa, xb, pair_weights=v)
    _same_bits(scores, sens.scores, "dense host call: scores")
    _same_bits(ga, want_a, "dense host call: grad_a")
    _same_bits(gb, want_b, "dense host call: grad_b")
    _, ha, hb = l.gradient_from_coords(seq_a, seq_b, xa, xb, pair_weights=v)
    ref_a, ref_b = dsu.gradient_coords(sens, xa, xb, v)  # the longdouble assembly of the same lists
    dev_native = max(np.max(np.abs(ga - ref_a)), np.max(np.abs(gb - ref_b)))
    dev_host = max(np.max(np.abs(ha - ref_a)), np.max(np.abs(hb - ref_b)))
    print(f"dense, n = 24: max |native - longdouble| = {dev_native:.3g}, max |gradient_from_coords - longdouble| = {dev_host:.3g}")
    assert dev_native <= dev_host


# ---- autograd -----------------------------------------------------------------------------------------------------------------------
def test_autograd_native_backward_is_the_native_call(forty):
    from loco_hd_amd.autograd import locohd_scores, locohd_scores_dense

    xa, ca, xb, cb, pairs, v = forty
    with Session(_locohd()) as sess:
        torch = sess.torch
        a, b = sess.upload(xa, ca), sess.upload(xb, cb)
        anc = torch.tensor(pairs, dtype=torch.int64, device="cuda")
        w = torch.tensor(v, device="cuda")
        s_nat, ga_nat, _ = sess.native_gradient(a, b, anc, 10.0, pair_weights=w)
        x = torch.tensor(xa, device="cuda", requires_grad=True)
        scores = locohd_scores(sess, b, x, ca, None, anc, 10.0, native=True)
        _same_bits(scores.detach().cpu().numpy(), s_nat.cpu().numpy(), "autograd native: scores")
        (scores * w).sum().backward()
        _same_bits(x.grad.cpu().numpy(), ga_nat.cpu().numpy(), "autograd native: backward")
        # the default path is today's: the torch assembly of the sensitivity lists
        sens = sess.sensitivity(a, b, anc, 10.0)
        x0 = torch.tensor(xa, device="cuda", requires_grad=True)
        s0 = locohd_scores(sess, b, x0, ca, None, anc, 10.0)
        (s0 * w).sum().backward()
        today = sess.side_gradient(sens.scores, sens.idx_a, sens.dist_a, sens.g_a, torch.tensor(xa, device="cuda"), w)
        _same_bits(s0.detach().cpu().numpy(), sens.scores.cpu().numpy(), "autograd default: scores")
        assert np.max(np.abs(x0.grad.cpu().numpy() - today.cpu().numpy())) <= 1e-13  # (index_add_: torch's order, not a bit pattern)

        (xd, cd), (xe, ce) = _cloud(61, 24, 10.0), _cloud(62, 24, 10.0)
        d, e = sess.upload(xd, cd), sess.upload(xe, ce)
        wd = torch.tensor(np.linspace(0.5, 2.0, 24), device="cuda")
        s_nat, gd_nat, _ = sess.native_gradient_coords(d, e, pair_weights=wd)
        x = torch.tensor(xd, device="cuda", requires_grad=True)
        scores = locohd_scores_dense(sess, e, x, cd, native=True)
        _same_bits(scores.detach().cpu().numpy(), s_nat.cpu().numpy(), "autograd dense native: scores")
        (scores * wd).sum().backward()
        _same_bits(x.grad.cpu().numpy(), gd_nat.cpu().numpy(), "autograd dense native: backward")
        sens = sess.sensitivity_coords(d, e)
        x0 = torch.tensor(xd, device="cuda", requires_grad=True)
        (locohd_scores_dense(sess, e, x0, cd) * wd).sum().backward()
        today = sess.dense_side_gradient(sens.idx_a, sens.dist_a, sens.g_a, torch.tensor(xd, device="cuda"), wd)
        _same_bits(x0.grad.cpu().numpy(), today.cpu().numpy(), "autograd dense default: backward")
