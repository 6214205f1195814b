"""Periodic boundaries on the device: image clouds (loco_hd_amd/csrc/lchd_images.hip) in front of the unchanged from_primitives pass.

Reference value.  The CPU oracle knows no boxes and needs none: for wrapped coordinates w the test builds the replicated system in
NumPy -- the originals first, then the 26 copies w + (i Lx, j Ly, k Lz), each shift one f64 addition per axis, with the same
categories and tags -- and gives it to oracle.from_arrays with the same anchors and threshold.  Every image coordinate is the same
single addition on both sides, so distances agree bit for bit, membership at the threshold cannot differ, and the bound is the
project's own TIGHT = 1e-11 (tests/test_gpu_parity.py).  Where the session exposes environment sizes (last_env_points) they are
compared with the oracle's exactly.

One case of the issue is asserted differently from its text: "one atom at the origin, reach = L: 7 ghosts".  By the emission rule
the same issue prescribes (w - L exists iff w >= L - reach, which is w >= 0 at reach = L) and by its lattice case ("every atom has
26 images", the atom at the origin included) that atom has 26 ghosts at reach = L; it has 7 for any reach below L.  Both are tested.
"""
import itertools
import shutil
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
TIGHT = 1e-11
L32 = (32.0, 32.0, 32.0)
CATS = ["A", "B", "C", "D", "E"]
# image order of the device: code cx + 3 cy + 9 cz ascending (x fastest), per-axis choice 0 original, 1 +L, 2 -L
CHOICE_SHIFT = (0.0, 1.0, -1.0)
SHIFTS = [(CHOICE_SHIFT[cx], CHOICE_SHIFT[cy], CHOICE_SHIFT[cz]) for cz in range(3) for cy in range(3) for cx in range(3)][1:]

WFS = {"hyper_exp": [1.0, 0.2, 2.0, 0.05], "dagum": [2.0, 1.5, 6.0], "uniform": [3.0, 10.0], "kumaraswamy": [2.0, 14.0, 2.0, 3.0]}
SDS = {"H2": ("Hellinger", [2.0]), "KS": ("Kolmogorov-Smirnov", [])}


@pytest.fixture(scope="module")
def lh():
    import loco_hd_amd

    return loco_hd_amd


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


@pytest.fixture(scope="module")
def scan_span():
    """Atoms one workgroup of the image kernels covers (kImgScanSpan of lchd_images.hip): up to it the scan of the ghost counts is
    one workgroup, beyond it block scans plus a scan of the block sums."""
    from loco_hd_amd import _native as N

    return int(N.lib().lchd_images_scan_span())


# ------------------------------------------------------------------------------------------------------------------------
# the contract in NumPy
# ------------------------------------------------------------------------------------------------------------------------
def wrap(x, box):
    box = np.asarray(box, dtype=np.float64)
    w = x - np.floor(x / box) * box
    return np.where(w == box, 0.0, w)


def replicate(w, box):
    """Originals first, then the 26 shifted copies; each shift is one addition per axis."""
    box = np.asarray(box, dtype=np.float64)
    return np.concatenate([w] + [w + np.asarray(s) * box for s in SHIFTS])


def image_cloud(w, box, reach):
    """What the device must hold: the wrapped originals, then per atom its ghosts in ascending image code."""
    box = np.asarray(box, dtype=np.float64) * np.ones((len(w), 3))
    plus, minus = w < reach, w >= box - reach
    ghosts = []
    for i in range(len(w)):
        ok = [(True, plus[i, k], minus[i, k]) for k in range(3)]
        for cz, cy, cx in itertools.product(range(3), repeat=3):
            if (cx or cy or cz) and ok[0][cx] and ok[1][cy] and ok[2][cz]:
                ghosts.append([(w[i, k], w[i, k] + box[i, k], w[i, k] - box[i, k])[c] for k, c in enumerate((cx, cy, cz))])
    return np.concatenate([w, np.asarray(ghosts, dtype=np.float64).reshape(-1, 3)])


def make(mod, wf="uniform", sd="H2", cats=CATS, accept_same=True, **kw):
    name, prm = SDS[sd]
    return mod.LoCoHD(cats, mod.WeightFunction(wf, WFS[wf]), mod.TagPairingRule({"accept_same": accept_same}),
                      statistical_distance=mod.StatisticalDistance(name, prm), **kw)


def want_periodic(o, xa, ca, ta, box_a, xb, cb, tb, box_b, pairs, thr):
    """(scores, environment sizes) of the replicated systems; a box of None leaves that side open."""
    def side(x, c, t, box):
        if box is None:
            return x, c, t
        return replicate(wrap(x, box), box), np.tile(c, 27), np.tile(t, 27)
    ra, rb = side(xa, ca, ta, box_a), side(xb, cb, tb, box_b)
    return o.from_arrays(*ra, *rb, pairs, thr, return_env_sizes=True, interner={})


def cloud(rng, n, box=L32, n_cat=len(CATS), n_tag=5):
    return (rng.uniform(0.0, 1.0, (n, 3)) * np.asarray(box), rng.integers(0, n_cat, n).astype(np.int32),
            rng.integers(0, n_tag, n).astype(np.int32))


class Rig:
    """A session with two uploaded structures and the image clouds of both."""

    def __init__(self, lh, torch, lchd, a, b, box_a, box_b, reach):
        from loco_hd_amd.device import DeviceSession

        self.torch, self.sess = torch, DeviceSession(lchd, interner={})
        self.a, self.b = self.sess.upload(*a), self.sess.upload(*b)
        self.ia = self.sess.periodic_images(self.a, box_a, reach)
        self.ib = self.sess.periodic_images(self.b, box_b, reach)

    def score(self, pairs, thr, a=None, b=None):
        anchors = self.torch.from_numpy(np.ascontiguousarray(pairs, dtype=np.int64)).cuda()
        return self.sess.from_primitives(self.ia if a is None else a, self.ib if b is None else b, anchors, thr).cpu().numpy()

    def size(self, cl):
        from loco_hd_amd import _native as N

        return int(N.lib().lchd_cloud_size(cl))

    def close(self):
        self.sess.close()


def check(got, want, what):
    err = float(np.max(np.abs(got - want))) if len(want) else 0.0
    print(f"{what}: max |hip - oracle| = {err:.3e} over {len(want)} pairs")
    assert np.all(np.isfinite(got)), what
    assert err <= TIGHT, (what, err)


# ------------------------------------------------------------------------------------------------------------------------
# the smallest cases
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reach, ghosts", [(8.0, 26), (np.nextafter(8.0, 0.0), 7), (4.0, 7)])
def test_one_atom_at_the_origin(lh, torch, reach, ghosts):
    """reach = L: w - L exists iff w >= L - reach = 0, so the atom has all 26 images (see the module docstring); below L only
    the seven + images.  One atom, one category: the score is 0 either way."""
    one = (np.zeros((1, 3)), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32))
    rig = Rig(lh, torch, make(lh), one, one, (8.0, 8.0, 8.0), (8.0, 8.0, 8.0), reach)
    try:
        assert rig.size(rig.ia) == 1 + ghosts and rig.size(rig.ib) == 1 + ghosts
        got = rig.sess.coords_of(rig.ia, 1 + ghosts)
        assert np.array_equal(got, image_cloud(np.zeros((1, 3)), (8.0, 8.0, 8.0), reach))
        assert rig.score([[0, 0]], float(reach)).tolist() == [0.0]
    finally:
        rig.close()


def lattice():
    """3 x 3 x 3 lattice of spacing L / 3 = 4: ties at every distance, categories cycling over 7 names, 3 atoms per tag."""
    i = np.arange(27)
    xyz = np.stack([i % 3, (i // 3) % 3, i // 9], 1) * 4.0
    return xyz, (i % 7).astype(np.int32), ((3 * i + 1) % 7).astype(np.int32), (i // 3).astype(np.int32)


CATS7 = list("ABCDEFG")
BOX12 = (12.0, 12.0, 12.0)


def test_lattice_that_fills_its_box(lh, torch, oracle):
    xyz, ca, cb, tag = lattice()
    pairs = np.stack([np.arange(27), (np.arange(27) + 5) % 27], 1)
    want, sizes = want_periodic(make(oracle, cats=CATS7, accept_same=False), xyz, ca, tag, BOX12, xyz, cb, tag, BOX12, pairs, 12.0)
    rig = Rig(lh, torch, make(lh, cats=CATS7, accept_same=False), (xyz, ca, tag), (xyz, cb, tag), BOX12, BOX12, 12.0)
    try:
        assert rig.size(rig.ia) == 27 * 27  # every atom has 26 images
        assert np.array_equal(rig.sess.coords_of(rig.ia, 27 * 27), image_cloud(xyz, BOX12, 12.0))
        check(rig.score(pairs, 12.0), want, "lattice")
        assert rig.sess.last_env_points() == int(sizes.sum())
    finally:
        rig.close()
    # the same through the reference-shaped entry point (PrimitiveAtom lists, lchd_from_primitives_periodic)
    lchd = make(lh, cats=CATS7, accept_same=False)
    pa = [lh.PrimitiveAtom(CATS7[c], f"t{t}", x) for c, t, x in zip(ca, tag, xyz)]
    pb = [lh.PrimitiveAtom(CATS7[c], f"t{t}", x) for c, t, x in zip(cb, tag, xyz)]
    got = np.asarray(lchd.from_primitives(pa, pb, [tuple(p) for p in pairs.tolist()], 12.0, box_a=BOX12, box_b=BOX12))
    check(got, want, "lattice, LoCoHD.from_primitives(box_a=, box_b=)")
    # one side open
    want_open, _ = want_periodic(make(oracle, cats=CATS7, accept_same=False), xyz, ca, tag, BOX12, xyz, cb, tag, None, pairs, 12.0)
    got = np.asarray(lchd.from_primitives(pa, pb, [tuple(p) for p in pairs.tolist()], 12.0, box_a=BOX12))
    check(got, want_open, "lattice, side B open")


def test_c_client_of_the_periodic_entry_point(oracle, tmp_path):
    """tests/cabi_periodic.c: compiled as C99 against the header, linked with the library, run; its scores against the oracle."""
    if shutil.which("gcc") is None:
        pytest.fail("gcc is needed to build the C client")
    exe = tmp_path / "cabi_periodic"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", str(ROOT / "include"),
                           str(ROOT / "tests" / "cabi_periodic.c"), "-o", str(exe), "-L", str(ROOT / "loco_hd_amd"), "-lloco_hd_hip",
                           "-lm", f"-Wl,-rpath,{ROOT / 'loco_hd_amd'}"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    assert "cabi periodic ok" in out.stdout
    got = np.asarray([float(ln.split()[2]) for ln in out.stdout.splitlines() if ln.startswith("score ")])
    xyz, ca, cb, tag = lattice()
    pairs = np.stack([np.arange(27), (np.arange(27) + 5) % 27], 1)
    want, _ = want_periodic(make(oracle, cats=CATS7, accept_same=False), xyz, ca, tag, BOX12, xyz, cb, tag, BOX12, pairs, 12.0)
    check(got, want, "C client")


# ------------------------------------------------------------------------------------------------------------------------
# random clouds at every size at which the image kernels take another path
# ------------------------------------------------------------------------------------------------------------------------
def scan_sizes(span):
    return [63, 64, 65, span - 1, span, span + 1, 2 * span - 1, 2 * span, 2 * span + 1]


@pytest.mark.parametrize("thr", [6.0, 16.0, 20.0])
@pytest.mark.parametrize("which", range(9))
def test_random_clouds_around_the_scan_span(lh, torch, oracle, scan_span, which, thr):
    """L = 32; thresholds below, at and above L / 2; n around the wavefront and around one and two block spans of the scan;
    the four weight-function families, Hellinger-2 and Kolmogorov-Smirnov; anchors (i, i) for all i."""
    n = scan_sizes(scan_span)[which]
    rng = np.random.default_rng(1000 * which + int(thr))
    a, b = cloud(rng, n), cloud(rng, n)
    pairs = np.stack([np.arange(n), np.arange(n)], 1)
    first = True
    for (wf, sd) in itertools.product(WFS, SDS):
        same = sd == "H2"  # (the tag rule both ways)
        want, sizes = want_periodic(make(oracle, wf, sd, accept_same=same), *a, L32, *b, L32, pairs, thr)
        rig = Rig(lh, torch, make(lh, wf, sd, accept_same=same), a, b, L32, L32, thr)
        try:
            if first:  # the image cloud itself, bit for bit
                for cl, src in ((rig.ia, a), (rig.ib, b)):
                    exp = image_cloud(src[0], L32, thr)
                    assert rig.size(cl) == len(exp), (n, thr)
                    assert np.array_equal(rig.sess.coords_of(cl, len(exp)), exp), (n, thr)
                first = False
            check(rig.score(pairs, thr), want, f"n = {n}, threshold {thr}, {wf}, {sd}")
            assert rig.sess.last_env_points() == int(sizes.sum())
        finally:
            rig.close()


def test_thin_box_with_both_images_of_every_atom(lh, torch, oracle):
    box = (8.0, 32.0, 32.0)
    rng = np.random.default_rng(7)
    a, b = cloud(rng, 100, box), cloud(rng, 100, box)
    pairs = np.stack([np.arange(100), rng.permutation(100)], 1)
    want, sizes = want_periodic(make(oracle), *a, box, *b, box, pairs, 8.0)
    rig = Rig(lh, torch, make(lh), a, b, box, box, 8.0)
    try:
        got = rig.sess.coords_of(rig.ia, rig.size(rig.ia))
        for i in range(100):  # both x images of every atom, whatever else it has
            for s in (8.0, -8.0):
                assert np.any(np.all(got[100:] == a[0][i] + np.asarray([s, 0.0, 0.0]), axis=1)), (i, s)
        assert np.array_equal(got, image_cloud(a[0], box, 8.0))
        check(rig.score(pairs, 8.0), want, "thin box")
        assert rig.sess.last_env_points() == int(sizes.sum())
    finally:
        rig.close()


def test_no_atom_near_a_face(lh, torch, oracle):
    """Every atom further than `reach` from every face: no ghost, the image cloud is the wrapped cloud, and the scores are those
    of today's call on the wrapped coordinates -- exactly.  The input is given unwrapped."""
    rng = np.random.default_rng(11)
    n = 150
    cells = rng.integers(-3, 4, (n, 3)) * 32.0

    def inner():
        x, c, t = cloud(rng, n, (16.0, 16.0, 16.0))
        x = np.round((x + 8.0) * 2.0 ** 20) / 2.0 ** 20  # (on a 2^-20 grid: wrapping the shifted cloud is exact)
        return x, c, t
    a, b = inner(), inner()
    pairs = np.stack([np.arange(n), np.arange(n)], 1)
    # (deterministic: one sweep family, so that two calls of one session can be compared bit for bit)
    rig = Rig(lh, torch, make(lh, deterministic=True), (a[0] + cells, a[1], a[2]), (b[0] + cells, b[1], b[2]), L32, L32, 6.0)
    try:
        assert rig.size(rig.ia) == n and rig.size(rig.ib) == n
        assert np.array_equal(rig.sess.coords_of(rig.ia, n), a[0])
        got = rig.score(pairs, 6.0)
        wa, wb = rig.sess.upload(*a), rig.sess.upload(*b)
        today = rig.score(pairs, 6.0, wa, wb)
        assert np.array_equal(got, today)
        check(got, make(oracle).from_arrays(*a, *b, pairs, 6.0, interner={}), "no ghosts")
    finally:
        rig.close()


def test_unwrapped_input_scores_as_the_wrapped_one(lh, torch, oracle):
    """The same clouds shifted per atom by integer multiples of L = 32, coordinates on a 2^-20 grid: every operation of the wrap is
    exact, the image clouds are the same bits and so are the scores."""
    rng = np.random.default_rng(13)
    n = 120

    def grid_cloud():
        x, c, t = cloud(rng, n)
        return np.floor(x * 2.0 ** 20) / 2.0 ** 20, c, t
    a, b = grid_cloud(), grid_cloud()
    sa, sb = rng.integers(-5, 6, (n, 3)) * 32.0, rng.integers(-5, 6, (n, 3)) * 32.0
    pairs = np.stack([np.arange(n), np.arange(n)], 1)
    res = []
    for xa, xb in ((a[0], b[0]), (a[0] + sa, b[0] + sb)):
        rig = Rig(lh, torch, make(lh, "hyper_exp", deterministic=True), (xa, a[1], a[2]), (xb, b[1], b[2]), L32, L32, 10.0)
        try:
            res.append((rig.sess.coords_of(rig.ia, rig.size(rig.ia)), rig.score(pairs, 10.0)))
        finally:
            rig.close()
    assert np.array_equal(res[0][0], res[1][0])
    assert np.array_equal(res[0][1], res[1][1])
    check(res[1][1], want_periodic(make(oracle, "hyper_exp"), *a, L32, *b, L32, pairs, 10.0)[0], "unwrapped")


# ------------------------------------------------------------------------------------------------------------------------
# batches, wide categories, refusals
# ------------------------------------------------------------------------------------------------------------------------
def test_ragged_batch_with_a_box_per_structure(lh, torch, oracle):
    """Structures of 40, 1 and 130 atoms in three different boxes, the middle one too large for any ghost; anchor pairs across
    structures; the same image cloud on both sides."""
    from loco_hd_amd.device import DeviceSession

    rng = np.random.default_rng(17)
    boxes = np.asarray([[30.0, 34.0, 28.0], [200.0, 200.0, 200.0], [24.0, 40.0, 32.0]])
    thr = 9.0
    sts = [cloud(rng, 40, boxes[0]), (np.full((1, 3), 100.0), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)), cloud(rng, 130, boxes[2])]
    jobs = [(0, 2, np.stack([rng.integers(0, 40, 60), rng.integers(0, 130, 60)], 1)),
            (2, 0, np.stack([rng.integers(0, 130, 50), rng.integers(0, 40, 50)], 1)),
            (1, 2, np.stack([np.zeros(7, dtype=np.int64), rng.integers(0, 130, 7)], 1)),
            (2, 2, np.stack([rng.integers(0, 130, 40), rng.integers(0, 130, 40)], 1)),
            (1, 1, np.zeros((1, 2), dtype=np.int64))]
    o = make(oracle, "dagum")
    want = [want_periodic(o, *sts[sa], boxes[sa], *sts[sb], boxes[sb], pr, thr) for sa, sb, pr in jobs]
    sess = DeviceSession(make(lh, "dagum"), interner={})
    try:
        batch, offs = sess.upload_batch(sts)
        img = sess.periodic_images(batch, boxes, thr)
        from loco_hd_amd import _native as N
        n_img = int(N.lib().lchd_cloud_size(img))
        exp = [image_cloud(st[0], bx, thr) for st, bx in zip(sts, boxes)]
        assert len(exp[1]) == 1  # (the large box: no ghost)
        assert n_img == sum(len(e) for e in exp)
        got_xyz = sess.coords_of(img, n_img)
        assert np.array_equal(got_xyz[:171], np.concatenate([e[:len(st[0])] for e, st in zip(exp, sts)]))
        assert np.array_equal(got_xyz[171:], np.concatenate([e[len(st[0]):] for e, st in zip(exp, sts)]))
        flat = np.concatenate([pr + np.asarray([offs[sa], offs[sb]]) for sa, sb, pr in jobs])
        got = sess.from_primitives(img, img, torch.from_numpy(flat).cuda(), thr).cpu().numpy()
        check(got, np.concatenate([w[0] for w in want]), "ragged batch")
        assert sess.last_env_points() == int(sum(w[1].sum() for w in want))
        with pytest.raises(ValueError, match="boxes"):
            sess.periodic_images(batch, boxes[:2], thr)
    finally:
        sess.close()
    # the same through LoCoHD.from_primitives_batch(boxes=...)
    lchd = make(lh, "dagum")
    prims = [[lh.PrimitiveAtom(CATS[c], f"t{t}", x) for c, t, x in zip(st[1], st[2], st[0])] for st in sts]
    got = lchd.from_primitives_batch(prims, [(sa, sb, pr.tolist()) for sa, sb, pr in jobs], thr, boxes=boxes)
    for g, w, job in zip(got, want, jobs):
        check(np.asarray(g), w[0], f"from_primitives_batch job {job[:2]}")


def test_more_than_255_categories(lh, torch, oracle):
    """300 names over 200 atoms: the image kernels copy the high bytes and the one-byte view of the category ids as well."""
    cats = [f"c{i}" for i in range(300)]
    rng = np.random.default_rng(19)
    a, b = cloud(rng, 200, n_cat=300), cloud(rng, 200, n_cat=300)
    pairs = np.stack([np.arange(200), np.arange(200)], 1)
    want, sizes = want_periodic(make(oracle, cats=cats), *a, L32, *b, L32, pairs, 10.0)
    rig = Rig(lh, torch, make(lh, cats=cats), a, b, L32, L32, 10.0)
    try:
        check(rig.score(pairs, 10.0), want, "300 categories")
        assert rig.sess.last_env_points() == int(sizes.sum())
    finally:
        rig.close()


def test_image_cloud_refuses_what_it_cannot_do(lh, torch):
    rng = np.random.default_rng(23)
    a = cloud(rng, 70)
    rig = Rig(lh, torch, make(lh), a, a, L32, L32, 8.0)
    try:
        pairs = np.stack([np.arange(70), np.arange(70)], 1)
        rig.score(pairs, 8.0)
        with pytest.raises(ValueError, match="reach"):
            rig.score(pairs, np.nextafter(8.0, 9.0))
        with pytest.raises(ValueError, match="reach"):
            rig.score(pairs, 8.5, rig.a, rig.ib)
        with pytest.raises(ValueError, match="image cloud"):
            rig.sess.set_coords(rig.ia, a[0])
        with pytest.raises(ValueError):
            rig.sess.load_frames(rig.ia, a[0][None])
        with pytest.raises(ValueError, match="image cloud"):
            rig.sess.periodic_images(rig.ia, L32, 8.0)
        with pytest.raises(ValueError, match="reach"):
            rig.sess.periodic_images(rig.a, (32.0, 7.0, 32.0), 8.0)
        rig.score(pairs, 8.0)  # (still usable)
        rig.sess.set_coords(rig.a, a[0] + 1.0)  # the source moves, the image cloud follows on request
        rig.sess.update_images(rig.ia, rig.a, L32)
        assert np.array_equal(rig.sess.coords_of(rig.ia, rig.size(rig.ia)), image_cloud(wrap(a[0] + 1.0, L32), L32, 8.0))
    finally:
        rig.close()


# ------------------------------------------------------------------------------------------------------------------------
# trajectories
# ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def traj():
    """5 frames of 90 atoms, a box per frame.  Frame 3 sits in a corner of its box (every atom within reach of three faces: 7
    ghosts each) and frame 4 in the middle of a box of less than twice the reach (26 ghosts each), so the image arrays of both
    buffers must grow past what their earlier frames needed: buffer 1 while it is created, buffer 0 in its update."""
    rng = np.random.default_rng(29)
    n, thr = 90, 8.0
    boxes = np.asarray([[30.0, 31.0, 32.0], [30.5, 31.5, 32.5], [31.0, 32.0, 33.0], [31.5, 32.5, 33.5], [12.0, 12.5, 13.0]])
    ref = cloud(rng, n, (30.0, 30.0, 30.0))
    frames = np.stack([rng.uniform(0.0, 1.0, (n, 3)) * boxes[f] for f in range(5)])
    frames[3] = rng.uniform(0.0, 4.0, (n, 3))
    frames[4] = rng.uniform(5.0, 7.5, (n, 3))
    lp = np.stack([np.arange(n), rng.permutation(n)], 1)
    return SimpleNamespace(n=n, thr=thr, boxes=boxes, ref=ref, ref_box=np.asarray([30.0, 30.0, 30.0]), frames=frames, lp=lp)


def test_score_trajectory_with_boxes(lh, torch, oracle, traj):
    """chunk = 2: three chunks, the last one partial, both buffers reused, image arrays that grow; against the replicated oracle
    frame by frame.  Without boxes the call is today's (open) one."""
    from loco_hd_amd.device import DeviceSession

    t = traj
    o = make(oracle, "kumaraswamy")
    want = np.stack([want_periodic(o, *t.ref, t.ref_box, t.frames[f], t.ref[1], t.ref[2], t.boxes[f], t.lp, t.thr)[0] for f in range(5)])
    want_open = np.stack([o.from_arrays(*t.ref, t.frames[f], t.ref[1], t.ref[2], t.lp, t.thr, interner={}) for f in range(5)])
    assert image_cloud(t.frames[3], t.boxes[3], t.thr).shape[0] == 8 * t.n and image_cloud(t.frames[4], t.boxes[4], t.thr).shape[0] == 27 * t.n
    sess = DeviceSession(make(lh, "kumaraswamy"), interner={})
    try:
        ref = sess.upload(*t.ref)
        got = sess.score_trajectory(ref, t.frames, t.lp, t.thr, chunk=2, ref_box=t.ref_box, boxes=t.boxes)
        check(got.reshape(-1), want.reshape(-1), "trajectory, a box per frame")
        assert len(sess._clouds) == 1  # (buffers and image clouds of the call are gone)
        got = sess.score_trajectory(ref, t.frames, t.lp, t.thr, chunk=2)
        check(got.reshape(-1), want_open.reshape(-1), "trajectory, boxes=None")
        assert float(np.max(np.abs(want - want_open))) > 1e-3
        # one box for all frames, the reference open
        want_one = np.stack([want_periodic(o, *t.ref, None, t.frames[f], t.ref[1], t.ref[2], t.boxes[2], t.lp, t.thr)[0] for f in range(5)])
        got = sess.score_trajectory(ref, t.frames, t.lp, t.thr, chunk=2, boxes=t.boxes[2])
        check(got.reshape(-1), want_one.reshape(-1), "trajectory, one box")
        with pytest.raises(ValueError, match="boxes"):
            sess.score_trajectory(ref, t.frames, t.lp, t.thr, chunk=2, boxes=t.boxes[:3])
    finally:
        sess.close()


# ---- stream order: the delayed-producer pattern of tests/test_gpu_streams.py (copied: its helpers are private to that module) ----
class Delay:
    """Enqueue ~`ms` of idle GPU time on a torch stream."""

    def __init__(self, torch, ms=20.0):
        self.torch = torch
        self.native = hasattr(torch.cuda, "_sleep")
        self._pad = torch.zeros(1 << 22, device="cuda")
        unit = 2_000_000 if self.native else 8  # cycles / kernels in a chain
        self._measure(unit)  # warm-up
        per_ms = max(unit / max(self._measure(unit), 1e-3), 1.0)
        self.amount, self.ms = int(np.ceil(ms * per_ms)), ms

    def _enqueue(self, amount):
        if self.native:
            self.torch.cuda._sleep(int(amount))
        else:
            for _ in range(int(amount)):
                self._pad.add_(1.0)

    def _measure(self, amount):
        torch = self.torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        self._enqueue(amount)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def on(self, stream):
        with self.torch.cuda.stream(stream):
            self._enqueue(self.amount)

    def _runs_beside(self, busy, other):
        """True if work queued on `other` completes while `busy` is held by a short delay."""
        torch = self.torch
        torch.cuda.synchronize()
        done = torch.cuda.Event()
        with torch.cuda.stream(busy):
            self._enqueue(max(self.amount // 10, 1))
            done.record(busy)
        with torch.cuda.stream(other):
            self._pad[:64].add_(1.0)
        other.synchronize()
        beside = not done.query()
        busy.synchronize()
        return beside

    def streams(self, k):
        """k torch streams that the device runs side by side (two streams that share a hardware queue run in submission order: a
        delay on one would hold the other back, and a missing wait between them could not show)."""
        chosen = []
        for _ in range(32):
            cand = self.torch.cuda.Stream()
            if all(self._runs_beside(x, cand) and self._runs_beside(cand, x) for x in chosen):
                chosen.append(cand)
            if len(chosen) == k:
                return chosen
        pytest.fail(f"no {k} streams that run side by side among 32 candidates")


def test_image_build_waits_for_a_late_frames_upload(lh, torch, oracle, traj):
    """The buffer holds frames X; frames Y are loaded behind a delay on the copy stream and the image cloud is built at once, on
    the session's stream.  A build that did not wait for the upload's event would wrap X."""
    from loco_hd_amd.device import DeviceSession

    t = traj
    o = make(oracle)
    x, y = t.frames[:2], t.frames[2:4]
    anchors = np.concatenate([t.lp + np.asarray([0, f * t.n]) for f in range(2)])
    want = {k: np.concatenate([want_periodic(o, *t.ref, None, fr[f], t.ref[1], t.ref[2], t.boxes[0], t.lp, t.thr)[0] for f in range(2)])
            for k, fr in (("X", x), ("Y", y))}
    assert float(np.max(np.abs(want["X"] - want["Y"]))) > 1e-3
    delay = Delay(torch)
    s, cs = delay.streams(2)
    with torch.cuda.stream(s):
        sess = DeviceSession(make(lh), interner={})
        try:
            ref = sess.upload(*t.ref)
            buf = sess.frames_buffer(ref, 2)
            d_anchors = torch.from_numpy(anchors).cuda()
            sess.load_frames(buf, x, cs)
            img = sess.periodic_images(buf, t.boxes[0], t.thr)
            check(sess.from_primitives(ref, img, d_anchors, t.thr).cpu().numpy(), want["X"], "X")
            torch.cuda.synchronize()
            delay.on(cs)
            sess.load_frames(buf, y, cs)
            behind = torch.cuda.Event()
            behind.record(cs)
            assert not behind.query(), "the copy stream had drained when the load returned: the delay did not hold the load back"
            sess.update_images(img, buf, t.boxes[0])
            check(sess.from_primitives(ref, img, d_anchors, t.thr).cpu().numpy(), want["Y"], "Y behind the delay")
        finally:
            sess.close()


# ------------------------------------------------------------------------------------------------------------------------
# the feature matters
# ------------------------------------------------------------------------------------------------------------------------
SANITY_SEED = 0  # picked on the CPU with the oracle: see the docstring below


def test_a_rim_anchor_scores_differently_in_a_box(lh, torch, oracle):
    """Seed 0, 300 atoms per side in L = 32, threshold 10, anchors = the atoms closest to the corner at the origin (259 and 16):
    with the oracle alone the pair scores 0.52278 in the box and 0.78493 in the open, 0.262 apart (seeds 0 .. 7 gave 0.025 .. 0.27).
    The device must show the same difference."""
    rng = np.random.default_rng(SANITY_SEED)
    a, b = cloud(rng, 300), cloud(rng, 300)
    i, j = int(np.argmin(np.sum(a[0] ** 2, 1))), int(np.argmin(np.sum(b[0] ** 2, 1)))
    pairs = np.asarray([[i, j]])
    o = make(oracle)
    w_box, w_open = want_periodic(o, *a, L32, *b, L32, pairs, 10.0)[0][0], o.from_arrays(*a, *b, pairs, 10.0, interner={})[0]
    print(f"rim anchor pair ({i}, {j}): periodic {w_box:.6f}, open {w_open:.6f}")
    assert abs(w_box - w_open) > 1e-3
    rig = Rig(lh, torch, make(lh), a, b, L32, L32, 10.0)
    try:
        g_box, g_open = rig.score(pairs, 10.0)[0], rig.score(pairs, 10.0, rig.a, rig.b)[0]
    finally:
        rig.close()
    assert abs(g_box - w_box) <= TIGHT and abs(g_open - w_open) <= TIGHT
    assert abs(g_box - g_open) > 1e-3
