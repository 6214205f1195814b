"""Periodic boundaries in triclinic cells on the device: k_img_count_cell / k_img_emit_cell (loco_hd_amd/csrc/lchd_images.hip) in
front of the unchanged from_primitives pass.

Reference value.  The wrapped originals p are read back from the device (coords_of), checked against the input (equal modulo the
lattice to 1e-9, fractional coordinates in [0, 1) within 1e-12), and the replicated system is built from them in NumPy: the
originals, then the 26 copies p + t with t[d] = (i a[d] + j b[d]) + k c[d] -- the expression of include/loco_hd_hip.h, plain f64 in
that order -- with categories and tags tiled.  oracle.from_arrays scores it with the same anchors and threshold.  Every ghost the
device holds is one of those sums bit for bit, so distances agree exactly, membership at the threshold cannot differ, scores must
agree within the project's TIGHT = 1e-11 and environment sizes (last_env_points) exactly.

The helpers of tests/test_gpu_periodic.py (make, check, the weight-function and distance tables, the box-path replicate / wrap) are
imported, that file is not touched.
"""
import itertools
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests.periodic_cell_util import CELLS, widths
from tests.test_gpu_periodic import CATS, SDS, TIGHT, WFS, check, lh, make, scan_span, torch  # noqa: F401  (fixtures included)
from tests.test_gpu_periodic import replicate as replicate_box
from tests.test_gpu_periodic import wrap as wrap_box

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
COEF = (0.0, 1.0, -1.0)  # per-axis choice 0 original, 1 plus, 2 minus
CODES = [(c0, c1, c2) for c2 in range(3) for c1 in range(3) for c0 in range(3)][1:]  # ascending image code c0 + 3 c1 + 9 c2


# ------------------------------------------------------------------------------------------------------------------------
# the contract in NumPy
# ------------------------------------------------------------------------------------------------------------------------
def frac(x, cell):
    return np.asarray(x) @ np.linalg.inv(cell)


def shift(cell, c0, c1, c2):
    """t = i a + j b + k c per component as (i a[d] + j b[d]) + k c[d]."""
    return (COEF[c0] * cell[0] + COEF[c1] * cell[1]) + COEF[c2] * cell[2]


def replicate_cell(p, cell):
    return np.concatenate([p] + [p + shift(cell, *c) for c in CODES])


def slab(p, cell, reach):
    """(plus, minus, margin): the image rule per atom and axis, and how far the closest comparison is from `reach`."""
    g, w = frac(p, cell), widths(cell)
    lo, hi = g * w, (1.0 - g) * w
    return lo < reach, hi <= reach, float(min(np.min(np.abs(lo - reach)), np.min(np.abs(hi - reach)))) if len(p) else np.inf


def image_cloud_cell(p, cell, reach):
    """What the device must hold behind the wrapped originals p: per atom its ghosts in ascending image code."""
    plus, minus, _ = slab(p, cell, reach)
    ghosts = []
    for i in range(len(p)):
        ok = [(True, plus[i, k], minus[i, k]) for k in range(3)]
        ghosts += [p[i] + shift(cell, c0, c1, c2) for c0, c1, c2 in CODES if ok[0][c0] and ok[1][c1] and ok[2][c2]]
    return np.concatenate([p, np.asarray(ghosts, dtype=np.float64).reshape(-1, 3)])


def check_wrapped(p, x, cell):
    m = np.round(frac(p - x, cell))
    assert float(np.max(np.abs(x + m @ cell - p))) <= 1e-9  # the input modulo the lattice
    g = frac(p, cell)
    assert np.all(g >= -1e-12) and np.all(g < 1.0 + 1e-12)


def cloud_in(rng, n, cell, n_cat=len(CATS), n_tag=5):
    return (rng.uniform(0.0, 1.0, (n, 3)) @ cell, rng.integers(0, n_cat, n).astype(np.int32), rng.integers(0, n_tag, n).astype(np.int32))


class CellRig:
    """A session with two uploaded structures and what stands for each in a pass: per side None (open), ("box", L) or ("cell", M)."""

    def __init__(self, lh, torch, lchd, a, b, per_a, per_b, reach):
        from loco_hd_amd.device import DeviceSession

        self.torch, self.sess, self.reach = torch, DeviceSession(lchd, interner={}), reach
        self.src, self.per, self.n = [a, b], [per_a, per_b], [len(a[0]), len(b[0])]
        self.a, self.b = self.sess.upload(*a), self.sess.upload(*b)
        self.ia, self.ib = self.images(self.a, per_a), self.images(self.b, per_b)

    def images(self, cl, per):
        if per is None:
            return cl
        return self.sess.periodic_images(cl, per[1], self.reach) if per[0] == "box" else self.sess.periodic_images(cl, reach=self.reach, cell=per[1])

    def size(self, cl):
        from loco_hd_amd import _native as N

        return int(N.lib().lchd_cloud_size(cl))

    def coords(self, cl):
        return self.sess.coords_of(cl, self.size(cl))

    def replicated(self, k):
        """Side k as the oracle takes it: (xyz, cat, tag) of the replicated system, built from the device's wrapped originals."""
        x, c, t = self.src[k]
        per, cl = self.per[k], (self.ia, self.ib)[k]
        if per is None:
            return x, c, t
        if per[0] == "box":
            return replicate_box(wrap_box(x, per[1]), per[1]), np.tile(c, 27), np.tile(t, 27)
        p = self.coords(cl)[:self.n[k]]
        check_wrapped(p, x, per[1])
        return replicate_cell(p, per[1]), np.tile(c, 27), np.tile(t, 27)

    def want(self, o, pairs, thr):
        return o.from_arrays(*self.replicated(0), *self.replicated(1), pairs, thr, return_env_sizes=True, interner={})

    def score(self, pairs, thr, a=None, b=None):
        anchors = self.torch.from_numpy(np.ascontiguousarray(pairs, dtype=np.int64)).cuda()
        return self.sess.from_primitives(self.ia if a is None else a, self.ib if b is None else b, anchors, thr).cpu().numpy()

    def check_ghosts(self, k):
        """The image cloud of side k against the slab rule in NumPy: count and every coordinate, bit for bit.  The comparison
        means something only if no atom sits on a slab boundary: asserted, on the device's own wrapped coordinates."""
        cl, cell = (self.ia, self.ib)[k], self.per[k][1]
        got = self.coords(cl)
        p = got[:self.n[k]]
        assert slab(p, cell, self.reach)[2] > 1e-9, "an atom within 1e-9 of a slab boundary: pick another seed"
        exp = image_cloud_cell(p, cell, self.reach)
        assert len(got) == len(exp)
        assert np.array_equal(got, exp)
        return len(got) - self.n[k]

    def close(self):
        self.sess.close()


# ------------------------------------------------------------------------------------------------------------------------
# 1, 2: the smallest cases
# ------------------------------------------------------------------------------------------------------------------------
SKEW_MIN = float(np.min(widths(CELLS["skewed"])))


@pytest.mark.parametrize("reach, ghosts", [(SKEW_MIN, 11), (float(np.nextafter(SKEW_MIN, 0.0)), 7), (4.0, 7)])
def test_one_atom_at_the_origin_of_the_skewed_cell(lh, torch, reach, ghosts):
    """g = (0, 0, 0): the three plus images exist for any reach (0 < reach), a minus image along axis k iff w_k <= reach, that is at
    reach = min w along the axis of the smallest width alone: 2 x 2 x 2 - 1 = 7 ghosts below it, 3 x 2 x 2 - 1 = 11 at it."""
    cell = CELLS["skewed"]
    one = (np.zeros((1, 3)), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32))
    rig = CellRig(lh, torch, make(lh), one, one, ("cell", cell), ("cell", cell), reach)
    try:
        exp = image_cloud_cell(np.zeros((1, 3)), cell, reach)  # (from the rule)
        assert len(exp) == 1 + ghosts
        got = rig.coords(rig.ia)
        assert rig.size(rig.ia) == 1 + ghosts and rig.size(rig.ib) == 1 + ghosts
        assert np.array_equal(got, exp)
        if ghosts == 7:  # i a + j b + k c, i, j, k in {0, 1} not all zero, x fastest
            lattice = [(i * cell[0] + j * cell[1]) + k * cell[2] for k in (0.0, 1.0) for j in (0.0, 1.0) for i in (0.0, 1.0)][1:]
            assert np.array_equal(got[1:], np.asarray(lattice))
        else:  # the axis of the smallest width has its minus image too, alone and on top of the four combinations of the others
            k = int(np.argmin(widths(cell)))
            assert sum(1 for g in got[1:] if np.array_equal(g, -cell[k])) == 1
            assert len({tuple(g) for g in got[1:].tolist()}) == 11
        assert rig.score([[0, 0]], float(reach)).tolist() == [0.0]
    finally:
        rig.close()


def test_lattice_that_fills_the_dodecahedron(lh, torch, oracle):
    """4 x 4 x 4 atoms at the fractional coordinates (i, j, k) / 4, every atom an anchor, threshold 8: every anchor sees the same
    periodic lattice, so every environment has the same size (a tag per atom: the tag rule leaves nobody out)."""
    cell = CELLS["dodecahedron"]
    i = np.arange(64)
    x = (np.stack([i % 4, (i // 4) % 4, i // 16], 1) / 4.0) @ cell
    ca, cb, tag = (i % 5).astype(np.int32), ((3 * i + 1) % 5).astype(np.int32), i.astype(np.int32)
    pairs = np.stack([i, i], 1)
    rig = CellRig(lh, torch, make(lh, accept_same=False), (x, ca, tag), (x, cb, tag), ("cell", cell), ("cell", cell), 8.0)
    try:
        want, sizes = rig.want(make(oracle, accept_same=False), pairs, 8.0)
        assert len(set(sizes.reshape(-1).tolist())) == 1 and sizes[0, 0] > 1
        check(rig.score(pairs, 8.0), want, "dodecahedron lattice")
        assert rig.sess.last_env_points() == int(sizes.sum())
    finally:
        rig.close()


# ------------------------------------------------------------------------------------------------------------------------
# 3: random clouds at every size at which the image kernels take another path, in every cell
# ------------------------------------------------------------------------------------------------------------------------
def scan_sizes(span):
    return [span - 1, span, span + 1, 2 * span + 3]


COMBOS = list(itertools.product(WFS, SDS))  # 8: the four weight-function families x (H2, accept_same) / (KS, not)
# (cell, index into scan_sizes, threshold: 6 or None = the smallest width; the latter at n <= span + 1 only)
RANDOM_CASES = [("monoclinic", 0, 6.0), ("monoclinic", 2, None), ("dodecahedron", 1, 6.0), ("dodecahedron", 3, 6.0), ("dodecahedron", 0, None),
                ("octahedron", 2, 6.0), ("octahedron", 1, None), ("skewed", 3, 6.0), ("skewed", 2, None), ("left-handed", 0, 6.0),
                ("left-handed", 1, None), ("left-handed", 3, 6.0)]


@pytest.mark.parametrize("case", range(len(RANDOM_CASES)))
def test_random_clouds_around_the_scan_span(lh, torch, oracle, scan_span, case):
    name, which, thr = RANDOM_CASES[case]
    cell = CELLS[name]
    thr = float(np.min(widths(cell))) if thr is None else thr
    n = scan_sizes(scan_span)[which]
    rng = np.random.default_rng(7000 + case)
    a, b = cloud_in(rng, n, cell), cloud_in(rng, n, cell)
    pairs = np.stack([np.arange(n), np.arange(n)], 1)
    for k, (wf, sd) in enumerate((COMBOS[case % 8], COMBOS[(case + 5) % 8])):  # (both distances and both tag rules in every case)
        same = sd == "H2"
        rig = CellRig(lh, torch, make(lh, wf, sd, accept_same=same), a, b, ("cell", cell), ("cell", cell), thr)
        try:
            if k == 0:
                assert rig.check_ghosts(0) > 0 and rig.check_ghosts(1) > 0
            want, sizes = rig.want(make(oracle, wf, sd, accept_same=same), pairs, thr)
            check(rig.score(pairs, thr), want, f"{name}, n = {n}, threshold {thr}, {wf}, {sd}")
            assert rig.sess.last_env_points() == int(sizes.sum())
        finally:
            rig.close()


# ------------------------------------------------------------------------------------------------------------------------
# 4, 5, 6: unwrapped input, the diagonal cell against the box path, mixed sides
# ------------------------------------------------------------------------------------------------------------------------
def test_unwrapped_input_scores_as_the_wrapped_one(lh, torch, oracle):
    cell = CELLS["octahedron"]
    rng = np.random.default_rng(31)
    n = 120
    a, b = cloud_in(rng, n, cell), cloud_in(rng, n, cell)
    sa, sb = rng.integers(-3, 4, (n, 3)).astype(np.float64) @ cell, rng.integers(-3, 4, (n, 3)).astype(np.float64) @ cell
    pairs = np.stack([np.arange(n), rng.permutation(n)], 1)
    res = []
    for xa, xb in ((a[0], b[0]), (a[0] + sa, b[0] + sb)):
        rig = CellRig(lh, torch, make(lh, "hyper_exp"), (xa, a[1], a[2]), (xb, b[1], b[2]), ("cell", cell), ("cell", cell), 10.0)
        try:
            ghosts = (rig.check_ghosts(0), rig.check_ghosts(1))
            got = rig.score(pairs, 10.0)
            check(got, rig.want(make(oracle, "hyper_exp"), pairs, 10.0)[0], "octahedron, wrapped / unwrapped input")
            res.append((ghosts, got))
        finally:
            rig.close()
    assert res[0][0] == res[1][0]
    check(res[1][1], res[0][1], "unwrapped against wrapped")


def test_diagonal_cell_against_the_box_path(lh, torch):
    """diag(L) through the cell arguments runs the triclinic kernels (the host layer has no shortcut: the cloud is a cell cloud and
    refuses a box update) and must give what the box kernels give: the same ghosts, the same scores, bit for bit."""
    L = (30.0, 30.0, 30.0)
    cell = np.diag(L)
    rng = np.random.default_rng(37)
    n = 150
    a, b = cloud_in(rng, n, cell), cloud_in(rng, n, cell)
    pairs = np.stack([np.arange(n), rng.permutation(n)], 1)
    res = []
    for per in (("box", L), ("cell", cell)):
        rig = CellRig(lh, torch, make(lh, deterministic=True), a, b, per, per, 10.0)
        try:
            res.append((rig.coords(rig.ia), rig.coords(rig.ib), rig.score(pairs, 10.0)))
            if per[0] == "cell":
                with pytest.raises(ValueError, match="cells"):
                    rig.sess.update_images(rig.ia, rig.a, L)
        finally:
            rig.close()
    assert len(res[0][0]) == len(res[1][0]) > n and len(res[0][1]) == len(res[1][1]) > n
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    assert np.array_equal(res[0][2], res[1][2])
    # the same through the reference-shaped entry point
    lchd = make(lh, deterministic=True)
    pa = [lh.PrimitiveAtom(CATS[c], f"t{t}", x) for c, t, x in zip(a[1], a[2], a[0])]
    pb = [lh.PrimitiveAtom(CATS[c], f"t{t}", x) for c, t, x in zip(b[1], b[2], b[0])]
    pl = [tuple(p) for p in pairs.tolist()]
    by_box = lchd.from_primitives(pa, pb, pl, 10.0, box_a=L, box_b=L)
    by_cell = lchd.from_primitives(pa, pb, pl, 10.0, cell_a=cell, cell_b=cell)
    assert by_box == by_cell


@pytest.mark.parametrize("sides", ["box A, cell B", "cell A, open B"])
def test_mixed_sides(lh, torch, oracle, sides):
    cell, box = CELLS["dodecahedron"], (28.0, 31.0, 26.0)
    rng = np.random.default_rng(41)
    n, thr = 110, 9.0
    if sides == "box A, cell B":
        a, b = (rng.uniform(0.0, 1.0, (n, 3)) * np.asarray(box), *cloud_in(rng, n, cell)[1:]), cloud_in(rng, n, cell)
        per_a, per_b, kw = ("box", box), ("cell", cell), {"box_a": box, "cell_b": cell}
    else:
        a, b = cloud_in(rng, n, cell), cloud_in(rng, n, cell)
        per_a, per_b, kw = ("cell", cell), None, {"cell_a": cell}
    pairs = np.stack([np.arange(n), rng.permutation(n)], 1)
    rig = CellRig(lh, torch, make(lh, "kumaraswamy"), a, b, per_a, per_b, thr)
    try:
        want, sizes = rig.want(make(oracle, "kumaraswamy"), pairs, thr)
        check(rig.score(pairs, thr), want, sides)
        assert rig.sess.last_env_points() == int(sizes.sum())
    finally:
        rig.close()
    pa = [lh.PrimitiveAtom(CATS[c], f"t{t}", x) for c, t, x in zip(a[1], a[2], a[0])]
    pb = [lh.PrimitiveAtom(CATS[c], f"t{t}", x) for c, t, x in zip(b[1], b[2], b[0])]
    got = make(lh, "kumaraswamy").from_primitives(pa, pb, [tuple(p) for p in pairs.tolist()], thr, **kw)
    check(np.asarray(got), want, sides + ", LoCoHD.from_primitives")
    # an index beyond the structure would name a ghost of the image cloud: a panic, as through the one-family calls
    for bad in ([(n, 0)], [(0, n)], [(0, 0), (n + 3, 1)]):  # (a negative index is no anchor at all: OverflowError, as for usize)
        with pytest.raises(lh.PanicException, match="anchor"):
            make(lh, "kumaraswamy").from_primitives(pa, pb, bad, thr, **kw)
    with pytest.raises(lh.PanicException, match="anchor"):
        make(lh, "kumaraswamy").from_primitives(pa, pb, [(n, 0)], thr, cell_a=cell, cell_b=cell)


# ------------------------------------------------------------------------------------------------------------------------
# 7, 8, 10: batches, wide categories, refusals
# ------------------------------------------------------------------------------------------------------------------------
def test_ragged_batch_with_a_cell_per_structure(lh, torch, oracle):
    """Structures of 40, 1 and 130 atoms in a diagonal cell, the dodecahedron and the skewed cell; anchor pairs across structures;
    through upload_batch + periodic_images(cell=...) and through from_primitives_batch(cells=...): both equal the per-pair calls
    bit for bit (one sweep family: deterministic) and the oracle within TIGHT."""
    from loco_hd_amd import _native as N
    from loco_hd_amd.device import DeviceSession

    rng = np.random.default_rng(43)
    cells = np.stack([np.diag([30.0, 34.0, 28.0]), CELLS["dodecahedron"], CELLS["skewed"]])
    thr, sizes_n = 9.0, (40, 1, 130)
    sts = [cloud_in(rng, n, cl) for n, cl in zip(sizes_n, cells)]
    jobs = [(0, 2, np.stack([rng.integers(0, 40, 60), rng.integers(0, 130, 60)], 1)),
            (2, 0, np.stack([rng.integers(0, 130, 50), rng.integers(0, 40, 50)], 1)),
            (1, 2, np.stack([np.zeros(7, dtype=np.int64), rng.integers(0, 130, 7)], 1)),
            (2, 2, np.stack([rng.integers(0, 130, 40), rng.integers(0, 130, 40)], 1)),
            (1, 1, np.zeros((1, 2), dtype=np.int64))]
    lchd = make(lh, "dagum", deterministic=True)
    sess = DeviceSession(lchd, interner={})
    try:
        batch, offs = sess.upload_batch(sts)
        img = sess.periodic_images(batch, reach=thr, cell=cells)
        n_img = int(N.lib().lchd_cloud_size(img))
        got_xyz = sess.coords_of(img, n_img)
        wrapped = [got_xyz[offs[k]:offs[k + 1]] for k in range(3)]
        for p, st, cl in zip(wrapped, sts, cells):
            check_wrapped(p, st[0], cl)
            assert slab(p, cl, thr)[2] > 1e-9
        exp = [image_cloud_cell(p, cl, thr) for p, cl in zip(wrapped, cells)]
        assert n_img == sum(len(e) for e in exp)
        assert np.array_equal(got_xyz[offs[3]:], np.concatenate([e[n:] for e, n in zip(exp, sizes_n)]))  # ghosts follow their atoms' order
        flat = np.concatenate([pr + np.asarray([offs[sa], offs[sb]]) for sa, sb, pr in jobs])
        got = sess.from_primitives(img, img, torch.from_numpy(flat).cuda(), thr).cpu().numpy()
        env_points = sess.last_env_points()
        with pytest.raises(ValueError, match="cells"):
            sess.periodic_images(batch, reach=thr, cell=cells[:2])
    finally:
        sess.close()
    o = make(oracle, "dagum")
    rep = [(replicate_cell(p, cl), np.tile(st[1], 27), np.tile(st[2], 27)) for p, st, cl in zip(wrapped, sts, cells)]
    want = [o.from_arrays(*rep[sa], *rep[sb], pr, thr, return_env_sizes=True, interner={}) for sa, sb, pr in jobs]
    check(got, np.concatenate([w[0] for w in want]), "ragged batch, a cell per structure")
    assert env_points == int(sum(w[1].sum() for w in want))
    prims = [[lh.PrimitiveAtom(CATS[c], f"t{t}", x) for c, t, x in zip(st[1], st[2], st[0])] for st in sts]
    by_batch = lchd.from_primitives_batch(prims, [(sa, sb, pr.tolist()) for sa, sb, pr in jobs], thr, cells=cells)
    pos = 0
    for (sa, sb, pr), g, w in zip(jobs, by_batch, want):
        single = lchd.from_primitives(prims[sa], prims[sb], [tuple(p) for p in pr.tolist()], thr, cell_a=cells[sa], cell_b=cells[sb])
        assert g == single, (sa, sb)
        assert got[pos:pos + len(pr)].tolist() == single, (sa, sb)
        check(np.asarray(g), w[0], f"from_primitives_batch(cells=...) job {(sa, sb)}")
        pos += len(pr)


def test_more_than_255_categories(lh, torch, oracle):
    """300 names over 200 atoms: the cell kernels copy the high bytes and the one-byte view of the category ids as well."""
    cats = [f"c{i}" for i in range(300)]
    cell = CELLS["left-handed"]
    rng = np.random.default_rng(47)
    a, b = cloud_in(rng, 200, cell, n_cat=300), cloud_in(rng, 200, cell, n_cat=300)
    pairs = np.stack([np.arange(200), np.arange(200)], 1)
    rig = CellRig(lh, torch, make(lh, cats=cats), a, b, ("cell", cell), ("cell", cell), 10.0)
    try:
        want, sizes = rig.want(make(oracle, cats=cats), pairs, 10.0)
        check(rig.score(pairs, 10.0), want, "300 categories in a cell")
        assert rig.sess.last_env_points() == int(sizes.sum())
    finally:
        rig.close()


def test_cell_cloud_refuses_what_a_box_cloud_refuses(lh, torch):
    cell, L32 = CELLS["dodecahedron"], (32.0, 32.0, 32.0)
    rng = np.random.default_rng(53)
    a = cloud_in(rng, 70, cell)
    rig = CellRig(lh, torch, make(lh), a, a, ("cell", cell), ("box", L32), 8.0)
    try:
        pairs = np.stack([np.arange(70), np.arange(70)], 1)
        rig.score(pairs, 8.0)
        with pytest.raises(ValueError, match="reach"):
            rig.score(pairs, np.nextafter(8.0, 9.0))
        with pytest.raises(ValueError, match="reach"):
            rig.score(pairs, 8.5, rig.ia, rig.b)
        with pytest.raises(ValueError, match="image cloud"):
            rig.sess.set_coords(rig.ia, a[0])
        with pytest.raises(ValueError):
            rig.sess.load_frames(rig.ia, a[0][None])
        with pytest.raises(ValueError, match="image cloud"):
            rig.sess.periodic_images(rig.ia, reach=8.0, cell=cell)
        with pytest.raises(ValueError, match="reach"):
            rig.sess.periodic_images(rig.a, reach=8.0, cell=[[30.0, 0.0, 0.0], [29.0, 7.0, 0.0], [0.0, 0.0, 30.0]])
        with pytest.raises(ValueError, match="box or a cell"):
            rig.sess.periodic_images(rig.a, L32, 8.0, cell=cell)
        # the other family's update
        with pytest.raises(ValueError, match="cells"):
            rig.sess.update_images(rig.ia, rig.a, L32)
        with pytest.raises(ValueError, match="boxes"):
            rig.sess.update_images(rig.ib, rig.b, cell=cell)
        rig.score(pairs, 8.0)  # (still usable)
        rig.sess.set_coords(rig.a, a[0] + 1.0)  # the source moves, the image cloud follows on request
        rig.sess.update_images(rig.ia, rig.a, cell=cell)
        got = rig.coords(rig.ia)
        check_wrapped(got[:70], a[0] + 1.0, cell)
        assert np.array_equal(got, image_cloud_cell(got[:70], cell, 8.0))
    finally:
        rig.close()


# ------------------------------------------------------------------------------------------------------------------------
# 9: trajectories
# ------------------------------------------------------------------------------------------------------------------------
def test_score_trajectory_with_cells(lh, torch, oracle):
    """The dodecahedron scaled by up to +- 2 % per frame (NPT), 7 frames of 60 atoms, chunk = 3: two chunk boundaries and a last
    chunk of one frame; the reference in the unscaled cell.  Against the oracle frame by frame, the wrapped originals of every frame
    read from an image cloud of that frame alone (the same kernel on the same numbers)."""
    from loco_hd_amd.device import DeviceSession

    rng = np.random.default_rng(59)
    n, thr, n_frames = 60, 8.0, 7
    ref_cell = CELLS["dodecahedron"]
    cells = np.stack([ref_cell * s for s in (1.0, 1.02, 0.98, 1.01, 0.99, 1.015, 0.985)])
    ref = cloud_in(rng, n, ref_cell)
    frames = np.stack([rng.uniform(-0.5, 1.5, (n, 3)) @ cells[f] for f in range(n_frames)])  # (not wrapped)
    lp = np.stack([np.arange(n), rng.permutation(n)], 1)
    o = make(oracle, "kumaraswamy")
    sess = DeviceSession(make(lh, "kumaraswamy"), interner={})
    try:
        rc = sess.upload(*ref)

        def wrapped(cl, x, cell):
            img = sess.periodic_images(cl, reach=thr, cell=cell)
            from loco_hd_amd import _native as N
            p = sess.coords_of(img, int(N.lib().lchd_cloud_size(img)))[:n]
            check_wrapped(p, x, cell)
            return replicate_cell(p, cell), np.tile(ref[1], 27), np.tile(ref[2], 27)
        rep_ref = wrapped(rc, ref[0], ref_cell)
        want = np.stack([o.from_arrays(*rep_ref, *wrapped(sess.upload(frames[f], ref[1], ref[2]), frames[f], cells[f]), lp, thr, interner={})
                         for f in range(n_frames)])
        held = len(sess._clouds)
        got = sess.score_trajectory(rc, frames, lp, thr, chunk=3, ref_cell=ref_cell, cells=cells)
        check(got.reshape(-1), want.reshape(-1), "trajectory, a cell per frame")
        assert len(sess._clouds) == held  # (buffers and image clouds of the call are gone)
        # one cell for all frames, the reference open
        want_one = np.stack([o.from_arrays(*ref, *wrapped(sess.upload(frames[f], ref[1], ref[2]), frames[f], cells[1]), lp, thr, interner={})
                             for f in range(n_frames)])
        got = sess.score_trajectory(rc, frames, lp, thr, chunk=3, cells=cells[1])
        check(got.reshape(-1), want_one.reshape(-1), "trajectory, one cell")
        assert float(np.max(np.abs(want - want_one))) > 1e-3
        with pytest.raises(ValueError, match="cells"):
            sess.score_trajectory(rc, frames, lp, thr, chunk=3, cells=cells[:3])
        with pytest.raises(ValueError, match="both"):
            sess.score_trajectory(rc, frames, lp, thr, chunk=3, cells=cells, boxes=(30.0, 30.0, 30.0))
    finally:
        sess.close()


# ------------------------------------------------------------------------------------------------------------------------
# 11: a C client
# ------------------------------------------------------------------------------------------------------------------------
C_CLIENT = r"""
/* A plain-C client of lchd_from_primitives_periodic_cell: the numbers of the test that wrote this file, as hexadecimal literals. */
#include <math.h>
#include <stdio.h>

#include "loco_hd_hip.h"

#define CHECK(call)                                                           \
    do {                                                                      \
        int rc_ = (call);                                                     \
        if (rc_ != LCHD_OK) {                                                 \
            fprintf(stderr, "%s -> %d: %s\n", #call, rc_, lchd_last_error()); \
            return 1;                                                         \
        }                                                                     \
    } while (0)

enum { N = @N@ };
static const double cell[9] = {@CELL@};
static const double xyz[N][3] = {@XYZ@};
static const int32_t cat_a[N] = {@CAT_A@}, cat_b[N] = {@CAT_B@}, tag[N] = {@TAG@};

int main(void) {
    lchd_ctx *ctx = NULL;
    CHECK(lchd_ctx_create(-1, &ctx));
    double wf_params[2] = {3.0, 10.0};
    lchd_weight_function wf = {LCHD_WF_UNIFORM, 2, wf_params};
    double weights[5] = {1.0, 1.0, 1.0, 1.0, 1.0};
    lchd_config cfg = {0};
    cfg.n_categories = 5;
    cfg.category_weights = weights;
    cfg.n_weight_functions = 1;
    cfg.weight_functions = &wf;
    cfg.sd_kind = LCHD_SD_HELLINGER;
    cfg.sd_n_params = 1;
    cfg.sd_params[0] = 2.0;
    cfg.tag_mode = 0;
    cfg.tag_accept_same = 0;

    double out[N], self[N];
    int64_t anchors[N][2];
    for (int i = 0; i < N; ++i) { anchors[i][0] = i; anchors[i][1] = (i + 5) % N; }
    CHECK(lchd_from_primitives_periodic_cell(ctx, &cfg, &xyz[0][0], cat_a, tag, N, &xyz[0][0], cat_b, tag, N, &anchors[0][0], NULL, N, @THR@,
                                             cell, cell, out));
    for (int i = 0; i < N; ++i) printf("score %d %.17g\n", i, out[i]);

    /* the same periodic structure on both sides, pair (i, i): identical environments */
    for (int i = 0; i < N; ++i) anchors[i][1] = i;
    CHECK(lchd_from_primitives_periodic_cell(ctx, &cfg, &xyz[0][0], cat_a, tag, N, &xyz[0][0], cat_a, tag, N, &anchors[0][0], NULL, N, @THR@,
                                             cell, cell, self));
    for (int i = 0; i < N; ++i)
        if (!(fabs(self[i]) <= 1e-12)) { fprintf(stderr, "a periodic structure against itself scored %.17g\n", self[i]); return 2; }

    /* one side periodic, the other open (NULL cell) */
    CHECK(lchd_from_primitives_periodic_cell(ctx, &cfg, &xyz[0][0], cat_a, tag, N, &xyz[0][0], cat_a, tag, N, &anchors[0][0], NULL, N, @THR@,
                                             cell, NULL, self));
    double far = 0.0;
    for (int i = 0; i < N; ++i) far = fmax(far, fabs(self[i]));
    if (!(far > 1e-3)) { fprintf(stderr, "the cell made no difference\n"); return 3; }

    /* error paths: a threshold beyond the smallest width, a singular cell, an anchor outside its structure */
    const double flat[9] = {10.0, 0.0, 0.0, 0.0, 10.0, 0.0, 10.0, 10.0, 0.0};
    if (lchd_from_primitives_periodic_cell(ctx, &cfg, &xyz[0][0], cat_a, tag, N, &xyz[0][0], cat_a, tag, N, &anchors[0][0], NULL, N, 22.0, cell,
                                           cell, self) != LCHD_EVALUE) { fprintf(stderr, "expected LCHD_EVALUE beyond the smallest width\n"); return 4; }
    if (lchd_cell_validate(flat, 1, 1.0) != LCHD_EVALUE || lchd_cell_validate(cell, 1, 21.0) != LCHD_OK) { fprintf(stderr, "lchd_cell_validate\n"); return 5; }
    anchors[3][1] = N; /* a ghost atom of the image cloud, not an atom of the structure */
    if (lchd_from_primitives_periodic_cell(ctx, &cfg, &xyz[0][0], cat_a, tag, N, &xyz[0][0], cat_a, tag, N, &anchors[0][0], NULL, N, @THR@, cell,
                                           cell, self) != LCHD_EPANIC) { fprintf(stderr, "expected LCHD_EPANIC for an anchor beyond the structure\n"); return 6; }
    lchd_ctx_destroy(ctx);
    printf("cabi periodic cell ok\n");
    return 0;
}
"""


def test_c_client_of_the_periodic_cell_entry_point(lh, torch, oracle, tmp_path):
    if shutil.which("gcc") is None:
        pytest.fail("gcc is needed to build the C client")
    cell = CELLS["dodecahedron"]
    rng = np.random.default_rng(61)
    n, thr = 48, 9.0
    x, ca, tag = cloud_in(rng, n, cell, n_tag=16)
    cb = ((3 * ca + 1) % 5).astype(np.int32)

    def hexes(v):
        return ", ".join(float(t).hex() for t in np.asarray(v, dtype=np.float64).reshape(-1))
    text = C_CLIENT
    for key, val in (("N", str(n)), ("CELL", hexes(cell)), ("XYZ", ", ".join("{" + hexes(row) + "}" for row in x)), ("CAT_A", ", ".join(map(str, ca))), ("CAT_B", ", ".join(map(str, cb))),
                     ("TAG", ", ".join(map(str, tag))), ("THR", float(thr).hex())):
        text = text.replace(f"@{key}@", val)
    src, exe = tmp_path / "cabi_periodic_cell.c", tmp_path / "cabi_periodic_cell"
    src.write_text(text)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe),
                           "-L", str(ROOT / "loco_hd_amd"), "-lloco_hd_hip", "-lm", f"-Wl,-rpath,{ROOT / 'loco_hd_amd'}"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    assert "cabi periodic cell ok" in out.stdout
    got = np.asarray([float(ln.split()[2]) for ln in out.stdout.splitlines() if ln.startswith("score ")])
    pairs = np.stack([np.arange(n), (np.arange(n) + 5) % n], 1)
    rig = CellRig(lh, torch, make(lh, cats=CATS, accept_same=False), (x, ca, tag), (x, cb, tag), ("cell", cell), ("cell", cell), thr)
    try:
        want, _ = rig.want(make(oracle, cats=CATS, accept_same=False), pairs, thr)
    finally:
        rig.close()
    check(got, want, "C client")


# ------------------------------------------------------------------------------------------------------------------------
# 12: the command line
# ------------------------------------------------------------------------------------------------------------------------
def test_cli_periodic_cell_end_to_end(lh, torch, oracle, tmp_path, capsys):
    """`python -m loco_hd_amd --periodic-cell` on two small PDB texts with a monoclinic CRYST1 record, against the oracle chain
    (independent reader -> loop-for-loop assigner -> replicated system -> C oracle)."""
    from loco_hd_amd import __main__ as cli
    from loco_hd_amd.device import DeviceSession
    from oracle import atom_converter_oracle as aco
    from tests import pdb_util

    cryst1 = "CRYST1   27.500   28.250   26.000  90.00 101.50  90.00 P 1           1"  # (about the size of the structures: images matter)
    cell = lh.cell_from_lengths_angles(27.5, 28.25, 26.0, 90.0, 101.5, 90.0)
    scheme = pdb_util.write_scheme(tmp_path / "scheme.json")
    texts = []
    for k, seed in enumerate((71, 72)):
        lines = pdb_util.synthetic_pdb(seed=seed, n_res=14, chains="A", box=25.0, altlocs=False).split("\n")
        texts.append("\n".join(lines[:1] + [cryst1] + lines[1:]))
        (tmp_path / f"s{k + 1}.pdb").write_text(texts[-1])
    types = lh.PrimitiveAssigner(scheme).all_primitive_types
    sides = []
    for text, sid in zip(texts, ("s1", "s2")):
        templates = aco.assign_primitive_structure(aco.load_scheme(scheme), aco.read_pdb(text, sid)[0])
        ident = [f"{fid[2]}/{fid[3][1]}-{resname}/{','.join(names)}" for _t, _c, (fid, resname, names) in templates]
        sides.append((templates, ident))
    rng = np.random.default_rng(0)
    picks = [(int(a), int(b)) for a, b in zip(rng.integers(0, len(sides[0][0]), 10), rng.integers(0, len(sides[1][0]), 10))]
    entries = [f"{sides[0][1][a]}:{sides[1][1][b]}" for a, b in picks]
    last = [{name: k for k, name in enumerate(ident)} for _, ident in sides]  # (a repeated id keeps its last index, as in the CLI)
    picks = [(last[0][sides[0][1][a]], last[1][sides[1][1][b]]) for a, b in picks]
    (tmp_path / "pairs.txt").write_text(";\n".join(entries))
    argv = ["-s1", str(tmp_path / "s1.pdb"), "-s2", str(tmp_path / "s2.pdb"), "-pts", str(scheme), "-apf", str(tmp_path / "pairs.txt"),
            "--periodic-cell"]
    assert cli.main(argv) == 0
    got = capsys.readouterr().out.splitlines()
    # the oracle on the replicated systems (wrapped originals from the device)
    sess = DeviceSession(lh.LoCoHD(types), interner={})
    try:
        prims = []
        for templates, _ in sides:
            x = np.asarray([c for _t, c, _s in templates], dtype=np.float64)
            from loco_hd_amd import _native as N
            img = sess.periodic_images(sess.upload(x, np.zeros(len(x), dtype=np.int32)), reach=10.0, cell=cell)
            p = sess.coords_of(img, int(N.lib().lchd_cloud_size(img)))[:len(x)]
            check_wrapped(p, x, cell)
            rep = replicate_cell(p, cell)
            prims.append([oracle.PrimitiveAtom(t[0], f"{t[2][0][2]}/{t[2][0][3][1]}-{t[2][1]}", c) for t, c in zip(list(templates) * 27, rep)])
    finally:
        sess.close()
    o = oracle.LoCoHD(types, oracle.WeightFunction("uniform", [3.0, 10.0]), oracle.TagPairingRule({"accept_same": False}))
    want = o.from_primitives(prims[0], prims[1], picks, 10.0)
    want_open = aco.cli_lines(texts[0], texts[1], scheme, ";\n".join(entries), types)
    assert len(got) == len(want) == len(entries)
    for g, w, e in zip(got, want, entries):
        assert g.startswith(f"LoCoHD({e}) = ")
        assert abs(float(g.split(" = ")[1]) - w) < TIGHT
    assert max(abs(float(g.split(" = ")[1]) - float(w.split(" = ")[1])) for g, w in zip(got, want_open)) > 1e-3  # the cell matters
    with pytest.raises(SystemExit, match="orthorhombic"):  # --periodic still refuses this cell
        cli.main(argv[:-1] + ["--periodic"])
