"""Minimum-image periodic boundaries of the dense calls: LoCoHD.from_coords(box_a= / cell_a= ...), from_coords_ensemble(boxes= / cells=)
and their DeviceSession forms (lchd_from_coords_periodic*, lchd_ensemble_from_coords_periodic*; the row producers k_min_image_rows of
loco_hd_amd/csrc/lchd_ensemble.hip in front of the given-row sorts and sweeps).  Every periodic call is compared with from_dmxs on the
minimum-image matrices numpy builds in the arithmetic the header prescribes (1e-13: two device paths on the same rows) and, on sampled
rows, with the CPU oracle's from_anchors on rows found by brute force over the shifts of the ORIGINAL cell (1e-11)."""
import numpy as np
import pytest

from dense_rows_util import oracle_rows
from min_image_util import brute_rows, min_image_matrix
from periodic_cell_util import CELLS

pytestmark = pytest.mark.gpu

TIGHT = 1e-11   # against the oracle
SAME = 1e-13    # between two device paths
NAMES = [f"c{i}" for i in range(300)]
WF = ("hyper_exp", [1.0, 0.1])

# n, categories, statistical distance, the row kernel the shape reaches
SHAPES = {
    "a-fused": (1025, 5, None),
    "b-rows2": (300, 5, None),
    "c-rows-cat16": (300, 300, None),
    "d-kl": (1025, 5, ("Kullback-Leibler", [1e-10])),
}
GEOMETRIES = ["box", "skewed", "dodecahedron"]


@pytest.fixture(scope="module")
def lh():
    import loco_hd_amd

    return loco_hd_amd


def reduce(cell):
    from loco_hd_amd.api import cell_reduce

    return cell_reduce(cell)


def build(mod, n_cat, sd=None, **kw):
    if sd is not None:
        kw["statistical_distance"] = mod.StatisticalDistance(*sd)
    return mod.LoCoHD(NAMES[:n_cat], mod.WeightFunction(*WF), **kw)


def fused_flag(lchd):
    from loco_hd_amd import _native as N

    return int(N.lib().lchd_ctx_last_dense_fused(lchd._context()))


def geometry(rng, name, n):
    """(keyword for side A / B, the cell as a 3 x 3 matrix, coordinates of two structures)."""
    if name == "box":
        side = (n / 0.05) ** (1 / 3)
        box = np.asarray([side, 0.9 * side, 1.1 * side])
        xa, xb = rng.uniform(0.0, 1.0, (n, 3)) * box, rng.uniform(0.0, 1.0, (n, 3)) * box  # every atom inside the box
        return {"box_a": box, "box_b": box}, np.diag(box), xa, xb
    cell = CELLS[name]
    xa, xb = rng.uniform(-2.0, 2.0, (n, 3)) @ cell, rng.uniform(-2.0, 2.0, (n, 3)) @ cell  # spread over +-2 cells, unwrapped
    return {"cell_a": cell, "cell_b": cell}, cell, xa, xb


def matrix(x, cell):
    return min_image_matrix(x, cell=cell, reduce=reduce)


@pytest.mark.parametrize("geo", GEOMETRIES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_periodic_from_coords_against_given_rows_and_oracle(lh, oracle, shape, geo):
    n, n_cat, sd = SHAPES[shape]
    rng = np.random.default_rng(100 * list(SHAPES).index(shape) + GEOMETRIES.index(geo))
    kw, cell, xa, xb = geometry(rng, geo, n)
    sa, sb = [NAMES[k] for k in rng.integers(0, n_cat, n)], [NAMES[k] for k in rng.integers(0, n_cat, n)]
    lchd = build(lh, n_cat, sd)
    got = np.asarray(lchd.from_coords(sa, sb, xa, xb, **kw))
    if shape == "a-fused":
        assert fused_flag(lchd) == 1
    elif shape == "d-kl":
        assert fused_flag(lchd) == 0
    assert np.all(np.isfinite(got)) and got.min() >= 0.0
    ma, mb = matrix(xa, cell), matrix(xb, cell)
    assert np.all(np.diagonal(ma) == 0.0) and np.all(np.diagonal(mb) == 0.0)
    given = np.asarray(lchd.from_dmxs(sa, sb, ma, mb))
    print(shape, geo, "periodic from_coords vs from_dmxs on the numpy rows:", np.max(np.abs(got - given)))
    assert np.max(np.abs(got - given)) <= SAME
    rows = sorted(set(rng.integers(0, n, 24).tolist()) | {0, n - 1})
    want = oracle_rows(build(oracle, n_cat, sd), sa, sb, brute_rows(xa, rows, cell), brute_rows(xb, rows, cell))
    print(shape, geo, "vs the oracle on brute-force rows:", np.max(np.abs(got[rows] - want)))
    assert np.max(np.abs(got[rows] - want)) <= TIGHT
    # ... and the periodic rows are not the open ones
    assert np.max(np.abs(got - np.asarray(lchd.from_coords(sa, sb, xa, xb)))) > 1e-3


@pytest.fixture(scope="module")
def small(lh):
    """One 300-atom pair in the skewed cell, shared by the property tests below."""
    rng = np.random.default_rng(7)
    n, n_cat = 300, 6
    cell = CELLS["skewed"]
    xa, xb = rng.uniform(-2.0, 2.0, (n, 3)) @ cell, rng.uniform(-2.0, 2.0, (n, 3)) @ cell
    sa, sb = [NAMES[k] for k in rng.integers(0, n_cat, n)], [NAMES[k] for k in rng.integers(0, n_cat, n)]
    lchd = build(lh, n_cat)
    return dict(n=n, n_cat=n_cat, cell=cell, xa=xa, xb=xb, sa=sa, sb=sb, lchd=lchd, rng=rng,
                got=np.asarray(lchd.from_coords(sa, sb, xa, xb, cell_a=cell, cell_b=cell)))


def test_lattice_invariance(small):
    s = small
    shift_a = s["rng"].integers(-3, 4, (s["n"], 3)).astype(float) @ s["cell"]
    shift_b = s["rng"].integers(-3, 4, (s["n"], 3)).astype(float) @ s["cell"]
    moved = np.asarray(s["lchd"].from_coords(s["sa"], s["sb"], s["xa"] + shift_a, s["xb"] + shift_b, cell_a=s["cell"], cell_b=s["cell"]))
    print("lattice invariance:", np.max(np.abs(moved - s["got"])))
    assert np.max(np.abs(moved - s["got"])) <= TIGHT


def test_box_and_diagonal_cell_are_bit_equal(lh):
    rng = np.random.default_rng(8)
    for n, n_cat in ((300, 6), (1025, 5)):  # k_env_rows2, k_dense_fused
        box = np.asarray([21.5, 19.25, 24.0])
        xa, xb = rng.uniform(-30.0, 50.0, (n, 3)), rng.uniform(-30.0, 50.0, (n, 3))
        sa, sb = [NAMES[k] for k in rng.integers(0, n_cat, n)], [NAMES[k] for k in rng.integers(0, n_cat, n)]
        lchd = build(lh, n_cat)
        with_box = np.asarray(lchd.from_coords(sa, sb, xa, xb, box_a=box, box_b=box))
        with_cell = np.asarray(lchd.from_coords(sa, sb, xa, xb, cell_a=np.diag(box), cell_b=np.diag(box)))
        assert np.array_equal(with_box, with_cell)
        mixed = np.asarray(lchd.from_coords(sa, sb, xa, xb, box_a=box, cell_b=np.diag(box)))
        assert np.array_equal(with_box, mixed)


def test_open_side_keeps_the_rows_of_the_open_call(small):
    """box_a with an open side B: side B's rows are the open call's -- the call equals from_dmxs on (minimum-image A, open B), and with the
    same periodic structure on both sides of a second call only side B's openness makes a difference."""
    s = small
    box = np.asarray([23.0, 26.5, 22.0])
    d = s["xb"][:, None, :] - s["xb"][None, :, :]
    open_b = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])  # utils.rs:1-8 order
    half = np.asarray(s["lchd"].from_coords(s["sa"], s["sb"], s["xa"], s["xb"], box_a=box))
    want = np.asarray(s["lchd"].from_dmxs(s["sa"], s["sb"], min_image_matrix(s["xa"], box=box), open_b))
    assert np.max(np.abs(half - want)) <= SAME
    # open on BOTH sides through the periodic route is the open call (side A open, side B open: no producer runs)
    other = np.asarray(s["lchd"].from_coords(s["sb"], s["sa"], s["xb"], s["xa"], box_b=box))  # sides swapped: B periodic, A open
    want2 = np.asarray(s["lchd"].from_dmxs(s["sb"], s["sa"], open_b, min_image_matrix(s["xa"], box=box)))
    assert np.max(np.abs(other - want2)) <= SAME


def test_default_call_is_unchanged(lh, small):
    s = small
    det = build(lh, s["n_cat"], deterministic=True)
    plain = np.asarray(det.from_coords(s["sa"], s["sb"], s["xa"], s["xb"]))
    periodic = det.from_coords(s["sa"], s["sb"], s["xa"], s["xb"], cell_a=s["cell"])  # a periodic call in between leaves no trace
    assert len(periodic) == s["n"]
    assert np.array_equal(plain, np.asarray(det.from_coords(s["sa"], s["sb"], s["xa"], s["xb"])))
    assert np.array_equal(plain, np.asarray(det.from_coords(s["sa"], s["sb"], s["xa"], s["xb"], box_a=None, cell_b=None)))
    m = 3
    xs = np.stack([s["xa"], s["xb"], s["xa"][::-1]])
    ens = det.from_coords_ensemble(s["sa"], xs)
    det.from_coords_ensemble(s["sa"], xs, cells=s["cell"])
    assert np.array_equal(ens, det.from_coords_ensemble(s["sa"], xs))
    assert np.array_equal(ens, det.from_coords_ensemble(s["sa"], xs, boxes=None, cells=None))
    assert ens.shape == (m * (m - 1) // 2, s["n"])


@pytest.mark.parametrize("geo", ["box", "dodecahedron"])
def test_atoms_on_the_minimum_image_surface_and_a_lattice_vector_apart(lh, oracle, geo):
    """An atom exactly half a box edge / half a lattice vector from another (two images tie), and two atoms one lattice vector apart
    (distance 0: a tie with the row's own atom)."""
    rng = np.random.default_rng(9)
    n, n_cat = 300, 6
    if geo == "box":
        cell = np.diag([24.0, 20.0, 28.0])
        kw = {"box_a": np.diagonal(cell).copy(), "box_b": np.diagonal(cell).copy()}
    else:
        cell = CELLS[geo]
        kw = {"cell_a": cell, "cell_b": cell}
    xa, xb = rng.uniform(-1.0, 1.0, (n, 3)) @ cell, rng.uniform(-1.0, 1.0, (n, 3)) @ cell
    xa[1] = xa[0] + 0.5 * cell[0]              # on the surface: +a/2 and -a/2 tie
    xa[2] = xa[0] + cell[1]                    # one lattice vector apart
    xb[n - 2] = xb[n - 1] - 0.5 * cell[2]
    xb[n - 3] = xb[n - 1] + cell[0] - cell[2]
    sa, sb = [NAMES[k] for k in rng.integers(0, n_cat, n)], [NAMES[k] for k in rng.integers(0, n_cat, n)]
    lchd = build(lh, n_cat)
    got = np.asarray(lchd.from_coords(sa, sb, xa, xb, **kw))
    assert np.all(np.isfinite(got)) and got.min() >= 0.0 and got.max() <= 1.0
    rows = [0, 1, 2, n - 3, n - 2, n - 1] + rng.integers(3, n - 3, 18).tolist()
    want = oracle_rows(build(oracle, n_cat), sa, sb, brute_rows(xa, rows, cell), brute_rows(xb, rows, cell))
    print("surface atoms,", geo, ":", np.max(np.abs(got[rows] - want)))
    assert np.max(np.abs(got[rows] - want)) <= TIGHT


# ---- ensembles ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def npt():
    """M = 4 structures of 300 atoms, one cell per structure with a volume of its own (NPT)."""
    rng = np.random.default_rng(21)
    m, n, n_cat = 4, 300, 6
    cells = np.stack([CELLS["skewed"] * s for s in (1.0, 1.03, 0.96, 1.1)])
    frac = rng.uniform(-2.0, 2.0, (n, 3))
    xs = np.stack([(frac + rng.normal(0.0, 0.02, (n, 3))) @ cells[k] for k in range(m)])
    seq = [NAMES[k] for k in rng.integers(0, n_cat, n)]
    excluded = [(r, c) for r in range(0, n, 7) for c in (r + 1, r + 2) if c < n]
    excluded += [(c, r) for r, c in excluded]
    return dict(m=m, n=n, n_cat=n_cat, cells=cells, xs=xs, seq=seq, excluded=excluded)


def all_pairs(m):
    return [(i, j) for i in range(m) for j in range(i + 1, m)]


def test_ensemble_with_a_cell_per_structure(lh, npt, monkeypatch):
    e = npt
    det = build(lh, e["n_cat"], deterministic=True)
    got = det.from_coords_ensemble(e["seq"], e["xs"], cells=e["cells"])
    assert got.shape == (6, e["n"])
    for p, (i, j) in enumerate(all_pairs(e["m"])):  # bit for bit the per-pair periodic calls
        assert np.array_equal(got[p], np.asarray(det.from_coords(e["seq"], e["seq"], e["xs"][i], e["xs"][j], cell_a=e["cells"][i], cell_b=e["cells"][j])))
    mats = np.stack([min_image_matrix(e["xs"][k], cell=e["cells"][k], reduce=reduce) for k in range(e["m"])])
    given = det.from_dmxs_ensemble(e["seq"], mats)
    print("ensemble vs from_dmxs_ensemble on the numpy rows:", np.max(np.abs(got - given)))
    assert np.max(np.abs(got - given)) <= SAME
    # excluded pairs on top of the minimum-image rows
    banned = det.from_coords_ensemble(e["seq"], e["xs"], cells=e["cells"], excluded_pairs=e["excluded"])
    for r, c in e["excluded"]:
        mats[:, r, c] = np.inf
    given_banned = det.from_dmxs_ensemble(e["seq"], mats)
    assert np.max(np.abs(banned - given_banned)) <= SAME
    assert np.max(np.abs(banned - got)) > 1e-6
    # blocks of one structure: rows rebuilt per block pair
    monkeypatch.setenv("LCHD_ENSEMBLE_BLOCK", "2")
    blocked = build(lh, e["n_cat"], deterministic=True)
    assert np.array_equal(blocked.from_coords_ensemble(e["seq"], e["xs"], cells=e["cells"]), got)
    assert np.array_equal(blocked.from_coords_ensemble(e["seq"], e["xs"], cells=e["cells"], excluded_pairs=e["excluded"]), banned)
    pairs = [(3, 0), (1, 1), (2, 3)]
    some = blocked.from_coords_ensemble(e["seq"], e["xs"], structure_pairs=pairs, cells=e["cells"])
    assert np.array_equal(some[0], np.asarray(det.from_coords(e["seq"], e["seq"], e["xs"][3], e["xs"][0], cell_a=e["cells"][3], cell_b=e["cells"][0])))
    assert np.all(some[1] == 0.0)


def test_ensemble_with_one_box_and_mixed_cells(lh, npt):
    """One box for all structures (the orthorhombic producer), and a cell per structure of which some are diagonal (the cell
    producer's per-row choice): both equal the per-pair calls bit for bit."""
    e = npt
    det = build(lh, e["n_cat"], deterministic=True)
    box = np.asarray([22.0, 25.0, 19.5])
    got = det.from_coords_ensemble(e["seq"], e["xs"][:3], boxes=box)
    for p, (i, j) in enumerate(all_pairs(3)):
        assert np.array_equal(got[p], np.asarray(det.from_coords(e["seq"], e["seq"], e["xs"][i], e["xs"][j], box_a=box, box_b=box)))
    cells = np.stack([np.diag(box), e["cells"][1], np.diag(1.1 * box)])
    mixed = det.from_coords_ensemble(e["seq"], e["xs"][:3], cells=cells)
    for p, (i, j) in enumerate(all_pairs(3)):
        assert np.array_equal(mixed[p], np.asarray(det.from_coords(e["seq"], e["seq"], e["xs"][i], e["xs"][j], cell_a=cells[i], cell_b=cells[j])))


def test_device_session_frames_buffer_and_pair(lh, npt):
    from loco_hd_amd.device import DeviceSession

    e = npt
    det = build(lh, e["n_cat"], deterministic=True)
    want = det.from_coords_ensemble(e["seq"], e["xs"], cells=e["cells"])
    banned = det.from_coords_ensemble(e["seq"], e["xs"], cells=e["cells"], excluded_pairs=e["excluded"])
    sess = DeviceSession(det)
    try:
        cat = det._cats(e["seq"])
        tmpl = sess.upload(e["xs"][0], cat)
        buf = sess.frames_buffer(tmpl, e["m"])
        sess.load_frames(buf, e["xs"])
        assert np.array_equal(sess.from_coords_ensemble(buf, cells=e["cells"]).cpu().numpy(), want)
        assert np.array_equal(sess.from_coords_ensemble(buf, cells=e["cells"], excluded=e["excluded"]).cpu().numpy(), banned)
        batch, _ = sess.upload_batch([(x, cat) for x in e["xs"]])
        assert np.array_equal(sess.from_coords_ensemble(batch, cells=e["cells"]).cpu().numpy(), want)
        one = det.from_coords_ensemble(e["seq"], e["xs"], cells=e["cells"][2])
        assert np.array_equal(sess.from_coords_ensemble(batch, cells=e["cells"][2]).cpu().numpy(), one)
        # a single pair on uploaded structures
        a, b = sess.upload(e["xs"][0], cat), sess.upload(e["xs"][1], cat)
        pair = sess.from_coords(a, b, cell_a=e["cells"][0], cell_b=e["cells"][1]).cpu().numpy()
        assert np.array_equal(pair, want[0])
        plain = sess.from_coords(a, b).cpu().numpy()
        assert np.array_equal(plain, np.asarray(det.from_coords(e["seq"], e["seq"], e["xs"][0], e["xs"][1])))
        with pytest.raises(ValueError, match="both given"):
            sess.from_coords(a, b, box_a=[20.0, 20.0, 20.0], cell_a=e["cells"][0])
        with pytest.raises(ValueError, match="both given"):
            sess.from_coords_ensemble(batch, boxes=[20.0, 20.0, 20.0], cells=e["cells"])
        with pytest.raises(ValueError, match="3 cells given for 4 structures"):
            sess.from_coords_ensemble(batch, cells=e["cells"][:3])
        with pytest.raises(ValueError):
            sess.from_coords(batch, batch, box_a=[20.0, 20.0, 20.0])  # a batch is not a single structure
        assert np.array_equal(sess.from_coords(a, b, cell_a=e["cells"][0], cell_b=e["cells"][1]).cpu().numpy(), want[0])
    finally:
        sess.close()


def test_errors(lh, small):
    s = small
    lchd, sa, sb, xa, xb, cell = s["lchd"], s["sa"], s["sb"], s["xa"], s["xb"], s["cell"]
    box = [20.0, 21.0, 22.0]
    with pytest.raises(ValueError, match="box_a and cell_a were both given"):
        lchd.from_coords(sa, sb, xa, xb, box_a=box, cell_a=cell)
    with pytest.raises(ValueError, match="box_b and cell_b were both given"):
        lchd.from_coords(sa, sb, xa, xb, box_b=box, cell_b=cell)
    with pytest.raises(ValueError, match="boxes and cells were both given"):
        lchd.from_coords_ensemble(sa, [xa, xb], boxes=box, cells=cell)
    for bad in ([20.0, 21.0], [[20.0, 21.0, 22.0]] * 2, [20.0, -1.0, 22.0], [20.0, np.nan, 22.0]):  # wrong shapes, bad edges
        with pytest.raises(ValueError):
            lchd.from_coords(sa, sb, xa, xb, box_a=bad)
    with pytest.raises(ValueError, match="shape"):
        lchd.from_coords(sa, sb, xa, xb, cell_b=np.zeros((3, 2)))
    with pytest.raises(ValueError, match="3 cells given for 2 structures"):
        lchd.from_coords_ensemble(sa, [xa, xb], cells=[cell] * 3)
    singular = np.array(cell)
    singular[2] = singular[0] - 2.0 * singular[1]
    with pytest.raises(ValueError, match="singular"):
        lchd.from_coords(sa, sb, xa, xb, cell_a=singular)
    with pytest.raises(ValueError, match="singular"):
        lchd.from_coords_ensemble(sa, [xa, xb], cells=[cell, singular])
    nan = np.array(xb)
    nan[5, 1] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        lchd.from_coords(sa, sb, xa, nan, cell_a=cell, cell_b=cell)
    with pytest.raises(ValueError, match="non-finite"):
        lchd.from_coords_ensemble(sa, [xa, nan], cells=cell)
    with pytest.raises(ValueError, match="same length"):
        lchd.from_coords(sa, sb, xa, xb[:-1], cell_a=cell)
    group = lh.LoCoHD(NAMES[:s["n_cat"]], lh.WeightFunction(*WF), devices=[0])
    with pytest.raises(ValueError, match="drop devices"):
        group.from_coords(sa, sb, xa, xb, box_a=box)
    with pytest.raises(ValueError, match="drop devices"):
        group.from_coords_ensemble(sa, [xa, xb], cells=cell)
    # the context is usable after every refusal
    assert np.max(np.abs(np.asarray(lchd.from_coords(sa, sb, xa, xb, cell_a=cell, cell_b=cell)) - s["got"])) <= SAME
