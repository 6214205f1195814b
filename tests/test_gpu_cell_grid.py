"""Every thresholded call buckets its atoms into a uniform grid planned on the host (lchd_plan_grid) and built by one of four
cell-list builds (loco_hd_amd/csrc/lchd_prologue.hip); k_env_group (reach 2) and k_env_cells (reach 1) then read the neighbour
cells with geometric pruning.  A wrong cell list or an eager pruning test drops points from environments and leaves plausible
scores.  Each case here puts the grid at one of the planner's or the builds' limits, ASSERTS through DeviceSession.last_grid()
that the limit was reached, and compares the scores with the CPU oracle and the environment sizes with a brute-force count
(reference: env_from_idx, /root/reference/src/locohd.rs:514-542: every point with d^2 < thr^2).

Clouds are made of small blobs (about 25 points within a threshold of each other) scattered over a box whose extent is pinned
by two corner atoms, so a grid of millions of cells still has environments of tens of points.  Every cloud also carries one
clump of more than 512 points inside one threshold.  A call scores two pair lists: anchors with at most 300 neighbours (one pass
of the kernel under test: k_env_group by default, k_env_cells under LCHD_NO_ENV_GROUP=1), then anchors inside the clump -- every
environment overflows the 512-point slots, the whole pass is repeated with 1024-point slots, and that is k_env_cells on the
reach-1 grid of the same cloud.  (k_env_collect takes environments of more than 16 384 points only: beyond the "few thousand
atoms" of these cases; tests/test_gpu_env_kernels.py runs it with a 20 000-point cluster.)"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TIGHT = 1e-11
CATS = ["A", "B", "C", "D", "E"]
WF = ("hyper_exp", [1.0, 0.3])
THR = 4.0
ORIGIN = np.array([-37.25, 12.5, 3.0])  # (exactly representable: a shifted lattice stays a lattice)
STRUCT_CELLS, SCAN_CELLS, MAX_CELLS = 4096, 1 << 16, 1 << 23  # kStructCellsMax, kPrepScanCells, the planner's bound
N_PAIRS = 300
FUSED, PER_STRUCT, GENERAL, GENERAL_MULTI = 1, 2, 3, 4  # lchd_ctx_last_grid build codes (0: shared with side A)


@pytest.fixture(scope="module")
def lh():
    import loco_hd_amd

    return loco_hd_amd


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def blob_cloud(seed, ext, thr, n_blobs, pin_ext=None, n_clump=600, per_blob=25, origin=ORIGIN):
    """[2 corner atoms][n_blobs blobs of per_blob points][a clump of n_clump points] inside [0, ext]^3 (+ origin).  An axis of
    extent 0 stays flat.  pin_ext: where the second corner atom sits (the first is at 0), default ext."""
    rng = np.random.default_rng(seed)
    ext = np.asarray(ext, dtype=np.float64)
    live = ext > 0.0
    clump_c = ext * rng.uniform(0.3, 0.7, 3)
    centres = []
    while len(centres) < n_blobs:
        c = ext * rng.uniform(0.0, 1.0, 3)
        if np.linalg.norm(c - clump_c) > 3.5 * thr:
            centres.append(c)
    centres = np.repeat(np.asarray(centres), per_blob, axis=0)
    blobs = centres + rng.normal(0.0, 1.0, centres.shape) * np.where(live, 0.3 * thr, 0.0)
    v = rng.normal(0.0, 1.0, (n_clump, 3)) * live
    v /= np.linalg.norm(v, axis=1)[:, None]
    clump = clump_c + v * 0.45 * thr * rng.uniform(0.0, 1.0, (n_clump, 1)) ** (1.0 / max(int(live.sum()), 1))
    pins = np.stack([np.zeros(3), ext if pin_ext is None else np.asarray(pin_ext, dtype=np.float64)])
    xyz = np.concatenate([pins, np.clip(np.concatenate([blobs, clump]), 0.0, ext)]) + origin  # (clipped points sit ON the box's faces)
    return xyz, rng.integers(0, len(CATS), len(xyz)).astype(np.int32)


def lattice_cloud(seed, n_keep=3300):
    """Integer lattice 0 .. 16 per axis (+ an integer origin), thinned to n_keep points with the 8 corners first, and a clump of
    9^3 points on a lattice of spacing 1/8 inside one unit cube: every coordinate and every squared distance is exact."""
    rng = np.random.default_rng(seed)
    g = np.arange(17, dtype=np.float64)
    full = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    corner = np.all((full == 0.0) | (full == 16.0), axis=1)
    rest = full[~corner]
    body = rest[rng.choice(len(rest), n_keep - 8, replace=False)]
    f = (np.arange(9, dtype=np.float64) + 0.5) / 8.0
    clump = np.array([4.0, 9.0, 6.0]) + np.stack(np.meshgrid(f, f, f, indexing="ij"), -1).reshape(-1, 3)
    xyz = np.concatenate([full[corner], body, clump]) + np.array([-8.0, 32.0, 5.0])
    return xyz, rng.integers(0, len(CATS), len(xyz)).astype(np.int32)


def brute_env_sizes(xyz, sid, thr):
    """Points of every atom's environment: same structure, d^2 < thr^2 with d^2 summed in the kernels' order (x, y, z)."""
    n, thr2 = len(xyz), np.float64(thr) * np.float64(thr)
    out = np.zeros(n, dtype=np.int64)
    for i0 in range(0, n, 512):
        d = xyz[i0:i0 + 512, None, :] - xyz[None, :, :]
        d2 = d[..., 0] * d[..., 0]
        d2 = d2 + d[..., 1] * d[..., 1]
        d2 = d2 + d[..., 2] * d[..., 2]
        out[i0:i0 + 512] = np.sum((d2 < thr2) & (sid[i0:i0 + 512, None] == sid[None, :]), axis=1)
    return out


class Side:
    def __init__(self, structures, thr):
        self.structures = structures  # [(xyz, cat)], one entry unless the side is a batch
        self.xyz = np.concatenate([s[0] for s in structures])
        self.cat = np.concatenate([s[1] for s in structures])
        self.sid = np.concatenate([np.full(len(s[0]), k) for k, s in enumerate(structures)])
        self.offsets = np.concatenate([[0], np.cumsum([len(s[0]) for s in structures])])
        self.sizes = brute_env_sizes(self.xyz, self.sid, thr)
        self.bbox = (self.xyz.min(axis=0), self.xyz.max(axis=0))


def pick_pairs(rng, a, b, lo, hi, n_pairs, first=()):
    """n_pairs anchor pairs (global indices) whose environments hold lo < points <= hi on both sides, both anchors in the structure
    of the same number; `first`: local indices (in structure 0) that open the list as (i, i) pairs."""
    pairs = [(int(i), int(i)) for i in first]
    ok_a, ok_b = (a.sizes > lo) & (a.sizes <= hi), (b.sizes > lo) & (b.sizes <= hi)
    structs = [k for k in range(len(a.structures)) if np.any(ok_a & (a.sid == k)) and np.any(ok_b & (b.sid == k))]
    assert structs
    while len(pairs) < n_pairs:
        k = int(rng.choice(structs))
        pairs.append((int(rng.choice(np.flatnonzero(ok_a & (a.sid == k)))), int(rng.choice(np.flatnonzero(ok_b & (b.sid == k))))))
    return np.asarray(pairs, dtype=np.int64)


def cube(reach, cells, thr=THR):
    return tuple((k + 0.5) * thr / reach if k else 0.0 for k in cells)  # (k + 0.5 cells of the minimum width: floor -> k)


def one(seed, reach, cells, pin_cells=None, n_blobs=100):
    return [blob_cloud(seed, cube(reach, cells), THR, n_blobs, None if pin_cells is None else cube(reach, pin_cells))]


def batch(seed, reach, cells, n_struct):
    """n_struct copies of one 10-blob structure, each point moved by a fraction of a cell: every structure's atoms lie within the
    threshold of every other structure's.  The clump is in structure 0 only."""
    rng = np.random.default_rng(seed + 1000)
    ext = np.asarray(cube(reach, cells))
    x0, c0 = blob_cloud(seed, ext, THR, 10)
    out = [(x0, c0)]
    for _ in range(n_struct - 1):
        x = x0[:252].copy()
        x[2:] = np.clip(x[2:] - ORIGIN + rng.normal(0.0, 0.1 * THR, (250, 3)), 0.0, ext) + ORIGIN
        out.append((x, rng.integers(0, len(CATS), 252).astype(np.int32)))
    return out


# name -> (thr, builder(reach) -> (structures A, structures B or None for "the same object"), expected dims per structure,
#          expected (build A, build B), predicate on (cells per structure, cells in all) that names the side of the limit)
CASES = {
    # a. the structure cell-count limit: the same points, the x extent nudged by a corner atom
    "struct_limit_at": (THR, lambda r: (one(1, r, (16, 16, 16)), one(2, r, (16, 16, 16))), (16, 16, 16), (FUSED, FUSED),
                        lambda cps, total: cps == STRUCT_CELLS),
    "struct_limit_above": (THR, lambda r: (one(1, r, (16, 16, 16), (17, 16, 16)), one(2, r, (16, 16, 16), (17, 16, 16))), (17, 16, 16),
                           (GENERAL, GENERAL), lambda cps, total: STRUCT_CELLS < cps == 4352),
    # b. the one-workgroup scan limit: a slab
    "scan_limit_at": (THR, lambda r: (one(3, r, (256, 16, 16), None, 250), one(4, r, (256, 16, 16), None, 250)), (256, 16, 16),
                      (GENERAL, GENERAL), lambda cps, total: total == SCAN_CELLS),
    "scan_limit_above": (THR, lambda r: (one(3, r, (256, 16, 16), (257, 16, 16), 250), one(4, r, (256, 16, 16), (257, 16, 16), 250)),
                         (257, 16, 16), (GENERAL_MULTI, GENERAL_MULTI), lambda cps, total: SCAN_CELLS < total == 65792),
    # c. the per-axis clamp: x cells 1500.5 / 1024 = 1.47 times the minimum width, y and z cells 3.5 / 3 = 1.17 times
    "axis_clamp": (THR, lambda r: (one(5, r, (1500, 3, 3)), one(6, r, (1500, 3, 3))), (1024, 3, 3), (GENERAL, GENERAL),
                   lambda cps, total: cps == 9216),
    # d. coarsening: a sheet that plans as 1024 x 1024 x 16 and has its first axis halved
    "coarsened_sheet": (THR, lambda r: (one(7, r, (1024, 1024, 16)), one(8, r, (1024, 1024, 16))), (512, 1024, 16),
                        (GENERAL_MULTI, GENERAL_MULTI), lambda cps, total: total == MAX_CELLS),
    # e. a batch coarsens where each of its structures alone would not
    "batch_of_8": (THR, lambda r: (batch(9, r, (128, 128, 64), 8), batch(10, r, (128, 128, 64), 8)), (128, 128, 64),
                   (GENERAL_MULTI, GENERAL_MULTI), lambda cps, total: total == MAX_CELLS and cps == 1 << 20),
    "batch_of_9": (THR, lambda r: (batch(9, r, (128, 128, 64), 9), batch(10, r, (128, 128, 64), 9)), (64, 128, 64),
                   (GENERAL_MULTI, GENERAL_MULTI), lambda cps, total: total == 9 << 19),
    # f. mixed sides, both orders, and the large grid as one object on both sides
    "compact_vs_slab": (THR, lambda r: (one(1, r, (16, 16, 16)), one(4, r, (256, 16, 16), (257, 16, 16), 250)), ((16, 16, 16), (257, 16, 16)),
                        (PER_STRUCT, GENERAL_MULTI), lambda cps, total: True),
    "slab_vs_compact": (THR, lambda r: (one(4, r, (256, 16, 16), (257, 16, 16), 250), one(1, r, (16, 16, 16))), ((257, 16, 16), (16, 16, 16)),
                        (GENERAL_MULTI, PER_STRUCT), lambda cps, total: True),
    "slab_vs_itself": (THR, lambda r: (one(4, r, (256, 16, 16), (257, 16, 16), 250), None), (257, 16, 16), (GENERAL_MULTI, 0),
                       lambda cps, total: total > SCAN_CELLS),
    # h. flat and rod-shaped structures on the general build (more than 4096 cells / more than 4096 atoms: no axis can hold more
    #    than 1024 cells, so a rod cannot exceed the cell limit)
    "flat_sheet": (THR, lambda r: (one(11, r, (80, 80, 0)), one(12, r, (80, 80, 0))), (80, 80, 1), (GENERAL, GENERAL),
                   lambda cps, total: cps == 6400 > STRUCT_CELLS),
    "rod": (THR, lambda r: (one(13, r, (1100, 0, 0), None, 160), one(14, r, (1100, 0, 0), None, 160)), (1024, 1, 1), (GENERAL, GENERAL),
            lambda cps, total: cps == 1024),
}
# g. points on cell faces: lattice spacing 1, extent 16.  thr just below 2: reach 2 gives 16 cells of width exactly 1 per axis --
#    inv = 1 / (1 + 1e-12) puts lattice point k at the upper face of cell k - 1 -- and reach 1 gives 8 cells of width 2; thr = 1.88
#    gives 17 / 8 cells.  Lattice distances of exactly 2 are outside both thresholds, sqrt(3) is inside.
LATTICE = {
    "lattice_faces": (1.99999999, {2: (16, 16, 16), 1: (8, 8, 8)}, {2: (FUSED, FUSED), 1: (FUSED, FUSED)}),
    "lattice_17": (1.88, {2: (17, 17, 17), 1: (8, 8, 8)}, {2: (GENERAL, GENERAL), 1: (FUSED, FUSED)}),
}

_built = {}


def build_case(name, reach, oracle):
    """Inputs, pair lists, oracle scores and brute-force environment sizes of one case: built once per module run."""
    if (name, reach) in _built:
        return _built[(name, reach)]
    if name in LATTICE:
        thr, dims, builds = LATTICE[name]
        sa, sb = [lattice_cloud(21)], [lattice_cloud(22)]
        dims, builds, side_of_limit = dims[reach], builds[reach], (lambda cps, total: cps == dims[0] ** 3)
        first = range(8)  # the 8 corners: bbmin / bbmax on every axis
    else:
        thr, make, dims, builds, side_of_limit = CASES[name]
        sa, sb = make(reach)
        first = (0, 1)    # the two corner atoms
    a = Side(sa, thr)
    b = a if sb is None else Side(sb, thr)
    rng = np.random.default_rng(77)
    lo = oracle.LoCoHD(CATS, oracle.WeightFunction(*WF))
    case = {"thr": thr, "a": a, "b": b, "same": sb is None, "builds": builds, "side_of_limit": side_of_limit,
            "dims": dims if isinstance(dims[0], tuple) else (dims, dims), "lists": {}}
    for kind, (smallest, largest, n_pairs, head) in {"regular": (0, 300, N_PAIRS, first), "clump": (512, 1 << 30, 40, ())}.items():
        pairs = pick_pairs(rng, a, b, smallest, largest, n_pairs, head)
        want = np.empty(len(pairs))
        for k in range(len(a.structures)):  # (the oracle scores one structure pair per call)
            rows = np.flatnonzero(a.sid[pairs[:, 0]] == k)
            local = pairs[rows] - np.array([a.offsets[k], b.offsets[k]])
            (xa, ca), (xb, cb) = a.structures[k], b.structures[k]
            if len(rows):
                want[rows] = np.asarray(lo.from_arrays(xa, ca, np.zeros(len(ca), np.int32), xb, cb, np.zeros(len(cb), np.int32), local, thr))
        case["lists"][kind] = {"pairs": pairs, "want": want, "n_a": a.sizes[pairs[:, 0]], "n_b": b.sizes[pairs[:, 1]]}
    _built[(name, reach)] = case
    return case


def plan_grid(side, thr, reach):
    from loco_hd_amd import _native as N

    lo, hi = (C.c_double * 3)(*side.bbox[0]), (C.c_double * 3)(*side.bbox[1])
    dims, cell, n_cells = (C.c_int32 * 3)(), (C.c_double * 3)(), C.c_int64()
    assert N.lib().lchd_plan_grid(lo, hi, len(side.structures), thr, reach, dims, cell, C.byref(n_cells)) == 0
    return tuple(dims), tuple(cell), int(n_cells.value)


def check_inputs(case):
    """Conditions on the inputs (they hold on the oracle alone): a later edit cannot hollow a case out."""
    reg = case["lists"]["regular"]
    assert np.mean(np.concatenate([reg["n_a"], reg["n_b"]])) >= 10.0
    assert np.mean((reg["n_a"] > 1) & (reg["n_b"] > 1)) >= 0.9
    assert np.max(np.concatenate([reg["n_a"], reg["n_b"]])) <= 300
    assert np.min(np.concatenate([case["lists"]["clump"]["n_a"], case["lists"]["clump"]["n_b"]])) > 512
    for lst in case["lists"].values():
        assert np.all(np.isfinite(lst["want"]))


# ---- the test -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reach", [2, 1], ids=["env_group", "env_cells"])
@pytest.mark.parametrize("name", list(CASES) + list(LATTICE))
def test_cell_grid_regime(lh, oracle, monkeypatch, name, reach):
    import torch
    from loco_hd_amd.device import DeviceSession

    case = build_case(name, reach, oracle)
    check_inputs(case)
    thr, a, b = case["thr"], case["a"], case["b"]
    if reach == 1:
        monkeypatch.setenv("LCHD_NO_ENV_GROUP", "1")  # (read when the context is created)
    sess = DeviceSession(lh.LoCoHD(CATS, lh.WeightFunction(*WF)))
    try:
        def upload(side):
            if len(side.structures) == 1:
                return sess.upload(side.xyz, side.cat)
            handle, offsets = sess.upload_batch(side.structures)
            assert np.array_equal(offsets, side.offsets)
            return handle

        ha = upload(a)
        hb = ha if case["same"] else upload(b)

        def run(kind, grid_reach, check_builds):
            lst = case["lists"][kind]
            before = sess.pass_counts()
            got = sess.from_primitives(ha, hb, torch.from_numpy(lst["pairs"]).cuda(), thr).cpu().numpy()
            grid = sess.last_grid()
            points = sess.last_env_points()
            print(name, kind, "reach", grid_reach, grid, "env points", points, "passes", sess.pass_counts()["passes"] - before["passes"])
            # 1. the regime was reached
            assert sess.pass_counts()["subset_passes"] == before["subset_passes"]
            assert grid is not None
            for k, side in enumerate((a, b)):
                if case["same"] and k == 1:
                    assert grid[1]["build"] == 0
                    continue
                dims, _, n_cells = plan_grid(side, thr, grid_reach)
                assert grid[k]["dims"] == dims and grid[k]["n_cells"] == n_cells == len(side.structures) * dims[0] * dims[1] * dims[2]
                if check_builds:
                    assert dims == case["dims"][k]
                    assert grid[k]["build"] == case["builds"][k]
            if check_builds:
                d = grid[0]["dims"]
                assert case["side_of_limit"](d[0] * d[1] * d[2], grid[0]["n_cells"])
            # 2. the oracle's scores
            assert np.array_equal(np.isfinite(got), np.isfinite(lst["want"]))
            assert np.max(np.abs(got - lst["want"])) < TIGHT
            # 3. exact environment membership
            assert points == int(np.sum(lst["n_a"]) + np.sum(lst["n_b"]))

        run("regular", reach, True)
        # every anchor inside the clump: the 512-point slots overflow, the whole pass runs again with k_env_cells on the reach-1 grid
        # (under LCHD_NO_ENV_GROUP that is the grid of the first call: same dims, same builds)
        run("clump", 1, reach == 1)
    finally:
        sess.close()
