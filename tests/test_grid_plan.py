"""The cell-list grid of a thresholded pass is planned on the host (lchd_plan_grid, loco_hd_amd/csrc/lchd_capi.hip): cells at
least (1 + 1e-9) thr / reach wide, at most 1024 per axis, the largest axis halved until all structures together have at most
2^23 cells.  The environment kernels read the (2 reach + 1)^3 neighbourhood of the anchor's cell and nothing else, so a cell
narrower than thr / reach silently drops points.  Property tests over random boxes and the exact edges of every limit; no GPU."""
import ctypes as C
import math

import numpy as np
import pytest

MAX_CELLS = 1 << 23
MARGIN = 1.0 + 1e-9


@pytest.fixture(scope="module")
def lib():
    from loco_hd_amd import _native

    handle = C.CDLL(str(_native.LIB_PATH))
    res, args = _native._PROTOS["lchd_plan_grid"]
    handle.lchd_plan_grid.restype, handle.lchd_plan_grid.argtypes = res, args
    return handle


def plan(lib, bbmin, bbmax, n_struct, thr, reach):
    lo, hi = (C.c_double * 3)(*bbmin), (C.c_double * 3)(*bbmax)
    dims, cell, n_cells = (C.c_int32 * 3)(), (C.c_double * 3)(), C.c_int64()
    rc = lib.lchd_plan_grid(lo, hi, n_struct, thr, reach, dims, cell, C.byref(n_cells))
    assert rc == 0
    return tuple(dims), tuple(cell), int(n_cells.value)


def cell_coord(x, lo, inv, dim):
    """cell_coord of loco_hd_amd/csrc/lchd_kcommon.h: floor, then clamp into the grid."""
    return min(max(int(math.floor((x - lo) * inv)), 0), dim - 1)


def check_invariants(bbmin, bbmax, n_struct, thr, reach, dims, cell, n_cells):
    what = (bbmin, bbmax, n_struct, thr, reach, dims)
    assert all(1 <= d <= 1024 for d in dims), what
    assert n_cells == n_struct * dims[0] * dims[1] * dims[2], what
    assert n_cells <= MAX_CELLS or dims == (1, 1, 1), what
    for k in range(3):
        ext = bbmax[k] - bbmin[k]
        if ext > 0.0:
            if dims[k] > 1:  # (one cell holds the whole axis, whatever its width)
                assert ext / dims[k] >= thr / reach * MARGIN, what
            assert cell[k] == ext / dims[k], what
        else:
            assert dims[k] == 1 and cell[k] == 1.0, what
        if math.isinf(thr):
            assert dims[k] == 1, what
        inv = 1.0 / (cell[k] * (1.0 + 1e-12))
        assert cell_coord(bbmax[k], bbmin[k], inv, dims[k]) == dims[k] - 1, what
        assert cell_coord(bbmin[k], bbmin[k], inv, dims[k]) == 0, what
        if dims[k] > 1:  # the last cell is not reached through the clamp alone: a point just inside the box's maximum is in it as well
            assert cell_coord(bbmin[k] + ext * (1.0 - 1e-9), bbmin[k], inv, dims[k]) == dims[k] - 1, what


@pytest.mark.parametrize("seed", range(4))
def test_random_boxes_keep_the_planner_invariants(lib, seed):
    rng = np.random.default_rng(4100 + seed)
    for _ in range(1500):
        # extents: log-uniform over 1e-3 .. 1e7, with zero, tiny and equal axes mixed in
        ext = 10.0 ** rng.uniform(-3.0, 7.0, 3)
        ext[rng.random(3) < 0.15] = 0.0
        if rng.random() < 0.1:
            ext[:] = ext[0]
        lo = rng.uniform(-1e6, 1e6, 3)
        hi = lo + ext
        thr = float(10.0 ** rng.uniform(-3.0, 3.0)) if rng.random() > 0.05 else math.inf
        reach = int(rng.integers(1, 3))
        n_struct = int(rng.choice([1, 1, 2, 8, 9, 64, 4096, int(rng.integers(1, 4097))]))
        dims, cell, n_cells = plan(lib, lo, hi, n_struct, thr, reach)
        check_invariants(tuple(lo), tuple(hi), n_struct, thr, reach, dims, cell, n_cells)


def box(cells, cell0, below=False):
    """Extents that hold exactly `cells` cells of width cell0 per axis (just above k cell0), or just below."""
    f = (1.0 - 1e-12) if below else (1.0 + 1e-12)
    return tuple(k * cell0 * f for k in cells)


@pytest.mark.parametrize("reach", [1, 2])
@pytest.mark.parametrize("thr", [0.75, 7.0, 1.9999])
def test_the_edges_of_every_limit(lib, reach, thr):
    cell0 = thr / reach * MARGIN
    zero = (0.0, 0.0, 0.0)

    def dims_of(cells, n_struct=1, below=False, origin=zero):
        ext = box(cells, cell0, below)
        hi = tuple(o + e for o, e in zip(origin, ext))
        dims, cell, n_cells = plan(lib, origin, hi, n_struct, thr, reach)
        check_invariants(origin, hi, n_struct, thr, reach, dims, cell, n_cells)
        return dims

    # the structure cell-count limit (4096) and the one-workgroup scan limit (65536): the dims product lands on either side
    assert dims_of((16, 16, 16)) == (16, 16, 16)
    assert dims_of((17, 16, 16)) == (17, 16, 16)
    assert dims_of((17, 16, 16), below=True) == (16, 15, 15)
    assert dims_of((256, 16, 16)) == (256, 16, 16)
    assert dims_of((257, 16, 16)) == (257, 16, 16)
    # the per-axis clamp
    assert dims_of((1024, 3, 3)) == (1024, 3, 3)
    assert dims_of((1024, 3, 3), below=True) == (1023, 2, 2)
    assert dims_of((1025, 3, 3)) == (1024, 3, 3)
    assert dims_of((5000, 3, 3)) == (1024, 3, 3)
    assert dims_of((3, 1e6, 3)) == (3, 1024, 3)
    # exactly 2^23 cells stay; above it the largest axis is halved, the FIRST of equal axes first, and no further than needed
    assert dims_of((1024, 1024, 8)) == (1024, 1024, 8)
    assert dims_of((1024, 1024, 16)) == (512, 1024, 16)
    assert dims_of((1024, 16, 1024)) == (512, 16, 1024)
    assert dims_of((16, 1024, 1024)) == (16, 512, 1024)
    assert dims_of((1024, 1024, 9)) == (512, 1024, 9)
    assert dims_of((1024, 1024, 1024)) == (128, 256, 256)
    assert dims_of((1023, 1024, 16)) == (1023, 512, 16)
    assert dims_of((1023, 1023, 9)) == (512, 1023, 9)  # (odd axes round up)
    # a batch coarsens where each of its structures alone would not
    assert dims_of((128, 128, 64), n_struct=8) == (128, 128, 64)
    assert dims_of((128, 128, 64), n_struct=9) == (64, 128, 64)
    assert dims_of((128, 128, 64), n_struct=16) == (64, 128, 64)
    assert dims_of((128, 128, 64), n_struct=17) == (64, 64, 64)
    assert dims_of((1, 1, 1), n_struct=4096) == (1, 1, 1)
    assert dims_of((16, 16, 16), n_struct=2048) == (16, 16, 16)
    assert dims_of((16, 16, 16), n_struct=2049) == (8, 16, 16)
    # a box far from the origin (the subtraction bbmax - bbmin has rounded): same dims one cell below the limits
    assert dims_of((15.5, 15.5, 15.5), origin=(1e6, -1e6, 123456.789)) == (15, 15, 15)


def test_degenerate_boxes(lib):
    for thr in (1e-3, 1.0, 1e3, math.inf):
        for reach in (1, 2):
            assert plan(lib, (5.0, 5.0, 5.0), (5.0, 5.0, 5.0), 1, thr, reach) == ((1, 1, 1), (1.0, 1.0, 1.0), 1)
            dims, cell, n_cells = plan(lib, (0.0, -3.0, 2.0), (1e7, -3.0, 2.0), 3, thr, reach)  # a rod: two zero extents
            assert dims[1:] == (1, 1) and cell[1:] == (1.0, 1.0) and n_cells == 3 * dims[0]
            assert dims[0] == (1 if math.isinf(thr) else min(1024, math.floor(1e7 / (thr / reach * MARGIN))))
            dims, cell, n_cells = plan(lib, (0.0, 0.0, 0.0), (400.0, 400.0, 0.0), 1, thr, reach)  # a sheet
            assert dims[2] == 1 and cell[2] == 1.0 and dims[0] == dims[1]
    # more structures than the cell bound: nothing left to coarsen
    assert plan(lib, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (1 << 23) + 5, 10.0, 2) == ((1, 1, 1), (1.0, 1.0, 1.0), (1 << 23) + 5)


def test_bad_arguments_are_refused(lib):
    lo, hi = (C.c_double * 3)(0, 0, 0), (C.c_double * 3)(1, 1, 1)
    dims, cell, n_cells = (C.c_int32 * 3)(), (C.c_double * 3)(), C.c_int64()
    for n_struct, thr, reach in ((0, 1.0, 1), (1, 0.0, 1), (1, -1.0, 2), (1, float("nan"), 1), (1, 1.0, 0)):
        assert lib.lchd_plan_grid(lo, hi, n_struct, thr, reach, dims, cell, C.byref(n_cells)) != 0
    assert lib.lchd_plan_grid(None, hi, 1, 1.0, 1, dims, cell, C.byref(n_cells)) != 0
