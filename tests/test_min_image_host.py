"""lchd_cell_reduce (host only, no device): the cell the dense minimum-image calls compute their rows with.  The row producers look at
the 27 shifts {-1, 0, 1}^3 of a displacement whose fractional coordinates are wrapped to [-1/2, 1/2]; that finds the nearest image
only in a Minkowski-reduced cell.  So for every cell: the reduced basis spans the same lattice, and the 27-shift rule on it equals a
brute force over the shifts -4 .. 4 of the ORIGINAL cell."""
import ctypes as C

import numpy as np
import pytest

from min_image_util import brute_min_image, brute_rows, min_image_cell
from periodic_cell_util import CELLS

ALL_CELLS = dict(CELLS)
# two vectors nearly parallel: a and b 8.5 degrees apart; c within 8 degrees of -a.  (Their short difference vectors are perpendicular
# to the long ones, so the nearest image of a displacement of +-3 cells stays within the shifts -4 .. 4 of the cell as given: the
# brute force below is checked against a wider one.)
ALL_CELLS["nearly-parallel"] = np.asarray([[10.0, 0.0, 0.0], [10.0, 1.5, 0.0], [3.0, 0.5, 12.0]])
ALL_CELLS["nearly-antiparallel"] = np.asarray([[0.0, 11.0, 0.0], [13.0, 1.0, 0.2], [0.0, -11.0, 1.5]])
SHEARED = np.asarray([[10.0, 0.0, 0.0], [9.9, 0.6, 0.0], [3.0, 4.0, 12.0]])  # reduces with coefficients up to 6


def reduce_cell(cell):
    from loco_hd_amd import _native as N

    cell = np.ascontiguousarray(cell, dtype=np.float64)
    reduced, inverse = np.full((3, 3), np.nan), np.full((3, 3), np.nan)
    rc = N.lib().lchd_cell_reduce(N.dp(cell), N.dp(reduced), N.dp(inverse))
    return rc, reduced, inverse


@pytest.mark.parametrize("name", list(ALL_CELLS))
def test_reduced_cell_is_a_basis_of_the_same_lattice(name):
    cell = ALL_CELLS[name]
    rc, reduced, inverse = reduce_cell(cell)
    assert rc == 0
    t = reduced @ np.linalg.inv(cell)  # reduced = T . cell
    assert np.max(np.abs(t - np.rint(t))) < 1e-9
    assert abs(abs(np.linalg.det(np.rint(t))) - 1.0) < 1e-9
    assert np.max(np.abs(np.rint(t) @ cell - reduced)) <= 1e-12 * np.max(np.abs(cell))
    assert np.max(np.abs(reduced @ inverse - np.eye(3))) < 1e-12
    # no vector gets shorter by a {-1, 0, 1} combination of the other two (Minkowski's conditions in three dimensions)
    for k in range(3):
        p, q = (k + 1) % 3, (k + 2) % 3
        for i in (-1, 0, 1):
            for j in (-1, 0, 1):
                w = reduced[k] + i * reduced[p] + j * reduced[q]
                assert w @ w >= (reduced[k] @ reduced[k]) * (1.0 - 1e-12), (name, k, i, j)


@pytest.mark.parametrize("name", list(ALL_CELLS))
def test_27_shifts_of_the_reduced_cell_find_the_nearest_image(name):
    cell = ALL_CELLS[name]
    rc, reduced, inverse = reduce_cell(cell)
    assert rc == 0
    rng = np.random.default_rng(sorted(ALL_CELLS).index(name))
    d = rng.uniform(-3.0, 3.0, (2000, 3)) @ cell  # displacements spanning +-3 cells
    got = min_image_cell(d, reduced, inverse)
    want = brute_min_image(d, cell, 4)
    assert np.max(np.abs(got - want) / want) <= 1e-12


def test_the_brute_force_is_converged_for_the_cells_of_this_file():
    for k, name in enumerate(("nearly-parallel", "nearly-antiparallel", "skewed")):
        cell = ALL_CELLS[name]
        d = np.random.default_rng(sorted(ALL_CELLS).index(name)).uniform(-3.0, 3.0, (2000, 3)) @ cell
        assert np.array_equal(brute_min_image(d, cell, 4), brute_min_image(d, cell, 6))


@pytest.mark.parametrize("name", ["skewed", "dodecahedron"])
def test_reference_rows_of_unwrapped_coordinates(name):
    """brute_rows (the oracle rows of tests/test_gpu_dense_periodic.py: atoms spread over +-2 cells, shifts -3 .. 3 after moving
    each displacement by whole lattice vectors) against a brute force over the shifts -7 .. 7 of the displacements as they are."""
    cell = CELLS[name]
    x = np.random.default_rng(11).uniform(-2.0, 2.0, (60, 3)) @ cell
    rows = [0, 17, 59]
    got = brute_rows(x, rows, cell)
    for r, row in zip(rows, got):
        want = brute_min_image(x[r] - x, cell, 7)
        assert np.max(np.abs(row - want)) <= 1e-12 * np.max(want)


def test_a_sheared_cell_needs_the_reduction():
    """In a strongly sheared cell the 27 shifts of the cell as given miss the nearest image; those of the reduced cell find it."""
    d = np.random.default_rng(5).uniform(-3.0, 3.0, (2000, 3)) @ SHEARED
    want = brute_min_image(d, SHEARED, 8)
    assert np.max(min_image_cell(d, SHEARED, np.linalg.inv(SHEARED)) - want) > 1e-3
    rc, reduced, inverse = reduce_cell(SHEARED)
    assert rc == 0
    assert np.max(np.abs(min_image_cell(d, reduced, inverse) - want) / want) <= 1e-12


def test_diagonal_cell_comes_back_unchanged():
    cell = np.diag([31.5, 28.25, 40.0])
    rc, reduced, inverse = reduce_cell(cell)
    assert rc == 0
    assert np.array_equal(reduced, cell)
    assert np.array_equal(inverse, np.diag(1.0 / np.diagonal(cell)))


@pytest.mark.parametrize("bad", ["singular", "flat", "nan", "inf"])
def test_singular_and_non_finite_cells_are_value_errors(bad):
    from loco_hd_amd import _native as N

    cell = np.array(CELLS["skewed"])
    if bad == "singular":
        cell[2] = 2.0 * cell[0] - cell[1]
    elif bad == "flat":
        cell[2] = cell[0] + 1e-14 * cell[2]  # |det| below 1e-12 |a| |b| |c|
    elif bad == "nan":
        cell[1, 1] = np.nan
    else:
        cell[0, 2] = np.inf
    rc, _, _ = reduce_cell(cell)
    assert rc == N.EVALUE
    with pytest.raises(ValueError):
        N.check(rc)


def test_null_pointers_are_value_errors():
    from loco_hd_amd import _native as N

    out = (C.c_double * 9)()
    assert N.lib().lchd_cell_reduce(None, out, out) == N.EVALUE


def test_python_helpers_mirror_the_shape_checks():
    from loco_hd_amd.api import cell_reduce, dense_cells

    assert dense_cells(None, None, 3) is None
    assert np.array_equal(dense_cells([3.0, 4.0, 5.0], None, 7), np.diag([3.0, 4.0, 5.0])[None])
    assert dense_cells(None, [CELLS["skewed"]] * 4, 4).shape == (4, 3, 3)
    assert dense_cells(None, CELLS["skewed"], 4).shape == (1, 3, 3)
    for box in ([1.0, 2.0], [[1.0, 2.0, 3.0]] * 2, [1.0, 0.0, 3.0], [1.0, np.inf, 3.0], "box"):
        with pytest.raises(ValueError):
            dense_cells(box, None, 3)
    for cell in (np.zeros((2, 3)), [CELLS["skewed"]] * 2, np.zeros((3, 3)), "cell"):
        with pytest.raises(ValueError):
            dense_cells(None, cell, 3)
    reduced, inverse = cell_reduce(CELLS["skewed"])
    assert np.max(np.abs(reduced @ inverse - np.eye(3))) < 1e-12
    with pytest.raises(ValueError):
        cell_reduce(np.zeros((2, 2)))
