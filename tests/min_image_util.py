"""numpy restatements of the minimum-image arithmetic include/loco_hd_hip.h prescribes for the dense periodic calls (the row producers
of loco_hd_amd/csrc/lchd_ensemble.hip), and the brute force they are checked against: shared by tests/test_min_image_host.py (no
device), tests/test_gpu_dense_periodic.py and tests/test_cabi_dense_periodic.py."""
import itertools

import numpy as np

SHIFTS27 = [(i, j, k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)]  # i outermost, k innermost


def norm3(w):
    return np.sqrt((w[..., 0] * w[..., 0] + w[..., 1] * w[..., 1]) + w[..., 2] * w[..., 2])


def min_image_box(d, box):
    """d [..., 3] displacements, box (Lx, Ly, Lz): per axis d - L rint(d / L)."""
    box = np.asarray(box, dtype=np.float64)
    return norm3(d - box * np.rint(d / box))


def min_image_cell(d, reduced, inverse):
    """d [..., 3] displacements; reduced / inverse from lchd_cell_reduce: wrap the fractional coordinates, then the 27 shifts."""
    R, I = np.asarray(reduced, dtype=np.float64), np.asarray(inverse, dtype=np.float64)
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    f = [(dx * I[0, k] + dy * I[1, k]) + dz * I[2, k] for k in range(3)]
    f = [fk - np.rint(fk) for fk in f]
    v = [(f[0] * R[0, c] + f[1] * R[1, c]) + f[2] * R[2, c] for c in range(3)]
    best = np.full(d.shape[:-1], np.inf)
    for i, j, k in SHIFTS27:
        w = [v[c] + ((float(i) * R[0, c] + float(j) * R[1, c]) + float(k) * R[2, c]) for c in range(3)]
        best = np.minimum(best, (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    return np.sqrt(best)


def brute_min_image(d, cell, span):
    """The nearest image by brute force over the shifts -span .. span of `cell` (the caller's, unreduced)."""
    cell = np.asarray(cell, dtype=np.float64)
    best = np.full(d.shape[:-1], np.inf)
    for s in itertools.product(range(-span, span + 1), repeat=3):
        best = np.minimum(best, norm3(d + np.asarray(s, dtype=np.float64) @ cell))
    return best


def min_image_matrix(x, box=None, cell=None, reduce=None):
    """The n x n minimum-image matrix of the coordinates x in the prescribed arithmetic: row r, column i = (x[r] - x[i]).  `reduce` is
    loco_hd_amd.api.cell_reduce (needed for a cell)."""
    d = x[:, None, :] - x[None, :, :]
    if box is not None:
        return min_image_box(d, box)
    reduced, inverse = reduce(cell)
    if np.count_nonzero(reduced - np.diag(np.diagonal(reduced))) == 0:  # a diagonal cell is the box
        return min_image_box(d, np.diagonal(reduced))
    return min_image_cell(d, reduced, inverse)


def brute_rows(x, rows, cell, span=3):
    """Reference rows for the oracle: for each r of `rows` the distances from x[r] to every atom's nearest image, by brute force over
    the shifts -span .. span of the ORIGINAL cell.  The coordinates need not be wrapped, so a displacement is first moved by whole
    lattice vectors (the rounded fractional coordinates in the cell as given) to within half a cell; tests/test_min_image_host.py
    checks this against a brute force wide enough to need no such step."""
    cell = np.asarray(cell, dtype=np.float64)
    inv = np.linalg.inv(cell)
    out = []
    for r in rows:
        d = x[r] - x
        d = d - np.rint(d @ inv) @ cell
        row = brute_min_image(d, cell, span)
        row[r] = 0.0
        out.append(row)
    return out
