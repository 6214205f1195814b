"""The five cells of the periodic-cell tests and their perpendicular widths: shared by tests/test_periodic_cell_host.py (no device)
and tests/test_gpu_periodic_cell.py."""
import math

import numpy as np

D = 30.0
CELLS = {
    "monoclinic": [[58.5, 0.0, 0.0], [0.0, 60.25, 0.0], [31.0 * math.cos(math.radians(101.5)), 0.0, 31.0 * math.sin(math.radians(101.5))]],
    "dodecahedron": [[D, 0.0, 0.0], [0.0, D, 0.0], [D / 2, D / 2, D * math.sqrt(2.0) / 2]],
    "octahedron": [[D, 0.0, 0.0], [D / 3, 2 * math.sqrt(2.0) * D / 3, 0.0], [-D / 3, math.sqrt(2.0) * D / 3, math.sqrt(6.0) * D / 3]],
    "skewed": [[20.0, 0.0, 0.0], [15.0, 18.0, 0.0], [-9.0, 7.0, 16.0]],  # not reduced
    "left-handed": [[0.0, 18.0, 0.0], [20.0, 3.0, 0.0], [4.0, -5.0, 17.0]],
}
CELLS = {k: np.asarray(v, dtype=np.float64) for k, v in CELLS.items()}
TABLE = {"monoclinic": (57.3, 60.25, 30.4), "dodecahedron": (24.5, 24.5, 21.2), "octahedron": (24.5, 24.5, 24.5),
         "skewed": (12.5, 16.5, 16.0), "left-handed": (16.9, 19.5, 17.0)}


def widths(cell):
    """w_k = |det| / |cross of the other two vectors|, in the arithmetic the header prescribes (so that reach = min w is the very
    number lchd_cell_validate compares with)."""
    a, b, c = ([float(v) for v in row] for row in np.asarray(cell, dtype=np.float64))

    def cross(u, v):
        return [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]

    def norm(u):
        return math.sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2])
    x = [cross(b, c), cross(c, a), cross(a, b)]
    det = a[0] * x[0][0] + a[1] * x[0][1] + a[2] * x[0][2]
    return np.asarray([abs(det) / norm(x[k]) for k in range(3)])
