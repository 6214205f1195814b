"""The oracle on given dense rows: shared by tests/test_gpu_dense_periodic.py and tests/fuzz_surface.py."""
import numpy as np


def oracle_rows(lo, sa, sb, rows_a, rows_b, keys=None):
    """stat_dist_integral on the stably sorted rows (utils.rs:25-39), one from_anchors call per row pair; a row shorter than its
    sequence is sorted with the prefix of that length (a ragged from_dmxs row).  `keys`: one weight-function key per row pair."""
    out = []
    for k, (ra, rb) in enumerate(zip(rows_a, rows_b)):
        ra, rb = np.asarray(ra, dtype=float) + 0.0, np.asarray(rb, dtype=float) + 0.0
        oa, ob = np.argsort(ra, kind="stable"), np.argsort(rb, kind="stable")
        args = ([sa[i] for i in oa], [sb[i] for i in ob], ra[oa].tolist(), rb[ob].tolist())
        out.append(lo.from_anchors(*args) if keys is None else lo.from_anchors(*args, keys[k]))
    return np.asarray(out)
