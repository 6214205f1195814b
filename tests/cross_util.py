"""A numpy restatement of the nearest-matches rule of the cross-scoring calls, and the acceptance check of a device result against a
score matrix computed elsewhere (the CPU oracle).  Nothing here calls the library under test."""
import numpy as np


def nearest(matrix, k):
    """Per row the k columns with the smallest (score, j), ascending: (scores (Na, k), cols (Na, k) int32).  A stable argsort by score
    keeps equal scores in column order, which is the secondary key."""
    m = np.asarray(matrix, dtype=np.float64)
    order = np.argsort(m, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(m, order, axis=1), order.astype(np.int32)


def accept(scores, cols, S, k, tol):
    """The three-part acceptance of a nearest result against the matrix S, which may differ from the device's own scores by up to tol:
    (a) every returned score is S at the returned column, to tol; (b) every row is non-decreasing with distinct columns; (c) every
    column that was not returned is no better than the last one returned, to 2 tol.  Independent of the order among scores that differ
    in the last bits.  Returns the largest deviation seen in (a)."""
    scores, cols, S = np.asarray(scores), np.asarray(cols), np.asarray(S)
    na, nb = S.shape
    assert scores.shape == (na, k) and cols.shape == (na, k), (scores.shape, cols.shape)
    assert cols.dtype == np.int32 and scores.dtype == np.float64
    assert (cols >= 0).all() and (cols < nb).all()
    picked = np.take_along_axis(S, cols.astype(np.int64), axis=1)
    err = float(np.max(np.abs(scores - picked)))
    assert err <= tol, f"(a) a returned score is {err} from the matrix"
    assert (np.diff(scores, axis=1) >= 0).all(), "(b) a row is not in non-decreasing order"
    for i in range(na):
        assert len(set(cols[i].tolist())) == k, f"(b) row {i} repeats a column"
        rest = np.ones(nb, dtype=bool)
        rest[cols[i]] = False
        if rest.any():
            assert S[i][rest].min() >= S[i][cols[i][k - 1]] - 2 * tol, f"(c) row {i} leaves out a better column"
    return err
