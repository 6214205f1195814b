"""What the strain derivative W means, by central differences of the ordinary periodic scoring calls.

Coordinates and cell of both sides are strained together by I +/- eps E for the six symmetric E (E_ii = 1; E_ij = E_ji = 1, whose
derivative is W_ij + W_ji = 2 W_ij), and the central difference of sum_p v_p S_p is compared with W_a + W_b of the native call.  One
thresholded case in a triclinic cell (threshold 10), one dense case in a box, the default weight function uniform [3, 10].

The bound is not a constant: the same central difference is taken with the numpy / longdouble models (tests/periodic_sensitivity_util.py,
tests/min_image_sensitivity_util.py) against the model's own analytic W on the same case, and the library is allowed 4 x that error --
the margin of the two earlier periodic gradient tests: the truncation of the difference quotient dominates, not the library.

eps = 3e-5.  The generator's cases keep every member distance 1e-3 away from the knots 3 and 10 (the second is the threshold) and from
every other member distance of its pair (both environments: ranks across the sides count too); a distance of at most ~10.4 moves by at most 3.2e-4 under the strain, two neighbours in
a list by at most 6.3e-4 towards each other, so no member enters, leaves or changes rank between the two strained states.  The condition
is checked on the model's lists -- for the thresholded case also on the lists of a threshold 2e-3 further out, which hold what waits just
outside -- and asserted.  Below the margin's limit eps balances two errors of the LIBRARY's quotient: truncation,
which grows as eps^2 and which the model shares, and the rounding of float64 scores, sum |v| * few * 2^-53 / (2 eps), which the long
double model does not have.  At eps = 1e-5 the two were level (measured on an MI355X: thresholded model 3.03e-11 / library 5.1e-11,
dense model 3.07e-11 / library 1.31e-10, the dense case 7 % over 4 x the model's error although W itself equals the integer model of
the library's own lists in every bit); at 3e-5 truncation is nine times larger and the rounding floor three times smaller, so the
comparison measures what it is meant to.

`cell_gradient` in the same cases: one cell entry (lattice vector b along x) perturbed by +/- delta = 3e-4 at fixed fractional coordinates
against inv(h).T (W_a + W_b), with the same bound of 4 x the model's error.  delta is chosen as eps is: the shear moves an atom by its
fractional coordinate along b times delta, so a displacement (fractional differences within +/- 1) changes by at most 3e-4 and the
generator's margin holds as it does for the strain.  At delta = 1e-4 the rounding of the library's float64 scores, divided by 2 delta,
lay above the model's error (measured on an MI355X: model 1.1e-12, library 7.5e-12, thresholded case); it falls as 1 / delta, so
3e-4 is the largest step of the margin's kind that the bound can be given.  The model's own error here is 1.9e-12 / 2.0e-12 (thresholded
/ dense), not nine times its value at 1e-4: for this shear the truncation term is small and part of that figure is the model's own
rounding.
"""
import numpy as np
import pytest

import min_image_sensitivity_util as mu
import periodic_sensitivity_util as psu
import strain_native_util as sn

pytestmark = pytest.mark.gpu

EPS = 3e-5
DELTA = 3e-4
UNI = ("uniform", [3.0, 10.0])
SYMMETRIC = [(i, j) for i in range(3) for j in range(i, 3)]
LD = np.longdouble


def _lh():
    import loco_hd_amd as lh

    return lh


def margin(sens):
    """The smallest gap of any member distance of a pair to a knot (3, 10) or to another member distance of the pair, on either side:
    the score's integrand changes where the merged breakpoints of the two environments change order, so two members of different sides
    that swap ranks put a kink into the score just as two of one side do."""
    m = np.inf
    for p in range(len(sens.count_a)):
        r = np.sort(np.concatenate([np.asarray(sens.dist_a[p, 1: sens.count_a[p]], dtype=np.float64),
                                    np.asarray(sens.dist_b[p, 1: sens.count_b[p]], dtype=np.float64)]))
        if len(r):
            m = min(m, float(np.min(np.abs(r[:, None] - np.asarray(UNI[1])[None, :]))))
        if len(r) > 1:
            m = min(m, float(np.min(np.diff(r))))
    return m


def strain_matrix(i, j, sign):
    e = np.zeros((3, 3))
    e[i, j] = e[j, i] = 1.0
    return np.eye(3) + sign * EPS * e


def differences(loss, cell, analytic):
    """max |central difference - analytic| over the six strains and over one cell entry at fixed fractional coordinates.
    loss(F, h): sum v S with coordinates x F in cell h (F = None: fractional coordinates kept, cell h)."""
    err = 0.0
    for i, j in SYMMETRIC:
        fd = (loss(strain_matrix(i, j, +1), None) - loss(strain_matrix(i, j, -1), None)) / (2 * EPS)
        err = max(err, abs(float(fd - analytic[i, j] * (1 if i == j else 2))))
    k, l, delta = 1, 0, DELTA  # one entry of the cell, lattice vector b along x: a shear of the cell
    moved = [cell.copy(), cell.copy()]
    moved[0][k, l] += delta
    moved[1][k, l] -= delta
    fd = (loss(None, moved[0]) - loss(None, moved[1])) / (2 * delta)
    want = np.linalg.solve(cell.T.astype(np.float64), np.asarray(analytic, dtype=np.float64))[k, l]
    return err, abs(float(fd - want))


def test_thresholded_triclinic():
    lh = _lh()
    per = psu.PERIODS["skewed"]
    cell = np.asarray(per[1], dtype=np.float64)
    for seed in range(400):  # the first case that meets the generator's condition
        a, b = psu.side(700 + 2 * seed, 60, per), psu.side(701 + 2 * seed, 60, per)
        rng = np.random.default_rng(seed)
        pairs = [(int(i), int(j)) for i, j in rng.integers(0, 60, (8, 2))]
        v = rng.uniform(0.5, 2.0, len(pairs))
        model = psu.from_primitives(a, per, b, per, pairs, psu.THR, 7)
        # (the lists at a threshold 2e-3 further out also hold what waits just outside: an atom within 1e-3 beyond the threshold fails too)
        beyond = psu.from_primitives(a, per, b, per, pairs, psu.THR + 2e-3, 7)
        if min(margin(model), margin(beyond)) >= 1e-3:
            break
    assert min(margin(model), margin(beyond)) >= 1e-3, "the generator placed a member within 1e-3 of a knot, the threshold or another member"
    assert np.array_equal(model.count_a, beyond.count_a) and np.array_equal(model.count_b, beyond.count_b)
    inv = np.linalg.inv(cell)

    def place(s, f, h):
        x = s[0] @ f if h is None else (s[0] @ inv) @ h
        return x, (cell @ f if h is None else h)

    def model_loss(f, h):
        (xa, ha), (xb, _) = place(a, f, h), place(b, f, h)
        return np.dot(v.astype(LD), psu.scores((xa, a[1], a[2]), ("cell", ha), (xb, b[1], b[2]), ("cell", ha), pairs, psu.THR, 7))

    wa, wb = sn.strain_longdouble(model, v)
    model_err = differences(model_loss, cell, wa + wb)

    l = lh.LoCoHD(psu.CATS7, lh.WeightFunction(*UNI))
    atoms = lambda s, x: [lh.PrimitiveAtom(psu.CATS7[c], f"t{t}", list(p)) for p, c, t in zip(x, s[1], s[2])]  # noqa: E731

    def lib_loss(f, h):
        (xa, ha), (xb, _) = place(a, f, h), place(b, f, h)
        return float(np.dot(v, l.from_primitives(atoms(a, xa), atoms(b, xb), pairs, psu.THR, cell_a=ha, cell_b=ha)))

    got = l.native_gradient_from_primitives_periodic(atoms(a, a[0]), atoms(b, b[0]), pairs, psu.THR, pair_weights=v, cell_a=cell, cell_b=cell,
                                                     strain=True)
    w = got.strain_a + got.strain_b
    lib_err = differences(lib_loss, cell, w)
    assert np.max(np.abs(lh.cell_gradient(w, cell) - np.linalg.inv(cell).T @ w)) <= 1e-14 * np.max(np.abs(w))
    print(f"thresholded, skewed cell, eps = {EPS}: |FD - W| model {model_err[0]:.3g} library {lib_err[0]:.3g}; "
          f"|FD - cell_gradient| model {model_err[1]:.3g} library {lib_err[1]:.3g}")
    assert np.any(w != 0.0)
    assert lib_err[0] <= 4 * model_err[0]
    assert lib_err[1] <= 4 * model_err[1]


def test_dense_box():
    lh = _lh()
    from loco_hd_amd.api import cell_reduce

    box = np.asarray([12.0, 10.5, 13.25])
    cell = np.diag(box)
    cats = [f"c{k}" for k in range(4)]
    n = 16
    for seed in range(2000):
        rng = np.random.default_rng(seed)
        ca, cb = rng.integers(0, 4, n), rng.integers(0, 4, n)
        xa, xb = rng.uniform(0.0, 1.0, (n, 3)) * box, rng.uniform(0.0, 1.0, (n, 3)) * box
        v = rng.uniform(0.5, 2.0, n)
        model = mu.sensitivity(ca, xa, ("box", box), cb, xb, ("box", box), 4, UNI, reduce=cell_reduce)
        if margin(model) >= 1e-3:
            break
    assert margin(model) >= 1e-3, "the generator placed a member within 1e-3 of a knot or another member"

    def strained_cell(f, h):
        return cell @ f if h is None else h

    def model_loss_cell(f, h):
        hh = strained_cell(f, h)
        pa, pb = (xa @ f, xb @ f) if h is None else ((xa / box) @ h, (xb / box) @ h)
        return np.dot(v.astype(LD), mu.scores(ca, pa, ("cell", hh), cb, pb, ("cell", hh), 4, UNI, reduce=cell_reduce))

    wa, wb = sn.strain_longdouble(model, v, dense=True)
    model_err = differences(model_loss_cell, cell, wa + wb)

    l = lh.LoCoHD(cats, lh.WeightFunction(*UNI))
    seq_a, seq_b = [cats[c] for c in ca], [cats[c] for c in cb]

    def lib_loss(f, h):
        hh = strained_cell(f, h)
        pa, pb = (xa @ f, xb @ f) if h is None else ((xa / box) @ h, (xb / box) @ h)
        return float(np.dot(v, l.from_coords(seq_a, seq_b, pa, pb, cell_a=hh, cell_b=hh)))

    got = l.native_gradient_from_coords_periodic(seq_a, seq_b, xa, xb, pair_weights=v, box_a=box, box_b=box, strain=True)
    w = got.strain_a + got.strain_b
    lib_err = differences(lib_loss, cell, w)
    assert np.allclose(lh.cell_gradient(w, box), np.linalg.inv(cell).T @ w, rtol=1e-14, atol=0)
    print(f"dense, box, n = {n}, eps = {EPS}: |FD - W| model {model_err[0]:.3g} library {lib_err[0]:.3g}; "
          f"|FD - cell_gradient| model {model_err[1]:.3g} library {lib_err[1]:.3g}")
    assert np.any(w != 0.0)
    assert lib_err[0] <= 4 * model_err[0]
    assert lib_err[1] <= 4 * model_err[1]
