"""tests/periodic_sensitivity_util.py (the restatement the GPU tests compare against) pinned to its own periodic score by central
differences in the atoms' coordinates, and the inputs of tests/test_gpu_sensitivity_periodic.py checked for what those tests rely on.
CPU only.

Measured here: max |model gradient - central difference (h = 1e-4)| = 2.7e-11 over the cases below (truncation of the quotient: the
score is piecewise smooth in a coordinate, not piecewise linear).  4 x that is periodic_sensitivity_util.FD_BOUND, the bound the GPU test
puts on difference quotients of from_primitives(box_a=...) at the same atoms and step."""
import numpy as np
import pytest

import periodic_sensitivity_util as pu


@pytest.mark.parametrize("case", ["box/box", "open/cell"])
def test_gradient_against_central_differences_of_the_periodic_score(case):
    a, per_a, b, per_b, pairs = pu.random_case(case)
    picks, grads = pu.fd_atoms(case)
    worst = 0.0
    for side, atom in picks:
        q = pu.central_difference(a, per_a, b, per_b, pairs, pu.THR, 7, side, atom, lambda *args: pu.scores(*args, 7))
        worst = max(worst, float(np.max(np.abs(q - grads[side][atom]))))
        assert np.any(grads[side][atom] != 0.0)
    print(f"{case}: max |model gradient - central difference| = {worst:.4g} at atoms {picks}")
    assert worst <= pu.FD_MEASURED


@pytest.mark.parametrize("case", sorted(pu.RANDOM_SIDES))
def test_translation_invariance_and_ghost_members(case):
    a, per_a, b, per_b, pairs = pu.random_case(case)
    ps = pu.from_primitives(a, per_a, b, per_b, pairs, pu.THR, 7)
    ga, gb = pu.gradient(ps, len(a[0]), len(b[0]))
    assert np.max(np.abs(ga.sum(0))) <= 1e-12 and np.max(np.abs(gb.sum(0))) <= 1e-12 and np.any(ga != 0) and np.any(gb != 0)
    # every periodic side has members that entered through an image, an open one has none
    for per, image in ((per_a, ps.image_a), (per_b, ps.image_b)):
        assert bool(np.any(image != 0)) == (per is not None)
    # dist is the length of disp in the scoring order
    for dist, disp in ((ps.dist_a, ps.disp_a), (ps.dist_b, ps.disp_b)):
        assert np.array_equal(dist, np.sqrt(disp[..., 0] * disp[..., 0] + disp[..., 1] * disp[..., 1] + disp[..., 2] * disp[..., 2]))


def test_thin_box_has_an_atom_that_enters_twice():
    a, per_a, b, per_b, pairs = pu.thin_case()
    ps = pu.from_primitives(a, per_a, b, per_b, pairs, pu.THR, 7)
    found = pu.twice(ps)
    assert found, "no source atom under two image codes: pick another seed"
    # ... and both of its terms reach the gradient: dropping one of the two slots changes that atom's row
    p, s, atom = found[0]
    idx, g = (ps.idx_a, ps.g_a) if s == 0 else (ps.idx_b, ps.g_b)
    slots = np.flatnonzero(idx[p] == atom)
    assert len(slots) == 2


def test_lattice_has_ties_between_home_atoms_and_ghosts():
    a, per_a, b, per_b, pairs = pu.lattice_case()
    ps = pu.from_primitives(a, per_a, b, per_b, pairs, pu.THR, 7)
    assert pu.tie_order_ok(ps) > 0
    assert np.all(ps.scores == 0.0) and np.any(ps.g_a != 0.0)
    pu.tie_groups_cancel(ps, 1e-15)


def test_image_cloud_restatement_on_one_atom():
    xyz, origin, code = pu.image_cloud(np.zeros((1, 3)), (8.0, 8.0, 8.0), 8.0)
    assert len(xyz) == 27 and origin.tolist() == [0] * 27 and code.tolist() == list(range(27))
    xyz, origin, code = pu.image_cloud(np.full((1, 3), 4.0), (8.0, 8.0, 8.0), 3.0)
    assert len(xyz) == 1 and code.tolist() == [0]
    for o in range(27):
        got = pu.image_of(np.zeros((1, 3)), ("box", (8.0, 8.0, 8.0)), 0, o)
        assert np.array_equal(got, pu.image_cloud(np.zeros((1, 3)), (8.0, 8.0, 8.0), 8.0)[0][o])
