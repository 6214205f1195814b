"""The numpy model of the dense minimum-image sensitivities (tests/min_image_sensitivity_util.py) against what it restates: the chosen
vectors have the lengths min_image_matrix computes, bit for bit; they are the brute-force nearest images wherever those are unique; and
the model gradient assembled from them is the derivative of the model's own score (central differences).  No device: cell_reduce is the
library's host-only lchd_cell_reduce."""
import numpy as np
import pytest

import min_image_sensitivity_util as mu
from min_image_util import min_image_matrix, norm3
from periodic_cell_util import CELLS
from periodic_sensitivity_util import H_STEP

UNI = ("uniform", [3.0, 10.0])
HYP = ("hyper_exp", [1.0, 0.1])
UNREDUCED = np.asarray([CELLS["skewed"][0] + 2.0 * CELLS["skewed"][1], CELLS["skewed"][1] - CELLS["skewed"][2], CELLS["skewed"][2]])
GEOMETRIES = {
    "box": ("box", np.asarray([21.5, 19.25, 24.0])),
    "skewed": ("cell", CELLS["skewed"]),
    "dodecahedron": ("cell", CELLS["dodecahedron"]),
    "unreduced": ("cell", UNREDUCED),
}


def reduce(cell):
    from loco_hd_amd.api import cell_reduce

    return cell_reduce(cell)


def cell_of(per):
    return np.diag(per[1]) if per[0] == "box" else np.asarray(per[1])


def coords(seed, n, per, unwrapped=False):
    rng = np.random.default_rng(seed)
    lo, hi = (-2.0, 3.0) if unwrapped else (0.0, 1.0)
    return rng.uniform(lo, hi, (n, 3)) @ cell_of(per)


def kw(per):
    return {per[0]: per[1]}


@pytest.mark.parametrize("unwrapped", [False, True], ids=["wrapped", "unwrapped"])
@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
def test_chosen_vectors_have_the_rows_lengths_and_are_the_nearest_images(geo, unwrapped):
    per = GEOMETRIES[geo]
    x = coords(11, 60, per, unwrapped)
    if geo == "unreduced":
        assert not np.array_equal(reduce(per[1])[0], per[1])
    disp = mu.disp_matrix(x, reduce=reduce, **kw(per))
    rows = min_image_matrix(x, reduce=reduce, **kw(per))
    assert np.array_equal(norm3(disp).view(np.uint64), rows.view(np.uint64))
    brute, unique = mu.brute_disp(x, cell_of(per))
    assert unique.mean() > 0.99
    err = float(np.max(np.abs(disp - brute)[unique]))
    print(geo, "unwrapped" if unwrapped else "wrapped", "max |disp - brute force| =", err)
    assert err <= 1e-9 * float(np.abs(x).max() + 1.0)


def test_open_structure_and_a_tie():
    x = coords(3, 9, GEOMETRIES["box"])
    assert np.array_equal(mu.disp_matrix(x), x[None, :, :] - x[:, None, :])
    # exactly half an edge apart: rint rounds 0.5 and -0.5 to 0, so both atoms see the other at +-L/2 unwrapped; the length ties
    box = np.asarray([16.0, 20.0, 24.0])
    y = np.asarray([[1.0, 2.0, 3.0], [9.0, 2.0, 3.0]])
    d = mu.disp_matrix(y, box=box)
    assert np.array_equal(d[0, 1], [8.0, 0.0, 0.0]) and np.array_equal(d[1, 0], [-8.0, 0.0, 0.0])


FD_CASES = [("box", UNI), ("skewed", HYP), ("dodecahedron", UNI), ("box/open", HYP)]


@pytest.mark.parametrize("case", range(len(FD_CASES)), ids=[c[0] for c in FD_CASES])
def test_model_gradient_against_central_differences(case):
    name, wf = FD_CASES[case]
    per_a = GEOMETRIES[name.split("/")[0]]
    per_b = None if name.endswith("/open") else per_a
    n, n_cat = 24, 4
    scale = 0.55 if per_a[0] == "cell" else 0.6  # a denser cell: most members inside the weight function's support
    per_a = (per_a[0], np.asarray(per_a[1]) * scale)
    per_b = None if per_b is None else per_a
    rng = np.random.default_rng(40 + case)
    xa, xb = coords(50 + case, n, per_a, True), coords(60 + case, n, per_a, False)
    ca, cb = rng.integers(0, n_cat, n), rng.integers(0, n_cat, n)
    v = rng.uniform(0.5, 1.5, n)
    ms = mu.sensitivity(ca, xa, per_a, cb, xb, per_b, n_cat, wf, reduce=reduce)
    grads = mu.gradient(ms, v)
    fn = lambda a, b: mu.scores(ca, a, per_a, cb, b, per_b, n_cat, wf, reduce=reduce)  # noqa: E731
    picks = [(0, i) for i in mu.quiet_atoms(0, xa, per_a, xb, per_b, reduce, 2)] + [(1, i) for i in mu.quiet_atoms(1, xa, per_a, xb, per_b, reduce, 1)]
    assert len(picks) == 3
    worst = 0.0
    for side, atom in picks:
        fd = mu.central_difference(xa, xb, side, atom, fn, v, H_STEP)
        err = float(np.max(np.abs(fd - grads[side][atom])))
        print(name, "side", side, "atom", atom, "gradient", grads[side][atom], "|fd - model| =", err)
        assert np.abs(grads[side][atom]).max() > 1e-6
        worst = max(worst, err)
    print(name, "largest deviation:", worst, "(FD_MEASURED =", mu.FD_MEASURED, ")")
    assert worst <= mu.FD_MEASURED


@pytest.mark.parametrize("mix", mu.GRAD_MIXES, ids=lambda m: f"{m[0]}/{m[1]}")
def test_model_gradient_on_the_cases_the_device_test_differentiates(mix):
    """The very structures, weight function, row weights and atoms of tests/test_gpu_min_image_sensitivity.py's difference quotients:
    FD_MEASURED covers them, so FD_BOUND is a bound for that test."""
    ca, xa, per_a, cb, xb, per_b, v, picks = mu.gradient_case(mix, reduce)
    assert len(picks) == 3
    grads = mu.gradient(mu.sensitivity(ca, xa, per_a, cb, xb, per_b, 4, mu.GRAD_WF, reduce=reduce), v)
    fn = lambda a, b: mu.scores(ca, a, per_a, cb, b, per_b, 4, mu.GRAD_WF, reduce=reduce)  # noqa: E731
    worst = 0.0
    for side, atom in picks:
        fd = mu.central_difference(xa, xb, side, atom, fn, v, H_STEP)
        err = float(np.max(np.abs(fd - grads[side][atom])))
        print(mix, "side", side, "atom", atom, "|fd - model| =", err)
        worst = max(worst, err)
    print(mix, "largest deviation:", worst, "(FD_MEASURED =", mu.FD_MEASURED, ")")
    assert worst <= mu.FD_MEASURED
