"""tests/dense_sensitivity_util.py (the restatement the GPU tests of the dense sensitivity calls compare against) pinned to the score model
tests/integral_form.score by central differences: in one entry of a distance matrix, and in one coordinate of a structure.  CPU only.

A dense row has no threshold, so g is the whole derivative of the row's score and the central difference must reproduce it for ANY
weight function.  The step is h = 1e-6.  The difference quotient's own error is truncation, h^2 / 6 |S'''| (the weight function's third
derivative: not a rounding quantity), plus the float64 rounding of the two scores, 2 * 1.1e-16 / (2 h) = 1.1e-10 for |S| of order 1.  The
bound is 10 x the largest deviation MEASURED over this file's draws ("Dense sensitivities"):
    one dmx entry        4.93e-11  (hyper_exp; dagum 2.78e-11, kumaraswamy 4.07e-11)
    one coordinate       9.85e-10  (hyper_exp; dagum 6.72e-10, kumaraswamy 7.52e-10 -- the loss sums 12 row scores with weights up to 2, so
                                    its float64 rounding is that much larger than one score's)
Draws whose smallest gap between two distances of a row pair (or to a support edge) is below 10 h are rejected: at ties the derivative
is one-sided and the central difference does not converge to it."""
import numpy as np
import pytest

import dense_sensitivity_util as du
import integral_form as model

H_STEP = 1e-6
MEASURED_DMX = 4.93e-11
MEASURED_XYZ = 9.85e-10
FAMILIES = {"hyper_exp": [1.0, 0.5, 0.2, 0.05], "dagum": [4.0, 6.0, 1.5], "kumaraswamy": [2.0, 11.0, 2.0, 3.0]}
EDGES = {"hyper_exp": [], "dagum": [], "kumaraswamy": [2.0, 11.0]}
ROWS, COLS, N_CAT = 3, 12, 3
SEEDS = list(range(6))
SD = ("Hellinger", [2.0])


def _matrices(seed):
    rng = np.random.default_rng(seed)
    cats = [rng.integers(0, N_CAT, COLS) for _ in range(2)]
    dmx = [rng.uniform(0.3, 11.7, (ROWS, COLS)) for _ in range(2)]
    for m in dmx:
        m[np.arange(ROWS), rng.integers(0, COLS, ROWS)] = 0.0  # every row holds its 0, in any column
    return cats, dmx


def _gap(rows_a, rows_b, edges):
    return min(float(np.min(np.diff(np.sort(np.concatenate([ra[ra > 0], rb[rb > 0], [0.0], edges]))))) for ra, rb in zip(rows_a, rows_b))


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_g_against_central_differences_in_one_dmx_entry(family):
    wf = (family, FAMILIES[family])
    worst, used = 0.0, 0
    for seed in SEEDS:
        cats, dmx = _matrices(seed)
        if _gap(dmx[0], dmx[1], EDGES[family]) < 10 * H_STEP:
            continue
        used += 1
        sens = du.from_dmxs(cats[0], dmx[0], cats[1], dmx[1], N_CAT, wf, SD)
        G = du.gradient_dmx(sens, COLS, COLS)
        for r in range(ROWS):
            assert abs(sens.scores[r] - model.score(cats[0], dmx[0][r], cats[1], dmx[1][r], N_CAT, wf, SD)) <= 1e-15
            for side in range(2):
                for j in range(COLS):
                    if dmx[side][r, j] == 0.0:
                        assert G[side][r, j] == 0.0  # the slot-0 column
                        continue
                    s = []
                    for sign in (+1, -1):
                        rows = [dmx[0][r].copy(), dmx[1][r].copy()]
                        rows[side][j] += sign * H_STEP
                        s.append(model.score(cats[0], rows[0], cats[1], rows[1], N_CAT, wf, SD))
                    worst = max(worst, abs(G[side][r, j] - (s[0] - s[1]) / (2 * H_STEP)))
    print(f"{family}: max |g - central difference| over {used} draws = {worst:.3g}")
    assert used >= len(SEEDS) - 1 and worst <= 10 * MEASURED_DMX


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_coordinate_gradient_against_central_differences(family):
    wf = (family, FAMILIES[family])
    worst, used = 0.0, 0
    for seed in SEEDS[:3]:
        rng = np.random.default_rng(100 + seed)
        cats = [rng.integers(0, N_CAT, COLS) for _ in range(2)]
        xyz = [rng.uniform(0.0, 7.0, (COLS, 3)) for _ in range(2)]
        v = rng.uniform(0.5, 2.0, COLS)
        rows = [du.coords_rows(x) for x in xyz]
        if _gap(rows[0], rows[1], EDGES[family]) < 10 * H_STEP * 2:  # (a coordinate step moves a distance by at most the step)
            continue
        used += 1
        sens = du.from_dmxs(cats[0], rows[0], cats[1], rows[1], N_CAT, wf, SD)
        grads = du.gradient_coords(sens, xyz[0], xyz[1], v)
        assert np.max(np.abs(grads[0].sum(0))) <= 1e-14 and np.max(np.abs(grads[1].sum(0))) <= 1e-14  # translation invariance

        def loss(xa, xb):
            return float(np.dot(v, model.from_coords(cats[0], xa, cats[1], xb, N_CAT, wf, SD)))

        for side in range(2):
            for atom in range(COLS):
                for axis in range(3):
                    s = []
                    for sign in (+1, -1):
                        moved = [xyz[0].copy(), xyz[1].copy()]
                        moved[side][atom, axis] += sign * H_STEP
                        s.append(loss(moved[0], moved[1]))
                    worst = max(worst, abs(grads[side][atom, axis] - (s[0] - s[1]) / (2 * H_STEP)))
    print(f"{family}: max |grad - central difference| over {used} draws = {worst:.3g}")
    assert used >= 2 and worst <= 10 * MEASURED_XYZ


def test_sorted_rows_follow_the_stable_co_sort():
    """Ties come out in column order and slot 0 is the lowest column among the smallest entries (utils.rs:25-39)."""
    idx, d = du.sorted_row([2.0, 0.0, 2.0, 0.0, 1.0])
    assert idx.tolist() == [1, 3, 4, 0, 2] and d.tolist() == [0.0, 0.0, 1.0, 2.0, 2.0]
    sens = du.from_dmxs([0, 1, 0, 1, 0], [[2.0, 0.0, 2.0, 0.0, 1.0]], [1, 0, 0], [[0.0, 3.0, 1.5]], 2, ("uniform", [0.5, 5.0]))
    assert sens.idx_a.tolist() == [[1, 3, 4, 0, 2]] and sens.idx_b.tolist() == [[0, 2, 1, -1, -1]]
    assert sens.count_a.tolist() == [5] and sens.count_b.tolist() == [3] and sens.g_a[0, 0] == 0.0 and sens.g_b[0, 0] == 0.0
