"""The numpy restatement of the category-weight gradient (tests/category_gradient_util.py, longdouble) pinned to the unchanged CPU oracle,
without a GPU.

  finite differences   G[p][c] against Richardson-extrapolated central differences of oracle.LoCoHD(..., category_weights=w +- h e_c)
                       scores at steps h = 1e-3 w_c and h / 2; the reference's own error is estimated as the difference between the
                       (h, h/2) and the (h/2, h/4) extrapolations.  7 categories, weights from uniform(0.3, 3), 300-atom clouds, 40
                       pairs, threshold 8; Hellinger exponents 2, 1 and 3.5 and Kullback-Leibler 1e-3 under uniform [3, 10], Hellinger 2
                       under a hyper_exp weight function, and dense rows of 40 points.
  Euler                sum_c w_c G[p][c] = 0 to 1e-12: the score is homogeneous of degree 0 in the weights
  attribution          Hellinger: w_c G_c + integral of (p_c sum x + q_c sum y) = A_c / e against tests/attribution_util.py

BOUND, restatement against finite differences: 10 x the largest error estimate over the cases below, measured on the CPU (estimate /
max |restatement - finite difference|):
  hellinger 2              1.5e-12  / 7.6e-13        hellinger 1 (275 of 280 elements)   1.6e-12 / 6.2e-13
  hellinger 3.5            1.9e-12  / 9.5e-13        kl 1e-3                             9.0e-12 / 3.8e-12
  hellinger 2, hyper_exp   3.6e-12  / 1.1e-12        dense rows: hellinger 2, kl 1e-3    1.7e-12 / 7.2e-13, 1.9e-12 / 8.1e-13
so BOUND = 10 x 9.0e-12 = 9e-11 (below the 1e-7 a smooth case set has to meet).
Exponent 1 (total variation) is piecewise linear in w: over all 280 elements the same estimate is 2.5e-4, because 5 stencils straddle a
kink of |p_k - q_k|.  Those 5 elements are left out of the exponent-1 comparison, decided from the geometry alone
(_smooth_within_the_stencil); the other 275 meet the bound.
"""
import numpy as np
import pytest

import attribution_util as au
import category_gradient_util as cg
from radial_util import environment

CATS = ["A", "B", "C", "D", "E", "F", "G"]
UNI = ("uniform", [3.0, 10.0])
HYP = ("hyper_exp", [1.0, 0.5, 0.2, 0.05])
CASES = {
    "hellinger 2": (("Hellinger", 2.0), UNI),
    "hellinger 1": (("Hellinger", 1.0), UNI),
    "hellinger 3.5": (("Hellinger", 3.5), UNI),
    "kl 1e-3": (("Kullback-Leibler", 1e-3), UNI),
    "hellinger 2, hyper_exp": (("Hellinger", 2.0), HYP),
}
BOUND = cg.FD_BOUND  # 9e-11
EULER = 1e-12


class Cloud:
    def __init__(self, seed, n, edge):
        rng = np.random.default_rng(seed)
        self.xyz = rng.uniform(0.0, edge, (n, 3))
        self.cat = rng.integers(0, len(CATS), n)
        self.tag = rng.integers(0, 4, n)

    def atoms(self, oracle):
        return [oracle.PrimitiveAtom(CATS[k], f"t{g}", list(x)) for k, g, x in zip(self.cat, self.tag, self.xyz)]


@pytest.fixture(scope="module")
def clouds():
    rng = np.random.default_rng(9)
    return Cloud(101, 300, 20.0), Cloud(102, 300, 20.0), [(int(i), int(j)) for i, j in rng.integers(0, 300, (40, 2))]


WEIGHTS = np.random.default_rng(3).uniform(0.3, 3.0, len(CATS))


def _sd(oracle, distance):
    return oracle.StatisticalDistance(distance[0], [distance[1]])


def _finite_differences(score_of):
    """(dS/dw by finite differences [P][C], the estimate of its own error [P][C])"""
    cols, errs = zip(*[cg.richardson(score_of, WEIGHTS, c) for c in range(len(CATS))])
    return np.stack(cols, 1), np.stack(errs, 1)


def _smooth_within_the_stencil(a, b, pairs, wf):
    """Exponent 1 is total variation, 1/2 sum_k |p_k - q_k|: piecewise linear in w, with a kink wherever some p_k - q_k of some piece
    changes sign.  A difference stencil that straddles a kink measures neither one-sided slope, so element (p, c) is compared only where
    the signs of p_k - q_k of every piece of pair p are the same at w_c - h and at w_c + h (p_k - q_k is monotone in w_c in between:
    both are ratios of functions linear in w_c).  Decided from the geometry alone.  Returns a bool array [P][C]."""
    keep = np.zeros((len(pairs), len(CATS)), dtype=bool)
    for p, (i, j) in enumerate(pairs):
        ca, da = environment(i, a.cat, a.xyz, a.tag, 8.0, True)
        cb, db = environment(j, b.cat, b.xyz, b.tag, 8.0, True)
        for c in range(len(CATS)):
            signs = []
            for step in (-1e-3, 1e-3):
                w = WEIGHTS.copy()
                w[c] *= 1.0 + step
                _, P, Q, _ = cg.pieces(ca, da, cb, db, len(CATS), wf, w)
                signs.append(np.sign(P - Q))
            keep[p, c] = np.array_equal(signs[0], signs[1])
    return keep


@pytest.mark.parametrize("case", sorted(CASES))
def test_thresholded_gradient_is_the_oracles_finite_difference(oracle, clouds, case):
    a, b, pairs = clouds
    distance, wf = CASES[case]
    pa, pb = a.atoms(oracle), b.atoms(oracle)

    def score_of(w):
        l = oracle.LoCoHD(CATS, oracle.WeightFunction(*wf), category_weights=list(w), statistical_distance=_sd(oracle, distance))
        return l.from_primitives(pa, pb, pairs, 8.0)

    want, errs = _finite_differences(score_of)
    got = cg.from_primitives(a.cat, a.xyz, a.tag, b.cat, b.xyz, b.tag, pairs, 8.0, len(CATS), wf, distance, WEIGHTS, log_form=False)
    assert got.shape == (40, len(CATS))
    keep = _smooth_within_the_stencil(a, b, pairs, wf) if distance == ("Hellinger", 1.0) else np.ones(got.shape, dtype=bool)
    estimate = float(np.max(errs[keep]))
    worst = float(np.max(np.abs(got.astype(np.float64) - want)[keep]))
    print(f"{case}: {int(keep.sum())} of {keep.size} elements, reference error estimate {estimate:.3g}, "
          f"max |model - finite difference| = {worst:.3g}")
    assert keep.sum() >= keep.size // 2
    assert BOUND <= 1e-7
    assert worst <= BOUND


@pytest.mark.parametrize("case", ["hellinger 2", "kl 1e-3"])
def test_dense_rows_of_40_points(oracle, case):
    distance, wf = CASES[case]
    rng = np.random.default_rng(41)
    ma, mb = np.round(rng.uniform(0.5, 12.0, (12, 40)), 3), np.round(rng.uniform(0.5, 12.0, (12, 40)), 3)
    ma[np.arange(12), np.arange(12)] = 0.0
    mb[np.arange(12), np.arange(12)] = 0.0
    ca, cb = rng.integers(0, len(CATS), 40), rng.integers(0, len(CATS), 40)
    sa, sb = [CATS[k] for k in ca], [CATS[k] for k in cb]

    def score_of(w):
        l = oracle.LoCoHD(CATS, oracle.WeightFunction(*wf), category_weights=list(w), statistical_distance=_sd(oracle, distance))
        return l.from_dmxs(sa, sb, ma, mb)

    want, errs = _finite_differences(score_of)
    got = cg.from_rows(ca, ma, cb, mb, len(CATS), wf, distance, WEIGHTS, log_form=False)
    worst = float(np.max(np.abs(got.astype(np.float64) - want)))
    print(f"dense rows, {case}: reference error estimate {float(np.max(errs)):.3g}, max |model - finite difference| = {worst:.3g}")
    assert BOUND <= 1e-7
    assert worst <= BOUND


@pytest.mark.parametrize("case", sorted(CASES))
def test_euler_identity(clouds, case):
    a, b, pairs = clouds
    distance, wf = CASES[case]
    got = cg.from_primitives(a.cat, a.xyz, a.tag, b.cat, b.xyz, b.tag, pairs, 8.0, len(CATS), wf, distance, WEIGHTS)
    worst = float(np.max(np.abs(got.sum(1))))
    print(f"{case}: max |sum_c w_c G_c| = {worst:.3g}")
    assert np.any(np.abs(got) > 1e-4)
    assert worst <= EULER


@pytest.mark.parametrize("e", [2.0, 1.0, 3.5])
def test_hellinger_direct_part_is_the_attribution_over_e(clouds, e):
    """x_c + y_c = (D / (e T)) |d_c|^e = D t_c / (e T): the direct part of w_c dD/dw_c is the attribution's integrand over e."""
    a, b, pairs = clouds
    worst = 0.0
    for i, j in pairs:
        ca, da = environment(i, a.cat, a.xyz, a.tag, 8.0, True)
        cb, db = environment(j, b.cat, b.xyz, b.tag, 8.0, True)
        wg, direct, mean = cg.log_gradient(ca, da, cb, db, len(CATS), UNI, ("Hellinger", e), WEIGHTS, parts=True)
        attr = au.attribution(ca, da, cb, db, len(CATS), UNI, e, WEIGHTS)
        worst = max(worst, float(np.max(np.abs((wg + mean).astype(np.float64) - attr / e))))
        assert float(np.max(np.abs((wg + mean - direct).astype(np.float64)))) <= 1e-15
    print(f"exponent {e}: max |w G + mean part - A / e| = {worst:.3g}")
    assert worst <= 1e-12


def test_conventions():
    """An unused category, identical environments, one category: exact zeros."""
    rng = np.random.default_rng(5)
    da, db = rng.uniform(0.0, 9.0, 30), rng.uniform(0.0, 9.0, 25)
    ca, cb = rng.integers(0, 5, 30), rng.integers(0, 5, 25)  # categories 5 and 6 occur in neither environment
    da[0] = db[0] = 0.0  # the anchors
    for distance in (("Hellinger", 2.0), ("Hellinger", 1.0), ("Hellinger", 3.5), ("Kullback-Leibler", 1e-3)):
        g = cg.log_gradient(ca, da, cb, db, 7, UNI, distance, WEIGHTS)
        assert np.all(g[5:] == 0.0) and np.any(g[:5] != 0.0)
        assert np.all(cg.log_gradient(np.zeros(30, int), da, np.zeros(25, int), db, 1, UNI, distance) == 0.0)
        if distance[0] == "Hellinger":
            assert np.all(cg.log_gradient(ca, da, ca, da, 7, UNI, distance, WEIGHTS) == 0.0)
