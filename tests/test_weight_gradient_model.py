"""The numpy restatement of the weight-function gradient (tests/weight_gradient_util.py, longdouble) pinned to the unchanged CPU oracle,
without a GPU.

  finite differences   grad[p][k] against Richardson-extrapolated central differences of the oracle's scores under theta_k +- h at steps
                       h = 1e-4 theta_k, h / 2 and h / 4; the reference's own error is estimated as the difference between the (h, h/2)
                       and the (h/2, h/4) extrapolations.  7 categories, 300-atom clouds (seeds 101, 102, edge 20), 40 pairs from
                       default_rng(9), threshold 8: Hellinger 2 under each of the four families and under uniform [2.5, 6.5] (both
                       bounds inside the threshold), Kolmogorov-Smirnov and Kullback-Leibler 1e-3 under uniform [3, 10], and dense rows
                       of 40 points.
  excluded elements    an element (p, k) whose stencil straddles a kink of F is left out: theta_k a support bound of uniform /
                       kumaraswamy and a member of pair p within h of it (weight_gradient_util.smooth_within_the_stencil, from the
                       geometry alone).  At most 4 of the 40 rows of a column may be left out; here at most 1 is.
  identities           sum_i a_i grad[p][a_i] = 0 for hyper_exp; the summation-by-parts form equals the interval form

BOUND, restatement against finite differences: 10 x the largest error estimate over the cases below, measured on the CPU (estimate /
max |restatement - finite difference|, elements compared):
  hellinger 2, uniform [3, 10]     4.5e-12 / 1.8e-12,  80 of  80     hellinger 2, uniform [2.5, 6.5]   4.3e-12 / 1.7e-12,  79 of 80
  hellinger 2, hyper_exp           6.1e-10 / 1.7e-10, 160 of 160     ks, uniform [3, 10]               1.8e-12 / 8.2e-13,  80 of 80
  hellinger 2, dagum               4.2e-12 / 2.2e-12, 120 of 120     kl 1e-3, uniform [3, 10]          1.3e-11 / 8.0e-12,  80 of 80
  hellinger 2, kumaraswamy         8.1e-12 / 3.5e-12, 160 of 160     dense rows: uniform, hyper_exp    3.7e-12 / 1.3e-12, 2.7e-10 / 9.4e-11
so BOUND = 10 x 6.1e-10 = 6.1e-9 (below the 1e-7 a smooth case set has to meet).  The hyper_exp estimate is the largest because its rates
are small: h = 1e-4 * 0.05 divides the oracle's rounding by 5e-6.
"""
import numpy as np
import pytest

import weight_gradient_util as wg
from category_gradient_util import richardson
from radial_util import environment

CATS = ["A", "B", "C", "D", "E", "F", "G"]
FAMILIES = {"uniform": [3.0, 10.0], "hyper_exp": [1.0, 0.5, 0.2, 0.05], "dagum": [4.0, 6.0, 1.5], "kumaraswamy": [2.0, 11.0, 2.0, 3.0]}
H2 = ("Hellinger", [2.0])
CASES = {
    "hellinger 2, uniform": (H2, ("uniform", FAMILIES["uniform"])),
    "hellinger 2, hyper_exp": (H2, ("hyper_exp", FAMILIES["hyper_exp"])),
    "hellinger 2, dagum": (H2, ("dagum", FAMILIES["dagum"])),
    "hellinger 2, kumaraswamy": (H2, ("kumaraswamy", FAMILIES["kumaraswamy"])),
    "hellinger 2, uniform [2.5, 6.5]": (H2, ("uniform", [2.5, 6.5])),
    "ks, uniform": (("Kolmogorov-Smirnov", []), ("uniform", FAMILIES["uniform"])),
    "kl 1e-3, uniform": (("Kullback-Leibler", [1e-3]), ("uniform", FAMILIES["uniform"])),
}
BOUND = wg.FD_BOUND
REL = 1e-4


class Cloud:
    def __init__(self, seed, n, edge):
        rng = np.random.default_rng(seed)
        self.xyz = rng.uniform(0.0, edge, (n, 3))
        self.cat = rng.integers(0, len(CATS), n)
        self.tag = rng.integers(0, 4, n)

    def atoms(self, oracle):
        return [oracle.PrimitiveAtom(CATS[k], f"t{g}", list(x)) for k, g, x in zip(self.cat, self.tag, self.xyz)]


@pytest.fixture(scope="module", autouse=True)
def library_leaf():
    """Every conclusion of this module is about the restated leaf; it carries over to the library only where the library's host leaf
    (the function the kernel calls) is that leaf: 1e-13 on theta_k * G_k, a few ulp of values of size <= 1."""
    worst = wg.library_leaf_deviation(FAMILIES)
    print(f"max |theta (library leaf - restated leaf)| = {worst:.3g}")
    assert worst <= 1e-13


@pytest.fixture(scope="module")
def clouds():
    rng = np.random.default_rng(9)
    return Cloud(101, 300, 20.0), Cloud(102, 300, 20.0), [(int(i), int(j)) for i, j in rng.integers(0, 300, (40, 2))]


def _finite_differences(score_of, theta):
    """(dS/dtheta by finite differences [P][n_params], the estimate of its own error [P][n_params])"""
    cols, errs = zip(*[richardson(score_of, theta, k, REL) for k in range(len(theta))])
    return np.stack(cols, 1), np.stack(errs, 1)


def _compare(case, got, want, errs, keep):
    for k in range(keep.shape[1]):
        assert (~keep[:, k]).sum() <= 4, f"{case}: column {k} leaves out {(~keep[:, k]).sum()} of {len(keep)} rows"
    estimate = float(np.max(errs[keep]))
    worst = float(np.max(np.abs(got.astype(np.float64) - want)[keep]))
    print(f"{case}: {int(keep.sum())} of {keep.size} elements, reference error estimate {estimate:.3g}, "
          f"max |model - finite difference| = {worst:.3g}")
    assert np.any(np.abs(got) > 1e-4)
    assert BOUND <= 1e-7
    assert worst <= BOUND


@pytest.mark.parametrize("case", sorted(CASES))
def test_thresholded_gradient_is_the_oracles_finite_difference(oracle, clouds, case):
    a, b, pairs = clouds
    sd, wf = CASES[case]
    pa, pb = a.atoms(oracle), b.atoms(oracle)

    def score_of(theta):
        l = oracle.LoCoHD(CATS, oracle.WeightFunction(wf[0], list(theta)), statistical_distance=oracle.StatisticalDistance(sd[0], sd[1]))
        return l.from_primitives(pa, pb, pairs, 8.0)

    want, errs = _finite_differences(score_of, wf[1])
    scores, got = wg.from_primitives(a.cat, a.xyz, a.tag, b.cat, b.xyz, b.tag, pairs, 8.0, len(CATS), wf, sd)
    assert got.shape == (40, len(wf[1]))
    assert float(np.max(np.abs(scores.astype(np.float64) - np.asarray(score_of(wf[1]))))) <= 1e-12
    keep = np.stack([wg.smooth_within_the_stencil(np.concatenate([environment(i, a.cat, a.xyz, a.tag, 8.0)[1],
                                                                  environment(j, b.cat, b.xyz, b.tag, 8.0)[1]]), wf, REL) for i, j in pairs])
    _compare(case, got, want, errs, keep)


@pytest.mark.parametrize("family", ["uniform", "hyper_exp"])
def test_dense_rows_of_40_points(oracle, family):
    wf = (family, FAMILIES[family])
    rng = np.random.default_rng(41)
    ma, mb = rng.uniform(0.5, 12.0, (12, 40)), rng.uniform(0.5, 12.0, (12, 40))
    ma[np.arange(12), np.arange(12)] = 0.0
    mb[np.arange(12), np.arange(12)] = 0.0
    ca, cb = rng.integers(0, len(CATS), 40), rng.integers(0, len(CATS), 40)
    sa, sb = [CATS[k] for k in ca], [CATS[k] for k in cb]

    def score_of(theta):
        return oracle.LoCoHD(CATS, oracle.WeightFunction(wf[0], list(theta))).from_dmxs(sa, sb, ma, mb)

    want, errs = _finite_differences(score_of, wf[1])
    _, got = wg.from_rows(ca, ma, cb, mb, len(CATS), wf)
    keep = np.stack([wg.smooth_within_the_stencil(np.concatenate([ra, rb]), wf, REL) for ra, rb in zip(ma, mb)])
    assert (~keep).sum(0).max() <= 1  # (of 12 rows)
    _compare(f"dense rows, {family}", got, want, errs, keep)


def test_euler_identity_of_hyper_exp(clouds):
    """F depends on the a_i through their ratios alone: sum_i a_i dS/da_i = 0."""
    a, b, pairs = clouds
    wf = ("hyper_exp", FAMILIES["hyper_exp"])
    _, got = wg.from_primitives(a.cat, a.xyz, a.tag, b.cat, b.xyz, b.tag, pairs, 8.0, len(CATS), wf)
    worst = float(np.max(np.abs((got[:, :2] * np.asarray(wf[1][:2], dtype=wg.LD)).sum(1))))
    print(f"max |sum_i a_i grad_i| = {worst:.3g}")
    assert np.any(np.abs(got[:, :2]) > 1e-4)
    assert worst <= 1e-15


@pytest.mark.parametrize("case", sorted(CASES))
def test_summation_by_parts_equals_the_interval_form(clouds, case):
    a, b, pairs = clouds
    sd, wf = CASES[case]
    _, one = wg.from_primitives(a.cat, a.xyz, a.tag, b.cat, b.xyz, b.tag, pairs, 8.0, len(CATS), wf, sd)
    _, two = wg.from_primitives(a.cat, a.xyz, a.tag, b.cat, b.xyz, b.tag, pairs, 8.0, len(CATS), wf, sd, by_parts=True)
    worst = float(np.max(np.abs(one - two)))
    print(f"{case}: max |interval form - by parts| = {worst:.3g}")
    assert worst <= 1e-15
