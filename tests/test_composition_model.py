"""The numpy restatement of the composition profile (tests/composition_util.py) against the CPU oracle, without a GPU.

With the Hellinger distance of exponent 1 (total variation) a score against a one-point environment of category X is
(F(inf) - F(0)) - P_X, so the unchanged oracle yields every entry of a profile.  Bound: 1e-12 (the identity and the restatement are
two summation orders of at most 60 terms of size <= 1 in f64; the issue's own run saw 5.6e-16)."""
import numpy as np
import pytest

from composition_util import profile, tv_identity

FAMILIES = {
    "uniform": [3.0, 10.0],
    "hyper_exp": [1.0, 0.5, 0.2, 0.05],
    "dagum": [4.0, 6.0, 1.5],
    "kumaraswamy": [2.0, 11.0, 2.0, 3.0],
}
CATS = ["A", "B", "C", "D", "E", "F"]


def _cdf(name):
    import loco_hd_amd as lh

    wf = lh.WeightFunction(name, FAMILIES[name])
    return lambda x: np.asarray(wf.integral_vec(x))


def _environment(rng, n):
    d = np.round(rng.uniform(0.0, 12.0, n), 1)  # one decimal: ties are frequent
    d[0] = 0.0
    d.sort()
    return d, rng.integers(0, len(CATS), n)


@pytest.mark.parametrize("name", sorted(FAMILIES))
@pytest.mark.parametrize("weighted", [False, True])
def test_restatement_matches_the_oracle_identity(oracle, name, weighted):
    rng = np.random.default_rng(sorted(FAMILIES).index(name) * 2 + int(weighted))
    weights = rng.uniform(0.3, 3.0, len(CATS)) if weighted else np.ones(len(CATS))
    wf = oracle.WeightFunction(name, FAMILIES[name])
    f0, finf = wf.integral_vec([0.0, np.inf])
    worst = worst_sum = 0.0
    for n in [1, 2, 3, 59] + list(rng.integers(1, 60, 6)):
        d, c = _environment(rng, int(n))
        got = profile(d, c, weights, _cdf(name))
        want = tv_identity(oracle, CATS, weights, wf, [CATS[k] for k in c], d)
        worst = max(worst, float(np.max(np.abs(got - want))))
        worst_sum = max(worst_sum, abs(float(got.sum()) - (finf - f0)))
    print(f"{name} weighted={weighted}: max |restatement - identity| = {worst:.3g}, sum rule off by {worst_sum:.3g}")
    assert worst <= 1e-12
    assert worst_sum <= 1e-12


def test_tie_order_does_not_matter():
    rng = np.random.default_rng(7)
    d, c = _environment(rng, 40)
    weights = rng.uniform(0.3, 3.0, len(CATS))
    base = profile(d, c, weights, _cdf("hyper_exp"))
    perm = rng.permutation(40)
    assert np.max(np.abs(profile(d[perm], c[perm], weights, _cdf("hyper_exp")) - base)) <= 1e-15


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_one_point_environment(oracle, name):
    wf = oracle.WeightFunction(name, FAMILIES[name])
    f0, finf = wf.integral_vec([0.0, np.inf])
    got = profile([0.0], [2], [0.5, 1.0, 2.0, 1.0, 1.0, 1.0], _cdf(name))
    want = np.zeros(len(CATS))
    want[2] = finf - f0
    assert np.array_equal(got, want)
