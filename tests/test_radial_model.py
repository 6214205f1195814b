"""The numpy restatement of the radial profile (tests/radial_util.py) pinned to the unchanged CPU oracle in three ways, without a GPU.

  row sum        edges = [0, ..., inf]: a row sums to the oracle's score
  uniform        under uniform[a, b]: bin_k = (e'_{k+1} - e'_k) / (b - a) * oracle_score(uniform[e'_k, e'_{k+1}]), e' clipped to [a, b]
  clamped lists  any family: C(e) = from_anchors(seq, min(d, e)) - (F(inf) - F(e)) * H_full, (F(inf) - F(0)) * H_full =
                 from_anchors(seq, all zeros); bin_k = C(e_{k+1}) - C(e_k)

Bound 1e-12, integral form against oracle: both are sums of at most ~10^2 terms of size <= 1, the restatement in longdouble, the oracle
in f64 (its own rounding: a few 1e-16 per term).  All distances here have a finite H (Kullback-Leibler / Renyi with eps > 0)."""
import numpy as np
import pytest

import radial_util
from integral_form import score

CATS = ["A", "B", "C", "D", "E", "F", "G"]
FAMILIES = {
    "uniform": [3.0, 10.0],
    "hyper_exp": [1.0, 0.5, 0.2, 0.05],
    "dagum": [4.0, 6.0, 1.5],
    "kumaraswamy": [2.0, 11.0, 2.0, 3.0],
}
DISTANCES = {
    "hellinger2": ("Hellinger", [2.0]),
    "hellinger1": ("Hellinger", [1.0]),
    "hellinger3.5": ("Hellinger", [3.5]),
    "ks": ("Kolmogorov-Smirnov", []),
    "kl": ("Kullback-Leibler", [1e-3]),
    "renyi": ("Renyi", [2.5, 1e-3]),
}
EDGES = [0.0, 2.0, 3.0, 4.5, 6.0, 7.25, 9.0, 10.0, 12.0, np.inf]
BOUND = 1e-12


def _env(rng, n):
    d = np.round(rng.uniform(0.0, 12.0, n), 1)  # one decimal: ties within and across the lists, and with the edges
    d[0] = 0.0
    d.sort()
    return rng.integers(0, len(CATS), n), d


def _lchd(oracle, wf, sd, weights):
    return oracle.LoCoHD(CATS, oracle.WeightFunction(*wf), category_weights=weights, statistical_distance=oracle.StatisticalDistance(*sd))


def _seq(c):
    return [CATS[k] for k in c]


@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("dist", sorted(DISTANCES))
@pytest.mark.parametrize("weighted", [False, True])
def test_row_sum_is_the_oracle_score(oracle, family, dist, weighted):
    rng = np.random.default_rng(11)
    weights = rng.uniform(0.3, 3.0, len(CATS)) if weighted else None
    wf, sd = (family, FAMILIES[family]), DISTANCES[dist]
    l = _lchd(oracle, wf, sd, weights)
    worst = 0.0
    for n_a, n_b in [(1, 1), (1, 40), (2, 3), (60, 45), (33, 64)]:
        (ca, da), (cb, db) = _env(rng, n_a), _env(rng, n_b)
        row = radial_util.profile(ca, da, cb, db, len(CATS), wf, EDGES, sd, weights)
        worst = max(worst, abs(row.sum() - l.from_anchors(_seq(ca), _seq(cb), da, db)))
        assert abs(row.sum() - score(ca, da, cb, db, len(CATS), wf, sd, weights)) <= BOUND
    print(f"{family} {dist} weighted={weighted}: max |row sum - oracle| = {worst:.3g}")
    assert worst <= BOUND


@pytest.mark.parametrize("accept_same", [True, False])
def test_row_sum_under_both_tag_rules(oracle, accept_same):
    rng = np.random.default_rng(5)
    n = 120
    xyz_a, xyz_b = rng.uniform(0, 14, (n, 3)), rng.uniform(0, 14, (n, 3))
    cat_a, cat_b = rng.integers(0, len(CATS), n), rng.integers(0, len(CATS), n)
    tag_a, tag_b = rng.integers(0, 6, n), rng.integers(0, 6, n)
    pairs = [(int(i), int(j)) for i, j in rng.integers(0, n, (12, 2))]
    wf = ("uniform", [3.0, 10.0])
    l = oracle.LoCoHD(CATS, oracle.WeightFunction(*wf), tag_pairing_rule=oracle.TagPairingRule({"accept_same": accept_same}))
    pa = [oracle.PrimitiveAtom(CATS[c], str(t), x) for c, t, x in zip(cat_a, tag_a, xyz_a)]
    pb = [oracle.PrimitiveAtom(CATS[c], str(t), x) for c, t, x in zip(cat_b, tag_b, xyz_b)]
    want = np.asarray(l.from_primitives(pa, pb, pairs, 8.0))
    got = radial_util.from_primitives(cat_a, xyz_a, tag_a, cat_b, xyz_b, tag_b, pairs, 8.0, len(CATS), wf, EDGES, accept_same=accept_same)
    assert np.max(np.abs(got.sum(1) - want)) <= BOUND


@pytest.mark.parametrize("dist", sorted(DISTANCES))
def test_uniform_identity(oracle, dist):
    rng = np.random.default_rng(23)
    a, b = 3.0, 10.0
    sd = DISTANCES[dist]
    worst = 0.0
    for n_a, n_b in [(1, 30), (50, 50), (64, 17)]:
        (ca, da), (cb, db) = _env(rng, n_a), _env(rng, n_b)
        row = radial_util.profile(ca, da, cb, db, len(CATS), ("uniform", [a, b]), EDGES, sd)
        for k in range(len(EDGES) - 1):
            lo, hi = min(max(EDGES[k], a), b), min(max(EDGES[k + 1], a), b)
            want = 0.0
            if hi > lo:
                want = (hi - lo) / (b - a) * _lchd(oracle, ("uniform", [lo, hi]), sd, None).from_anchors(_seq(ca), _seq(cb), da, db)
            else:
                assert row[k] == 0.0
            worst = max(worst, abs(row[k] - want))
    print(f"{dist}: max |bin - uniform identity| = {worst:.3g}")
    assert worst <= BOUND


@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("dist", sorted(DISTANCES))
def test_clamped_list_identity(oracle, family, dist):
    """Clamping both lists at e moves every point beyond e onto e: the oracle's score of the clamped lists is the integral up to e plus
    (F(inf) - F(e)) * H_full, H_full the distance of the two complete environments -- which the all-zero lists give."""
    rng = np.random.default_rng(31)
    wf, sd = (family, FAMILIES[family]), DISTANCES[dist]
    l = _lchd(oracle, wf, sd, None)
    F = oracle.WeightFunction(*wf).integral_vec
    worst = 0.0
    for n_a, n_b in [(1, 25), (40, 64), (57, 57)]:
        (ca, da), (cb, db) = _env(rng, n_a), _env(rng, n_b)
        f0, finf = F([0.0, np.inf])
        h_full = l.from_anchors(_seq(ca), _seq(cb), np.zeros(n_a), np.zeros(n_b)) / (finf - f0)

        def upto(e):
            if np.isinf(e):
                return l.from_anchors(_seq(ca), _seq(cb), da, db)
            return l.from_anchors(_seq(ca), _seq(cb), np.minimum(da, e), np.minimum(db, e)) - (finf - F([e])[0]) * h_full

        c = [upto(e) for e in EDGES]
        row = radial_util.profile(ca, da, cb, db, len(CATS), wf, EDGES, sd)
        worst = max(worst, float(np.max(np.abs(row - np.diff(c)))))
    print(f"{family} {dist}: max |bin - clamped-list identity| = {worst:.3g}")
    assert worst <= BOUND
