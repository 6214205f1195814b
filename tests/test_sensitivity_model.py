"""tests/sensitivity_util.py (the restatement the GPU tests compare against) pinned to the score model tests/integral_form.score by
difference quotients in one member's distance, and to identities that need no tolerance.  CPU only.

Under a uniform weight function S is piecewise linear in every distance: the central difference equals the derivative up to the rounding
of the two scores (float64, |S| of order 1: 2 * 1.1e-16 / (2 h) = 1.1e-12 at h = 1e-4; the bound below is ten times that) whenever no other
breakpoint and no support edge lies within the step.  Draws whose smallest gap is below 10 h are rejected (at most 10 % of them).
For the other families the quotient is Richardson-extrapolated; its own error is MEASURED here on F against the density (the same
extrapolation, the same steps, the same float64 cast) and the bound is 16 x that (measured: at most 1.3e-12)."""
import numpy as np
import pytest

import integral_form as model
import sensitivity_util as su

H_STEP = 1e-4
UNI = ("uniform", [3.0, 10.0])
FAMILIES = {"hyper_exp": [1.0, 0.5, 0.2, 0.05], "dagum": [4.0, 6.0, 1.5], "kumaraswamy": [2.0, 11.0, 2.0, 3.0]}
SEEDS = list(range(40))
N_CAT = 5


def _draw(seed, n=8):
    """Two sorted lists (slot 0 the anchor) of n members each with distances in (0, 12)."""
    rng = np.random.default_rng(seed)
    sides = []
    for _ in range(2):
        d = np.concatenate([[0.0], np.sort(rng.uniform(0.2, 12.0, n))])
        sides.append((rng.integers(0, N_CAT, n + 1), d))
    return sides


def _smallest_gap(sides, edges):
    pts = np.sort(np.concatenate([sides[0][1][1:], sides[1][1][1:], edges]))
    return float(np.min(np.diff(pts)))


def _accepted(edges, step, n=8):
    keep = [s for s in SEEDS if _smallest_gap(_draw(s, n), edges) >= 10 * step]
    assert len(keep) >= 0.9 * len(SEEDS), f"{len(SEEDS) - len(keep)} of {len(SEEDS)} draws rejected"
    return keep


def _quotient(sides, side, k, wf, sd, step):
    out = []
    for sign in (+1, -1):
        moved = [(c, d.copy()) for c, d in sides]
        moved[side][1][k] += sign * step
        out.append(model.score(moved[0][0], moved[0][1], moved[1][0], moved[1][1], N_CAT, wf, sd))
    return (out[0] - out[1]) / (2 * step)


@pytest.mark.parametrize("sd", [("Hellinger", [2.0]), ("Hellinger", [3.5]), ("Kolmogorov-Smirnov", []), ("Kullback-Leibler", [1e-3]), ("Renyi", [2.5, 1e-3])],
                         ids=lambda s: s[0] + "".join(str(v) for v in s[1]))
def test_uniform_central_differences(sd):
    worst = 0.0
    for seed in _accepted(np.asarray([3.0, 10.0]), H_STEP):
        sides = _draw(seed)
        s, ga, gb = su.sensitivity(sides[0][0], sides[0][1], sides[1][0], sides[1][1], N_CAT, UNI, sd)
        assert abs(s - model.score(sides[0][0], sides[0][1], sides[1][0], sides[1][1], N_CAT, UNI, sd)) <= 1e-15
        for side, g in ((0, ga), (1, gb)):
            for k in range(1, len(g)):
                worst = max(worst, abs(float(g[k]) - _quotient(sides, side, k, UNI, sd, H_STEP)))
    print(f"uniform, {sd}: max |g - central difference| = {worst:.3g}")
    assert worst <= 1.1e-11


def _richardson(f, x, step):
    d1 = (f(x + step) - f(x - step)) / (2 * step)
    d2 = (f(x + step / 2) - f(x - step / 2)) / step
    return (4 * d2 - d1) / 3


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_other_families_richardson(family):
    wf, step, sd = (family, FAMILIES[family]), 2 * H_STEP, ("Hellinger", [2.0])
    edges = np.asarray([2.0, 11.0]) if family == "kumaraswamy" else np.zeros(0)
    own, worst = 0.0, 0.0
    for seed in _accepted(edges, step, 5):  # (five members a side: the wider step of the extrapolation rejects more of a denser draw)
        sides = _draw(seed, 5)
        _, ga, gb = su.sensitivity(sides[0][0], sides[0][1], sides[1][0], sides[1][1], N_CAT, wf, sd)
        for side, g in ((0, ga), (1, gb)):
            for k in range(1, len(g)):
                x = sides[side][1][k]
                own = max(own, abs(_richardson(lambda t: float(model.cdf(wf[0], wf[1], [t])[0]), x, step) - float(su.pdf(wf[0], wf[1], [x])[0])))

                def q(st):
                    return _quotient(sides, side, k, wf, sd, st)

                worst = max(worst, abs(float(g[k]) - (4 * q(step / 2) - q(step)) / 3))
    print(f"{family}: extrapolation's own error on F = {own:.3g}, max |g - extrapolated quotient| = {worst:.3g}")
    assert own > 0.0 and worst <= 16 * own


def test_identities():
    rng = np.random.default_rng(1)
    sides = _draw(3)
    (ca, da), (cb, db) = sides
    # identical environments: the score is exactly 0 and so is every derivative under a COMMON displacement of the two tied members
    # (g_a == -g_b exactly: tied members are treated one at a time, side A first, so each side's own g is the one-sided derivative)
    s, ga, gb = su.sensitivity(ca, da, ca, da, N_CAT, UNI)
    assert s == 0.0 and np.all(ga + gb == 0) and ga[0] == 0 and gb[0] == 0
    # a member outside the support of uniform has g == 0 exactly
    s, ga, gb = su.sensitivity(ca, da, cb, db, N_CAT, UNI)
    assert np.all(ga[(da < 3.0) | (da >= 10.0)] == 0) and np.all(gb[(db < 3.0) | (db >= 10.0)] == 0) and np.any(ga != 0)
    # swapping sides swaps the outputs (no distance occurs on both sides)
    s2, gb2, ga2 = su.sensitivity(cb, db, ca, da, N_CAT, UNI)
    assert abs(s - s2) <= 1e-16 and np.max(np.abs(ga - ga2)) <= 1e-18 and np.max(np.abs(gb - gb2)) <= 1e-18
    # sum_k d_k g_k = dS/dlambda under a uniform scaling of one side's distances (the model's quotient; S is piecewise linear in lambda
    # as long as no two breakpoints cross: the smallest relative gap of this draw is far above the step)
    lam = 1e-7
    up = model.score(ca, da * (1 + lam), cb, db, N_CAT, UNI)
    dn = model.score(ca, da * (1 - lam), cb, db, N_CAT, UNI)
    assert abs(float((ga * da).sum()) - (up - dn) / (2 * lam)) <= 2 * 1.1e-16 / (2 * lam) * 10
    # translation invariance: the coordinate gradients of each side sum to zero
    xyz = rng.uniform(0, 12, (60, 3))
    cat = rng.integers(0, N_CAT, 60)
    pairs = [(int(i), int(j)) for i, j in rng.integers(0, 60, (8, 2))]
    sens = su.from_primitives(cat, xyz, None, cat[::-1], xyz[::-1] * 0.9, None, pairs, 7.0, N_CAT, UNI)
    g1, g2 = su.gradient(sens, xyz, xyz[::-1] * 0.9)
    assert np.max(np.abs(g1.sum(0))) <= 1e-14 and np.max(np.abs(g2.sum(0))) <= 1e-14 and np.any(g1 != 0)
    for idx, dist, cnt in ((sens.idx_a, sens.dist_a, sens.count_a), (sens.idx_b, sens.dist_b, sens.count_b)):
        for p in range(len(pairs)):
            rest = list(zip(dist[p, 1:cnt[p]], idx[p, 1:cnt[p]]))
            assert rest == sorted(rest) and dist[p, 0] == 0.0 and idx[p, 0] == pairs[p][0 if idx is sens.idx_a else 1]
