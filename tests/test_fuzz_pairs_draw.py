"""The pair-family axes and the CPU references of tests/fuzz_pairs.py on their own: what the default seeds cover, the references against
each other (attribution row sums and the sensitivity model's score against integral_form.score, the model's g against a difference
quotient of that score) and the mutation checks the references must not survive.  CPU only.

Covered by the default 40 seeds (asserted below):
    every prims / prims_batch seed runs sensitivity and cross (19), every prims / prims_batch / coords / dmxs seed attribution (28)
    attribution unfitted on seeds 1, 2, 3, 20, 22, 33, 37, 38 (2, 3, 33, 38 periodic); folded to W = 64, 63, 33, 32 and 2 elsewhere
    periodic session seeds for cross on image clouds: 3, 9, 24, 27, 36, 39
    Nb = 1, 63, 64, 65, 80; k = 1, 2, 8, 63, 64 after clipping, k = Nb = 64 among them; tile_rows = 0, 1, 5, Na
    general tag-pair rules, the default rule, thr = inf, more than 255 categories under cross, a dictionary key"""
import os

import numpy as np
import pytest

import fuzz_pairs as fq
import fuzz_profiles as fp
import fuzz_surface as fs
import integral_form as model
import sensitivity_util as su

N_SEEDS = int(os.environ.get("LCHD_FUZZ_SEEDS", "40"))
DEFAULT = range(40)
TOL = 1e-12  # tests/test_fuzz_profiles_draw.py


@pytest.fixture(scope="module")
def drawn():
    cases = [fs.draw(s) for s in DEFAULT]
    return cases, [fq.pair_axes(c) for c in cases]


def test_axes_are_a_function_of_the_seed_and_leave_the_draws_alone():
    before = fs.draw(18)
    prof = fp.profile_axes(before)
    a, b = fq.pair_axes(before), fq.pair_axes(fs.open_twin(fs.draw(18)))
    assert a["sample"] == b["sample"] and a["cross"] == b["cross"] and a["changed"] == b["changed"]
    assert np.array_equal(a["pair_weights"], b["pair_weights"])
    after = fs.draw(18)
    assert before["pairs"] == after["pairs"] and np.array_equal(before["xa"], after["xa"]) and before["thr"] == after["thr"]
    assert before["sa"] == after["sa"] and before["ncat"] == after["ncat"] == 300 and before["weights"] == after["weights"]
    again = fp.profile_axes(after)
    assert prof["sample"] == again["sample"] and np.array_equal(prof["edges"], again["edges"])
    assert all(abs(fq.STREAM - other) > 1_000_000 for other in (fs.STREAM, fp.STREAM, 77000, 88000))


def test_every_driver_seed_runs(drawn):
    cases, axes = drawn
    pair = [c["seed"] for c, a in zip(cases, axes) if a["runs"]["sensitivity"] and a["runs"]["cross"]]
    assert pair == [c["seed"] for c in cases if c["driver"] in ("prims", "prims_batch")] and len(pair) == 19
    att = [c["seed"] for c, a in zip(cases, axes) if a["runs"]["attribution"]]
    assert att == [c["seed"] for c in cases if c["driver"] in ("prims", "prims_batch", "coords", "dmxs")] and len(att) == 28
    for c, a in zip(cases, axes):
        for family in fq.FAMILIES:
            assert (family in a["fit"]) == a["runs"][family]  # zero seeds are left out after fitting
            if a["runs"][family]:
                assert not fq.refusals(a["fit"][family])[family] or family == "cross"
                assert family == "cross" or len(a["refused"][family]) == len(a["changed"][family])  # one change per refusal, no other
                assert a["changed"][family] or (a["fit"][family]["ncat"] == c["ncat"] and a["fit"][family]["sd"] == c["sd"] and a["fit"][family]["boundary"] == c["boundary"])


def test_every_value_of_the_new_axes_occurs(drawn):
    cases, axes = drawn
    unfitted = {c["seed"] for c, a in zip(cases, axes) if a["runs"]["attribution"] and not a["changed"]["attribution"]}
    assert unfitted >= {1, 2, 3, 20, 22, 33, 37, 38} and all(fs.is_periodic(cases[s]) for s in (2, 3, 33, 38))
    sessions = {c["seed"] for c, a in zip(cases, axes) if a["runs"]["cross"] and c["driver"] == "prims" and fs.is_periodic(c) and c["entry"] == "session"}
    assert sessions == {3, 9, 24, 27, 36, 39}
    for family in ("attribution", "sensitivity"):
        assert {a["fit"][family]["ncat"] for c, a in zip(cases, axes) if a["runs"][family] and c["ncat"] > 64} == set(fq.W_ROTATION)
    cross = [(c, a["cross"]) for c, a in zip(cases, axes) if a["runs"]["cross"]]
    assert {x["nb"] for _, x in cross} == {1, 63, 64, 65, 80} and {x["na"] for _, x in cross} == {1, 5, 12}
    assert {x["k"] for _, x in cross} == {1, 2, 8, 63, 64} and any(x["k"] == x["nb"] == 64 for _, x in cross)
    assert {x["tile_name"] for _, x in cross} == {0, 1, 5, "Na"}
    assert all(len(set(x["anchors_b"])) < x["nb"] for _, x in cross if x["nb"] > 1)  # exact ties for nearest
    assert any(c["ncat"] > 255 for c, _ in cross) and any(x["key"] is not None for _, x in cross)
    assert any(c["driver"] == "prims_batch" and len(x["groups"]) > 1 for c, x in cross)
    assert any("tag_pairs" in (c["rule"] or {}) for c, _ in cross) and any(c["rule"] is None for c, _ in cross)
    assert any(np.isinf(c["thr"]) for c, _ in cross)
    # what the family files never reach
    att = [(c, a) for c, a in zip(cases, axes) if a["runs"]["attribution"]]
    assert any(c["driver"] == "prims" and fs.is_periodic(c) and c["unwrapped"] and c["lattice"] for c, _ in att)
    assert {c["cell_kind"] for c, _ in att if fs.is_periodic(c)} >= {"skewed", "dodecahedron"}
    assert {a["fit"]["attribution"]["sd"][1][0] for _, a in att} >= {1.0, 2.0} and any(a["fit"]["attribution"]["sd"][1][0] not in (1.0, 2.0) for _, a in att)
    sens = [a["fit"]["sensitivity"] for _, a in att if a["runs"]["sensitivity"]]
    assert {f["sd"][0] for f in sens} == {"Hellinger", "Kolmogorov-Smirnov", "Kullback-Leibler", "Renyi"}
    assert {(f["wfs"] if not f["multi"] else list(f["wfs"].values())[0])[0] for f in sens} >= {"dagum", "kumaraswamy", "hyper_exp", "uniform"}
    assert any(s % 4 == 3 for s in (f["seed"] for f in sens)) and any(f["driver"] == "prims_batch" and f["entry"] == "session" for f in sens)


def _quotient(sides, side, k, ncat, wf, sd, weights, step):
    out = []
    for sign in (+1, -1):
        moved = [(c, d.copy()) for c, d in sides]
        moved[side][1][k] += sign * step
        out.append(model.score(moved[0][0], moved[0][1], moved[1][0], moved[1][1], ncat, wf, sd, weights))
    return (out[0] - out[1]) / (2 * step)


def _richardson(q, step):
    return (4 * q(step / 2) - q(step)) / 3


@pytest.mark.parametrize("seed", range(max(N_SEEDS, len(DEFAULT))))
def test_references_against_each_other(oracle, seed):
    case = fs.draw(seed)
    ax = fq.pair_axes(case)
    if ax["runs"]["attribution"]:
        fit = ax["fit"]["attribution"]
        rows, items = fq.attribution_reference(fit, ax)
        assert rows.shape == (len(items), fit["ncat"]) and len(rows) >= 1 and np.all(np.isfinite(rows)) and np.all(rows >= 0.0)
        want = np.asarray([model.score(ca, da, cb, db, fit["ncat"], fp._wf(fit, key), fit["sd"], fit["weights"]) for _, key, (ca, da), (cb, db) in items])
        err = float(np.max(np.abs(rows.sum(1) - want) / np.maximum(1.0, np.abs(want))))
        print(seed, "attribution row sums vs integral_form.score:", err)
        assert err < TOL
        orc = fq.sampled_scores(fit, ax, oracle)
        assert float(np.max(np.abs(rows.sum(1) - orc) / np.maximum(1.0, np.abs(orc)))) < TOL
    if not ax["runs"]["sensitivity"]:
        return
    fit = ax["fit"]["sensitivity"]
    sens = fq.sensitivity_reference(fit, ax)
    clouds = fq.sensitivity_clouds(fit)
    pairs = fq.sensitivity_pairs(fit, ax)
    want = np.asarray([model.score(clouds[a][1][sens.idx_a[r, :sens.count_a[r]]], sens.dist_a[r, :sens.count_a[r]],
                                   clouds[b][1][sens.idx_b[r, :sens.count_b[r]]], sens.dist_b[r, :sens.count_b[r]], fit["ncat"], fp._wf(fit, key),
                                   fit["sd"], fit["weights"]) for r, (_, a, b, _, _, key) in enumerate(pairs)])
    err = float(np.max(np.abs(sens.scores - want) / np.maximum(1.0, np.abs(want))))
    print(seed, "sensitivity model scores vs integral_form.score:", err)
    assert err < TOL and np.all(np.isfinite(sens.g_a)) and np.all(np.isfinite(sens.g_b))
    orc = fq.sampled_scores(fit, ax, oracle)
    assert float(np.max(np.abs(sens.scores - orc) / np.maximum(1.0, np.abs(orc)))) < TOL
    if fit["lattice"]:
        return
    # g against a Richardson-extrapolated central difference of the model score, on two members.  The quotient's own error is measured
    # on F against the density with the same steps (tests/test_sensitivity_model.py) and scales with |H- - H+| = |g| / w; the rounding
    # of two float64 scores adds 2 * 1.1e-16 max(1, |S|) / (2 h) per quotient.
    rng = np.random.default_rng(fq.STREAM + 500_000_000 + seed)
    done = 0
    for r in rng.permutation(len(pairs)):
        _, a, b, _, _, key = pairs[r]
        wf = fp._wf(fit, key)
        na, nb = int(sens.count_a[r]), int(sens.count_b[r])
        sides = [(clouds[a][1][sens.idx_a[r, :na]], sens.dist_a[r, :na].copy()), (clouds[b][1][sens.idx_b[r, :nb]], sens.dist_b[r, :nb].copy())]
        edges = np.asarray(wf[1][:2]) if wf[0] in ("uniform", "kumaraswamy") else np.zeros(0)
        pts = np.sort(np.concatenate([sides[0][1], sides[1][1][1:], edges]))
        side = int(rng.integers(2))
        g, d = (sens.g_a, sens.g_b)[side][r], sides[side][1]
        if len(d) < 2:
            continue
        k = int(rng.integers(1, len(d)))
        gap = float(np.min(np.abs(pts[pts != d[k]] - d[k]), initial=np.inf)) if np.count_nonzero(pts == d[k]) == 1 else 0.0
        step = min(2e-4, gap / 10)
        if step < 1e-6:
            continue
        w = float(su.pdf(wf[0], wf[1], [d[k]])[0])
        own = abs(_richardson(lambda st: float((model.cdf(wf[0], wf[1], [d[k] + st])[0] - model.cdf(wf[0], wf[1], [d[k] - st])[0]) / (2 * st)), step) - w)
        quot = _richardson(lambda st: _quotient(sides, side, k, fit["ncat"], wf, fit["sd"], fit["weights"], st), step)
        scale = max(1.0, abs(float(g[k])) / w) if w > 0 else 1.0
        bound = 16 * max(own, 1.1e-16 * max(1.0, abs(sens.scores[r])) / step) * scale
        print(seed, f"pair {r} side {side} member {k}: g = {float(g[k]):.6g}, quotient = {quot:.6g}, bound {bound:.3g}")
        assert abs(float(g[k]) - quot) <= bound
        done += 1
        if done == 2:
            break


# ---- mutation checks: a reference that survives one of these would not notice the same mistake in the library ------------------------
def _differs(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)), initial=0.0)) > 1e-7


def test_mutations_change_the_references(oracle, drawn):
    cases, axes = drawn
    hits = {"sides": {f: [] for f in fq.FAMILIES}, "rule": {f: [] for f in ("sensitivity", "cross")}, "open": {f: [] for f in ("attribution", "cross")}}
    for c, a in zip(cases, axes):
        if c["seed"] % 3 and c["driver"] == "prims":
            continue  # (a third of the from_primitives seeds and every other driver's: the check is about the references, not the seeds)
        if a["runs"]["attribution"]:
            fit = a["fit"]["attribution"]
            rows, _ = fq.attribution_reference(fit, a)
            # (a row is symmetric in its sides by definition: swapping them must NOT change it, swapping one side's columns must)
            assert not _differs(fq.attribution_reference(fit, a, swap_sides=True)[0], rows)
            if fs.is_periodic(fit) and _differs(fq.attribution_reference(fs.open_twin(fit), a)[0], rows):
                hits["open"]["attribution"].append(c["seed"])
        if a["runs"]["sensitivity"]:
            fit = a["fit"]["sensitivity"]
            ref = fq.sensitivity_reference(fit, a)
            swapped = fq.sensitivity_reference(fit, a, swap_sides=True)
            if _differs(swapped.g_a, ref.g_a) or _differs(swapped.g_b, ref.g_b):
                hits["sides"]["sensitivity"].append(c["seed"])
            if fit["rule"] != {"accept_same": True} and not np.array_equal(fq.sensitivity_reference(fit, a, rule={"accept_same": True}).count_a, ref.count_a):
                hits["rule"]["sensitivity"].append(c["seed"])
        if a["runs"]["cross"] and a["cross"]["na"] * a["cross"]["nb"] <= 400:
            want = fq.cross_reference(c, a, oracle)
            if _differs(fq.cross_reference(c, a, oracle, swap_sides=True), want):
                hits["sides"]["cross"].append(c["seed"])
            if c["rule"] != {"accept_same": True} and _differs(fq.cross_reference(c, a, oracle, rule={"accept_same": True}), want):
                hits["rule"]["cross"].append(c["seed"])
            if fs.is_periodic(c) and _differs(fq.cross_reference(fs.open_twin(c), a, oracle), want):
                hits["open"]["cross"].append(c["seed"])
    print(hits)
    assert hits["sides"]["sensitivity"] and hits["sides"]["cross"]
    assert hits["rule"]["sensitivity"] and hits["rule"]["cross"]
    assert hits["open"]["attribution"] and hits["open"]["cross"]
