"""The draw and the CPU references of the whole-surface fuzz (tests/fuzz_surface.py) on their own: what the default seeds cover, that the
oracle's scores of every seed are finite and inside the library's conditions, that one layer of images is all a periodic from_primitives
environment can hold, and that the image-cloud / brute-force-row references give the same score through tests/integral_form.py.  CPU only."""
import itertools
import os

import numpy as np
import pytest

import fuzz_surface as fs
from min_image_util import brute_min_image, brute_rows

N_SEEDS = int(os.environ.get("LCHD_FUZZ_SEEDS", "40"))
DEFAULT = range(40)  # the coverage below is a property of the default range
TOL = 1e-12          # tests/test_integral_form.py


@pytest.fixture(scope="module")
def cases():
    return [fs.draw(s) for s in DEFAULT]


@pytest.fixture(scope="module")
def wants(oracle):
    """expected() of every seed that is run, computed once."""
    return {s: fs.expected(fs.draw(s), oracle) for s in range(max(N_SEEDS, len(DEFAULT)))}


def flat(want):
    return np.concatenate([np.ravel(w) for w in want]) if isinstance(want, list) else np.ravel(want)


def test_draw_is_a_function_of_the_seed():
    a, b = fs.draw(12), fs.draw(12)  # a from_primitives seed
    assert a["pairs"] == b["pairs"] and np.array_equal(a["xa"], b["xa"]) and a["thr"] == b["thr"] and a["wfs"] == b["wfs"]


def test_every_value_of_every_axis_occurs(cases):
    def seen(f):
        return {f(c) for c in cases}
    assert seen(lambda c: c["driver"]) == set(fs.DRIVERS)
    assert seen(lambda c: c["boundary"]) == {"open", "box", "cell", "mixed"}
    assert seen(lambda c: c["det"]) == {False, True}
    assert seen(lambda c: c["entry"]) == {"host", "session"}
    assert seen(lambda c: c["ncat"]) == set(fs.BIG_CATS) | set(fs.OLD_CATS)
    assert seen(lambda c: c["multi"]) == {False, True}
    assert seen(lambda c: len(c["wfs"]) if c["multi"] else 1) >= {1, 2, 3, 4}
    assert seen(lambda c: c["weights"] is None) == {False, True}
    assert seen(lambda c: c["sd"][0]) == {"Hellinger", "Kolmogorov-Smirnov", "Kullback-Leibler", "Renyi"}
    families = {"hyper_exp", "dagum", "uniform", "kumaraswamy"}
    assert {c["wfs"][0] for c in cases if not c["multi"]} == families                      # as the single function ...
    assert {w[0] for c in cases if c["multi"] for w in c["wfs"].values()} == families       # ... and inside a dictionary
    assert {len(w[1]) for c in cases for w in (c["wfs"].values() if c["multi"] else [c["wfs"]]) if w[0] == "hyper_exp"} == {2, 6}
    assert {(c["sd"][0], c["sd"][1] == [2.0]) for c in cases if c["sd"][0] == "Hellinger"} == {("Hellinger", True), ("Hellinger", False)}
    assert seen(lambda c: c["lattice"]) == {False, True}
    periodic = [c for c in cases if fs.is_periodic(c)]
    assert {c["cell_kind"] for c in periodic} >= set(fs.CELL_KINDS)
    assert {c["unwrapped"] for c in periodic} == {False, True}
    prims = [c for c in cases if c["driver"] in ("prims", "prims_batch")]
    assert {None if c["rule"] is None else tuple(sorted(k for k in c["rule"] if k != "tag_pairs")) for c in prims} == \
        {None, ("accept_same",), ("accepted_pairs", "ordered")}
    assert {c["rule"]["accept_same"] for c in prims if c["rule"] and "accept_same" in c["rule"]} == {False, True}
    assert any(c["driver"] == "prims" and np.isinf(c["thr"]) for c in cases)
    # the width itself as the threshold: on a box and in a triclinic cell (where lchd_images.hip culls image shells against the widths)
    wide = [c for c in cases if c["driver"] == "prims" and c["at_width"]]
    assert any(c["boundary"] == "box" for c in wide) and any(c["boundary"] == "cell" and c["cell_kind"] in ("skewed", "dodecahedron") for c in wide)
    for c in wide:
        assert c["inside"] == [p is not None and fs.is_orthorhombic(p) for p in (c["per_a"], c["per_b"])]
    mixed = {(c["per_a"][0], None if c["per_b"] is None else c["per_b"][0]) for c in cases if c["boundary"] == "mixed"}
    assert mixed == {("box", "cell"), ("cell", None)}
    ens = [c for c in cases if c["driver"] in fs.ENSEMBLES]
    assert {c["spairs"] is None for c in ens} == {False, True} and {c["excluded"] is None for c in ens} == {False, True}
    assert {c["block"] for c in ens} == {False, True}
    assert {c["m"] for c in ens} == {2, 3, 4, 5}
    per_structure = {np.ndim(c["per"][1]) == 3 for c in ens if c["per"] is not None and c["per"][0] == "cell"}
    assert per_structure == {False, True}
    # sizes: odd and even dense rows (k_min_image_rows has a two-wide path for even n), more than one trip of a 256-lane workgroup
    dense = [c["n"] for c in cases if c["driver"] == "coords" and fs.is_periodic(c)]
    assert {n % 2 for n in dense} == {0, 1} and max(dense) > 256
    assert max(max(len(c["sa"]), len(c["sb"])) for c in cases if c["driver"] == "prims") > 256


def test_every_allowed_pair_of_axes_occurs(cases):
    def pairs(f, g, keep=lambda c: True):
        return {(f(c), g(c)) for c in cases if keep(c)}
    drv = lambda c: c["driver"]
    want = {(d, b) for d in fs.DRIVERS for b in fs.BOUNDARIES.get(d, ["open"])}
    assert pairs(drv, lambda c: c["boundary"]) == want
    assert pairs(drv, lambda c: c["det"]) == set(itertools.product(fs.DRIVERS, (False, True)))
    assert pairs(drv, lambda c: c["multi"]) == {(d, False) for d in fs.DRIVERS} | {(d, True) for d in fs.DICT_DRIVERS}
    assert pairs(lambda c: c["boundary"], lambda c: c["entry"]) == set(itertools.product(("open", "box", "cell", "mixed"), ("host", "session")))
    assert pairs(drv, lambda c: True, lambda c: c["ncat"] >= 255) == {(d, True) for d in fs.DRIVERS}
    # what the three mutations of the pull request's description need at least twice
    assert sum(c["driver"] == "coords" and fs.is_periodic(c) and c["multi"] for c in cases) >= 2
    weighted = [c for c in cases if c["driver"] in fs.ENSEMBLES and c["weights"] is not None]
    # (Hellinger-2 on its own: its sweep kernels come in a unit-weight and a weighted form, the other distances in one)
    assert sum(c["sd"] == ("Hellinger", [2.0]) for c in weighted) >= 2 and sum(c["sd"] != ("Hellinger", [2.0]) for c in weighted) >= 1
    assert {c["driver"] for c in weighted} == set(fs.ENSEMBLES)
    assert sum(c["driver"] == "prims" and fs.is_periodic(c) for c in cases) >= 2
    # the combinations the issue names as untested: 16-bit category ids in a box and in a cell image cloud, and a dictionary with
    # excluded pairs under blocking in from_coords_ensemble
    assert {c["boundary"] for c in cases if c["driver"] == "prims" and c["ncat"] > 255} >= {"box", "cell"}
    assert any(c["driver"] == "coords_ensemble" and c["multi"] and c["excluded"] is not None and c["block"] for c in cases)


@pytest.mark.parametrize("seed", range(max(N_SEEDS, len(DEFAULT))))
def test_reference_stays_inside_its_conditions(wants, oracle, seed):
    case = fs.draw(seed)
    want, rows = wants[seed]
    assert np.all(np.isfinite(flat(want)))  # nothing is left out of the comparison
    if case["driver"] == "prims" and fs.is_periodic(case):
        for per in (case["per_a"], case["per_b"]):
            assert per is None or 0.0 < case["thr"] <= fs.reach_of(per)
        assert case["thr"] >= 0.2 * min(fs.reach_of(p) for p in (case["per_a"], case["per_b"]) if p is not None)
    if case["driver"] in fs.ENSEMBLES:
        pairs = fs.structure_pairs(case)
        assert len(pairs) >= 1 and want.shape == (len(pairs), len(rows))
        if case["spairs"] is not None:
            assert any(i == k for i, k in pairs) and any((k, i) in pairs for i, k in pairs if i != k)
        if case["excluded"] is not None:
            assert all((c, r) in set(case["excluded"]) for r, c in case["excluded"])
        assert 2 <= case["m"] <= 5 and 30 <= case["n"] <= 200
    if rows is not None:
        assert len(rows) <= fs.MAX_ROWS and rows[0] == 0 and rows[-1] == case["n"] - 1
    if fs.is_periodic(case):  # the oracle itself shows that the periodic keywords matter
        open_want, open_rows = fs.expected(fs.open_twin(case), oracle)
        open_want = open_want if open_rows is not None or rows is None else np.asarray(open_want)[rows]
        assert np.max(np.abs(flat(open_want) - flat(want))) > 1e-6


def periodic_prims_seeds():
    """Four periodic from_primitives seeds: the first at a threshold equal to the width of a triclinic cell, the first at the edge of a
    box, the first other one in a dodecahedron, and the first of the rest."""
    chosen, plain = {}, []
    for s in range(0, 3 * 400, 3):
        c = fs.draw(s)
        if not fs.is_periodic(c):
            continue
        triclinic = c["cell_kind"] in ("skewed", "dodecahedron")
        if c["at_width"] and triclinic and c["boundary"] == "cell" and "width in a cell" not in chosen:
            chosen["width in a cell"] = s
        elif c["at_width"] and c["boundary"] == "box" and "width of a box" not in chosen:
            chosen["width of a box"] = s
        elif c["cell_kind"] == "dodecahedron" and not c["at_width"] and "dodecahedron" not in chosen:
            chosen["dodecahedron"] = s
        elif len(plain) < 1 and not c["at_width"]:
            plain.append(s)
        if len(chosen) == 3 and len(plain) == 1:
            return list(chosen.values()) + plain
    raise AssertionError("the draw offers no such seeds")


@pytest.mark.parametrize("seed", periodic_prims_seeds())
def test_one_layer_of_images_is_enough(seed):
    """On every anchor the (atom, distance) pairs within the threshold from the shifts -1 .. 1 are those from the shifts -3 .. 3."""
    case = fs.draw(seed)
    assert case["driver"] == "prims" and fs.is_periodic(case)
    thr2 = case["thr"] * case["thr"]
    for x, per, col in ((case["xa"], case["per_a"], 0), (case["xb"], case["per_b"], 1)):
        if per is None:
            continue
        near, wide = fs.image_cloud(x, per, 1), fs.image_cloud(x, per, 3)
        assert np.array_equal(near[0][:len(x)], wide[0][:len(x)])
        for anchor in sorted({p[col] for p in case["pairs"]}):
            found = []
            for pts, atom in (near, wide):
                d = pts - pts[anchor]
                d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
                keep = d2 < thr2
                found.append(sorted(zip(atom[keep].tolist(), d2[keep].tolist())))
            assert found[0] == found[1], (seed, anchor)


def test_brute_rows_of_an_unwrapped_dense_seed():
    """brute_rows(span=3), the reference of the periodic dense cases, against a brute force over -7 .. 7 of the displacements as they
    are (tests/test_min_image_host.py has the precedent on its own coordinates)."""
    seed = next(s for s in range(2, 9 * 200, 9) if fs.is_periodic(fs.draw(s)) and fs.draw(s)["unwrapped"] and fs.draw(s)["cell_kind"] in ("skewed", "dodecahedron")
                and fs.draw(s)["per_a"][0] == "cell")
    case = fs.draw(seed)
    cell, x = fs.cell_of(case["per_a"]), case["xa"]
    rows = fs.sampled_rows(case, case["n"])[:6]
    for r, row in zip(rows, brute_rows(x, rows, cell, span=3)):
        want = brute_min_image(x[r] - x, cell, 7)
        assert np.max(np.abs(row - want)) <= 1e-12 * np.max(want)


def integral_seeds():
    ok = [c for c in (fs.draw(s) for s in DEFAULT) if c["driver"] in ("prims", "coords") + fs.ENSEMBLES]
    return [c["seed"] for c in ok if not fs.is_periodic(c)][:6] + [c["seed"] for c in ok if fs.is_periodic(c)][:6]


@pytest.mark.parametrize("seed", integral_seeds())
def test_references_agree_with_the_integral_form(oracle, seed):
    mine, theirs = fs.integral_check(fs.draw(seed), oracle)
    assert len(mine) >= 1 and np.all(np.isfinite(mine))
    err = np.max(np.abs(mine - theirs) / np.maximum(1.0, np.abs(theirs)))
    print(seed, "integral form vs oracle:", err)
    assert err < TOL


def test_integral_seeds_are_six_open_and_six_periodic():
    seeds = integral_seeds()
    assert len(seeds) == 12 and sum(fs.is_periodic(fs.draw(s)) for s in seeds) == 6
