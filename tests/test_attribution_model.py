"""The numpy restatement of the score attribution (tests/attribution_util.py) pinned to the unchanged CPU oracle, without a GPU.

  row sum      a row sums to the oracle's from_primitives score of the pair (exponents 1, 2 and 3.5, every weight-function family,
               category weights, both tag rules)
  projection   exponent 1, unit weights: two-category total variation is |a_c - b_c|, so column c is 1/2 of the oracle's score of the
               same geometry with every category other than c relabelled to one "rest" category
  lattice      both of the above on a lattice, where whole shells of points are tied in distance

Bound 1e-12, restatement against oracle: sums of a few hundred terms of size <= 1, the restatement in longdouble, the oracle in f64."""
import numpy as np
import pytest

import attribution_util as au

CATS = ["A", "B", "C", "D", "E", "F", "G"]
FAMILIES = {
    "uniform": [3.0, 10.0],
    "hyper_exp": [1.0, 0.5, 0.2, 0.05],
    "dagum": [4.0, 6.0, 1.5],
    "kumaraswamy": [2.0, 11.0, 2.0, 3.0],
}
BOUND = 1e-12


class Cloud:
    def __init__(self, seed, n, edge):
        rng = np.random.default_rng(seed)
        self.xyz = rng.uniform(0.0, edge, (n, 3))
        self.cat = rng.integers(0, len(CATS), n)
        self.tag = rng.integers(0, 4, n)

    def atoms(self, oracle, names=None):
        names = [CATS[k] for k in self.cat] if names is None else names
        return [oracle.PrimitiveAtom(t, f"t{g}", list(x)) for t, g, x in zip(names, self.tag, self.xyz)]


@pytest.fixture(scope="module")
def clouds():
    rng = np.random.default_rng(9)
    return Cloud(101, 300, 20.0), Cloud(102, 300, 20.0), [(int(i), int(j)) for i, j in rng.integers(0, 300, (40, 2))]


@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("exponent", [1.0, 2.0, 3.5])
@pytest.mark.parametrize("variant", ["plain", "weighted", "other tags"])
def test_row_sum_is_the_oracle_score(oracle, clouds, family, exponent, variant):
    a, b, pairs = clouds
    wf = (family, FAMILIES[family])
    weights = np.random.default_rng(3).uniform(0.3, 3.0, len(CATS)) if variant == "weighted" else None
    accept_same = variant != "other tags"
    l = oracle.LoCoHD(CATS, oracle.WeightFunction(*wf), oracle.TagPairingRule({"accept_same": accept_same}),
                      category_weights=None if weights is None else list(weights), statistical_distance=oracle.StatisticalDistance("Hellinger", [exponent]))
    want = np.asarray(l.from_primitives(a.atoms(oracle), b.atoms(oracle), pairs, 8.0))
    got = au.from_primitives(a.cat, a.xyz, a.tag, b.cat, b.xyz, b.tag, pairs, 8.0, len(CATS), wf, exponent, weights, accept_same)
    assert got.shape == (40, len(CATS)) and np.all(got >= 0.0)
    worst = float(np.max(np.abs(got.sum(1) - want)))
    print(f"{family} e={exponent} {variant}: max |row sum - oracle| = {worst:.3g}")
    assert worst <= BOUND


def _projection(oracle, a_atoms_of, b_atoms_of, cat_a, cat_b, pairs, thr, wf):
    """Column c from the oracle: 1/2 of the two-category total-variation score, for every c."""
    l = oracle.LoCoHD(["c", "rest"], oracle.WeightFunction(*wf), statistical_distance=oracle.StatisticalDistance("Hellinger", [1.0]))
    cols = []
    for c in range(len(CATS)):
        pa = a_atoms_of(["c" if k == c else "rest" for k in cat_a])
        pb = b_atoms_of(["c" if k == c else "rest" for k in cat_b])
        cols.append(0.5 * np.asarray(l.from_primitives(pa, pb, pairs, thr)))
    return np.stack(cols, 1)


@pytest.mark.parametrize("family", ["uniform", "hyper_exp"])
def test_exponent_1_columns_are_two_category_oracle_scores(oracle, clouds, family):
    a, b, pairs = clouds
    wf = (family, FAMILIES[family])
    want = _projection(oracle, lambda names: a.atoms(oracle, names), lambda names: b.atoms(oracle, names), a.cat, b.cat, pairs, 8.0, wf)
    got = au.from_primitives(a.cat, a.xyz, a.tag, b.cat, b.xyz, b.tag, pairs, 8.0, len(CATS), wf, 1.0)
    worst = float(np.max(np.abs(got - want)))
    print(f"{family}: max |column - projection| = {worst:.3g}")
    assert worst <= BOUND


def test_lattice_with_tied_distances(oracle):
    rng = np.random.default_rng(77)
    g = np.stack(np.meshgrid(*[np.arange(6.0)] * 3, indexing="ij"), -1).reshape(-1, 3) * 1.5  # 216 points, spacing 1.5
    ca, cb = rng.integers(0, 7, len(g)), rng.integers(0, 7, len(g))
    pairs = [(int(i), int(j)) for i, j in rng.integers(0, len(g), (30, 2))]

    def atoms(names):
        return [oracle.PrimitiveAtom(t, "x", list(x)) for t, x in zip(names, g)]

    wf = ("uniform", FAMILIES["uniform"])
    want = _projection(oracle, atoms, atoms, ca, cb, pairs, 6.1, wf)
    got = au.from_primitives(ca, g, None, cb, g, None, pairs, 6.1, 7, wf, 1.0)
    assert np.max(np.abs(got - want)) <= BOUND
    for e in (2.0, 3.5):
        l = oracle.LoCoHD(CATS, oracle.WeightFunction(*wf), statistical_distance=oracle.StatisticalDistance("Hellinger", [e]))
        score = np.asarray(l.from_primitives(atoms([CATS[k] for k in ca]), atoms([CATS[k] for k in cb]), pairs, 6.1))
        rows = au.from_primitives(ca, g, None, cb, g, None, pairs, 6.1, 7, wf, e)
        assert np.max(np.abs(rows.sum(1) - score)) <= BOUND
    same = au.from_primitives(ca, g, None, ca, g, None, [(i, i) for i, _ in pairs], 6.1, 7, wf, 2.0)
    assert np.all(same == 0.0)
