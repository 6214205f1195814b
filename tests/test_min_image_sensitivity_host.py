"""The host side of the dense minimum-image sensitivity calls: every refusal that needs no device, and the gradient assembly
(LoCoHD._assemble_gradient_min_image) against the longdouble model of tests/min_image_sensitivity_util.py on a hand-made
MinImageSensitivity.  No device is touched."""
import numpy as np
import pytest

import min_image_sensitivity_util as mu
from periodic_cell_util import CELLS

CATS = ["c0", "c1", "c2"]
BOX = [20.0, 21.0, 22.0]


@pytest.fixture(scope="module")
def lh():
    import loco_hd_amd

    return loco_hd_amd


@pytest.fixture(scope="module")
def case(lh):
    rng = np.random.default_rng(1)
    n = 12
    x = rng.uniform(0.0, 20.0, (n, 3))
    seq = [CATS[k] for k in rng.integers(0, 3, n)]
    return lh.LoCoHD(CATS, lh.WeightFunction("uniform", [3.0, 10.0])), seq, x


@pytest.mark.parametrize("call", ["sensitivity_from_coords_periodic", "gradient_from_coords_periodic"])
def test_argument_errors(lh, case, call):
    lchd, seq, x = case
    fn = getattr(lchd, call)
    with pytest.raises(ValueError, match="box_a and cell_a were both given"):
        fn(seq, seq, x, x, box_a=BOX, cell_a=CELLS["skewed"])
    with pytest.raises(ValueError, match="box_b and cell_b were both given"):
        fn(seq, seq, x, x, box_b=BOX, cell_b=CELLS["skewed"])
    for bad in ([20.0, 21.0], [[20.0, 21.0, 22.0]] * 2, [20.0, -1.0, 22.0], [20.0, np.nan, 22.0]):
        with pytest.raises(ValueError):
            fn(seq, seq, x, x, box_a=bad)
    with pytest.raises(ValueError, match="shape"):
        fn(seq, seq, x, x, cell_b=np.zeros((3, 2)))
    singular = np.array(CELLS["skewed"])
    singular[2] = singular[0] - 2.0 * singular[1]
    with pytest.raises(ValueError, match="singular"):
        fn(seq, seq, x, x, cell_a=singular)
    with pytest.raises(ValueError, match="same length"):
        fn(seq, seq, x, x[:-1], box_a=BOX)
    with pytest.raises((ValueError, TypeError)):
        fn(seq, seq, x[:, :2], x, box_a=BOX)
    group = lh.LoCoHD(CATS, lh.WeightFunction("uniform", [3.0, 10.0]), devices=[0])
    with pytest.raises(NotImplementedError, match="drop devices"):
        getattr(group, call)(seq, seq, x, x, box_a=BOX)


def test_width_and_weights(case):
    lchd, seq, x = case
    with pytest.raises(ValueError, match="at least one member"):
        lchd.sensitivity_from_coords_periodic(seq, seq, x, x, width=0, box_a=BOX)
    with pytest.raises(ValueError, match="pair_weights has 3 entries for 12 rows"):
        lchd.gradient_from_coords_periodic(seq, seq, x, x, pair_weights=[1.0, 2.0, 3.0], box_a=BOX)


def test_the_open_calls_keep_refusing_periodic_keywords(case):
    lchd, seq, x = case
    with pytest.raises(TypeError):
        lchd.sensitivity_from_coords(seq, seq, x, x, box_a=BOX)
    with pytest.raises(TypeError):
        lchd.gradient_from_coords(seq, seq, x, x, cell_a=CELLS["skewed"])


def test_named_tuple_and_export(lh):
    assert lh.MinImageSensitivity._fields == ("scores", "count_a", "idx_a", "dist_a", "g_a", "disp_a", "count_b", "idx_b", "dist_b", "g_b",
                                              "disp_b")
    assert "MinImageSensitivity" in lh.__all__


@pytest.mark.parametrize("width", [None, 19])
def test_gradient_assembly_equals_the_model(lh, width):
    """A hand-made MinImageSensitivity: the model's lists and displacements in a skewed cell (side A) and a box (side B), g replaced by
    random numbers with a NaN and a zero distance among them; padded rows with `width`."""
    from loco_hd_amd.api import cell_reduce

    rng = np.random.default_rng(7)
    n = 16
    per_a, per_b = ("cell", CELLS["skewed"] * 0.6), ("box", np.asarray([11.0, 12.5, 10.0]))
    xa, xb = rng.uniform(-1.0, 2.0, (n, 3)) @ per_a[1], rng.uniform(0.0, 1.0, (n, 3)) * per_b[1]
    xb[9] = [2.5, 3.25, 4.0]
    xb[3] = xb[9] + np.asarray([per_b[1][0], 0.0, 0.0])  # one lattice vector apart (exactly: every number is a dyadic fraction): a member at distance 0 beyond slot 0
    ca, cb = rng.integers(0, 3, n), rng.integers(0, 3, n)
    ms = mu.sensitivity(ca, xa, per_a, cb, xb, per_b, 3, ("uniform", [3.0, 10.0]), width=width, reduce=cell_reduce)
    k = ms.idx_a.shape[1]
    g_a, g_b = rng.normal(0.0, 1.0, (n, k)), rng.normal(0.0, 1.0, (n, k))
    g_a[2, 5] = np.nan
    g_a[ms.idx_a < 0] = 0.0
    g_b[ms.idx_b < 0] = 0.0
    assert (ms.dist_b[:, 1:n] == 0.0).any()
    hand = lh.MinImageSensitivity(ms.scores, ms.count_a, ms.idx_a, ms.dist_a, g_a, ms.disp_a, ms.count_b, ms.idx_b, ms.dist_b, g_b, ms.disp_b)
    v = rng.uniform(0.5, 2.0, n)
    for weights in (None, v):
        got = lh.LoCoHD._assemble_gradient_min_image(hand, weights)
        want = mu.gradient(mu.MSens(*hand), weights)
        for side in range(2):
            err = float(np.max(np.abs(got[side] - want[side])))
            print("width", width, "weights" if weights is not None else "ones", "side", side, "max |assembly - model| =", err)
            assert got[side].shape == (n, 3) and np.isfinite(got[side]).all()
            # 2 n terms of magnitude <= max |v g| per component, each rounded once, summed in f64 against longdouble
            assert err <= 4 * n * np.finfo(np.float64).eps * float(np.nanmax(np.abs(g_a)) + np.nanmax(np.abs(g_b))) * 2.0
    with pytest.raises(ValueError, match="pair_weights has 3 entries"):
        lh.LoCoHD._assemble_gradient_min_image(hand, [1.0, 2.0, 3.0])
