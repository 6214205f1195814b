"""Host layer of the sensitivity calls: the weight-function densities, argument errors that need no device, and the host assembly of
the coordinate gradient.  CPU only."""
import numpy as np
import pytest

import loco_hd_amd as lh
from loco_hd_amd import _native as N
from loco_hd_amd.api import Sensitivity

FAMILIES = {"hyper_exp": [1.0, 0.5, 0.2, 0.05], "dagum": [4.0, 6.0, 1.5], "uniform": [3.0, 10.0], "kumaraswamy": [2.0, 11.0, 2.0, 3.0]}
KINDS = {"hyper_exp": 0, "dagum": 1, "uniform": 2, "kumaraswamy": 3}


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_wf_pdf_against_central_differences_of_wf_cdf(family):
    """h = 1e-5: truncation h^2 / 6 * |F'''| (< 2e-11 for these parameters away from support edges) + rounding 2.2e-16 / (2 h) = 1.1e-11."""
    p = np.asarray(FAMILIES[family])
    x = np.linspace(3.2, 9.8, 34)
    h = 1e-5
    lib = N.lib()
    out, up, dn = np.empty_like(x), np.empty_like(x), np.empty_like(x)
    N.check(lib.lchd_wf_pdf(KINDS[family], N.dp(p), len(p), N.dp(x), len(x), N.dp(out)))
    N.check(lib.lchd_wf_cdf(KINDS[family], N.dp(p), len(p), N.dp(x + h), len(x), N.dp(up)))
    N.check(lib.lchd_wf_cdf(KINDS[family], N.dp(p), len(p), N.dp(x - h), len(x), N.dp(dn)))
    err = float(np.max(np.abs(out - (up - dn) / (2 * h))))
    print(f"{family}: max |pdf - central difference| = {err:.3g}")
    assert err <= 5e-11
    w = lh.WeightFunction(family, FAMILIES[family])
    assert w.density_vec(x) == out.tolist() and w.density_point(5.0) == w.density_vec([5.0])[0]
    assert w.density_point(-1.0) == 0.0


def test_uniform_density_is_a_box():
    w = lh.WeightFunction("uniform", [3.0, 10.0])
    assert w.density_vec([0.0, 2.999, 3.0, 9.999, 10.0, 12.0]) == [0.0, 0.0, 1 / 7, 1 / 7, 0.0, 0.0]
    assert lh.WeightFunction("kumaraswamy", FAMILIES["kumaraswamy"]).density_vec([1.0, 12.0]) == [0.0, 0.0]


def _atoms(n=6):
    return [lh.PrimitiveAtom("A", "t", [float(k), 0.0, 0.0]) for k in range(n)]


def test_argument_errors_before_any_device_is_touched():
    l = lh.LoCoHD(["A"], lh.WeightFunction("uniform", [3.0, 10.0]))
    at = _atoms()
    for kw in ({"box_a": [20.0, 20.0, 20.0]}, {"box_b": [20.0, 20.0, 20.0]}, {"cell_a": np.eye(3) * 20.0}, {"cell_b": np.eye(3) * 20.0}):
        with pytest.raises(NotImplementedError, match="boxes and cells"):
            l.sensitivity_from_primitives(at, at, [(0, 1)], 5.0, **kw)
        with pytest.raises(NotImplementedError, match="boxes and cells"):
            l.gradient_from_primitives(at, at, [(0, 1)], 5.0, **kw)
    with pytest.raises(NotImplementedError, match="device group"):
        lh.LoCoHD(["A"], lh.WeightFunction("uniform", [3.0, 10.0]), devices=[0, 1]).sensitivity_from_primitives(at, at, [(0, 1)], 5.0)
    with pytest.raises(ValueError):
        l.sensitivity_from_primitives(at, at, [(0, 1)], 5.0, width=0)
    d = lh.LoCoHD(["A"], {"u": lh.WeightFunction("uniform", [3.0, 10.0]), "h": lh.WeightFunction("hyper_exp", [1.0, 0.5])})
    with pytest.raises(ValueError):
        d.sensitivity_from_primitives(at, at, [(0, 1, "no-such-key")], 5.0)
    with pytest.raises(ValueError):
        d.sensitivity_from_primitives(at, at, [(0, 1)], 5.0)  # a dictionary needs a key per pair


def test_c_abi_refuses_null_arguments():
    lib = N.lib()
    nul = [None] * 9
    assert lib.lchd_sensitivity_primitives_dev(None, None, None, None, None, 1, 5.0, 8, *nul) == N.EVALUE
    assert lib.lchd_sensitivity_primitives(None, None, None, None, None, 0, None, None, None, 0, None, None, 1, 5.0, 8, *nul) == N.EVALUE
    assert lib.lchd_sensitivity_needed_width(None) == 0


def test_gradient_assembly_on_a_hand_made_tuple():
    xa = np.asarray([[0.0, 0.0, 0.0], [3.0, 0.0, 0.0], [0.0, 4.0, 0.0], [0.0, 0.0, 0.0]])
    xb = np.asarray([[1.0, 1.0, 1.0], [1.0, 1.0, 3.0]])
    sens = Sensitivity(
        scores=np.asarray([0.5, 0.25]), count_a=np.asarray([4, 1], dtype=np.int32),
        idx_a=np.asarray([[0, 3, 1, 2], [2, -1, -1, -1]], dtype=np.int32), dist_a=np.asarray([[0.0, 0.0, 3.0, 4.0], [0.0, 0.0, 0.0, 0.0]]),
        g_a=np.asarray([[0.0, 9.0, 2.0, -1.0], [0.0, 0.0, 0.0, 0.0]]), count_b=np.asarray([2, 2], dtype=np.int32),
        idx_b=np.asarray([[0, 1], [1, 0]], dtype=np.int32), dist_b=np.asarray([[0.0, 2.0], [0.0, 2.0]]), g_b=np.asarray([[0.0, 0.5], [0.0, 0.25]]))
    ga, gb = lh.LoCoHD._assemble_gradient(sens, xa, xb, pair_weights=[2.0, 4.0])
    # pair 0, side A: atom 3 sits on the anchor (d == 0: skipped); atom 1: 2 * 2 * (3, 0, 0) / 3; atom 2: 2 * -1 * (0, 4, 0) / 4
    assert np.array_equal(ga, [[-4.0, 2.0, 0.0], [4.0, 0.0, 0.0], [0.0, -2.0, 0.0], [0.0, 0.0, 0.0]])
    # side B: pair 0 moves atom 1 along +z by 2 * 0.5, pair 1 (anchor 1) moves atom 0 along -z by 4 * 0.25
    assert np.array_equal(gb, [[0.0, 0.0, -1.0 - 1.0], [0.0, 0.0, 1.0 + 1.0]])
    ones_a, _ = lh.LoCoHD._assemble_gradient(sens, xa, xb)
    assert np.array_equal(ones_a, ga / 2.0)
    with pytest.raises(ValueError):
        lh.LoCoHD._assemble_gradient(sens, xa, xb, pair_weights=[1.0])
