"""Host layer of the reduced parameter-gradient calls: the tile planner's arithmetic and what the Python layer refuses before a device is
needed.  CPU only."""
import ctypes as C

import numpy as np
import pytest

import loco_hd_amd as lh
from loco_hd_amd import _native as N


def _plan(n_pairs, row_doubles, budget):
    out = C.c_int64(-1)
    rc = N.lib().lchd_param_sum_plan(n_pairs, row_doubles, budget, C.byref(out))
    return rc, out.value


@pytest.mark.parametrize("n_pairs,row_doubles", [(1, 1), (12, 5), (10 ** 6, 10), (10 ** 6, 64), (10 ** 6, 17)])
def test_plan_is_the_budget_over_the_bytes_of_a_pair_clamped(n_pairs, row_doubles):
    per_pair = 8 * row_doubles + 20  # the row; the pass's 16-byte pair record and 4-byte list entry
    last = 0
    for budget in sorted((0, 1, per_pair - 1, per_pair, 2 * per_pair + 5, 10 ** 6, 10 ** 9, 2 ** 62)):
        rc, tile = _plan(n_pairs, row_doubles, budget)
        assert rc == N.OK and tile == max(1, min(n_pairs, budget // per_pair)), (budget, tile)
        assert tile >= last
        last = tile
    assert f"tile * (8 row_doubles + 20) <= budget_bytes" in (N._PKG.parent / "include" / "loco_hd_hip.h").read_text()


def test_plan_refuses_bad_arguments():
    for args in ((0, 8, 100), (-3, 8, 100), (5, 0, 100), (5, 66, 100), (5, 8, -1)):
        rc, tile = _plan(*args)
        assert rc == N.EVALUE and tile == 0, args
    assert N.lib().lchd_param_sum_plan(5, 8, 100, None) == N.EVALUE


def _atoms(n=6):
    return [lh.PrimitiveAtom("A", "t", [float(k), 0.0, 0.0]) for k in range(n)]


def _locohd(sd=None, wf=("uniform", [3.0, 10.0]), **kw):
    if sd is not None:
        kw["statistical_distance"] = lh.StatisticalDistance(*sd)
    return lh.LoCoHD(["A"], lh.WeightFunction(*wf), **kw)


def test_argument_errors_before_any_device_is_touched():
    l, at = _locohd(), _atoms()
    xyz, seq = np.asarray([a.coordinates for a in at]), ["A"] * 6
    for call in (l.category_gradient_sum_from_primitives, l.weight_gradient_sum_from_primitives):
        with pytest.raises(ValueError, match="tile_pairs = -1 is negative"):
            call(at, at, [(0, 1)], 5.0, tile_pairs=-1)
        with pytest.raises(ValueError, match="pair_weights has 2 entries for 1 anchor pairs"):
            call(at, at, [(0, 1)], 5.0, pair_weights=[1.0, 2.0])
        with pytest.raises(ValueError, match="pair_weights must be real numbers"):
            call(at, at, [(0, 1)], 5.0, pair_weights=np.asarray([1.0 + 2.0j]))
        with pytest.raises(ValueError, match="pair_weights must be real numbers"):
            call(at, at, [(0, 1)], 5.0, pair_weights=["heavy"])
    for call in (l.category_gradient_sum_from_coords, l.weight_gradient_sum_from_coords):
        with pytest.raises(ValueError, match="pair_weights has 5 entries for 6 rows"):
            call(seq, seq, xyz, xyz, pair_weights=np.ones(5))
        with pytest.raises(ValueError, match="same length"):
            call(seq, seq, xyz, xyz[:5])
    with pytest.raises(ValueError, match="box_a and cell_a were both given"):
        l.category_gradient_sum_from_primitives(at, at, [(0, 1)], 5.0, box_a=[20.0] * 3, cell_a=np.eye(3) * 20.0)


@pytest.mark.parametrize("sd", [("Kolmogorov-Smirnov", []), ("Renyi", [2.5, 1e-3])])
def test_category_sum_is_refused_under_the_distances_the_per_pair_call_refuses(sd):
    l, at = _locohd(sd), _atoms()
    xyz, seq = np.asarray([a.coordinates for a in at]), ["A"] * 6
    with pytest.raises(NotImplementedError, match=sd[0]):
        l.category_gradient_sum_from_primitives(at, at, [(0, 1)], 5.0)
    with pytest.raises(NotImplementedError, match=sd[0]):
        l.category_gradient_sum_from_coords(seq, seq, xyz, xyz)


def test_weight_sum_limits():
    at = _atoms()
    xyz, seq = np.asarray([a.coordinates for a in at]), ["A"] * 6
    wide = _locohd(wf=("hyper_exp", [1.0] * 9 + [0.1 * (k + 1) for k in range(9)]))  # 18 parameters
    with pytest.raises(NotImplementedError, match="at most 16 parameters"):
        wide.weight_gradient_sum_from_primitives(at, at, [(0, 1)], 5.0)
    with pytest.raises(NotImplementedError, match="at most 16 parameters"):
        wide.weight_gradient_sum_from_coords(seq, seq, xyz, xyz)
    l = _locohd()
    for kw in ({"box_a": [20.0, 20.0, 20.0]}, {"box_b": [20.0, 20.0, 20.0]}, {"cell_a": np.eye(3) * 20.0}, {"cell_b": np.eye(3) * 20.0}):
        with pytest.raises(NotImplementedError, match="boxes and cells"):
            l.weight_gradient_sum_from_primitives(at, at, [(0, 1)], 5.0, **kw)
        with pytest.raises(NotImplementedError, match="boxes and cells"):
            l.weight_gradient_sum_from_coords(seq, seq, xyz, xyz, **kw)
    grouped = _locohd(devices=[0, 1])
    with pytest.raises(NotImplementedError, match="device group"):
        grouped.weight_gradient_sum_from_primitives(at, at, [(0, 1)], 5.0)
    with pytest.raises(NotImplementedError, match="device group"):
        grouped.category_gradient_sum_from_primitives(at, at, [(0, 1)], 5.0)


def test_c_abi_refuses_null_and_negative_arguments():
    lib = N.lib()
    assert lib.lchd_category_gradient_sum_primitives_dev(None, None, None, None, None, 1, 5.0, None, 0, None) == N.EVALUE
    assert lib.lchd_weight_gradient_sum_primitives_dev(None, None, None, None, None, 1, 5.0, None, 0, None, None) == N.EVALUE
    assert lib.lchd_category_gradient_sum_coords_dev(None, None, None, None, None, None, None, None) == N.EVALUE
    assert lib.lchd_weight_gradient_sum_coords_dev(None, None, None, None, None, None, None) == N.EVALUE
    assert lib.lchd_category_gradient_sum_primitives(None, None, None, None, None, 0, None, None, None, 0, None, None, 0, 5.0, None, None, None,
                                                     None, None, 0, None) == N.EVALUE
    assert lib.lchd_weight_gradient_sum_coords(None, None, None, 0, None, 0, None, None, 0, None, None, None, None) == N.EVALUE
