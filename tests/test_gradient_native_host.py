"""Host layer of the native gradient calls: the tile planner's arithmetic and the argument errors that need no device.  CPU only."""
import ctypes as C

import numpy as np
import pytest

import loco_hd_amd as lh
from loco_hd_amd import _native as N


def _plan(n_pairs, width, budget):
    out = C.c_int64(-1)
    rc = N.lib().lchd_gradient_plan(n_pairs, width, budget, C.byref(out))
    return rc, out.value


def test_header_constants_and_binding_agree():
    text = (N._PKG.parent / "include" / "loco_hd_hip.h").read_text()
    for name, value in (("LCHD_GRAD_LIMBS", "8"), ("LCHD_GRAD_QUANTUM_LOG2", "(-192)"), ("LCHD_GRAD_LIMIT_LOG2", "63")):
        assert f"#define {name} {value}" in text
    assert (N.GRAD_LIMBS, N.GRAD_QUANTUM_LOG2, N.GRAD_LIMIT_LOG2) == (8, -192, 63)
    assert 32 * N.GRAD_LIMBS + N.GRAD_QUANTUM_LOG2 == N.GRAD_LIMIT_LOG2 + 1  # the limbs span 2^-192 .. 2^64: a sign bit above the limit


@pytest.mark.parametrize("n_pairs,width", [(1, 1), (12, 128), (100000, 140), (10 ** 6, 65535)])
def test_plan_is_the_budget_over_the_bytes_of_a_pair_clamped(n_pairs, width):
    per_pair = 40 * width + 16  # idx (4), dist (8), g (8) per slot and side; the score and the two counts
    last = 0
    for budget in sorted((0, 1, per_pair - 1, per_pair, 2 * per_pair + 5, 10 ** 6, 10 ** 9, 10 ** 12, 2 ** 62)):
        rc, tile = _plan(n_pairs, width, budget)
        assert rc == N.OK and tile == max(1, min(n_pairs, budget // per_pair)), (budget, tile)
        assert 1 <= tile <= n_pairs and tile >= last  # clamped, monotone in the budget
        last = tile
    assert _plan(n_pairs, width, 2 ** 62)[1] == n_pairs


def test_plan_refuses_bad_arguments():
    for args in ((0, 8, 100), (-3, 8, 100), (5, 0, 100), (5, 65536, 100), (5, 8, -1)):
        rc, tile = _plan(*args)
        assert rc == N.EVALUE and tile == 0, args
    assert N.lib().lchd_gradient_plan(5, 8, 100, None) == N.EVALUE


def _atoms(n=6):
    return [lh.PrimitiveAtom("A", "t", [float(k), 0.0, 0.0]) for k in range(n)]


def test_argument_errors_before_any_device_is_touched():
    l = lh.LoCoHD(["A"], lh.WeightFunction("uniform", [3.0, 10.0]))
    at = _atoms()
    with pytest.raises(ValueError, match="tile_pairs = -1 is negative"):
        l.native_gradient_from_primitives(at, at, [(0, 1)], 5.0, tile_pairs=-1)
    with pytest.raises(ValueError, match="pair_weights has 2 entries for 1 anchor pairs"):
        l.native_gradient_from_primitives(at, at, [(0, 1)], 5.0, pair_weights=[1.0, 2.0])
    for kw in ({"box_a": [20.0, 20.0, 20.0]}, {"box_b": [20.0, 20.0, 20.0]}, {"cell_a": np.eye(3) * 20.0}, {"cell_b": np.eye(3) * 20.0}):
        with pytest.raises(NotImplementedError, match="boxes and cells"):
            l.native_gradient_from_primitives(at, at, [(0, 1)], 5.0, **kw)
    grouped = lh.LoCoHD(["A"], lh.WeightFunction("uniform", [3.0, 10.0]), devices=[0, 1])
    with pytest.raises(NotImplementedError, match="device group"):
        grouped.native_gradient_from_primitives(at, at, [(0, 1)], 5.0)
    xyz = np.asarray([a.coordinates for a in at])
    with pytest.raises(NotImplementedError, match="device group"):
        grouped.native_gradient_from_coords(["A"] * 6, ["A"] * 6, xyz, xyz)
    with pytest.raises(ValueError, match="pair_weights has 5 entries for 6 rows"):
        l.native_gradient_from_coords(["A"] * 6, ["A"] * 6, xyz, xyz, pair_weights=np.ones(5))
    with pytest.raises(ValueError, match="same length"):
        l.native_gradient_from_coords(["A"] * 6, ["A"] * 6, xyz, xyz[:5])


def test_c_abi_refuses_null_and_negative_arguments():
    lib = N.lib()
    assert lib.lchd_gradient_primitives_dev(None, None, None, None, None, 1, 5.0, None, 0, None, None, None) == N.EVALUE
    assert lib.lchd_gradient_coords_dev(None, None, None, None, None, None, None, None) == N.EVALUE
    assert lib.lchd_gradient_primitives(None, None, None, None, None, 0, None, None, None, 0, None, None, 1, 5.0, None, 0, None, None, None) == N.EVALUE
    assert lib.lchd_gradient_coords(None, None, None, 0, None, 0, None, None, 0, None, None, None, None, None) == N.EVALUE
