"""Argument errors of the native periodic gradient calls that need no device: the four C entry points through the built library (a null
context comes after the checks the arguments alone decide), the two LoCoHD methods through api.py's own checks, and the limits of
lchd_gradient_plan_periodic, the 2^31 slot rule included.  The two DeviceSession methods need a device: tests/test_gpu_gradient_periodic.py."""
import ctypes as C

import numpy as np
import pytest

import loco_hd_amd as lh
from loco_hd_amd import _native as N

STRAIN = r"one strain pointer is null and the other is not"
BOTH = r"a box and a cell were both given"


def _plan(n_pairs, width, resolve, budget):
    out = C.c_int64(-7)
    rc = N.lib().lchd_gradient_plan_periodic(n_pairs, width, resolve, budget, C.byref(out))
    return rc, out.value


def _last():
    return N.lib().lchd_last_error().decode()


def row_bytes(width, resolve):
    """Bytes per pair of a tile: the nine arrays; the two disp rows of a resolving call; the two int8 image rows rounded up to doubles."""
    return 40 * width + 16 + (48 * width if resolve else 0) + (8 * ((2 * width + 7) // 8) if resolve == 1 else 0)


@pytest.mark.parametrize("resolve", [0, 1, 2])
@pytest.mark.parametrize("n_pairs,width", [(1, 1), (7, 2), (1000, 64), (12345, 65), (3, 129), (10 ** 6, 300)])
def test_plan_is_the_budget_over_the_bytes_of_a_pair_clamped(n_pairs, width, resolve):
    per_pair = row_bytes(width, resolve)
    for budget in (0, 1, per_pair - 1, per_pair, 2 * per_pair + 5, 10 ** 6, 10 ** 9, 10 ** 12, 2 ** 62):
        rc, tile = _plan(n_pairs, width, resolve, budget)
        assert rc == N.OK and tile == max(1, min(budget // per_pair, n_pairs)), (budget, tile)
    if resolve == 0:
        plain = C.c_int64(0)
        assert N.lib().lchd_gradient_plan(n_pairs, width, 10 ** 7, C.byref(plain)) == N.OK
        assert plain.value == _plan(n_pairs, width, 0, 10 ** 7)[1]


def test_plan_limits():
    for args in ((0, 8, 1, 100), (-3, 8, 1, 100), (5, 0, 1, 100), (5, 65536, 1, 100), (5, 8, 1, -1), (5, 8, -1, 100), (5, 8, 3, 100)):
        rc, tile = _plan(*args)
        assert rc == N.EVALUE and tile == 0, args
    assert N.lib().lchd_gradient_plan_periodic(5, 8, 1, 100, None) == N.EVALUE
    # the slot rule: n_pairs x width per side below 2^31
    for n_pairs, width, ok in ((2 ** 31 - 1, 1, True), (2 ** 31, 1, False), (2 ** 24, 127, True), (2 ** 24, 128, False), (46340, 46340, True),
                               (46341, 46341, False), (32768, 65535, True), (32769, 65535, False)):
        for resolve in (0, 1, 2):
            rc, tile = _plan(n_pairs, width, resolve, 10 ** 9)
            assert (rc == N.OK and tile >= 1) if ok else (rc == N.EUNSUPPORTED and tile == 0), (n_pairs, width, resolve)
            if not ok:
                assert "exceed the 2^31 additions an exact accumulator takes" in _last()


def test_strain_grid_is_bounded():
    waves = int(N.lib().lchd_gradient_strain_waves())
    assert 4 <= waves <= 16384 and waves % 4 == 0


def test_c_abi_argument_errors_without_a_context():
    lib = N.lib()
    one = (C.c_double * 9)()
    d = C.cast(one, C.c_void_p)
    p = C.cast(one, C.POINTER(C.c_double))
    box = (C.c_double * 3)(20.0, 20.0, 20.0)
    cell = (C.c_double * 9)(20.0, 0, 0, 0, 20.0, 0, 0, 0, 20.0)
    # lchd_gradient_images_dev
    assert lib.lchd_gradient_images_dev(None, None, None, None, None, 1, 5.0, None, -1, None, None, None, None, None) == N.EVALUE
    assert "tile_pairs = -1 is negative" in _last()
    for sa, sb in ((d, None), (None, d)):
        assert lib.lchd_gradient_images_dev(None, None, None, None, None, 1, 5.0, None, 0, None, None, None, sa, sb) == N.EVALUE
        assert STRAIN in _last()
    assert lib.lchd_gradient_images_dev(None, None, None, None, None, 1, 5.0, None, 0, None, None, None, None, None) == N.EVALUE
    assert "null argument" in _last()
    # lchd_gradient_coords_periodic_dev
    for sa, sb in ((d, None), (None, d)):
        assert lib.lchd_gradient_coords_periodic_dev(None, None, None, None, None, None, None, None, None, None, sa, sb) == N.EVALUE
        assert STRAIN in _last()
    assert lib.lchd_gradient_coords_periodic_dev(None, None, None, None, None, None, None, None, None, None, None, None) == N.EVALUE
    assert "null argument" in _last()
    # lchd_gradient_primitives_periodic
    head = (None, None, None, None, None, 0, None, None, None, 0, None, None)
    assert lib.lchd_gradient_primitives_periodic(*head, 1, 5.0, None, None, None, None, None, -4, None, None, None, None, None) == N.EVALUE
    assert "tile_pairs = -4 is negative" in _last()
    assert lib.lchd_gradient_primitives_periodic(*head, -1, 5.0, None, None, None, None, None, 0, None, None, None, None, None) == N.EVALUE
    assert "negative pair count" in _last()
    for sa, sb in ((p, None), (None, p)):
        assert lib.lchd_gradient_primitives_periodic(*head, 1, 5.0, None, None, None, None, None, 0, None, None, None, sa, sb) == N.EVALUE
        assert STRAIN in _last()
    for boxes in ((box, cell, None, None), (None, None, box, cell)):
        assert lib.lchd_gradient_primitives_periodic(*head, 1, 5.0, *boxes, None, 0, None, None, None, None, None) == N.EVALUE
        assert "a box and a cell were both given" in _last()
    assert lib.lchd_gradient_primitives_periodic(*head, 1, 5.0, box, None, None, None, None, 0, None, None, None, None, None) == N.EVALUE
    assert "null context" in _last()
    # lchd_gradient_coords_periodic
    x = (C.c_double * 6)()
    assert lib.lchd_gradient_coords_periodic(None, None, None, 0, None, 0, x, x, -1, None, None, None, None, None, None, None, None, None) == N.EVALUE
    assert "negative structure size" in _last()
    assert lib.lchd_gradient_coords_periodic(None, None, None, 0, None, 0, None, None, 2, None, None, None, None, None, None, None, None, None) == N.EVALUE
    assert "null pointer" in _last()
    for sa, sb in ((p, None), (None, p)):
        assert lib.lchd_gradient_coords_periodic(None, None, None, 0, None, 0, x, x, 2, None, None, None, None, None, None, None, sa, sb) == N.EVALUE
        assert STRAIN in _last()
    assert lib.lchd_gradient_coords_periodic(None, None, None, 0, None, 0, x, x, 2, None, None, None, None, None, None, None, None, None) == N.EVALUE
    assert "null context" in _last()


def _atoms(n=6):
    return [lh.PrimitiveAtom("A", "t", [float(k), 0.0, 0.0]) for k in range(n)]


def test_python_argument_errors_before_any_device_is_touched():
    l = lh.LoCoHD(["A"], lh.WeightFunction("uniform", [3.0, 10.0]))
    at = _atoms()
    box, cell = [20.0, 20.0, 20.0], np.eye(3) * 20.0
    with pytest.raises(ValueError, match="tile_pairs = -1 is negative"):
        l.native_gradient_from_primitives_periodic(at, at, [(0, 1)], 5.0, tile_pairs=-1, box_a=box)
    for side in "ab":
        with pytest.raises(ValueError, match=f"box_{side} and cell_{side} were both given"):
            l.native_gradient_from_primitives_periodic(at, at, [(0, 1)], 5.0, **{f"box_{side}": box, f"cell_{side}": cell})
    with pytest.raises(ValueError, match="pair_weights has 2 entries for 1 anchor pairs"):
        l.native_gradient_from_primitives_periodic(at, at, [(0, 1)], 5.0, pair_weights=[1.0, 2.0], box_a=box)
    with pytest.raises(ValueError):  # a threshold beyond the box edge: the periodic scoring call's own check
        l.native_gradient_from_primitives_periodic(at, at, [(0, 1)], 25.0, box_a=box)
    with pytest.raises(ValueError, match="box_b must be three edge lengths"):
        l.native_gradient_from_primitives_periodic(at, at, [(0, 1)], 5.0, box_b=[1.0, 2.0])
    grouped = lh.LoCoHD(["A"], lh.WeightFunction("uniform", [3.0, 10.0]), devices=[0, 1])
    with pytest.raises(NotImplementedError, match="device group"):
        grouped.native_gradient_from_primitives_periodic(at, at, [(0, 1)], 5.0, box_a=box)
    xyz = np.asarray([a.coordinates for a in at])
    seq = ["A"] * 6
    with pytest.raises(NotImplementedError, match="device group"):
        grouped.native_gradient_from_coords_periodic(seq, seq, xyz, xyz, box_a=box)
    for side in "ab":
        with pytest.raises(ValueError, match=f"box_{side} and cell_{side} were both given"):
            l.native_gradient_from_coords_periodic(seq, seq, xyz, xyz, **{f"box_{side}": box, f"cell_{side}": cell})
    with pytest.raises(ValueError, match="pair_weights has 5 entries for 6 rows"):
        l.native_gradient_from_coords_periodic(seq, seq, xyz, xyz, pair_weights=np.ones(5), box_a=box)
    with pytest.raises(ValueError, match="same length"):
        l.native_gradient_from_coords_periodic(seq, seq, xyz, xyz[:5], cell_b=cell)
    with pytest.raises(ValueError, match="every edge must be finite and > 0"):
        l.native_gradient_from_coords_periodic(seq, seq, xyz, xyz, box_a=[10.0, -1.0, 10.0])


def test_cell_gradient_is_inverse_transpose_times_strain():
    rng = np.random.default_rng(4)
    w = rng.normal(size=(3, 3))
    w = w + w.T
    h = np.asarray([[11.0, 0.0, 0.0], [2.0, 9.5, 0.0], [-1.5, 3.0, 12.0]])
    got = lh.cell_gradient(w, h)
    assert np.allclose(got, np.linalg.inv(h).T @ w, rtol=1e-13, atol=0)
    box = [10.0, 12.0, 8.0]
    assert np.allclose(lh.cell_gradient(w, box), w / np.asarray(box)[:, None], rtol=1e-14, atol=0)
    assert "cell_gradient" in lh.__all__ and "NativeGradient" in lh.__all__
    assert lh.NativeGradient._fields == ("scores", "grad_a", "grad_b", "strain_a", "strain_b")
    for bad in (np.zeros((3, 3)), np.ones((2, 2))):
        with pytest.raises(ValueError):
            lh.cell_gradient(w, bad)
    with pytest.raises(ValueError):
        lh.cell_gradient(np.ones(3), h)


def test_header_and_binding_name_the_new_entry_points():
    text = (N._PKG.parent / "include" / "loco_hd_hip.h").read_text()
    for name in ("lchd_gradient_images_dev", "lchd_gradient_primitives_periodic", "lchd_gradient_coords_periodic_dev",
                 "lchd_gradient_coords_periodic", "lchd_gradient_plan_periodic", "lchd_gradient_strain_waves"):
        assert f"{name}(" in text and hasattr(N.lib(), name)
    for name, value in (("LCHD_GRAD_PLAIN", 0), ("LCHD_GRAD_IMAGES", 1), ("LCHD_GRAD_MIN_IMAGE", 2)):
        assert f"#define {name} {value}" in text
