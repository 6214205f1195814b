"""Host layer of the periodic sensitivity calls: argument errors that need no device, the host assembly of a gradient from a
PeriodicSensitivity, the new symbols of the header, and the refusals of the calls that stay as they were.  CPU only."""
import numpy as np
import pytest

import loco_hd_amd as lh
from loco_hd_amd import _native as N
from loco_hd_amd.api import LoCoHD, PeriodicSensitivity, Sensitivity
from test_cabi_symbols import declared_functions

BOX = [20.0, 20.0, 20.0]
CELL = np.eye(3) * 20.0


def _atoms(n=6):
    return [lh.PrimitiveAtom("A", "t", [float(k), 0.0, 0.0]) for k in range(n)]


def _lchd(**kw):
    return lh.LoCoHD(["A"], lh.WeightFunction("uniform", [3.0, 10.0]), **kw)


def test_argument_errors_before_any_device_is_touched():
    l, at = _lchd(), _atoms()
    for call in (l.sensitivity_from_primitives_periodic, l.gradient_from_primitives_periodic):
        with pytest.raises(ValueError, match="box_a and cell_a were both given"):
            call(at, at, [(0, 1)], 5.0, box_a=BOX, cell_a=CELL)
        with pytest.raises(ValueError, match="box_b and cell_b were both given"):
            call(at, at, [(0, 1)], 5.0, box_b=BOX, cell_b=CELL)
        with pytest.raises(ValueError):  # from_primitives' box checks: the threshold exceeds an edge
            call(at, at, [(0, 1)], 5.0, box_a=[4.0, 20.0, 20.0])
        with pytest.raises(ValueError):
            call(at, at, [(0, 1)], 5.0, cell_b=np.zeros((3, 3)))
    with pytest.raises(ValueError, match="width = 0"):
        l.sensitivity_from_primitives_periodic(at, at, [(0, 1)], 5.0, width=0, box_a=BOX)
    with pytest.raises(ValueError, match="pair_weights has 3 entries for 2 anchor pairs"):
        l.gradient_from_primitives_periodic(at, at, [(0, 1), (1, 2)], 5.0, pair_weights=[1.0, 2.0, 3.0], box_a=BOX)
    group = _lchd(devices=[0, 1])
    with pytest.raises(NotImplementedError, match="device group"):
        group.sensitivity_from_primitives_periodic(at, at, [(0, 1)], 5.0, box_a=BOX)
    with pytest.raises(NotImplementedError, match="device group"):
        group.gradient_from_primitives_periodic(at, at, [(0, 1)], 5.0, cell_b=CELL)


def test_the_old_calls_keep_refusing_boxes_and_cells():
    l, at = _lchd(), _atoms()
    for kw in ({"box_a": BOX}, {"box_b": BOX}, {"cell_a": CELL}, {"cell_b": CELL}):
        with pytest.raises(NotImplementedError, match="boxes and cells"):
            l.sensitivity_from_primitives(at, at, [(0, 1)], 5.0, **kw)
        with pytest.raises(NotImplementedError, match="boxes and cells"):
            l.gradient_from_primitives(at, at, [(0, 1)], 5.0, **kw)
    assert Sensitivity._fields == ("scores", "count_a", "idx_a", "dist_a", "g_a", "count_b", "idx_b", "dist_b", "g_b")
    assert PeriodicSensitivity._fields == ("scores", "count_a", "idx_a", "image_a", "dist_a", "g_a", "disp_a", "count_b", "idx_b", "image_b", "dist_b",
                                           "g_b", "disp_b")


def test_header_library_and_prototypes_have_the_new_symbols():
    names = declared_functions()
    for fn in ("lchd_cloud_image_origin", "lchd_cloud_home_size", "lchd_sensitivity_images_dev", "lchd_sensitivity_primitives_periodic"):
        assert fn in names and fn in N._PROTOS and hasattr(N.lib(), fn)


def test_c_abi_refuses_null_arguments():
    lib = N.lib()
    assert lib.lchd_sensitivity_images_dev(None, None, None, None, None, 1, 5.0, 8, *[None] * 13) == N.EVALUE
    assert lib.lchd_sensitivity_primitives_periodic(None, None, None, None, None, 0, None, None, None, 0, None, None, 1, 5.0, 8, None, None, None,
                                                    None, *[None] * 13) == N.EVALUE
    assert lib.lchd_cloud_image_origin(None, None, None, None, 0) == N.EVALUE
    assert lib.lchd_cloud_home_size(None) == -1


def test_gradient_assembly_on_a_hand_made_tuple():
    """Two pairs on side A; atom 2 enters pair 0 twice (home and an image), slot 3 of pair 0 sits at d == 0, pair 1 has a NaN g."""
    disp_a = np.zeros((2, 4, 3))
    disp_a[0, 1], disp_a[0, 2] = (3.0, 0.0, 0.0), (0.0, -4.0, 0.0)
    disp_a[1, 1] = (0.0, 0.0, 2.0)
    sens = PeriodicSensitivity(
        scores=np.asarray([0.5, 0.25]), count_a=np.asarray([4, 2], dtype=np.int32),
        idx_a=np.asarray([[0, 2, 2, 1], [1, 0, -1, -1]], dtype=np.int32), image_a=np.asarray([[0, 0, 6, 0], [0, 1, 0, 0]], dtype=np.int8),
        dist_a=np.asarray([[0.0, 3.0, 4.0, 0.0], [0.0, 2.0, 0.0, 0.0]]), g_a=np.asarray([[0.0, 0.6, -0.8, 0.3], [0.0, np.nan, 0.0, 0.0]]), disp_a=disp_a,
        count_b=np.asarray([1, 1], dtype=np.int32), idx_b=np.asarray([[0], [1]], dtype=np.int32), image_b=np.zeros((2, 1), dtype=np.int8),
        dist_b=np.zeros((2, 1)), g_b=np.zeros((2, 1)), disp_b=np.zeros((2, 1, 3)))
    ga, gb = LoCoHD._assemble_gradient_periodic(sens, 3, 2, [2.0, 1.0])
    # atom 2: 2 * 0.6 * (3, 0, 0) / 3 + 2 * -0.8 * (0, -4, 0) / 4 = (1.2, 1.6, 0); the anchor (atom 0) takes the opposite; nothing else moves
    assert np.allclose(ga, [[-1.2, -1.6, 0.0], [0.0, 0.0, 0.0], [1.2, 1.6, 0.0]], rtol=0, atol=1e-16)
    assert np.array_equal(gb, np.zeros((2, 3)))
    with pytest.raises(ValueError, match="pair_weights has 1 entries for 2 anchor pairs"):
        LoCoHD._assemble_gradient_periodic(sens, 3, 2, [1.0])
