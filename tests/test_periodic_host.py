"""Periodic boundaries, the part that needs no device: box validation (lchd_box_validate), the Python layer's argument checks,
CRYST1 parsing and the command line's --periodic handling up to the point where a device is needed."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import loco_hd_amd as lh
from loco_hd_amd import __main__ as cli
from loco_hd_amd import _native as N
from loco_hd_amd.api import periodic_boxes
from loco_hd_amd.pdb_reader import PDBParser


def _validate(box, reach):
    arr = np.ascontiguousarray(box, dtype=np.float64).reshape(-1, 3)
    return N.lib().lchd_box_validate(N.dp(arr), len(arr), float(reach))


def test_box_validate_accepts_a_cube_and_a_slab():
    assert _validate([30.0, 30.0, 30.0], 10.0) == N.OK
    assert _validate([100.0, 100.0, 8.0], 6.0) == N.OK
    assert _validate([[30.0, 30.0, 30.0], [100.0, 100.0, 8.0]], 6.0) == N.OK


def test_box_validate_accepts_a_reach_equal_to_the_smallest_edge():
    assert _validate([8.0, 32.0, 32.0], 8.0) == N.OK
    assert _validate([8.0, 32.0, 32.0], np.nextafter(8.0, 9.0)) == N.EVALUE


@pytest.mark.parametrize("edge", [0.0, -3.0, float("nan"), float("inf")])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_box_validate_rejects_a_bad_edge(edge, axis):
    box = [30.0, 30.0, 30.0]
    box[axis] = edge
    assert _validate(box, 5.0) == N.EVALUE
    assert b"edge" in N.lib().lchd_last_error()
    assert _validate([[30.0, 30.0, 30.0], box], 5.0) == N.EVALUE  # (a later box of several)


@pytest.mark.parametrize("reach", [0.0, -1.0, float("nan"), float("inf"), 30.5])
def test_box_validate_rejects_a_bad_reach(reach):
    assert _validate([30.0, 40.0, 50.0], reach) == N.EVALUE
    assert b"reach" in N.lib().lchd_last_error()


def test_box_validate_rejects_no_boxes():
    assert N.lib().lchd_box_validate(None, 1, 1.0) == N.EVALUE
    arr = np.ones(3)
    assert N.lib().lchd_box_validate(N.dp(arr), 0, 1.0) == N.EVALUE


# ---- the Python layer: ValueError before any device call ---------------------------------------------------------------------
class _NoDevice:
    """Fails the test if the code under test asks for a context, a device group or a session."""

    def __init__(self, monkeypatch):
        def boom(*a, **k):
            raise AssertionError("a device was asked for before the arguments were checked")
        monkeypatch.setattr(lh.LoCoHD, "_context", boom)
        monkeypatch.setattr(lh.LoCoHD, "_device_group", boom)
        import loco_hd_amd.device as dev
        monkeypatch.setattr(dev.DeviceSession, "__init__", boom)


def _atoms(n=4):
    return [lh.PrimitiveAtom("A", f"t{i}", [float(i), 0.0, 0.0]) for i in range(n)]


def test_box_with_devices_raises(monkeypatch):
    _NoDevice(monkeypatch)
    lchd = lh.LoCoHD(["A"], devices=[0, 1])
    with pytest.raises(ValueError, match="devices"):
        lchd.from_primitives(_atoms(), _atoms(), [(0, 0)], 5.0, box_a=[20.0, 20.0, 20.0])
    with pytest.raises(ValueError, match="devices"):
        lchd.from_primitives(_atoms(), _atoms(), [(0, 0)], 5.0, box_b=[20.0, 20.0, 20.0])
    with pytest.raises(ValueError, match="devices"):
        lchd.from_primitives_batch([_atoms(), _atoms()], [(0, 1, [(0, 0)])], 5.0, boxes=[20.0, 20.0, 20.0])


@pytest.mark.parametrize("box", [[20.0, 20.0], [20.0, 20.0, 20.0, 20.0], [[20.0, 20.0, 20.0]] * 2, 20.0, "abc", [[[20.0] * 3]]])
def test_box_of_the_wrong_shape_raises(monkeypatch, box):
    _NoDevice(monkeypatch)
    lchd = lh.LoCoHD(["A"])
    with pytest.raises(ValueError):
        lchd.from_primitives(_atoms(), _atoms(), [(0, 0)], 5.0, box_a=box)
    with pytest.raises(ValueError):
        lchd.from_primitives(_atoms(), _atoms(), [(0, 0)], 5.0, box_b=box)


def test_box_smaller_than_the_threshold_raises(monkeypatch):
    _NoDevice(monkeypatch)
    lchd = lh.LoCoHD(["A"])
    with pytest.raises(ValueError, match="reach"):
        lchd.from_primitives(_atoms(), _atoms(), [(0, 0)], 5.0, box_a=[20.0, 4.9, 20.0])
    with pytest.raises(ValueError, match="reach"):
        lchd.from_primitives(_atoms(), _atoms(), [(0, 0)], float("inf"), box_a=[20.0, 20.0, 20.0])


@pytest.mark.parametrize("n_boxes", [2, 4])
def test_boxes_of_the_wrong_length_raise(monkeypatch, n_boxes):
    _NoDevice(monkeypatch)
    lchd = lh.LoCoHD(["A"])
    structures = [_atoms(), _atoms(), _atoms()]
    with pytest.raises(ValueError, match="3 structures"):
        lchd.from_primitives_batch(structures, [(0, 1, [(0, 0)])], 5.0, boxes=[[20.0, 20.0, 20.0]] * n_boxes)
    with pytest.raises(ValueError):
        lchd.from_primitives_batch(structures, [(0, 1, [(0, 0)])], 5.0, boxes=[20.0, 20.0])


def test_periodic_boxes_returns_one_or_one_per_structure():
    assert periodic_boxes((10.0, 11.0, 12.0), 5, 3.0).tolist() == [[10.0, 11.0, 12.0]]
    assert periodic_boxes([[10.0, 11.0, 12.0]] * 5, 5, 3.0).shape == (5, 3)


def test_new_c_abi_is_exported_with_prototypes():
    lib = N.lib()
    for name in ("lchd_box_validate", "lchd_cloud_create_images", "lchd_cloud_update_images", "lchd_from_primitives_periodic",
                 "lchd_images_scan_span"):
        assert name in N._PROTOS and getattr(lib, name).argtypes is not None
    assert lib.lchd_images_scan_span() >= 64 and lib.lchd_images_scan_span() % 64 == 0
    header = (Path(__file__).resolve().parent.parent / "include" / "loco_hd_hip.h").read_text()
    for name in ("lchd_box_validate", "lchd_cloud_create_images", "lchd_cloud_update_images", "lchd_from_primitives_periodic"):
        assert name + "(" in header


# ---- CRYST1 and the command line -----------------------------------------------------------------------------------------------
_ATOMS = ["ATOM      1  N   GLY A   1       1.000   2.000   3.000  1.00  0.00           N",
          "ATOM      2  CA  GLY A   1       2.000   2.000   3.000  1.00  0.00           C"]
_ORTHO = "CRYST1   58.500   60.250   31.000  90.00  90.00  90.00 P 1           1"
_TRICLINIC = "CRYST1   58.500   60.250   31.000  90.00 101.50  90.00 P 1           1"


def test_cryst1_present():
    st = PDBParser().parse_lines("s", ["HEADER    TEST", _ORTHO] + _ATOMS)
    assert st.cell == (58.5, 60.25, 31.0, 90.0, 90.0, 90.0)
    assert len(list(st.get_atoms())) == 2


def test_cryst1_absent():
    assert PDBParser().parse_lines("s", ["HEADER    TEST"] + _ATOMS).cell is None
    assert PDBParser().parse_lines("s", ["CRYST1 garbage"] + _ATOMS).cell is None


def test_cryst1_non_orthorhombic():
    st = PDBParser().parse_lines("s", [_TRICLINIC] + _ATOMS)
    assert st.cell == (58.5, 60.25, 31.0, 90.0, 101.5, 90.0)
    with pytest.raises(SystemExit, match="orthorhombic"):
        cli.orthorhombic_box(st.cell, "x.pdb")


def test_orthorhombic_box_of_a_cell():
    assert cli.orthorhombic_box((58.5, 60.25, 31.0, 90.0, 90.0005, 90.0), "x.pdb") == (58.5, 60.25, 31.0)
    with pytest.raises(SystemExit, match="orthorhombic"):
        cli.orthorhombic_box((58.5, 60.25, 31.0, 90.0, 90.002, 90.0), "x.pdb")
    with pytest.raises(SystemExit, match="CRYST1"):
        cli.orthorhombic_box(None, "x.pdb")


def _cli_args(tmp_path, head1, head2, extra):
    s1, s2, apf = tmp_path / "s1.pdb", tmp_path / "s2.pdb", tmp_path / "pairs.txt"
    s1.write_text("\n".join(head1 + _ATOMS) + "\n")
    s2.write_text("\n".join(head2 + _ATOMS) + "\n")
    apf.write_text("A/1-GLY/N:A/1-GLY/N")
    return ["-s1", str(s1), "-s2", str(s2), "-pts", str(tmp_path / "no_scheme.json"), "-apf", str(apf)] + extra


def test_cli_periodic_flag_is_parsed(tmp_path):
    assert cli.parse_cli_args(_cli_args(tmp_path, [_ORTHO], [_ORTHO], ["--periodic"])).periodic is True
    assert cli.parse_cli_args(_cli_args(tmp_path, [_ORTHO], [_ORTHO], [])).periodic is False


def test_cli_periodic_without_cryst1_exits_with_a_message(tmp_path):
    args = cli.parse_cli_args(_cli_args(tmp_path, [_ORTHO], [], ["--periodic"]))
    with pytest.raises(SystemExit, match="s2.pdb has no CRYST1 record"):
        cli.run(args)


def test_cli_periodic_with_a_triclinic_cell_exits_with_a_message(tmp_path):
    args = cli.parse_cli_args(_cli_args(tmp_path, [_TRICLINIC], [_ORTHO], ["--periodic"]))
    with pytest.raises(SystemExit, match="s1.pdb.*orthorhombic"):
        cli.run(args)


def test_cli_without_the_flag_does_not_look_at_the_cell(tmp_path):
    """Without --periodic a missing or triclinic cell is no error: the run goes on to the typing scheme (absent here)."""
    args = cli.parse_cli_args(_cli_args(tmp_path, [_TRICLINIC], [], []))
    with pytest.raises(FileNotFoundError):
        cli.run(args)
