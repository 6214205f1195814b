"""Periodic boundaries in triclinic cells, the part that needs no device: lchd_cell_validate, the Python layer's argument checks,
cell_from_lengths_angles and the command line's --periodic-cell handling up to the point where a device is needed."""
import math
from pathlib import Path

import numpy as np
import pytest

import loco_hd_amd as lh
from loco_hd_amd import __main__ as cli
from loco_hd_amd import _native as N
from loco_hd_amd.api import periodic_cells
from tests.periodic_cell_util import CELLS, TABLE, widths
from tests.test_periodic_host import _ATOMS, _ORTHO, _TRICLINIC, _atoms, _cli_args, _NoDevice


def _validate(cells, reach):
    arr = np.ascontiguousarray(cells, dtype=np.float64).reshape(-1, 9)
    return N.lib().lchd_cell_validate(N.dp(arr), len(arr), float(reach))


def test_widths_of_the_five_cells():
    for name, cell in CELLS.items():
        assert np.allclose(widths(cell), TABLE[name], atol=0.06), name


@pytest.mark.parametrize("name", list(CELLS))
def test_cell_validate_accepts_a_reach_up_to_the_smallest_width(name):
    """The widths come from the formula (tests/periodic_cell_util.py: widths, the header's arithmetic); the issue's table is only a
    check on them."""
    w = widths(CELLS[name])
    assert np.allclose(w, TABLE[name], atol=0.06)
    assert _validate(CELLS[name], float(w.min())) == N.OK
    assert _validate(CELLS[name], 1.0) == N.OK
    assert _validate(CELLS[name], np.nextafter(float(w.min()), np.inf)) == N.EVALUE
    assert b"reach" in N.lib().lchd_last_error() and b"width" in N.lib().lchd_last_error()


def test_cell_validate_checks_every_cell_of_several():
    both = np.stack([CELLS["monoclinic"], CELLS["skewed"]])
    assert _validate(both, 12.5) == N.OK
    assert _validate(both, 13.0) == N.EVALUE  # (the second cell's smallest width is 12.51)
    assert b"cell 1" in N.lib().lchd_last_error()


@pytest.mark.parametrize("cell", [
    [[10.0, 0.0, 0.0], [0.0, 10.0, 0.0], [10.0, 10.0, 0.0]],                 # coplanar
    [[10.0, 0.0, 0.0], [20.0, 0.0, 0.0], [0.0, 0.0, 10.0]],                  # two parallel vectors
    [[0.0, 0.0, 0.0], [0.0, 10.0, 0.0], [0.0, 0.0, 10.0]],                   # a zero vector
    [[10.0, 0.0, 0.0], [0.0, 10.0, 0.0], [10.0, 10.0, 1e-12]],               # |det| below 1e-12 |a| |b| |c|
])
def test_cell_validate_rejects_a_singular_cell(cell):
    assert _validate(cell, 1e-3) == N.EVALUE
    assert b"singular" in N.lib().lchd_last_error()


@pytest.mark.parametrize("entry", [float("nan"), float("inf"), -float("inf")])
@pytest.mark.parametrize("where", [0, 4, 8, 5])
def test_cell_validate_rejects_a_non_finite_entry(entry, where):
    cell = CELLS["skewed"].copy().reshape(-1)
    cell[where] = entry
    assert _validate(cell, 5.0) == N.EVALUE
    assert b"finite" in N.lib().lchd_last_error()
    assert _validate(np.stack([CELLS["skewed"].reshape(-1), cell]), 5.0) == N.EVALUE  # (a later cell of several)


@pytest.mark.parametrize("reach", [0.0, -1.0, float("nan"), float("inf")])
def test_cell_validate_rejects_a_bad_reach(reach):
    assert _validate(CELLS["dodecahedron"], reach) == N.EVALUE
    assert b"reach" in N.lib().lchd_last_error()


def test_cell_validate_rejects_no_cells():
    assert N.lib().lchd_cell_validate(None, 1, 1.0) == N.EVALUE
    arr = np.ascontiguousarray(CELLS["skewed"])
    assert N.lib().lchd_cell_validate(N.dp(arr), 0, 1.0) == N.EVALUE


def test_a_left_handed_and_a_permuted_cell_have_the_same_widths():
    w = widths(CELLS["left-handed"])
    assert np.allclose(widths(CELLS["left-handed"][[1, 0, 2]]), w[[1, 0, 2]], rtol=1e-14)
    assert _validate(CELLS["left-handed"][[1, 0, 2]], float(w.min()) * (1 - 1e-14)) == N.OK


# ---- the Python layer: ValueError before any device call ---------------------------------------------------------------------
SKEW = CELLS["skewed"]


@pytest.mark.parametrize("cell", [[20.0, 20.0, 20.0], [[20.0, 0.0, 0.0], [0.0, 20.0, 0.0]], [SKEW.tolist()] * 3, "abc", 20.0,
                                  np.zeros((3, 3, 3)).tolist()])
def test_cell_of_the_wrong_shape_raises(monkeypatch, cell):
    _NoDevice(monkeypatch)
    lchd = lh.LoCoHD(["A"])
    with pytest.raises(ValueError):
        lchd.from_primitives(_atoms(), _atoms(), [(0, 0)], 5.0, cell_a=cell)
    with pytest.raises(ValueError):
        lchd.from_primitives(_atoms(), _atoms(), [(0, 0)], 5.0, cell_b=cell)
    with pytest.raises(ValueError):
        lchd.from_primitives_batch([_atoms()], [(0, 0, [(0, 0)])], 5.0, cells=cell)


def test_box_and_cell_for_one_side_raise(monkeypatch):
    _NoDevice(monkeypatch)
    lchd = lh.LoCoHD(["A"])
    with pytest.raises(ValueError, match="box_a and cell_a"):
        lchd.from_primitives(_atoms(), _atoms(), [(0, 0)], 5.0, box_a=[20.0, 20.0, 20.0], cell_a=SKEW)
    with pytest.raises(ValueError, match="box_b and cell_b"):
        lchd.from_primitives(_atoms(), _atoms(), [(0, 0)], 5.0, box_b=[20.0, 20.0, 20.0], cell_b=SKEW, cell_a=SKEW)
    with pytest.raises(ValueError, match="both"):
        lchd.from_primitives_batch([_atoms(), _atoms()], [(0, 1, [(0, 0)])], 5.0, boxes=[20.0, 20.0, 20.0], cells=SKEW)


def test_cell_with_devices_raises(monkeypatch):
    _NoDevice(monkeypatch)
    lchd = lh.LoCoHD(["A"], devices=[0, 1])
    with pytest.raises(ValueError, match="devices"):
        lchd.from_primitives(_atoms(), _atoms(), [(0, 0)], 5.0, cell_a=SKEW)
    with pytest.raises(ValueError, match="devices"):
        lchd.from_primitives(_atoms(), _atoms(), [(0, 0)], 5.0, cell_b=SKEW)
    with pytest.raises(ValueError, match="devices"):
        lchd.from_primitives_batch([_atoms(), _atoms()], [(0, 1, [(0, 0)])], 5.0, cells=SKEW)


@pytest.mark.parametrize("n_cells", [2, 4])
def test_cells_of_the_wrong_length_raise(monkeypatch, n_cells):
    _NoDevice(monkeypatch)
    lchd = lh.LoCoHD(["A"])
    with pytest.raises(ValueError, match="3 structures"):
        lchd.from_primitives_batch([_atoms(), _atoms(), _atoms()], [(0, 1, [(0, 0)])], 5.0, cells=[SKEW.tolist()] * n_cells)


def test_threshold_above_the_smallest_width_raises(monkeypatch):
    _NoDevice(monkeypatch)
    lchd = lh.LoCoHD(["A"])
    with pytest.raises(ValueError, match="reach"):
        lchd.from_primitives(_atoms(), _atoms(), [(0, 0)], 12.6, cell_a=SKEW)  # (12.51 is the smallest width; every edge is longer)
    with pytest.raises(ValueError, match="reach"):
        lchd.from_primitives(_atoms(), _atoms(), [(0, 0)], float("inf"), cell_b=SKEW)
    with pytest.raises(ValueError, match="reach"):
        lchd.from_primitives_batch([_atoms(), _atoms()], [(0, 1, [(0, 0)])], 12.6, cells=[CELLS["dodecahedron"], SKEW])


def test_periodic_cells_returns_one_or_one_per_structure():
    assert periodic_cells(SKEW, 5, 3.0).shape == (1, 3, 3)
    assert periodic_cells([SKEW] * 5, 5, 3.0).shape == (5, 3, 3)
    assert periodic_cells(SKEW.tolist(), 1, 3.0).dtype == np.float64


# ---- cell_from_lengths_angles ---------------------------------------------------------------------------------------------------
def test_cell_from_lengths_angles_of_a_cube_is_exactly_diagonal():
    assert np.array_equal(lh.cell_from_lengths_angles(31.7, 31.7, 31.7, 90, 90, 90), np.diag([31.7, 31.7, 31.7]))
    assert np.array_equal(lh.cell_from_lengths_angles(58.5, 60.25, 31.0, 90.0, 90.0, 90.0), np.diag([58.5, 60.25, 31.0]))


def test_cell_from_lengths_angles_of_the_dodecahedron():
    d = 30.0
    assert float(np.max(np.abs(lh.cell_from_lengths_angles(d, d, d, 60, 60, 90) - CELLS["dodecahedron"]))) <= 1e-12


def test_cell_from_lengths_angles_reproduces_lengths_and_angles():
    cell = lh.cell_from_lengths_angles(58.5, 60.25, 31.0, 90.0, 101.5, 90.0)
    assert float(np.max(np.abs(cell - CELLS["monoclinic"]))) <= 1e-12
    assert cell[0, 1] == cell[0, 2] == cell[1, 0] == cell[1, 2] == cell[2, 1] == 0.0  # a along x, b in the xy plane, exact zeros
    a, b, c = cell
    for got, want in zip((np.linalg.norm(a), np.linalg.norm(b), np.linalg.norm(c)), (58.5, 60.25, 31.0)):
        assert abs(got - want) <= 1e-12

    def angle(u, v):
        return math.degrees(math.acos(float(u @ v) / float(np.linalg.norm(u) * np.linalg.norm(v))))
    for got, want in zip((angle(b, c), angle(a, c), angle(a, b)), (90.0, 101.5, 90.0)):
        assert abs(got - want) <= 1e-12
    general = lh.cell_from_lengths_angles(20.0, 23.4, 16.5, 77.0, 112.0, 95.5)  # (no right angle)
    a, b, c = general
    assert general[0, 1] == general[0, 2] == general[1, 2] == 0.0
    for got, want in zip((angle(b, c), angle(a, c), angle(a, b)), (77.0, 112.0, 95.5)):
        assert abs(got - want) <= 1e-11
    with pytest.raises(ValueError):
        lh.cell_from_lengths_angles(10.0, 10.0, 10.0, 150.0, 150.0, 150.0)  # no such cell


# ---- exports ---------------------------------------------------------------------------------------------------------------------
def test_new_c_abi_is_exported_with_prototypes():
    lib = N.lib()
    header = (Path(__file__).resolve().parent.parent / "include" / "loco_hd_hip.h").read_text()
    for name in ("lchd_cell_validate", "lchd_cloud_create_images_cell", "lchd_cloud_update_images_cell", "lchd_from_primitives_periodic_cell"):
        assert name in N._PROTOS and getattr(lib, name).argtypes is not None
        assert name + "(" in header
    assert "cell_from_lengths_angles" in lh.__all__ and callable(lh.cell_from_lengths_angles)


# ---- the command line ------------------------------------------------------------------------------------------------------------
def test_cli_periodic_cell_flag_is_parsed(tmp_path):
    ns = cli.parse_cli_args(_cli_args(tmp_path, [_TRICLINIC], [_TRICLINIC], ["--periodic-cell"]))
    assert ns.periodic_cell is True and ns.periodic is False
    ns = cli.parse_cli_args(_cli_args(tmp_path, [_ORTHO], [_ORTHO], []))
    assert ns.periodic_cell is False and ns.periodic is False


def test_cli_both_periodic_flags_exit(tmp_path, capsys):
    with pytest.raises(SystemExit):
        cli.parse_cli_args(_cli_args(tmp_path, [_ORTHO], [_ORTHO], ["--periodic", "--periodic-cell"]))
    assert "not allowed with" in capsys.readouterr().err


def test_cli_periodic_cell_without_cryst1_exits_with_the_files_name(tmp_path):
    args = cli.parse_cli_args(_cli_args(tmp_path, [_TRICLINIC], [], ["--periodic-cell"]))
    with pytest.raises(SystemExit, match="s2.pdb has no CRYST1 record"):
        cli.run(args)


def test_cli_periodic_cell_takes_a_triclinic_and_an_orthorhombic_cell(tmp_path):
    """Both cells are accepted: the run goes on to the typing scheme (absent here)."""
    assert np.array_equal(cli.cryst1_cell((58.5, 60.25, 31.0, 90.0, 90.0, 90.0), "x.pdb"), np.diag([58.5, 60.25, 31.0]))
    assert float(np.max(np.abs(cli.cryst1_cell((58.5, 60.25, 31.0, 90.0, 101.5, 90.0), "x.pdb") - CELLS["monoclinic"]))) <= 1e-12
    args = cli.parse_cli_args(_cli_args(tmp_path, [_TRICLINIC], [_ORTHO], ["--periodic-cell"]))
    with pytest.raises(FileNotFoundError):
        cli.run(args)
    assert len(_ATOMS) == 2
