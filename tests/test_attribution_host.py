"""The host side of the score attribution, without a GPU: the five entry points are declared in the header, exported by the library and
prototyped for ctypes, and the Python methods refuse what the radial methods refuse, with the same messages, before any device is
touched."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
NAMES = ["lchd_attribution_primitives_dev", "lchd_attribution_primitives", "lchd_attribution_coords_dev", "lchd_attribution_coords",
         "lchd_attribution_dmxs"]


def _header():
    return re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "loco_hd_hip.h").read_text(), flags=re.S)


def _arguments(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", _header())
    assert m, f"{name} is not declared"
    return [a.strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", NAMES)
def test_declared_exported_and_prototyped(name):
    from loco_hd_amd import _native

    radial = _arguments(name.replace("attribution", "radial"))
    assert _arguments(name) == [a for a in radial if a not in ("const double *edges", "int32_t n_edges")]
    assert hasattr(ctypes.CDLL(str(_native.LIB_PATH)), name)
    restype, argtypes = _native._PROTOS[name]
    r_restype, r_argtypes = _native._PROTOS[name.replace("attribution", "radial")]
    assert restype is r_restype and len(argtypes) == len(_arguments(name)) == len(r_argtypes) - 2
    assert list(argtypes) == list(r_argtypes[:-3]) + [r_argtypes[-1]]  # (edges and n_edges stand in front of the output)


def _setup(**kw):
    import loco_hd_amd as lh

    l = lh.LoCoHD(["A", "B"], lh.WeightFunction("uniform", [3.0, 10.0]), **kw)
    atoms = [lh.PrimitiveAtom("A", "x", [0.0, 0.0, 0.0]), lh.PrimitiveAtom("B", "y", [1.0, 0.0, 0.0])]
    return l, atoms, np.asarray([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]]), np.asarray([[0.0, 1.0], [1.0, 0.0]])


def _message(call):
    with pytest.raises(ValueError) as info:
        call()
    return str(info.value)


def test_device_groups_are_refused():
    l, atoms, xyz, dmx = _setup(devices=[0])
    seq = ["A", "B"]
    for call in (lambda: l.attribution_from_primitives(atoms, atoms, [(0, 1)], 5.0), lambda: l.attribution_from_coords(seq, seq, xyz, xyz),
                 lambda: l.attribution_from_dmxs(seq, seq, dmx, dmx)):
        assert "one device" in _message(call)
    assert l._ctx is None and l._group is None


def test_a_box_and_a_cell_together_are_refused_as_radial_refuses_them():
    l, atoms, xyz, dmx = _setup()
    seq, box, cell, ed = ["A", "B"], [20.0, 20.0, 20.0], np.eye(3) * 20.0, [0.0, float("inf")]
    for side in ("a", "b"):
        kw = {f"box_{side}": box, f"cell_{side}": cell}
        assert _message(lambda: l.attribution_from_primitives(atoms, atoms, [(0, 1)], 5.0, **kw)) == _message(
            lambda: l.radial_from_primitives(atoms, atoms, [(0, 1)], 5.0, ed, **kw))
        assert _message(lambda: l.attribution_from_coords(seq, seq, xyz, xyz, **kw)) == _message(
            lambda: l.radial_from_coords(seq, seq, xyz, xyz, ed, **kw))
        assert f"box_{side} and cell_{side} were both given" in _message(lambda: l.attribution_from_coords(seq, seq, xyz, xyz, **kw))
    assert l._ctx is None


def test_unequal_lengths_are_refused_as_radial_refuses_them():
    l, atoms, xyz, dmx = _setup()
    seq, ed = ["A", "B"], [0.0, float("inf")]
    assert _message(lambda: l.attribution_from_coords(seq, seq, xyz, xyz[:1])) == _message(lambda: l.radial_from_coords(seq, seq, xyz, xyz[:1], ed))
    assert _message(lambda: l.attribution_from_dmxs(seq, seq, dmx, dmx[:1])) == _message(lambda: l.radial_from_dmxs(seq, seq, dmx, dmx[:1], ed))
    assert "Expected matrices with the same length, got lengths 2 and 1!" == _message(lambda: l.attribution_from_dmxs(seq, seq, dmx, dmx[:1]))
    assert "rectangular" in _message(lambda: l.attribution_from_dmxs(seq, seq, [[0.0, 1.0], [0.0]], dmx))
    assert l._ctx is None


def test_empty_input_gives_an_empty_array():
    """(no pair, no row: nothing is sent to a device)"""
    l, atoms, xyz, dmx = _setup()
    assert l.attribution_from_coords([], [], np.zeros((0, 3)), np.zeros((0, 3))).shape == (0, 2)
    assert l.attribution_from_dmxs(["A", "B"], ["A", "B"], np.zeros((0, 2)), np.zeros((0, 2))).shape == (0, 2)
    assert l._ctx is None
