"""The host side of the category-weight gradient, without a GPU: the five entry points are declared in the header with the argument lists
of the attribution calls, exported by the library and prototyped for ctypes, and the Python methods refuse what they cannot take before any
device is touched."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
NAMES = ["lchd_category_gradient_primitives_dev", "lchd_category_gradient_primitives", "lchd_category_gradient_coords_dev",
         "lchd_category_gradient_coords", "lchd_category_gradient_dmxs"]


def _header():
    return re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "loco_hd_hip.h").read_text(), flags=re.S)


def _arguments(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", _header())
    assert m, f"{name} is not declared"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", NAMES)
def test_declared_exported_and_prototyped(name):
    from loco_hd_amd import _native

    twin = name.replace("category_gradient", "attribution")
    assert _arguments(name) == _arguments(twin)
    assert hasattr(ctypes.CDLL(str(_native.LIB_PATH)), name)
    assert _native._PROTOS[name][0] is _native._PROTOS[twin][0] and list(_native._PROTOS[name][1]) == list(_native._PROTOS[twin][1])


def test_the_header_section_states_the_formulas():
    text = (ROOT / "include" / "loco_hd_hip.h").read_text()
    section = text[text.index("category-weight gradients"):text.index("neighbour sensitivities (additive")]
    for phrase in ("w_c dD/dw_c = x_c + y_c - p_c sum_k x_k - q_c sum_k y_k", "sgn(d_c)", "T = 0", "LCHD_EUNSUPPORTED"):
        assert phrase in section


def _setup(cats=("A", "B"), **kw):
    import loco_hd_amd as lh

    l = lh.LoCoHD(list(cats), lh.WeightFunction("uniform", [3.0, 10.0]), **kw)
    atoms = [lh.PrimitiveAtom("A", "x", [0.0, 0.0, 0.0]), lh.PrimitiveAtom("B", "y", [1.0, 0.0, 0.0])]
    return l, atoms, np.asarray([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]]), np.asarray([[0.0, 1.0], [1.0, 0.0]])


def _calls(l, atoms, xyz, dmx):
    seq = ["A", "B"]
    return (lambda: l.category_gradient_from_primitives(atoms, atoms, [(0, 1)], 5.0), lambda: l.category_gradient_from_coords(seq, seq, xyz, xyz),
            lambda: l.category_gradient_from_dmxs(seq, seq, dmx, dmx))


def test_device_groups_are_refused():
    l, atoms, xyz, dmx = _setup(devices=[0])
    for call in _calls(l, atoms, xyz, dmx):
        with pytest.raises(NotImplementedError, match="one device"):
            call()
    assert l._ctx is None and l._group is None


@pytest.mark.parametrize("name,params", [("Kolmogorov-Smirnov", []), ("Renyi", [2.5, 1e-3])])
def test_distances_without_a_gradient_are_refused_by_name(name, params):
    import loco_hd_amd as lh

    l, atoms, xyz, dmx = _setup(statistical_distance=lh.StatisticalDistance(name, params))
    for call in _calls(l, atoms, xyz, dmx):
        with pytest.raises(NotImplementedError, match=name):
            call()
    assert l._ctx is None


def test_65_categories_are_refused():
    l, atoms, xyz, dmx = _setup(cats=["A", "B"] + [f"k{k}" for k in range(63)])
    for call in _calls(l, atoms, xyz, dmx):
        with pytest.raises(NotImplementedError, match="64 categories"):
            call()
    assert l._ctx is None


def test_lengths_and_shapes_are_refused_as_the_attribution_refuses_them():
    l, atoms, xyz, dmx = _setup()
    seq = ["A", "B"]

    def message(call):
        with pytest.raises(ValueError) as info:
            call()
        return str(info.value)

    assert message(lambda: l.category_gradient_from_coords(seq, seq, xyz, xyz[:1])) == message(lambda: l.attribution_from_coords(seq, seq, xyz, xyz[:1]))
    assert message(lambda: l.category_gradient_from_dmxs(seq, seq, dmx, dmx[:1])) == message(lambda: l.attribution_from_dmxs(seq, seq, dmx, dmx[:1]))
    assert "category_gradient_from_dmxs takes rectangular" in message(lambda: l.category_gradient_from_dmxs(seq, seq, [[0.0, 1.0], [0.0]], dmx))
    box, cell = [20.0, 20.0, 20.0], np.eye(3) * 20.0
    for side in ("a", "b"):
        kw = {f"box_{side}": box, f"cell_{side}": cell}
        assert f"box_{side} and cell_{side} were both given" in message(lambda: l.category_gradient_from_primitives(atoms, atoms, [(0, 1)], 5.0, **kw))
        assert f"box_{side} and cell_{side} were both given" in message(lambda: l.category_gradient_from_coords(seq, seq, xyz, xyz, **kw))
    assert l._ctx is None


def test_empty_input_gives_an_empty_array():
    l, atoms, xyz, dmx = _setup()
    assert l.category_gradient_from_coords([], [], np.zeros((0, 3)), np.zeros((0, 3))).shape == (0, 2)
    assert l.category_gradient_from_dmxs(["A", "B"], ["A", "B"], np.zeros((0, 2)), np.zeros((0, 2))).shape == (0, 2)
    assert l._ctx is None
