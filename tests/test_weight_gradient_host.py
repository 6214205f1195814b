"""The host side of the weight-function gradient, without a GPU: the entry points are declared in the header, exported by the library
and prototyped for ctypes, and the Python methods and DeviceSession.set_weight_function refuse what they cannot take before any device
is touched."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
NAMES = ["lchd_weight_gradient_width", "lchd_weight_gradient_primitives_dev", "lchd_weight_gradient_primitives",
         "lchd_weight_gradient_coords_dev", "lchd_weight_gradient_coords", "lchd_weight_gradient_dmxs", "lchd_wf_cdf_grad"]


def _arguments(name):
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "loco_hd_hip.h").read_text(), flags=re.S)
    m = re.search(r"\bint(?:32_t)?\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert m, f"{name} is not declared"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", NAMES)
def test_declared_exported_and_prototyped(name):
    from loco_hd_amd import _native

    assert hasattr(ctypes.CDLL(str(_native.LIB_PATH)), name)
    assert len(_native._PROTOS[name][1]) == len(_arguments(name))


@pytest.mark.parametrize("name,twin,dropped", [
    ("lchd_weight_gradient_primitives_dev", "lchd_sensitivity_primitives_dev", 10), ("lchd_weight_gradient_primitives", "lchd_sensitivity_primitives", 10),
    ("lchd_weight_gradient_coords_dev", "lchd_sensitivity_coords_dev", 10), ("lchd_weight_gradient_coords", "lchd_sensitivity_coords", 10),
    ("lchd_weight_gradient_dmxs", "lchd_sensitivity_dmxs", 10)])
def test_arguments_are_the_sensitivity_calls_without_width_and_lists(name, twin, dropped):
    """... the row width and the nine outputs go, one output block comes."""
    mine, theirs = _arguments(name), _arguments(twin)
    assert mine[:-1] == theirs[:-dropped] and mine[-1] in ("double *out", "double *d_out")


def test_the_header_section_states_the_formulas_and_limits():
    text = (ROOT / "include" / "loco_hd_hip.h").read_text()
    section = text[text.index("weight-function gradients (additive"):text.index("native coordinate gradients (additive")]
    for phrase in ("G_k(d_m) * (H- - H+)", "dF/dalpha", "dt/dB = A t / B", "scores[n] | grad[n][NP]", "at most 16 parameters", "LCHD_EUNSUPPORTED",
                   "F(+inf) is not 1"):
        assert phrase in section, phrase


def _setup(wf=None, cats=("A", "B"), **kw):
    import loco_hd_amd as lh

    l = lh.LoCoHD(list(cats), lh.WeightFunction("uniform", [3.0, 10.0]) if wf is None else wf, **kw)
    atoms = [lh.PrimitiveAtom("A", "x", [0.0, 0.0, 0.0]), lh.PrimitiveAtom("B", "y", [1.0, 0.0, 0.0])]
    return l, atoms, np.asarray([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]]), np.asarray([[0.0, 1.0], [1.0, 0.0]])


def _calls(l, atoms, xyz, dmx, **kw):
    seq = ["A", "B"]
    return (lambda: l.weight_gradient_from_primitives(atoms, atoms, [(0, 1)], 5.0, **kw), lambda: l.weight_gradient_from_coords(seq, seq, xyz, xyz, **kw),
            lambda: l.weight_gradient_from_dmxs(seq, seq, dmx, dmx))


def test_weight_gradient_is_exported():
    import loco_hd_amd as lh
    from loco_hd_amd.api import WeightGradient

    assert lh.WeightGradient is WeightGradient and "WeightGradient" in lh.__all__ and WeightGradient._fields == ("scores", "grad")


def test_device_groups_are_refused():
    l, atoms, xyz, dmx = _setup(devices=[0])
    for call in _calls(l, atoms, xyz, dmx):
        with pytest.raises(NotImplementedError, match="one device"):
            call()
    assert l._ctx is None and l._group is None


@pytest.mark.parametrize("key", ["box_a", "box_b", "cell_a", "cell_b"])
def test_boxes_and_cells_are_refused(key):
    l, atoms, xyz, dmx = _setup()
    value = [20.0, 20.0, 20.0] if key.startswith("box") else np.eye(3) * 20.0
    for call in _calls(l, atoms, xyz, dmx, **{key: value})[:2]:
        with pytest.raises(NotImplementedError, match="open structures"):
            call()
    assert l._ctx is None


def test_more_than_16_parameters_are_refused():
    import loco_hd_amd as lh

    l, atoms, xyz, dmx = _setup(lh.WeightFunction("hyper_exp", [1.0] * 9 + [0.1 * k for k in range(1, 10)]))
    for call in _calls(l, atoms, xyz, dmx):
        with pytest.raises(NotImplementedError, match="16 parameters"):
            call()
    eight = lh.WeightFunction("hyper_exp", [1.0] * 8 + [0.1 * k for k in range(1, 9)])
    d, atoms, xyz, dmx = _setup({"small": lh.WeightFunction("uniform", [3.0, 10.0]), "big": eight})
    assert d._weight_gradient_width("x") == 16  # (hyper_exp with 8 components fits, and sets the width of a dictionary)
    assert l._ctx is None and d._ctx is None


def test_65_categories_are_refused():
    l, atoms, xyz, dmx = _setup(cats=["A", "B"] + [f"k{k}" for k in range(63)])
    for call in _calls(l, atoms, xyz, dmx):
        with pytest.raises(NotImplementedError, match="64 categories"):
            call()
    assert l._ctx is None


def test_a_degenerate_dagum_is_a_value_error():
    import loco_hd_amd as lh

    l, atoms, xyz, dmx = _setup(lh.WeightFunction("dagum", [0.0, 5.0, 1.0]))  # A = 0: F = 2^-P everywhere, F(inf) != 1
    for call in _calls(l, atoms, xyz, dmx):
        with pytest.raises(ValueError, match="F\\(\\+inf\\) = 1"):
            call()
    assert l._ctx is None


def test_lengths_and_shapes_are_refused_as_the_sensitivity_refuses_them():
    l, atoms, xyz, dmx = _setup()
    seq = ["A", "B"]

    def message(call):
        with pytest.raises(ValueError) as info:
            call()
        return str(info.value)

    assert message(lambda: l.weight_gradient_from_coords(seq, seq, xyz, xyz[:1])) == message(lambda: l.sensitivity_from_coords(seq, seq, xyz, xyz[:1]))
    assert message(lambda: l.weight_gradient_from_dmxs(seq, seq, dmx, dmx[:1])) == message(lambda: l.sensitivity_from_dmxs(seq, seq, dmx, dmx[:1]))
    assert "weight_gradient_from_dmxs takes rectangular" in message(lambda: l.weight_gradient_from_dmxs(seq, seq, [[0.0, 1.0], [0.0]], dmx))
    assert "Invalid pairing" in message(lambda: l.weight_gradient_from_coords(seq, seq, xyz, xyz, ["k", "k"]))
    assert l._ctx is None


def test_empty_input_gives_empty_arrays():
    l, atoms, xyz, dmx = _setup()
    for got in (l.weight_gradient_from_coords([], [], np.zeros((0, 3)), np.zeros((0, 3))),
                l.weight_gradient_from_dmxs(["A", "B"], ["A", "B"], np.zeros((0, 2)), np.zeros((0, 2)))):
        assert got.scores.shape == (0,) and got.grad.shape == (0, 2) and got.grad.dtype == np.float64
    assert l._ctx is None


def _session_without_a_device(l):
    """A DeviceSession as far as set_weight_function's checks read it: the configuration alone, no context."""
    from loco_hd_amd.device import DeviceSession

    s = object.__new__(DeviceSession)
    s._cfg, s._keep = l._config()
    s._ctx = None  # (close() then has nothing to release)
    return s


def test_set_weight_function_refuses_before_any_device_call():
    import loco_hd_amd as lh

    single = _session_without_a_device(_setup()[0])
    with pytest.raises(ValueError, match="parameter count"):
        single.set_weight_function([3.0, 10.0, 1.0])
    with pytest.raises(ValueError, match="smaller than the second"):
        single.set_weight_function([10.0, 3.0])  # (validated as the WeightFunction constructor validates)
    with pytest.raises(ValueError, match="non-negative"):
        single.set_weight_function(np.asarray([-1.0, 3.0]))
    d = _session_without_a_device(_setup({"u": lh.WeightFunction("uniform", [3.0, 10.0]), "v": lh.WeightFunction("uniform", [2.0, 9.0])})[0])
    with pytest.raises(ValueError, match="dictionary"):
        d.set_weight_function([3.0, 10.0])
