"""The composition calls refuse what their scoring twins refuse, before any device is touched (CPU-only machine)."""
import numpy as np
import pytest

import loco_hd_amd as lh

CATS = ["A", "B", "C"]


def _atoms(n=6):
    return [lh.PrimitiveAtom(CATS[i % 3], f"t{i}", [float(i), 0.5 * i, 0.0]) for i in range(n)]


def _single():
    return lh.LoCoHD(CATS, lh.WeightFunction("uniform", [3.0, 10.0]))


def _dictionary():
    return lh.LoCoHD(CATS, {"near": lh.WeightFunction("uniform", [0.0, 5.0]), "far": lh.WeightFunction("uniform", [3.0, 10.0])})


def test_weight_function_keys_resolve_as_in_scoring():
    atoms, xyz, seq = _atoms(), np.zeros((6, 3)), [CATS[i % 3] for i in range(6)]
    pairing = "Invalid pairing for the LoCoHD instance's w_func option and the method's w_func_keys parameter!"
    for call in (lambda l, k: l.composition_from_primitives(atoms, [0, 1], 5.0, k[:2] if k else k),
                 lambda l, k: l.composition_from_coords(seq, xyz, k),
                 lambda l, k: l.composition_from_dmx(seq, np.zeros((6, 6)), k)):
        with pytest.raises(ValueError) as e:
            call(_single(), ["near"] * 6)      # a single function refuses keys
        assert str(e.value) == pairing
        with pytest.raises(ValueError) as e:
            call(_dictionary(), None)          # a dictionary needs keys
        assert str(e.value) == pairing
        with pytest.raises(ValueError, match="invalid weight function keys"):
            call(_dictionary(), ["near", "nowhere"] * 3)
    with pytest.raises(ValueError, match=r"invalid length \(3 instead of 6\)"):
        _dictionary().composition_from_coords(seq, xyz, ["near"] * 3)
    with pytest.raises(ValueError, match=r"invalid length \(1 instead of 2\)"):
        _dictionary().composition_from_primitives(atoms, [0, 1], 5.0, ["near"])


def test_shape_and_anchor_errors():
    lchd = _single()
    with pytest.raises(TypeError, match="coordinates must be a sequence of"):
        lchd.composition_from_coords(["A", "B"], np.zeros((2, 2)))
    with pytest.raises(TypeError, match="2-D sequence of floats"):
        lchd.composition_from_dmx(["A"], np.zeros((1, 1, 1)))
    with pytest.raises(lh.PanicException, match="an anchor index is outside its structure"):
        lchd.composition_from_primitives(_atoms(), [0, 6], 5.0)
    with pytest.raises(OverflowError):
        lchd.composition_from_primitives(_atoms(), [-1], 5.0)
    # nothing to do: empty tables of the right width, no device needed
    assert lchd.composition_from_primitives(_atoms(), [], 5.0).shape == (0, 3)
    assert lchd.composition_from_coords([], np.zeros((0, 3))).shape == (0, 3)


def test_box_and_cell_errors():
    lchd, atoms = _single(), _atoms()
    cell = [[20.0, 0.0, 0.0], [0.0, 20.0, 0.0], [0.0, 0.0, 20.0]]
    with pytest.raises(ValueError, match="both given"):
        lchd.composition_from_primitives(atoms, [0], 5.0, box=[20.0, 20.0, 20.0], cell=cell)
    with pytest.raises(ValueError, match="both given"):
        lchd.composition_from_coords(["A"] * 6, np.zeros((6, 3)), box=[20.0, 20.0, 20.0], cell=cell)
    # the threshold beyond the reach of the box / the cell: the scoring twin's message, word for word
    for kw, twin in (({"box": [20.0, 8.0, 20.0]}, {"box_a": [20.0, 8.0, 20.0]}),
                     ({"cell": [[20.0, 0.0, 0.0], [0.0, 8.0, 0.0], [0.0, 0.0, 20.0]]}, {"cell_a": [[20.0, 0.0, 0.0], [0.0, 8.0, 0.0], [0.0, 0.0, 20.0]]})):
        with pytest.raises(ValueError) as mine:
            lchd.composition_from_primitives(atoms, [0], 9.0, **kw)
        with pytest.raises(ValueError) as theirs:
            lchd.from_primitives(atoms, atoms, [(0, 0)], 9.0, **twin)
        assert str(mine.value) == str(theirs.value)
    with pytest.raises(ValueError, match="three edge lengths"):
        lchd.composition_from_primitives(atoms, [0], 5.0, box=[20.0, 20.0])
    with pytest.raises(ValueError):
        lchd.composition_from_coords(["A"] * 6, np.zeros((6, 3)), cell=[[1.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.0, 0.0, 1.0]])  # singular


def test_device_groups_refuse_the_composition_calls():
    grp = lh.LoCoHD(CATS, lh.WeightFunction("uniform", [3.0, 10.0]), devices=[0, 1])
    for call in (lambda: grp.composition_from_primitives(_atoms(), [0], 5.0),
                 lambda: grp.composition_from_coords(["A"], np.zeros((1, 3))),
                 lambda: grp.composition_from_dmx(["A"], np.zeros((1, 1)))):
        with pytest.raises(ValueError, match=r"applies to one device .*drop devices=\[\.\.\.\]"):
            call()
