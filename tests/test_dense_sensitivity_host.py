"""Host layer of the dense sensitivity calls: argument errors that need no device, the empty call, and the host assembly of the two
gradients from a hand-made Sensitivity.  CPU only."""
import re
from pathlib import Path

import numpy as np
import pytest

import dense_sensitivity_util as du
import loco_hd_amd as lh
from loco_hd_amd import _native as N
from loco_hd_amd.api import Sensitivity

UNI = ("uniform", [3.0, 10.0])


def _l(cats=("A", "B"), **kw):
    return lh.LoCoHD(list(cats), lh.WeightFunction(*UNI), **kw)


def test_argument_errors_before_any_device_is_touched():
    l = _l()
    seq = ["A", "B", "A"]
    x3, x4 = np.arange(9.0).reshape(3, 3), np.arange(12.0).reshape(4, 3)
    d3 = du.coords_rows(x3)
    for call in (l.sensitivity_from_coords, l.gradient_from_coords):
        with pytest.raises(ValueError, match="same length"):
            call(seq, seq + ["A"], x3, x4)
    with pytest.raises(ValueError, match="same length"):
        l.sensitivity_from_dmxs(seq, seq, d3, d3[:2])
    with pytest.raises(ValueError, match="rectangular"):
        l.sensitivity_from_dmxs(seq, seq, [[0.0, 1.0], [0.0]], d3[:2])
    with pytest.raises(ValueError, match="width"):
        l.sensitivity_from_coords(seq, seq, x3, x3, width=0)
    with pytest.raises(ValueError, match="width"):
        l.sensitivity_from_dmxs(seq, seq, d3, d3, width=0)
    with pytest.raises(ValueError, match="pair_weights"):
        l.gradient_from_coords(seq, seq, x3, x3, pair_weights=[1.0, 2.0])
    with pytest.raises(ValueError, match="pair_weights"):
        l.gradient_from_dmxs(seq, seq, d3, d3, pair_weights=np.ones(4))
    many = lh.LoCoHD([f"c{k}" for k in range(65)], lh.WeightFunction(*UNI))
    with pytest.raises(NotImplementedError, match="at most 64 categories"):
        many.sensitivity_from_dmxs(["c0"] * 3, ["c1"] * 3, d3, d3)
    with pytest.raises(NotImplementedError, match="at most 64 categories"):
        many.gradient_from_coords(["c0"] * 3, ["c1"] * 3, x3, x3)
    wide = np.zeros((1, 65536))
    with pytest.raises(NotImplementedError, match="at most 65535 points"):
        l.sensitivity_from_dmxs(["A"] * 65536, seq, wide, d3[:1])
    group = _l(devices=[0, 1])
    for call, args in ((group.sensitivity_from_coords, (x3, x3)), (group.sensitivity_from_dmxs, (d3, d3)), (group.gradient_from_coords, (x3, x3)),
                       (group.gradient_from_dmxs, (d3, d3))):
        with pytest.raises(NotImplementedError, match="device group"):
            call(seq, seq, *args)
    d = lh.LoCoHD(["A", "B"], {"u": lh.WeightFunction(*UNI), "h": lh.WeightFunction("hyper_exp", [1.0, 0.5])})
    with pytest.raises(ValueError, match="invalid weight function keys"):
        d.sensitivity_from_coords(seq, seq, x3, x3, ["u", "h", "no-such-key"])
    with pytest.raises(ValueError):
        d.sensitivity_from_dmxs(seq, seq, d3, d3)  # a dictionary needs a key per row
    with pytest.raises(ValueError):
        l.sensitivity_from_dmxs(seq, seq, d3, d3, ["u"] * 3)  # and a single function takes none


def test_empty_input_returns_empty_arrays():
    l = _l()
    for sens in (l.sensitivity_from_coords([], [], [], []), l.sensitivity_from_dmxs([], [], [], [])):
        assert isinstance(sens, Sensitivity)
        for name, arr in zip(sens._fields, sens):
            want = np.int32 if name.startswith(("count", "idx")) else np.float64
            assert arr.dtype == want and arr.shape == ((0,) if name in ("scores", "count_a", "count_b") else (0, 0)), name
    assert l.sensitivity_from_coords([], [], [], [], width=7).g_a.shape == (0, 7)
    s, ga, gb = l.gradient_from_coords([], [], [], [])
    assert s.shape == (0,) and ga.shape == (0, 3) and gb.shape == (0, 3) and ga.dtype == np.float64
    s, ga, gb = l.gradient_from_dmxs([], [], [], [])
    assert s.shape == (0,) and ga.shape == (0, 0) and gb.shape == (0, 0)


def test_c_abi_refuses_null_arguments():
    lib = N.lib()
    nul = [None] * 9
    assert lib.lchd_sensitivity_coords_dev(None, None, None, None, 8, *nul) == N.EVALUE
    assert lib.lchd_sensitivity_coords(None, None, None, 0, None, 0, None, None, 1, None, 8, *nul) == N.EVALUE
    assert lib.lchd_sensitivity_dmxs(None, None, None, 0, None, 0, None, None, 1, 1, 1, None, 8, *nul) == N.EVALUE


def test_the_exported_lds_capacity_matches_the_header():
    text = (Path(__file__).resolve().parent.parent / "include" / "loco_hd_hip.h").read_text()
    (value,) = re.findall(r"#define\s+LCHD_SENSITIVITY_ROWS_LDS_POINTS\s+(\d+)", text)
    assert int(value) == N.SENSITIVITY_ROWS_LDS_POINTS and int(value) & (int(value) - 1) == 0


def _hand_made():
    """Three atoms a side; the rows are wider (4) than the structure on purpose: the padding must not land anywhere."""
    xa = np.asarray([[0.0, 0.0, 0.0], [3.0, 0.0, 0.0], [0.0, 4.0, 0.0]])
    xb = np.asarray([[1.0, 1.0, 1.0], [1.0, 1.0, 3.0], [1.0, 1.0, 1.0]])  # atom 2 sits on atom 0
    da, db = du.coords_rows(xa), du.coords_rows(xb)
    idx, dist = [], []
    for d in (da, db):
        order = [du.sorted_row(r) for r in d]
        idx.append(np.asarray([list(o[0]) + [-1] for o in order], dtype=np.int32))
        dist.append(np.asarray([list(o[1]) + [0.0] for o in order]))
    g_a = np.asarray([[0.0, 2.0, -1.0, 0.0], [0.0, 0.5, 0.25, 0.0], [0.0, np.nan, 3.0, 0.0]])
    g_b = np.asarray([[0.0, 9.0, 0.5, 0.0], [0.0, -0.75, 1.5, 0.0], [0.0, 7.0, 0.125, 0.0]])
    cnt = np.full(3, 3, dtype=np.int32)
    return Sensitivity(np.asarray([0.5, 0.25, 0.125]), cnt, idx[0], dist[0], g_a, cnt, idx[1], dist[1], g_b), xa, xb


def test_gradient_assembly_on_a_hand_made_tuple():
    sens, xa, xb = _hand_made()
    assert sens.idx_b.tolist() == [[0, 2, 1, -1], [1, 0, 2, -1], [0, 2, 1, -1]]  # row 2: slot 0 is the lower-indexed twin
    v = np.asarray([2.0, 4.0, 0.5])
    # the G scatter: sorted rows back into column order, slot 0 and the non-finite entry 0
    G_a = lh.LoCoHD._dense_scatter(sens.idx_a, np.where(np.isfinite(sens.g_a), v[:, None] * sens.g_a, 0.0), 3)
    G_b = lh.LoCoHD._dense_scatter(sens.idx_b, v[:, None] * sens.g_b, 3)
    assert np.array_equal(G_a, [[0.0, 4.0, -2.0], [2.0, 0.0, 1.0], [0.0, 1.5, 0.0]])  # row 2: atom 0 (d = 4) carries the NaN
    assert np.array_equal(G_b, [[0.0, 1.0, 18.0], [-3.0, 0.0, 6.0], [0.0, 0.0625, 3.5]])
    want_a, want_b = du.gradient_dmx(sens, 3, 3, v)
    assert np.max(np.abs(G_a - want_a)) <= 1e-13 and np.max(np.abs(G_b - want_b)) <= 1e-13
    # the M form against the term-by-term longdouble sums; the zero-distance twin (g = 9 and g = 7) contributes no direction
    ga = lh.LoCoHD._dense_coords_gradient(sens.idx_a, sens.dist_a, sens.g_a, v, xa)
    gb = lh.LoCoHD._dense_coords_gradient(sens.idx_b, sens.dist_b, sens.g_b, v, xb)
    model_a, model_b = du.gradient_coords(sens, xa, xb, v)
    assert np.max(np.abs(ga - model_a)) <= 1e-13 and np.max(np.abs(gb - model_b)) <= 1e-13
    assert np.any(ga != 0) and np.array_equal(gb[:, :2], np.zeros((3, 2)))  # side B moves along z only
    # row 0 of B moves atom 1 by 2 * 0.5 along +z (atom 0 by the opposite); row 1 moves atoms 0 and 2; row 2 moves atom 1 and itself
    assert np.allclose(gb[:, 2], [-1.0 - 4.0 * -0.75, 1.0 + 4.0 * (-0.75 + 1.5) + 0.5 * 0.125, -4.0 * 1.5 - 0.5 * 0.125], rtol=0, atol=1e-15)
