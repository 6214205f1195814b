"""The host side of the radial profiles, without a GPU: edge validation (lchd_radial_validate and the Python methods raise before any
device is touched) and the interval-splitting header (loco_hd_amd/csrc/lchd_radial_bins.h), compiled with the host compiler alone and
compared with the definition in tests/radial_util.py."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import radial_util

ROOT = Path(__file__).resolve().parent.parent
INF = float("inf")
BAD_EDGES = {
    "one edge": [0.0],
    "no edge": [],
    "66 edges": list(np.arange(66.0)),
    "negative": [-1.0, 2.0],
    "nan": [0.0, float("nan"), 3.0],
    "descending": [0.0, 3.0, 2.0],
    "repeated": [0.0, 2.0, 2.0, 3.0],
    "inf first": [INF, INF],
    "inf in the middle": [0.0, INF, INF],
    "inf before a finite edge": [0.0, INF, 5.0],
}
GOOD_EDGES = [[0.0, INF], [0.0, 1.0], [2.5, 3.0, INF], list(np.arange(65.0)), list(np.arange(64.0)) + [INF]]


@pytest.mark.parametrize("name", sorted(BAD_EDGES))
def test_validate_refuses(name):
    from loco_hd_amd import _native as N

    ed = np.asarray(BAD_EDGES[name], dtype=np.float64)
    assert N.lib().lchd_radial_validate(N.dp(ed) if len(ed) else N.dp(np.zeros(1)), len(ed)) != 0


def test_validate_accepts():
    from loco_hd_amd import _native as N

    for e in GOOD_EDGES:
        ed = np.asarray(e, dtype=np.float64)
        assert N.lib().lchd_radial_validate(N.dp(ed), len(ed)) == 0, e


@pytest.mark.parametrize("name", sorted(BAD_EDGES))
def test_python_methods_raise_before_any_device_is_touched(name):
    import loco_hd_amd as lh

    l = lh.LoCoHD(["A", "B"], lh.WeightFunction("uniform", [3.0, 10.0]))
    atoms = [lh.PrimitiveAtom("A", "x", [0.0, 0.0, 0.0]), lh.PrimitiveAtom("B", "y", [1.0, 0.0, 0.0])]
    xyz = np.asarray([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
    dmx = np.asarray([[0.0, 1.0], [1.0, 0.0]])
    ed = BAD_EDGES[name]
    with pytest.raises(ValueError):
        l.radial_from_primitives(atoms, atoms, [(0, 1)], 5.0, ed)
    with pytest.raises(ValueError):
        l.radial_from_coords(["A", "B"], ["A", "B"], xyz, xyz, ed)
    with pytest.raises(ValueError):
        l.radial_from_dmxs(["A", "B"], ["A", "B"], dmx, dmx, ed)
    assert l._ctx is None  # no context was created


def test_device_groups_are_refused():
    import loco_hd_amd as lh

    l = lh.LoCoHD(["A", "B"], lh.WeightFunction("uniform", [3.0, 10.0]), devices=[0])
    atoms = [lh.PrimitiveAtom("A", "x", [0.0, 0.0, 0.0])]
    with pytest.raises(ValueError, match="one device"):
        l.radial_from_primitives(atoms, atoms, [(0, 0)], 5.0, [0.0, INF])
    assert l._ctx is None and l._group is None


# ---- the interval-splitting header --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def split_exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("a host C++ compiler is needed to build tests/radial_bins_cases.cpp")
    exe = tmp_path_factory.mktemp("radial_bins") / "radial_bins_cases"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", str(ROOT / "loco_hd_amd" / "csrc"),
                           str(ROOT / "tests" / "radial_bins_cases.cpp"), "-o", str(exe)])
    return exe


def run_split(exe, bounds, intervals):
    text = f"{len(bounds) - 1}\n" + " ".join(repr(float(b)) for b in bounds) + f"\n{len(intervals)}\n"
    text += "\n".join(f"{lo!r} {hi!r} {h!r}" for lo, hi, h in intervals) + "\n"
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, (out.returncode, out.stderr)
    sums, bins = out.stdout.splitlines()
    return np.asarray([float.fromhex(t) for t in sums.split()]), [int(t) for t in bins.split()]


def test_the_header_has_no_hip_include():
    text = (ROOT / "loco_hd_amd" / "csrc" / "lchd_radial_bins.h").read_text()
    assert "#include" not in text and "__global__" not in text


BOUNDS = [0.125, 0.25, 0.5, 0.5, 0.625, 0.875]  # (a bin of zero width: bounds 2 and 3 coincide)
SHAPES = {
    "inside one bin": [(0.3, 0.4, 0.7)],
    "spanning several bins": [(0.2, 0.8, 0.5)],
    "ending exactly on a bound": [(0.3, 0.5, 0.9), (0.5, 0.625, 0.25)],
    "starting exactly on a bound": [(0.25, 0.3, 1.0)],
    "before the first bound": [(0.0, 0.1, 0.6), (0.1, 0.125, 0.6)],
    "across the first bound": [(0.0625, 0.1875, 0.4)],
    "after the last bound": [(0.875, 0.9, 0.3), (0.9, 1.0, 0.3)],
    "across the last bound": [(0.75, 1.0, 0.8)],
    "everything": [(0.0, 1.0, 1.0)],
    "zero width": [(0.3, 0.3, 0.5), (0.5, 0.5, 0.5)],
    "a chunk": [(0.0, 0.13, 0.11), (0.13, 0.13, 0.5), (0.13, 0.26, 0.22), (0.26, 0.5, 0.33), (0.5, 0.51, 0.44), (0.51, 0.99, 0.55)],
}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_split_matches_the_definition(split_exe, shape):
    got, bins = run_split(split_exe, BOUNDS, SHAPES[shape])
    want = sum(radial_util.split(lo, hi, h, BOUNDS) for lo, hi, h in SHAPES[shape])
    assert np.max(np.abs(got - want)) <= 4e-16  # (a handful of products of numbers <= 1, f64 against longdouble)
    assert got[2] == 0.0  # the zero-width bin
    assert bins == sorted(bins) and all(0 <= b < len(BOUNDS) - 1 for b in bins)


def test_split_random_chunks(split_exe):
    rng = np.random.default_rng(3)
    for K in (1, 2, 7, 64):
        bounds = np.sort(rng.uniform(0.05, 0.95, K + 1))
        cuts = np.sort(np.concatenate([rng.uniform(0.0, 1.0, 40), bounds[rng.integers(0, K + 1, 5)]]))  # some cuts ON bounds
        intervals = [(float(a), float(b), float(h)) for a, b, h in zip(cuts[:-1], cuts[1:], rng.uniform(0, 1, len(cuts) - 1))]
        got, _ = run_split(split_exe, bounds, intervals)
        want = sum(radial_util.split(lo, hi, h, bounds) for lo, hi, h in intervals)
        assert np.max(np.abs(got - want)) <= 1e-15
