"""The host side of the cross-scoring calls, without a device: the tile planner lchd_cross_plan (through the C ABI, and its arithmetic
header under AddressSanitizer + UBSan in a stand-alone program, tests/cross_plan_cases.cpp) and the argument checks of
LoCoHD.cross_from_primitives / nearest_from_primitives that run before any device is touched.  The expected tile sizes are written out
by hand from the rule: the largest rows in 1 .. n_a with rows * n_b * 28 bytes <= budget and rows * n_b <= 2^31 - 1."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
PAIR = 28            # bytes per pair of a tile: a [2] int64 record, an int32 weight-function index, a float64 score
CAP = 2**31 - 1      # pairs of one pass
I64 = 2**63 - 1

# name -> ((n_a, n_b, budget), tile_rows or None: LCHD_EUNSUPPORTED); the same table as tests/cross_plan_cases.cpp
PLAN_CASES = {
    "fits_exactly": ((100, 130, 7 * 130 * PAIR), 7),
    "one_byte_below": ((100, 130, 7 * 130 * PAIR - 1), 6),
    "one_row_exactly": ((100, 130, 130 * PAIR), 1),
    "one_row_one_byte_below": ((100, 130, 130 * PAIR - 1), None),
    "no_budget": ((100, 130, 0), None),
    "clamped_to_n_a": ((37, 130, I64), 37),
    "single_anchor": ((1, 130, I64), 1),
    "single_anchor_tight": ((1, 130, 130 * PAIR), 1),
    "single_column": ((5, 1, 3 * PAIR), 3),
    "cap_row_at_limit": ((10, CAP, I64), 1),
    "cap_row_above_limit": ((10, CAP + 1, I64), None),      # n_b = 2^31: one row is more than a pass takes
    "cap_two_rows": ((10, CAP // 2, I64), 2),
    "cap_two_rows_plus_1": ((10, CAP // 2 + 1, I64), 1),
    "cap_65536": ((1 << 20, 65536, I64), 32767),            # 32 768 rows would be 2^31 pairs
    "largest_arguments": ((I64, I64, I64), None),
    "largest_rows": ((I64, 1, I64), CAP),
}


def _lh():
    import loco_hd_amd as lh

    return lh


def _plan(n_a, n_b, budget):
    from loco_hd_amd import _native as N

    rows = C.c_int64(-7)
    rc = N.lib().lchd_cross_plan(n_a, n_b, budget, C.byref(rows))
    return rc, int(rows.value)


@pytest.mark.parametrize("name", sorted(PLAN_CASES))
def test_cross_plan(name):
    from loco_hd_amd import _native as N

    (n_a, n_b, budget), want = PLAN_CASES[name]
    rc, rows = _plan(n_a, n_b, budget)
    if want is None:
        assert rc == N.EUNSUPPORTED and rows == 0
        assert str(n_b) in N.lib().lchd_last_error().decode()
    else:
        assert (rc, rows) == (N.OK, want)
        assert 1 <= rows <= n_a and rows * n_b <= CAP and rows * n_b * PAIR <= budget
        assert rows == n_a or (rows + 1) * n_b > CAP or (rows + 1) * n_b * PAIR > budget  # the largest such


def test_cross_plan_never_above_n_a_and_monotonic():
    last = 0
    for n_a in (1, 2, 3, 36, 37, 38, 1000):
        rc, rows = _plan(n_a, 130, 37 * 130 * PAIR)
        assert rc == 0 and rows == min(n_a, 37) and rows >= last
        last = rows


def test_cross_plan_bad_arguments():
    from loco_hd_amd import _native as N

    for args in ((0, 5, 1000), (5, 0, 1000), (-1, 5, 1000), (5, 5, -1)):
        rc, rows = _plan(*args)
        assert rc == N.EVALUE and rows == 0, args
    assert N.lib().lchd_cross_plan(5, 5, 1000, None) == N.EVALUE


def test_cross_plan_header_under_sanitizers(tmp_path):
    """The arithmetic itself (loco_hd_amd/csrc/lchd_cross_plan.h) in a stand-alone host program built with AddressSanitizer and UBSan:
    no report, and the same table."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("a host C++ compiler is needed to build tests/cross_plan_cases.cpp")
    text = (ROOT / "loco_hd_amd" / "csrc" / "lchd_cross_plan.h").read_text()
    assert "hip/" not in text and "__device__" not in text and "__global__" not in text
    exe = tmp_path / "cross_plan_cases"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", str(ROOT / "loco_hd_amd" / "csrc"), str(ROOT / "tests" / "cross_plan_cases.cpp"),
                           "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and not out.stderr, out.stderr
    got = {}
    for line in out.stdout.splitlines():
        name, _, rest = line.partition(": ")
        got[name] = dict(tok.split("=") for tok in rest.split())
    assert got.pop("constants") == dict(pair_bytes=str(PAIR), max_tile_pairs=str(CAP), max_k="64")
    assert sorted(got) == sorted(PLAN_CASES)
    for name, (_, want) in PLAN_CASES.items():
        assert int(got[name]["rows"]) == (want or 0), name


# ---- Python argument checks: each raises before a context (a device) is asked for ----------------------------------------------------
CATS = ["A", "B", "C"]


@pytest.fixture()
def atoms():
    lh = _lh()
    return [lh.PrimitiveAtom(CATS[i % 3], "", [float(i), 0.5 * i, 0.0]) for i in range(8)]


def _no_context(lchd):
    assert lchd._ctx is None and lchd._group is None, "the check touched a device"


@pytest.mark.parametrize("k, nb", [(0, 5), (65, 80), (6, 5), (-1, 5)])
def test_nearest_refuses_k_outside_its_range(atoms, k, nb):
    lchd = _lh().LoCoHD(CATS)
    with pytest.raises(ValueError) as e:
        lchd.nearest_from_primitives(atoms, atoms, [0, 1], [j % 8 for j in range(nb)], 5.0, k)
    assert str(k) in str(e.value) and str(nb) in str(e.value)
    _no_context(lchd)


def test_negative_tile_rows(atoms):
    lchd = _lh().LoCoHD(CATS)
    with pytest.raises(ValueError, match="tile_rows = -1"):
        lchd.cross_from_primitives(atoms, atoms, [0, 1], [2, 3], 5.0, tile_rows=-1)
    with pytest.raises(ValueError, match="tile_rows = -3"):
        lchd.nearest_from_primitives(atoms, atoms, [0, 1], [2, 3], 5.0, 1, tile_rows=-3)
    _no_context(lchd)


def test_empty_anchor_lists_raise_what_an_empty_pair_list_raises(atoms):
    lchd = _lh().LoCoHD(CATS)
    with pytest.raises(ValueError) as want:
        lchd.from_primitives(atoms, atoms, [], 5.0)
    for a, b in (([], [1, 2]), ([1, 2], []), ([], [])):
        with pytest.raises(ValueError) as e:
            lchd.cross_from_primitives(atoms, atoms, a, b, 5.0)
        assert str(e.value) == str(want.value)
    with pytest.raises(ValueError) as e:
        lchd.nearest_from_primitives(atoms, atoms, [], [1, 2], 5.0, 1)
    assert str(e.value) == str(want.value)
    with pytest.raises(ValueError):
        lchd.nearest_from_primitives(atoms, atoms, [1, 2], [], 5.0, 1)  # (k > Nb = 0 comes first)
    _no_context(lchd)


def test_weight_function_key_rules(atoms):
    lh = _lh()
    single = lh.LoCoHD(CATS)
    many = lh.LoCoHD(CATS, {"near": lh.WeightFunction("uniform", [0.0, 4.0]), "far": lh.WeightFunction("uniform", [3.0, 10.0])})
    with pytest.raises(ValueError, match="invalid weight function keys"):
        many.cross_from_primitives(atoms, atoms, [0], [1], 5.0, "nowhere")
    with pytest.raises(ValueError, match="invalid weight function keys"):
        many.nearest_from_primitives(atoms, atoms, [0], [1], 5.0, 1, "nowhere")
    with pytest.raises(ValueError, match="Invalid pairing"):
        many.cross_from_primitives(atoms, atoms, [0], [1], 5.0)
    with pytest.raises(ValueError, match="Invalid pairing"):
        single.cross_from_primitives(atoms, atoms, [0], [1], 5.0, "near")
    _no_context(single)
    _no_context(many)


def test_negative_anchor(atoms):
    lchd = _lh().LoCoHD(CATS)
    with pytest.raises(OverflowError):
        lchd.cross_from_primitives(atoms, atoms, [0, -1], [1], 5.0)
    _no_context(lchd)


def test_device_groups_are_refused_by_name(atoms):
    lchd = _lh().LoCoHD(CATS, devices=[0, 1])
    for call in (lambda: lchd.cross_from_primitives(atoms, atoms, [0], [1], 5.0),
                 lambda: lchd.nearest_from_primitives(atoms, atoms, [0], [1], 5.0, 1)):
        with pytest.raises(NotImplementedError, match=r"\[0, 1\]"):
            call()
    _no_context(lchd)
