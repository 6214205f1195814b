"""tests/cabi_cross.c: a C99 client of the cross-scoring entry points, compiled against the header, linked with the library and run.  The
client checks the matrix against lchd_from_primitives, the tiling, the selection rule and the error codes; here its matrix is compared
with the CPU oracle on the same input and its nearest rows pass the acceptance check of tests/cross_util.py against the oracle's matrix."""
import math
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import cross_util as cu

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent


def test_c_client_of_the_cross_entry_points(tmp_path, oracle):
    if shutil.which("gcc") is None:
        pytest.fail("gcc is needed to build the C client")
    exe = tmp_path / "cabi_cross"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", str(ROOT / "include"),
                           str(ROOT / "tests" / "cabi_cross.c"), "-o", str(exe), "-L", str(ROOT / "loco_hd_amd"), "-lloco_hd_hip",
                           "-lm", f"-Wl,-rpath,{ROOT / 'loco_hd_amd'}"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    assert "cabi cross ok" in out.stdout

    n, na, nb, k = 48, 7, 70, 5
    cats = [f"c{c}" for c in range(5)]
    xa = [[math.fmod(7.31 * i, 11.0) + 0.5, math.fmod(3.77 * i, 11.0) + 0.5, math.fmod(5.13 * i, 11.0) + 0.5] for i in range(n)]
    xb = [[math.fmod(2.91 * i, 11.0) + 0.5, math.fmod(6.43 * i, 11.0) + 0.5, math.fmod(4.57 * i, 11.0) + 0.5] for i in range(n)]
    pa = [oracle.PrimitiveAtom(cats[(3 * i + 1) % 5], f"t{i % 3}", xa[i]) for i in range(n)]
    pb = [oracle.PrimitiveAtom(cats[(2 * i + 3) % 5], f"t{i % 3}", xb[i]) for i in range(n)]
    anchors_a, anchors_b = [(7 * i) % n for i in range(na)], [(11 * j + 5) % n for j in range(nb)]
    lchd = oracle.LoCoHD(cats, oracle.WeightFunction("uniform", [3.0, 10.0]), category_weights=[1.0, 2.0, 0.5, 1.0, 1.5])
    want = np.asarray(lchd.from_primitives(pa, pb, [(i, j) for i in anchors_a for j in anchors_b], 6.5)).reshape(na, nb)

    cross, nearest = {}, {}
    for ln in out.stdout.splitlines():
        f = ln.split()
        if f and f[0] == "cross":
            cross[int(f[1])] = [float(v) for v in f[2:]]
        elif f and f[0] == "nearest":
            nearest[int(f[1])] = f[2:]
    assert sorted(cross) == sorted(nearest) == list(range(na))
    got = np.asarray([cross[i] for i in range(na)])
    assert got.shape == (na, nb) and float(np.max(np.abs(got - want))) <= 1e-11
    scores = np.asarray([[float(v) for v in nearest[i][1::2]] for i in range(na)])
    cols = np.asarray([[int(v) for v in nearest[i][0::2]] for i in range(na)], dtype=np.int32)
    cu.accept(scores, cols, want, k, 1e-11)
