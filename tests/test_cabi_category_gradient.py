"""tests/cabi_category_gradient.c: a C99 client of the host-array category-weight gradient entry points, compiled against the header,
linked with the library and run.  The client checks the Euler identity of every row; here its tables (printed with exact bits) must be
the bits of the Python calls on the same input."""
import math
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent


def test_c_client_of_the_category_gradient_entry_points(tmp_path):
    import loco_hd_amd as lh

    if shutil.which("gcc") is None:
        pytest.fail("gcc is needed to build the C client")
    exe = tmp_path / "cabi_category_gradient"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", str(ROOT / "include"),
                           str(ROOT / "tests" / "cabi_category_gradient.c"), "-o", str(exe), "-L", str(ROOT / "loco_hd_amd"), "-lloco_hd_hip",
                           "-lm", f"-Wl,-rpath,{ROOT / 'loco_hd_amd'}"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    assert "cabi category gradient ok" in out.stdout

    def table(name):
        return np.asarray([[float.fromhex(v) for v in ln.split()[2:]] for ln in out.stdout.splitlines() if ln.startswith(name + " ")])

    n, n_pairs = 48, 20
    xa = np.asarray([[math.fmod(7.31 * i, 11.0) + 0.5, math.fmod(3.77 * i, 11.0) + 0.5, math.fmod(5.13 * i, 11.0) + 0.5] for i in range(n)])
    xb = np.asarray([[math.fmod(2.91 * i, 11.0) + 0.5, math.fmod(6.43 * i, 11.0) + 0.5, math.fmod(4.57 * i, 11.0) + 0.5] for i in range(n)])
    cats = [f"c{k}" for k in range(5)]
    sa, sb = [cats[(3 * i + 1) % 5] for i in range(n)], [cats[(2 * i + 3) % 5] for i in range(n)]
    tags = [f"t{i % 3}" for i in range(n)]
    pa = [lh.PrimitiveAtom(t, g, list(x)) for t, g, x in zip(sa, tags, xa)]
    pb = [lh.PrimitiveAtom(t, g, list(x)) for t, g, x in zip(sb, tags, xb)]
    pairs = [((7 * k) % n, (11 * k + 5) % n) for k in range(n_pairs)]
    for suffix, sd in (("", lh.StatisticalDistance("Hellinger", [2.0])), ("_kl", lh.StatisticalDistance("Kullback-Leibler", [1e-3]))):
        l = lh.LoCoHD(cats, lh.WeightFunction("uniform", [3.0, 10.0]), category_weights=[1.0, 2.0, 0.5, 1.0, 1.5], statistical_distance=sd)
        prims, coords = table("prims" + suffix), table("coords" + suffix)
        assert prims.shape == (n_pairs, 5) and coords.shape == (n, 5) and np.any(prims != 0.0)
        assert np.array_equal(prims, l.category_gradient_from_primitives(pa, pb, pairs, 6.5))
        assert np.array_equal(coords, l.category_gradient_from_coords(sa, sb, xa, xb))
