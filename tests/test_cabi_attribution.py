"""tests/cabi_attribution.c: a C99 client of the host-array attribution entry points, compiled against the header, linked with the
library and run.  The client checks every row sum against the scoring call of the same name to 1e-12; here its thresholded tables are
compared with the numpy restatement (tests/attribution_util.py) on the same input."""
import math
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import attribution_util as au

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent


def test_c_client_of_the_attribution_entry_points(tmp_path):
    if shutil.which("gcc") is None:
        pytest.fail("gcc is needed to build the C client")
    exe = tmp_path / "cabi_attribution"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", str(ROOT / "include"),
                           str(ROOT / "tests" / "cabi_attribution.c"), "-o", str(exe), "-L", str(ROOT / "loco_hd_amd"), "-lloco_hd_hip",
                           "-lm", f"-Wl,-rpath,{ROOT / 'loco_hd_amd'}"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    assert "cabi attribution ok" in out.stdout

    def table(name):
        return np.asarray([[float(v) for v in ln.split()[2:]] for ln in out.stdout.splitlines() if ln.startswith(name + " ")])

    n, n_pairs = 48, 20
    xa = np.asarray([[math.fmod(7.31 * i, 11.0) + 0.5, math.fmod(3.77 * i, 11.0) + 0.5, math.fmod(5.13 * i, 11.0) + 0.5] for i in range(n)])
    xb = np.asarray([[math.fmod(2.91 * i, 11.0) + 0.5, math.fmod(6.43 * i, 11.0) + 0.5, math.fmod(4.57 * i, 11.0) + 0.5] for i in range(n)])
    ca, cb = np.asarray([(3 * i + 1) % 5 for i in range(n)]), np.asarray([(2 * i + 3) % 5 for i in range(n)])
    tag = np.asarray([i % 3 for i in range(n)])
    pairs = [((7 * k) % n, (11 * k + 5) % n) for k in range(n_pairs)]
    weights = [1.0, 2.0, 0.5, 1.0, 1.5]
    for suffix, e in (("", 2.0), ("3.5", 3.5)):
        want = au.from_primitives(ca, xa, tag, cb, xb, tag, pairs, 6.5, 5, ("uniform", [3.0, 10.0]), e, weights)
        got = table("prims" + suffix)
        assert got.shape == want.shape
        assert np.max(np.abs(got - want)) <= 1e-11
        rows = au.from_rows(ca, au.open_rows(xa), cb, au.open_rows(xb), 5, ("uniform", [3.0, 10.0]), e, weights)
        assert np.max(np.abs(table("coords" + suffix) - rows)) <= 1e-11
        assert table("box" + suffix).shape == (n_pairs, 5) and table("dmxs" + suffix).shape == (n, 5)
        assert np.max(np.abs(table("box" + suffix) - got)) > 1e-3  # the box made a difference
