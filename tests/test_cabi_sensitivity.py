"""tests/cabi_sensitivity.c: a C99 client of the sensitivity entry points, compiled against the header, linked with the library and run.
The client checks the scores against lchd_from_primitives, the list order, the padding and the error paths; here its rows are compared
with the numpy restatement (tests/sensitivity_util.py) on the same input, g within the bound of tests/test_gpu_sensitivity.py."""
import math
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import sensitivity_util as su
from test_gpu_sensitivity import TOL_G

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent


def test_c_client_of_the_sensitivity_entry_points(tmp_path):
    if shutil.which("gcc") is None:
        pytest.fail("gcc is needed to build the C client")
    exe = tmp_path / "cabi_sensitivity"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", str(ROOT / "include"),
                           str(ROOT / "tests" / "cabi_sensitivity.c"), "-o", str(exe), "-L", str(ROOT / "loco_hd_amd"), "-lloco_hd_hip",
                           "-lm", f"-Wl,-rpath,{ROOT / 'loco_hd_amd'}"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    assert "cabi sensitivity ok" in out.stdout

    n, n_pairs = 48, 20
    xa = np.asarray([[math.fmod(7.31 * i, 11.0) + 0.5, math.fmod(3.77 * i, 11.0) + 0.5, math.fmod(5.13 * i, 11.0) + 0.5] for i in range(n)])
    xb = np.asarray([[math.fmod(2.91 * i, 11.0) + 0.5, math.fmod(6.43 * i, 11.0) + 0.5, math.fmod(4.57 * i, 11.0) + 0.5] for i in range(n)])
    ca, cb = np.asarray([(3 * i + 1) % 5 for i in range(n)]), np.asarray([(2 * i + 3) % 5 for i in range(n)])
    tag = np.asarray([i % 3 for i in range(n)])
    pairs = [((7 * k) % n, (11 * k + 5) % n) for k in range(n_pairs)]
    want = su.from_primitives(ca, xa, tag, cb, xb, tag, pairs, 6.5, 5, ("uniform", [3.0, 10.0]), ("Hellinger", [2.0]), [1.0, 2.0, 0.5, 1.0, 1.5])
    rows = {"a": {}, "b": {}, "score": {}}
    for ln in out.stdout.splitlines():
        f = ln.split()
        if f and f[0] in rows:
            rows[f[0]][int(f[1])] = f[2:]
    assert len(rows["score"]) == len(rows["a"]) == len(rows["b"]) == n_pairs
    for p in range(n_pairs):
        assert abs(float(rows["score"][p][0]) - want.scores[p]) <= 1e-11
        for side, cnt, idx, dist, g in (("a", want.count_a, want.idx_a, want.dist_a, want.g_a), ("b", want.count_b, want.idx_b, want.dist_b, want.g_b)):
            f = rows[side][p]
            c = int(f[0])
            assert c == cnt[p]
            assert [int(v) for v in f[1::3]] == list(idx[p, :c]) and [float(v) for v in f[2::3]] == list(dist[p, :c])
            assert np.max(np.abs(np.asarray([float(v) for v in f[3::3]]) - g[p, :c])) <= TOL_G
