"""tests/cabi_sensitivity_coords_periodic.c: a C99 client of lchd_sensitivity_coords_periodic (a box on side A, a NULL cell on side B),
compiled against the header, linked with the library and run.  The client checks what needs no reference; here its rows are compared
with the numpy model (tests/min_image_sensitivity_util.py) on the same input: idx, dist and disp exactly, g within the bound of
tests/test_gpu_sensitivity.py."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import min_image_sensitivity_util as mu
from test_gpu_sensitivity import TOL_G

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent


def test_c_client_of_the_periodic_dense_sensitivity_entry_point(tmp_path):
    if shutil.which("gcc") is None:
        pytest.fail("gcc is needed to build the C client")
    exe = tmp_path / "cabi_sensitivity_coords_periodic"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", str(ROOT / "include"),
                           str(ROOT / "tests" / "cabi_sensitivity_coords_periodic.c"), "-o", str(exe), "-L", str(ROOT / "loco_hd_amd"),
                           "-lloco_hd_hip", "-lm", f"-Wl,-rpath,{ROOT / 'loco_hd_amd'}"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    assert "cabi sensitivity coords periodic ok" in out.stdout

    xa = np.asarray([[1.5, 2.25, 3.0], [9.5, 2.25, 3.0], [1.5, 14.25, 3.0], [6.0, 7.5, 11.25], [13.0, 1.0, 17.5], [-20.5, 30.0, 4.75]])
    xb = np.asarray([[0.0, 0.0, 0.0], [4.0, 1.0, 0.5], [2.5, 6.0, 3.25], [9.0, 2.0, 7.5], [1.0, 11.0, 2.0], [5.5, 5.5, 12.0]])
    want = mu.sensitivity([0, 1, 1, 0, 1, 0], xa, ("box", [16.0, 12.0, 20.0]), [1, 0, 0, 1, 1, 0], xb, None, 2, ("uniform", [3.0, 10.0]))
    rows = {"a": {}, "b": {}, "score": {}}
    for ln in out.stdout.splitlines():
        f = ln.split()
        if f and f[0] in rows:
            rows[f[0]][int(f[1])] = f[2:]
    assert len(rows["score"]) == len(rows["a"]) == len(rows["b"]) == 6
    for r in range(6):
        assert abs(float(rows["score"][r][0]) - want.scores[r]) <= 1e-11
        for side, cnt, idx, dist, g, disp in (("a", want.count_a, want.idx_a, want.dist_a, want.g_a, want.disp_a),
                                              ("b", want.count_b, want.idx_b, want.dist_b, want.g_b, want.disp_b)):
            f = rows[side][r]
            c = int(f[0])
            assert c == cnt[r] == 6
            assert [int(v) for v in f[1::6]] == list(idx[r, :c]) and [float(v) for v in f[2::6]] == list(dist[r, :c])
            assert np.max(np.abs(np.asarray([float(v) for v in f[3::6]]) - g[r, :c])) <= TOL_G
            got = np.asarray([[float(f[4 + 6 * t + k]) for k in range(3)] for t in range(c)])
            assert np.array_equal(got, disp[r, :c])
