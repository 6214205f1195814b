"""tests/cabi_sensitivity_dense.c: a C99 client of lchd_sensitivity_dmxs, compiled against the header, linked with the library and run.
The client checks the hand-computed list order, the counts, the padding, the scores against lchd_from_dmxs and the error paths; here
its rows are compared with the numpy restatement (tests/dense_sensitivity_util.py) on the same input, g within the bound of
tests/test_gpu_sensitivity.py."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import dense_sensitivity_util as du
from test_gpu_sensitivity import TOL_G

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent


def test_c_client_of_the_dense_sensitivity_entry_point(tmp_path):
    if shutil.which("gcc") is None:
        pytest.fail("gcc is needed to build the C client")
    exe = tmp_path / "cabi_sensitivity_dense"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", str(ROOT / "include"),
                           str(ROOT / "tests" / "cabi_sensitivity_dense.c"), "-o", str(exe), "-L", str(ROOT / "loco_hd_amd"), "-lloco_hd_hip",
                           "-lm", f"-Wl,-rpath,{ROOT / 'loco_hd_amd'}"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    assert "cabi sensitivity dense ok" in out.stdout

    dmx_a = np.asarray([[4.5, 0.0, 4.5, 0.0, 7.25], [9.0, 3.5, 12.0, 6.0, 0.0]])
    dmx_b = np.asarray([[0.0, 8.0, 5.0], [6.5, 0.0, 6.5]])
    want = du.from_dmxs([0, 1, 1, 0, 1], dmx_a, [1, 0, 0], dmx_b, 2, ("uniform", [3.0, 10.0]))
    assert want.idx_a.tolist() == [[1, 3, 0, 2, 4], [4, 1, 3, 0, 2]] and want.idx_b[:, :3].tolist() == [[0, 2, 1], [1, 0, 2]]  # the client's order
    rows = {"a": {}, "b": {}, "score": {}}
    for ln in out.stdout.splitlines():
        f = ln.split()
        if f and f[0] in rows:
            rows[f[0]][int(f[1])] = f[2:]
    assert len(rows["score"]) == len(rows["a"]) == len(rows["b"]) == 2
    for r in range(2):
        assert abs(float(rows["score"][r][0]) - want.scores[r]) <= 1e-11
        for side, cnt, idx, dist, g in (("a", want.count_a, want.idx_a, want.dist_a, want.g_a), ("b", want.count_b, want.idx_b, want.dist_b, want.g_b)):
            f = rows[side][r]
            c = int(f[0])
            assert c == cnt[r]
            assert [int(v) for v in f[1::3]] == list(idx[r, :c]) and [float(v) for v in f[2::3]] == list(dist[r, :c])
            assert np.max(np.abs(np.asarray([float(v) for v in f[3::3]]) - g[r, :c])) <= TOL_G
