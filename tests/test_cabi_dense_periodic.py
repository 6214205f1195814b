"""tests/cabi_dense_periodic.c: a C99 client of lchd_from_coords_periodic, compiled against the header, linked with the library and
run; its scores against the Python call on the same input."""
import math
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent


def test_c_client_of_the_dense_periodic_entry_point(tmp_path):
    import loco_hd_amd as lh

    if shutil.which("gcc") is None:
        pytest.fail("gcc is needed to build the C client")
    exe = tmp_path / "cabi_dense_periodic"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", str(ROOT / "include"),
                           str(ROOT / "tests" / "cabi_dense_periodic.c"), "-o", str(exe), "-L", str(ROOT / "loco_hd_amd"), "-lloco_hd_hip",
                           "-lm", f"-Wl,-rpath,{ROOT / 'loco_hd_amd'}"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    assert "cabi dense periodic ok" in out.stdout
    got = np.asarray([float(ln.split()[2]) for ln in out.stdout.splitlines() if ln.startswith("score ")])
    n = 40
    xa = np.asarray([[math.fmod(7.31 * i, 30.0) - 15.0, math.fmod(3.77 * i, 33.0) - 12.0, math.fmod(5.13 * i, 29.0) - 20.0] for i in range(n)])
    xb = np.asarray([[math.fmod(4.91 * i, 47.0) - 25.0, math.fmod(6.07 * i, 41.0) - 17.0, math.fmod(2.89 * i, 37.0) - 11.0] for i in range(n)])
    cats = [f"c{k}" for k in range(5)]
    sa, sb = [cats[i % 5] for i in range(n)], [cats[(3 * i + 1) % 5] for i in range(n)]
    lchd = lh.LoCoHD(cats, lh.WeightFunction("uniform", [3.0, 10.0]))
    want = np.asarray(lchd.from_coords(sa, sb, xa, xb, box_a=[12.0, 14.0, 13.0], cell_b=[[20.0, 0.0, 0.0], [15.0, 18.0, 0.0], [-9.0, 7.0, 16.0]]))
    assert len(got) == n
    assert np.max(np.abs(got - want)) <= 1e-13  # (two runs of one device path)
