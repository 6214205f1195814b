"""tests/cabi_composition.c: a C99 client of the host-array composition entry points, compiled against the header, linked with the
library and run; its tables against the Python calls on the same input."""
import math
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent


def test_c_client_of_the_composition_entry_points(tmp_path):
    import loco_hd_amd as lh

    if shutil.which("gcc") is None:
        pytest.fail("gcc is needed to build the C client")
    exe = tmp_path / "cabi_composition"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", str(ROOT / "include"),
                           str(ROOT / "tests" / "cabi_composition.c"), "-o", str(exe), "-L", str(ROOT / "loco_hd_amd"), "-lloco_hd_hip",
                           "-lm", f"-Wl,-rpath,{ROOT / 'loco_hd_amd'}"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    assert "cabi composition ok" in out.stdout

    def table(name):
        return np.asarray([[float(v) for v in ln.split()[2:]] for ln in out.stdout.splitlines() if ln.startswith(name + " ")])

    n, na, cats = 48, 20, [f"c{k}" for k in range(5)]
    xyz = np.asarray([[math.fmod(7.31 * i, 11.0) + 0.5, math.fmod(3.77 * i, 11.0) + 0.5, math.fmod(5.13 * i, 11.0) + 0.5] for i in range(n)])
    seq = [cats[(3 * i + 1) % 5] for i in range(n)]
    atoms = [lh.PrimitiveAtom(seq[i], f"t{i % 3}", list(xyz[i])) for i in range(n)]
    anchors = [(7 * k) % n for k in range(na)]
    anchors[-1] = anchors[0]
    d = xyz[:, None, :] - xyz[None, :, :]
    dmx = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    for i in range(n):
        for j in range(n):
            if i != j and i // 4 == j // 4:
                dmx[i, j] = np.inf
    box, cell = [12.0, 14.0, 13.0], [[13.0, 0.0, 0.0], [4.0, 12.0, 0.0], [-3.0, 5.0, 14.0]]
    lchd = lh.LoCoHD(cats, lh.WeightFunction("hyper_exp", [1.0, 0.2]), category_weights=[1.0, 2.0, 0.5, 1.0, 1.5])
    want = {
        "prims": lchd.composition_from_primitives(atoms, anchors, 6.0),
        "box": lchd.composition_from_primitives(atoms, anchors, 6.0, box=box),
        "cell": lchd.composition_from_primitives(atoms, anchors, 6.0, cell=cell),
        "coords": lchd.composition_from_coords(seq, xyz),
        "coordscell": lchd.composition_from_coords(seq, xyz, cell=cell),
        "dmx": lchd.composition_from_dmx(seq, dmx),
    }
    for name, w in want.items():
        got = table(name)
        assert got.shape == w.shape, name
        assert np.max(np.abs(got - w)) <= 1e-13, name  # (two runs of one device path)
    assert np.max(np.abs(want["box"] - want["prims"])) > 1e-3  # the box made a difference
