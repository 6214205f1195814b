"""tests/cabi_gradient.c: a C99 client of the native gradient entry points, compiled against the header, linked with the library and
run.  The expected bits come from here: the contribution rule and the model accumulator (tests/gradient_native_util.py) applied to the
outputs of the sensitivity call on the same inputs."""
import math
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import gradient_native_util as gn

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
ROCM = Path(os.environ.get("ROCM_PATH", "/opt/rocm"))


def test_c_client_of_the_gradient_entry_points(tmp_path):
    import loco_hd_amd as lh

    if shutil.which("gcc") is None:
        pytest.fail("gcc is needed to build the C client")
    n, n_pairs, cats = 40, 12, [f"c{k}" for k in range(5)]
    xa = np.asarray([[math.fmod(7.31 * i, 9.0) + 0.5, math.fmod(3.77 * i, 9.0) + 0.5, math.fmod(5.13 * i, 9.0) + 0.5] for i in range(n)])
    xb = np.asarray([[math.fmod(2.91 * i, 9.0) + 0.5, math.fmod(6.43 * i, 9.0) + 0.5, math.fmod(4.57 * i, 9.0) + 0.5] for i in range(n)])
    ca, cb = [(3 * i + 1) % 5 for i in range(n)], [(2 * i + 3) % 5 for i in range(n)]
    pairs = [((7 * k) % n, (11 * k + 5) % n) for k in range(n_pairs)]
    v = np.asarray([0.5 + 0.125 * k for k in range(n_pairs)])
    l = lh.LoCoHD(cats, lh.WeightFunction("uniform", [3.0, 10.0]), category_weights=[1.0, 2.0, 0.5, 1.0, 1.5])
    atoms_a = [lh.PrimitiveAtom(cats[c], "t", list(x)) for c, x in zip(ca, xa)]
    atoms_b = [lh.PrimitiveAtom(cats[c], "t", list(x)) for c, x in zip(cb, xb)]
    sens = l.sensitivity_from_primitives(atoms_a, atoms_b, pairs, 10.0)
    ga, gb, flag = gn.gradient(sens, xa, xb, v)
    assert flag == 0 and np.any(ga != 0.0) and np.any(gb != 0.0)
    expected = tmp_path / "expected.txt"
    expected.write_text("".join(f"{int(b):x}\n" for part in (sens.scores, ga, gb) for b in gn.bits(part).reshape(-1)))

    exe = tmp_path / "cabi_gradient"
    subprocess.check_call(["gcc", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-Wall", "-Wextra", "-pedantic", "-Werror",
                           "-I", str(ROOT / "include"), "-isystem", str(ROCM / "include"), str(ROOT / "tests" / "cabi_gradient.c"), "-o", str(exe),
                           "-L", str(ROOT / "loco_hd_amd"), "-lloco_hd_hip", "-L", str(ROCM / "lib"), "-lamdhip64", "-lm",
                           f"-Wl,-rpath,{ROOT / 'loco_hd_amd'}", f"-Wl,-rpath,{ROCM / 'lib'}"])
    out = subprocess.run([str(exe), str(expected)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    assert "cabi gradient ok" in out.stdout
