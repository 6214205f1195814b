"""tests/cabi_gradient_periodic.c: a C99 client of lchd_gradient_primitives_periodic and lchd_gradient_coords_periodic, compiled against the
header (-Wall -Wextra -pedantic -Werror: the prototypes as a C caller sees them), linked with the library and run.  The client makes its
own expected values: the lists of the periodic sensitivity calls reduced in long double, to 8 DBL_EPSILON of the largest sum of |terms|;
exact symmetry of both strain tensors; the sensitivity call's scores in every bit."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
ROCM = Path(os.environ.get("ROCM_PATH", "/opt/rocm"))


def test_c_client_of_the_periodic_gradient_entry_points(tmp_path):
    import loco_hd_amd  # noqa: F401  (the library the client links is the package's)

    if shutil.which("gcc") is None:
        pytest.fail("gcc is needed to build the C client")
    exe = tmp_path / "cabi_gradient_periodic"
    subprocess.check_call(["gcc", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", str(ROOT / "include"),
                           str(ROOT / "tests" / "cabi_gradient_periodic.c"), "-o", str(exe), "-L", str(ROOT / "loco_hd_amd"), "-lloco_hd_hip",
                           "-L", str(ROCM / "lib"), "-lamdhip64", "-lm", f"-Wl,-rpath,{ROOT / 'loco_hd_amd'}", f"-Wl,-rpath,{ROCM / 'lib'}"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    assert "cabi gradient periodic ok" in out.stdout
