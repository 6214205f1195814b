"""A plain-C client of lchd_ensemble_from_coords (tests/cabi_ensemble.c): the dense ensemble entry point through the C ABI only."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def _build(tmp_path):
    exe = tmp_path / "cabi_ensemble"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", str(ROOT / "include"),
                           str(ROOT / "tests" / "cabi_ensemble.c"), "-o", str(exe), "-L", str(ROOT / "loco_hd_amd"), "-lloco_hd_hip",
                           "-lm", f"-Wl,-rpath,{ROOT / 'loco_hd_amd'}"])
    return exe


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_ensemble_client_links(tmp_path):
    assert _build(tmp_path).exists()


@pytest.mark.gpu
def test_ensemble_client_runs(tmp_path):
    exe = _build(tmp_path)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cabi ensemble ok" in out.stdout
