"""A plain-C client that shares one context and one device group between POSIX threads (tests/cabi_threads.c): calls on one
context or group are serialised by the library, so every threaded output equals the serial one and errors stay with their thread."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def _build(tmp_path):
    exe = tmp_path / "cabi_threads"
    subprocess.check_call(["gcc", "-std=c99", "-pthread", "-D_POSIX_C_SOURCE=200809L", "-Wall", "-Wextra", "-pedantic", "-Werror",
                           "-I", str(ROOT / "include"), str(ROOT / "tests" / "cabi_threads.c"), "-o", str(exe),
                           "-L", str(ROOT / "loco_hd_amd"), "-lloco_hd_hip", "-lm", f"-Wl,-rpath,{ROOT / 'loco_hd_amd'}"])
    return exe


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_threads_client_links(tmp_path):
    assert _build(tmp_path).exists()


@pytest.mark.gpu
def test_threads_client_runs(tmp_path):
    exe = _build(tmp_path)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=180)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cabi threads ok" in out.stdout
