"""A plain-C client of the stream contract (tests/cabi_streams.c, HIP runtime only): the context on a non-blocking stream, anchor
pairs copied with hipMemcpyAsync on that stream right in front of the call, frames loaded on a second non-blocking stream and
scored by the split call -- bit for bit the NULL-stream outputs."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
ROCM = Path(os.environ.get("ROCM_PATH", "/opt/rocm"))


def _build(tmp_path):
    exe = tmp_path / "cabi_streams"
    subprocess.check_call(["gcc", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-Wall", "-Wextra", "-pedantic", "-Werror",
                           "-I", str(ROOT / "include"), "-isystem", str(ROCM / "include"), str(ROOT / "tests" / "cabi_streams.c"), "-o", str(exe),
                           "-L", str(ROOT / "loco_hd_amd"), "-lloco_hd_hip", "-L", str(ROCM / "lib"), "-lamdhip64", "-lm",
                           f"-Wl,-rpath,{ROOT / 'loco_hd_amd'}", f"-Wl,-rpath,{ROCM / 'lib'}"])
    return exe


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_streams_client_links(tmp_path):
    assert _build(tmp_path).exists()


@pytest.mark.gpu
def test_streams_client_runs(tmp_path):
    exe = _build(tmp_path)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=180)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cabi streams ok" in out.stdout
