"""tests/cabi_param_sum.c: a C99 client with its own main that replays the host path of loco_hd_amd/csrc/lchd_param_sum.h -- the text the
kernel runs per slot -- on the cases of tests/param_sum_util.py, read from a text file written here, and prints the sums with exact bits.
They must be the bits of the Python-integer model.  Built once with -fsanitize=address,undefined as a stand-alone program (the header
alone, no library): the sanitizers must stay silent.  Built once more against the library, the same client checks lchd_param_sum_plan
against the formula of include/loco_hd_hip.h.  No GPU is needed and no Python code runs under a sanitizer."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import gradient_native_util as gn
import param_sum_util as ps

ROOT = Path(__file__).resolve().parent.parent
CASES = ps.drawn_cases()


def _need(tool):
    if shutil.which(tool) is None:
        pytest.fail(f"{tool} is needed to build the C client")


def _write_cases(path):
    lines = []
    for name, (rows, w, bucket, nb) in sorted(CASES.items()):
        lines.append(f"case {name} {rows.shape[0]} {rows.shape[1]} {int(w is not None)} {int(bucket is not None)} {nb}")
        for p in range(rows.shape[0]):
            tok = [float(x).hex() for x in rows[p]]
            if w is not None:
                tok.append(float(w[p]).hex())
            if bucket is not None:
                tok.append(str(int(bucket[p])))
            lines.append(" ".join(tok))
    path.write_text("\n".join(lines) + "\n")


def _check_sums(stdout):
    seen = {}
    for ln in stdout.splitlines():
        if ln.startswith("sum "):
            tok = ln.split()
            seen[tok[1]] = (int(tok[2]), np.asarray([float.fromhex(v) for v in tok[3:]]))
    assert sorted(seen) == sorted(CASES)
    for name, (rows, w, bucket, nb) in CASES.items():
        want, flag = ps.param_sum(rows, w, bucket, nb)
        assert seen[name][0] == flag, name
        assert gn.bits(seen[name][1]).tolist() == gn.bits(want.reshape(-1)).tolist(), name
    assert seen["limit"][0] == 1 and seen["infinite"][0] == 1 and seen["below_limit"][0] == 0


def test_host_path_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    _need("gcc")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1", "-fno-omit-frame-pointer"]
    exe, cases = tmp_path / "param_sum_asan", tmp_path / "cases.txt"
    _write_cases(cases)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", *san, "-I", str(ROOT / "loco_hd_amd" / "csrc"),
                           str(ROOT / "tests" / "cabi_param_sum.c"), "-o", str(exe), "-lm"])
    out = subprocess.run([str(exe), str(cases)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    assert "cabi param sum ok" in out.stdout and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    _check_sums(out.stdout)


def test_c_client_of_the_plan_and_the_host_path(tmp_path):
    _need("gcc")
    exe, cases = tmp_path / "cabi_param_sum", tmp_path / "cases.txt"
    _write_cases(cases)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-DWITH_LIBRARY", "-I", str(ROOT / "include"), "-I",
                           str(ROOT / "loco_hd_amd" / "csrc"), str(ROOT / "tests" / "cabi_param_sum.c"), "-o", str(exe), "-L",
                           str(ROOT / "loco_hd_amd"), "-lloco_hd_hip", "-lm", f"-Wl,-rpath,{ROOT / 'loco_hd_amd'}"])
    out = subprocess.run([str(exe), str(cases)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    assert "plan ok" in out.stdout and "cabi param sum ok" in out.stdout
    _check_sums(out.stdout)
