"""The host path of loco_hd_amd/csrc/lchd_exact_sum.h against the Python-integer model: tests/cabi_exact_sum.c is compiled with
AddressSanitizer and UBSan, run as a child process on the vectors of tests/exact_sum_cases.py, and must print the model's limbs, flag and
finished double for every one of them.  CPU only; nothing is loaded into Python."""
import shutil
import struct
import subprocess
from pathlib import Path

import pytest

import gradient_native_util as gn
from exact_sum_cases import cases

ROOT = Path(__file__).resolve().parent.parent


def test_c_header_replays_the_model_vectors_under_sanitizers(tmp_path):
    if shutil.which("gcc") is None:
        pytest.fail("gcc is needed to build the C client")
    exe, vec = tmp_path / "cabi_exact_sum", tmp_path / "vectors.txt"
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-g", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", str(ROOT / "loco_hd_amd" / "csrc"), str(ROOT / "tests" / "cabi_exact_sum.c"),
                           "-o", str(exe)])
    names = sorted(cases())
    table = cases()
    with open(vec, "w") as f:
        for name in names:
            f.write(f"{len(table[name])}\n")
            f.writelines(f"{struct.unpack('<Q', struct.pack('<d', v))[0]:x}\n" for v in table[name])
    out = subprocess.run([str(exe), str(vec)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    lines = out.stdout.splitlines()
    assert len(lines) == len(names)
    for name, line in zip(names, lines):
        acc = gn.ExactSum()
        for v in table[name]:
            acc.add(v)
        f = line.split()
        assert [int(x) for x in f[:8]] == acc.limbs, name
        assert int(f[8]) == acc.flag, name
        assert int(f[9], 16) == int(gn.bits(acc.finish()).item()), (name, f[9], acc.finish())
