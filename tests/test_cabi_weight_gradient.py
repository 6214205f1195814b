"""tests/cabi_weight_gradient.c: a C99 client of lchd_wf_cdf_grad and of lchd_weight_gradient_width, compiled against the header, linked
with the library and run -- no GPU is needed.  The client checks the conventions by itself; here its tables (printed with exact bits)
must be the bits of WeightFunction.cdf_param_grad_vec on the same points.

The host leaf (cdf_param_grad of lchd_math.h, a host + device header) is also run under AddressSanitizer and UBSan in a stand-alone
program of its own: the same client, with the library's entry point replaced by a translation unit that wraps the header, both built
with -fsanitize=address,undefined.  No Python code runs under a sanitizer."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
X = [0.0, 1.0, 2.0, 3.0, 6.5, 10.0, 11.0, 12.5, float("inf")]
TABLES = {"uniform": [3.0, 10.0], "kumaraswamy": [2.0, 11.0, 0.5, 0.5], "dagum": [4.0, 6.0, 1.5], "hyper_exp": [1.0, 0.5, 0.2, 0.05]}

# The entry points the client calls, on the header alone: what loco_hd_amd/csrc/lchd_capi.hip does around cdf_param_grad.
SHIM = r"""
#include <cstdio>
#include "loco_hd_hip.h"
#include "lchd_math.h"
static int valid(int32_t kind, const double* p, int32_t np) {
    if (kind == LCHD_WF_UNIFORM) return np == 2 && p[0] >= 0.0 && p[1] > 0.0 && p[0] < p[1];
    if (kind == LCHD_WF_KUMARASWAMY) return np == 4 && p[0] >= 0.0 && p[1] > 0.0 && p[2] > 0.0 && p[3] > 0.0 && p[0] < p[1];
    if (kind == LCHD_WF_DAGUM) return np == 3 && p[0] >= 0.0 && p[1] >= 0.0 && p[2] >= 0.0;
    return kind == LCHD_WF_HYPER_EXP && np % 2 == 0;
}
extern "C" int lchd_wf_cdf_grad(int32_t kind, const double* p, int32_t np, const double* x, int64_t n, double* out) {
    if (!valid(kind, p, np)) return LCHD_EVALUE;
    if (n > 0 && (!x || !out)) return LCHD_EVALUE;
    for (int64_t i = 0; i < n; ++i) {
        if (x[i] < 0.0) return LCHD_EVALUE;
        lchd::cdf_param_grad(kind, p, np, x[i], out + i * (int64_t)np);
    }
    return LCHD_OK;
}
extern "C" int32_t lchd_weight_gradient_width(lchd_ctx*) { return 0; }
extern "C" const char* lchd_last_error(void) { return ""; }
"""


def _tables(stdout):
    return {name: np.asarray([[float.fromhex(v) for v in ln.split()[2:]] for ln in stdout.splitlines() if ln.startswith(name + " ")])
            for name in TABLES}


def _need(tool):
    if shutil.which(tool) is None:
        pytest.fail(f"{tool} is needed to build the C client")


def test_c_client_of_the_leaf_and_the_width_query(tmp_path):
    import loco_hd_amd as lh

    _need("gcc")
    exe = tmp_path / "cabi_weight_gradient"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", str(ROOT / "include"),
                           str(ROOT / "tests" / "cabi_weight_gradient.c"), "-o", str(exe), "-L", str(ROOT / "loco_hd_amd"), "-lloco_hd_hip",
                           "-lm", f"-Wl,-rpath,{ROOT / 'loco_hd_amd'}"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    assert "cabi weight gradient ok" in out.stdout
    for name, table in _tables(out.stdout).items():
        assert table.shape == (len(X), len(TABLES[name])) and np.any(table != 0.0)
        assert np.array_equal(table, lh.WeightFunction(name, TABLES[name]).cdf_param_grad_vec(X)), name


def test_the_host_leaf_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    _need("gcc")
    _need("g++")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1", "-fno-omit-frame-pointer"]
    shim, client, exe = tmp_path / "leaf_shim.cpp", tmp_path / "client.o", tmp_path / "leaf_asan"
    shim.write_text(SHIM)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", *san, "-I", str(ROOT / "include"), "-c",
                           str(ROOT / "tests" / "cabi_weight_gradient.c"), "-o", str(client)])
    subprocess.check_call(["g++", "-std=c++17", "-Wall", *san, "-I", str(ROOT / "include"), "-I", str(ROOT / "loco_hd_amd" / "csrc"),
                           str(shim), str(client), "-o", str(exe), "-lm"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    assert "cabi weight gradient ok" in out.stdout and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    plain = _tables(out.stdout)
    assert all(t.shape == (len(X), len(TABLES[name])) for name, t in plain.items())
