"""Host-side checks of the anchor de-duplication record (lchd_ctx_last_anchors); the device side is tests/test_gpu_anchor_dedup.py."""
import ctypes as C
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_last_anchors_is_exported_with_the_declared_signature():
    from loco_hd_amd import _native

    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "loco_hd_hip.h").read_text(), flags=re.S)
    decl = re.search(r"int\s+lchd_ctx_last_anchors\s*\(([^)]*)\)\s*;", header)
    assert decl is not None
    params = [re.sub(r"\s+", " ", p.strip()) for p in decl.group(1).split(",")]
    assert params == ["lchd_ctx *ctx", "int32_t side", "int64_t *n_unique_out", "int32_t *mode_out", "int64_t *n_repeated_out"]
    res, args = _native._PROTOS["lchd_ctx_last_anchors"]
    assert res is C.c_int and args == [C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    assert hasattr(C.CDLL(str(_native.LIB_PATH)), "lchd_ctx_last_anchors")


def test_no_record_before_the_first_call():
    """A handle that has not scored anything (here: no context at all -- one cannot be created without a device) has no record; the
    outputs are left alone."""
    from loco_hd_amd import _native
    from loco_hd_amd.device import last_anchors_of

    assert last_anchors_of(None) is None
    n_unique, mode, n_repeated = C.c_int64(-7), C.c_int32(-7), C.c_int64(-7)
    for side in (0, 1, 2, -1):
        assert _native.lib().lchd_ctx_last_anchors(None, side, C.byref(n_unique), C.byref(mode), C.byref(n_repeated)) == -1
    assert (n_unique.value, mode.value, n_repeated.value) == (-7, -7, -7)


def test_the_mode_boundaries_are_the_ones_the_device_tests_sit_on():
    """tests/test_gpu_anchor_dedup.py places its anchors by these literals; a changed constant fails here, by name, instead of moving a seam
    away from its case."""
    text = (ROOT / "loco_hd_amd" / "csrc" / "lchd_prologue.hip").read_text()

    def constant(name):
        m = re.search(r"constexpr\s+(?:int64_t|int)\s+(?:\w+\s*=\s*[^,;]+,\s*)*" + name + r"\s*=\s*([^,;]+)[,;]", text)
        assert m is not None, name
        expr = re.sub(r"\(int64_t\)", "", m.group(1))
        assert re.fullmatch(r"[\d\s<()+\-*/]+", expr), expr
        return eval(expr)

    assert constant("kFusedPairsMax") == 65536        # fused: at most 65 536 pairs
    assert constant("kStructCellsMax") == 4096        # fused: at most 4096 cells per structure
    assert constant("kPrepScanAtoms") == 262144       # one-workgroup scan: at most 2^18 atoms per side; k_prep_scatter: chunk = i >> 18
    assert constant("kDupSampleAbove") == 131072      # per pair: every pair counted up to 2^17 pairs
    assert "cs.n_struct >= 8 || cs.struct_size <= 4096" in text  # fused: a single structure of at most 4096 atoms (fits_struct_path)
    assert "stage[4096]" in text and "c0 += 4096" in text        # scan_wg_1024: 4096 words = 131 072 atoms per step
    assert "P.chunk_base[i >> 18]" in text
