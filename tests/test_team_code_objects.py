"""What the team sweeps (k_sweep_duo, loco_hd_amd/csrc/lchd_sweep_team.hip) are compiled for, read from the code objects inside the built
libloco_hd_hip.so -- registers, scratch and LDS decide how many wavefronts a SIMD holds, and several instantiations stand at their limit
(the 28-slot forms use all 168 registers of three waves per SIMD without scratch; the batch prologue recomputes the lane number through an
empty `asm` for that reason).  A compiler that allocates differently must show here, not as a slower benchmark.

The library's .hip_fatbin section is a sequence of clang offload bundles (one per translation unit); every gfx950 entry is an ELF whose
notes carry the kernels' metadata (llvm-readelf --notes).  No GPU is needed."""
import os
import re
import struct
import subprocess
from pathlib import Path

import pytest

from loco_hd_amd import _native as N

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
LLVM_BIN = Path(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")).resolve().parent.parent / "llvm" / "bin"
LDS_PER_CU = 163_840
# instantiations that had scratch before the batches came (16 slots with category weights, 32 slots): the bytes they used then
SCRATCH_BEFORE = {(16, True): 100, (32, False): 76}


def code_objects(tmp_path):
    fat = tmp_path / "fat.bin"
    subprocess.run([str(LLVM_BIN / "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", str(N.LIB_PATH), str(tmp_path / "copy.so")], check=True)
    blob = fat.read_bytes()
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), blob)]
    assert starts, "no offload bundle in the library"
    for s in starts:
        (n,) = struct.unpack_from("<Q", blob, s + len(MAGIC))
        at = s + len(MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", blob, at)
            triple = blob[at + 24:at + 24 + tlen].decode()
            at += 24 + tlen
            if "gfx950" in triple and size:
                yield blob[s + off:s + off + size]


def team_kernels(tmp_path):
    """{(CMAX, TL, TILE, WGT, KSM, PRE): metadata dict} of every k_sweep_duo in the library"""
    out = {}
    for k, co in enumerate(code_objects(tmp_path)):
        f = tmp_path / f"co{k}.elf"
        f.write_bytes(co)
        notes = subprocess.run([str(LLVM_BIN / "llvm-readelf"), "--notes", str(f)], check=True, capture_output=True, text=True).stdout
        for entry in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
            name = re.search(r"\.name:\s+(\S+)", entry).group(1)
            m = re.match(r"_ZN4lchd11k_sweep_duoILi(\d+)ELi(\d+)ELi(\d+)ELb([01])ELb([01])ELb([01])EEE", name)
            if m:
                key = (int(m[1]), int(m[2]), int(m[3]), m[4] == "1", m[5] == "1", m[6] == "1")
                out[key] = {f: int(re.search(rf"\.{f}:\s+(\d+)", entry).group(1))
                            for f in ("vgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")}
    return out


def test_team_kernels_keep_their_occupancy(tmp_path):
    kernels = team_kernels(tmp_path)
    assert len(kernels) >= 38 and (12, 32, 480, False, False, True) in kernels and (28, 32, 480, False, False, False) in kernels, sorted(kernels)
    bad = []
    for key, md in sorted(kernels.items()):
        cmax, _, _, wgt, _, _ = key
        waves = 4 if (cmax <= 16 and not (wgt and cmax > 8)) else 3  # (__launch_bounds__ of k_sweep_duo)
        regs = 512 // waves // 8 * 8
        scratch = SCRATCH_BEFORE.get((cmax, wgt), 0)
        print(key, md, f"compiled for {waves} waves per SIMD")
        if md["vgpr_count"] > regs or md["private_segment_fixed_size"] > scratch or md["group_segment_fixed_size"] * waves > LDS_PER_CU:
            bad.append((key, md))
    assert not bad, bad
