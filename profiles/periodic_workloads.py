#!/usr/bin/env python3
"""Periodic-boundary measurements quoted in DESIGN.md section 5 (run on the MI355X box from the repository root):
    python3 profiles/periodic_workloads.py > periodic_workloads.json
C2a cloud in its box (10^4 atoms, L = 58.5, threshold 10): image-build time, ghost count, pass time with and without the box; the
image build again through the triclinic kernels, with diag(L) and with the rhombic dodecahedron of the box's volume.
C4-shaped trajectory (2001 primitive atoms per frame, chunks of 500 frames): image rebuild per chunk against the chunk's pass.
"""
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import bench  # noqa: E402
import loco_hd_amd as lh  # noqa: E402
from loco_hd_amd import _native as N  # noqa: E402
from loco_hd_amd.device import DeviceSession  # noqa: E402

res = {}


def timed(fn, reps=5, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


# ---- C2a in its box ---------------------------------------------------------------------------------------------------------
w = bench.make_workload("c2a", 0, 1_000_000)
L = 58.5
lchd = lh.LoCoHD([f"c{i}" for i in range(w["C"])], lh.WeightFunction(*w["wf"]))
sess = DeviceSession(lchd)
sess.enable_timing(True)
a, b = sess.upload(w["xyz_a"], w["cat_a"]), sess.upload(w["xyz_b"], w["cat_b"])
anchors = torch.from_numpy(w["pairs"]).cuda()
out = torch.empty(len(w["pairs"]), dtype=torch.float64, device="cuda")
ia, ib = sess.periodic_images(a, (L, L, L), w["thr"]), sess.periodic_images(b, (L, L, L), w["thr"])
build_ms = timed(lambda: sess.update_images(ia, a, (L, L, L)), reps=20, warm=3)
open_ms = timed(lambda: sess.from_primitives(a, b, anchors, w["thr"], out=out))
open_phases, open_points = sess.last_ms(), sess.last_env_points()
box_ms = timed(lambda: sess.from_primitives(ia, ib, anchors, w["thr"], out=out))
n_img = int(N.lib().lchd_cloud_size(ia))
res["c2a_in_its_box"] = {"atoms": w["n"], "atoms_and_ghosts": n_img, "ghosts_per_atom": n_img / w["n"] - 1.0,
                         "geometric_expectation": ((L + 2 * w["thr"]) / L) ** 3 - 1.0, "image_build_ms_host_call": build_ms,
                         "pass_ms_open": open_ms, "pass_ms_in_the_box": box_ms, "kernel_ms_open": open_phases,
                         "kernel_ms_in_the_box": sess.last_ms(), "env_points_open": open_points, "env_points_in_the_box": sess.last_env_points()}


# the same cloud through the cell path (k_img_count_cell / k_img_emit_cell)
def cell_widths(cell):
    det = abs(np.linalg.det(cell))
    return [det / np.linalg.norm(np.cross(cell[(k + 1) % 3], cell[(k + 2) % 3])) for k in range(3)]


d = L * 2.0 ** (1.0 / 6.0)  # image distance of the rhombic dodecahedron of volume L^3 (d^3 sqrt(2) / 2)
for name, cell in (("diag", np.diag([L, L, L])), ("dodecahedron", np.array([[d, 0.0, 0.0], [0.0, d, 0.0], [d / 2, d / 2, d * np.sqrt(2.0) / 2]]))):
    ic = sess.periodic_images(a, reach=w["thr"], cell=cell)
    ms = timed(lambda: sess.update_images(ic, a, cell=cell), reps=20, warm=3)
    n_ic = int(N.lib().lchd_cloud_size(ic))
    res["c2a_in_its_box"]["cell_" + name] = {"widths": cell_widths(cell), "volume": abs(float(np.linalg.det(cell))), "atoms_and_ghosts": n_ic,
                                             "ghosts_per_atom": n_ic / w["n"] - 1.0, "image_build_ms_host_call": ms,
                                             "geometric_expectation": float(np.prod([1.0 + 2.0 * w["thr"] / wk for wk in cell_widths(cell)])) - 1.0}
# atoms uniform in the dodecahedron itself (the C2a cloud is uniform in the cube, which is no fundamental domain of that lattice)
uni = sess.upload(np.random.default_rng(5).uniform(0.0, 1.0, (w["n"], 3)) @ cell, w["cat_a"])
n_uni = int(N.lib().lchd_cloud_size(sess.periodic_images(uni, reach=w["thr"], cell=cell)))
res["c2a_in_its_box"]["cell_dodecahedron"]["ghosts_per_atom_of_a_cloud_uniform_in_the_cell"] = n_uni / w["n"] - 1.0
res["c2a_in_its_box"]["image_build_ms_host_call_box_again"] = timed(lambda: sess.update_images(ia, a, (L, L, L)), reps=20, warm=3)
sess.close()

# ---- a C4-shaped trajectory: one reference against frames of 2001 primitive atoms, every third atom an anchor ----------------
rng = np.random.default_rng(4)
n, n_frames, chunk, thr = 2001, 1000, 500, 10.0
side = (n / 0.023) ** (1 / 3)
ref = rng.uniform(0, side, (n, 3))
frames = (ref[None] + rng.normal(0, 1.0, (n_frames, n, 3))) % side
cat = rng.integers(0, 8, n).astype(np.int32)
tag = (np.arange(n) // 3).astype(np.int32)
lp = np.stack([np.arange(0, n, 3), np.arange(0, n, 3)], 1)
lchd = lh.LoCoHD([f"c{i}" for i in range(8)], lh.WeightFunction("uniform", [3.0, 10.0]), lh.TagPairingRule({"accept_same": False}))
sess = DeviceSession(lchd)
sess.enable_timing(True)
rc = sess.upload(ref, cat, tag)
buf = sess.frames_buffer(rc, chunk)
sess.load_frames(buf, frames[:chunk])
an = torch.from_numpy(np.concatenate([lp + np.asarray([0, f * n]) for f in range(chunk)])).cuda()
o = torch.empty(len(an), dtype=torch.float64, device="cuda")
ri = sess.periodic_images(rc, (side,) * 3, thr)
img = sess.periodic_images(buf, (side,) * 3, thr)
rebuild_ms = timed(lambda: sess.update_images(img, buf, (side,) * 3), reps=20, warm=3)
pass_open = timed(lambda: sess.from_primitives(rc, buf, an, thr, out=o))
pass_box = timed(lambda: sess.from_primitives(ri, img, an, thr, out=o))
t_open = timed(lambda: sess.score_trajectory(rc, frames, lp, thr, chunk=chunk), reps=3, warm=1)
t_box = timed(lambda: sess.score_trajectory(rc, frames, lp, thr, chunk=chunk, ref_box=(side,) * 3, boxes=(side,) * 3), reps=3, warm=1)
res["c4_shaped_trajectory"] = {"atoms_per_frame": n, "frames": n_frames, "chunk": chunk, "box": side, "pairs_per_chunk": len(an),
                               "chunk_atoms_and_ghosts": int(N.lib().lchd_cloud_size(img)), "image_rebuild_ms_per_chunk": rebuild_ms,
                               "pass_ms_per_chunk_open": pass_open, "pass_ms_per_chunk_in_the_box": pass_box,
                               "score_trajectory_ms_open": t_open, "score_trajectory_ms_in_the_box": t_box}
sess.close()
print(json.dumps(res, indent=1))
