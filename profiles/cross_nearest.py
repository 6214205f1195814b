"""DeviceSession.nearest against the path it replaces, on the C2a clouds of BASELINE.json (bench.make_workload("c2a")): the first n atoms
of side A against the first n atoms of side B, k = 8, for every n of --sizes.

  nearest        one DeviceSession.nearest call (pairs generated and rows reduced on the device; 2 n k numbers come back on request)
  pairs_on_dev   the explicit [n^2][2] pair list already on the device, DeviceSession.from_primitives, download of the n^2 scores,
                 np.argpartition + a sort of the k kept per row
  pairs_on_host  the same with the pair list built by numpy and uploaded inside the timed region (what a caller starts from)

One process, warm-up calls first, the median of the timed calls; the selected sets of the two paths are compared.  --new-only runs the
nearest calls alone (for a kernel trace of their own).  Prints one JSON line."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))  # repository root
import bench
import loco_hd_amd as lh
from loco_hd_amd.device import DeviceSession

K = 8


def median_ms(fn, warm, reps):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts) * 1e3), float(np.min(ts) * 1e3), float(np.max(ts) * 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2000,10000")
    ap.add_argument("--new-only", action="store_true")
    args = ap.parse_args()
    w = bench.make_workload("c2a", 0, 10_000)
    lchd = lh.LoCoHD([f"c{i}" for i in range(w["C"])], lh.WeightFunction(*w["wf"]))
    sess = DeviceSession(lchd)
    sess.enable_timing(True)
    a, b = sess.upload(w["xyz_a"], w["cat_a"]), sess.upload(w["xyz_b"], w["cat_b"])
    res = {"k": K, "workload": w["label"].split(",")[0]}
    for n in (int(s) for s in args.sizes.split(",")):
        warm, reps = (3, 9) if n <= 3000 else (1, 3)
        idx = torch.arange(n, dtype=torch.int64, device="cuda")
        keep = {}

        def new():
            keep["new"] = sess.nearest(a, b, idx, idx, w["thr"], K)

        r = {"nearest_ms": median_ms(new, warm, reps), "nearest_last_tile_phase_ms": sess.last_ms(), "passes_per_call": 0}
        p0 = sess.pass_counts()["passes"]
        new()
        r["passes_per_call"] = sess.pass_counts()["passes"] - p0
        if not args.new_only:
            def host_list():
                i = np.arange(n, dtype=np.int64)
                return np.ascontiguousarray(np.stack([np.repeat(i, n), np.tile(i, n)], 1))

            def old(pairs_dev):
                scores = sess.from_primitives(a, b, pairs_dev, w["thr"]).cpu().numpy().reshape(n, n)
                part = np.argpartition(scores, K - 1, axis=1)[:, :K]
                order = np.argsort(np.take_along_axis(scores, part, 1), axis=1, kind="stable")
                keep["old"] = np.take_along_axis(part, order, 1)

            pairs_dev = torch.from_numpy(host_list()).cuda()
            r["pairs_on_dev_ms"] = median_ms(lambda: old(pairs_dev), warm, reps)
            r["pairs_on_dev_phase_ms"] = sess.last_ms()
            del pairs_dev
            r["pairs_on_host_ms"] = median_ms(lambda: old(torch.from_numpy(host_list()).cuda()), warm, reps)
            got = np.sort(keep["new"].cols.cpu().numpy(), axis=1)
            r["rows_with_the_same_set"] = int((got == np.sort(keep["old"], axis=1)).all(axis=1).sum())
        res[str(n)] = r
    sess.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
