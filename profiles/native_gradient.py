"""DeviceSession.native_gradient / native_gradient_coords against DeviceSession.gradient / gradient_coords (the torch assembly of the
sensitivity lists), on the workloads of DESIGN.md section 5:

  thr:N:P     the first N atoms of the two C2a clouds (bench.make_workload("c2a")), its first P anchor pairs taken modulo N
  dense:N     the dense rows of the first N atoms of both clouds

Caller-supplied outputs for the native call, 3 warm-up calls, the median of 20 timed calls (host wall time around calls that return
complete; min - max in brackets in DESIGN.md).  Device memory: (total - free) of hipMemGetInfo after each path's timed calls -- the
library's grow-only blocks and torch's cached peak both stay allocated, so the growth over the state before is the path's footprint;
the native path runs first.  --native-only: the native calls alone (for a kernel trace of their own).  Prints one JSON line."""
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


def median_ms(fn, warm=3, reps=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return [float(np.median(ts) * 1e3), float(np.min(ts) * 1e3), float(np.max(ts) * 1e3)]


def used_mb():
    free, total = torch.cuda.mem_get_info()
    return (total - free) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="thr:3000:3000,thr:10000:100000,dense:500,dense:2000")
    ap.add_argument("--native-only", action="store_true")
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    w = bench.make_workload("c2a", 0, 1_000_000)
    lchd = lh.LoCoHD([f"c{i}" for i in range(w["C"])], lh.WeightFunction(*w["wf"]))
    res = {}
    for case in args.cases.split(","):
        kind, *nums = case.split(":")
        n = int(nums[0])
        sess = DeviceSession(lchd)
        a, b = sess.upload(w["xyz_a"][:n], w["cat_a"][:n]), sess.upload(w["xyz_b"][:n], w["cat_b"][:n])
        xa, xb = torch.from_numpy(np.ascontiguousarray(w["xyz_a"][:n])).cuda(), torch.from_numpy(np.ascontiguousarray(w["xyz_b"][:n])).cuda()
        p = int(nums[1]) if kind == "thr" else n
        v = torch.rand(p, dtype=torch.float64, device="cuda") + 0.5
        out = (torch.empty(p, dtype=torch.float64, device="cuda"), torch.empty((n, 3), dtype=torch.float64, device="cuda"),
               torch.empty((n, 3), dtype=torch.float64, device="cuda"))
        if kind == "thr":
            anc = torch.from_numpy(np.ascontiguousarray(w["pairs"][:p] % n)).cuda()
            native = lambda: sess.native_gradient(a, b, anc, w["thr"], pair_weights=v, out=out)  # noqa: E731
            old = lambda: sess.gradient(a, b, anc, w["thr"], xa, xb, pair_weights=v)  # noqa: E731
        else:
            native = lambda: sess.native_gradient_coords(a, b, pair_weights=v, out=out)  # noqa: E731
            old = lambda: sess.gradient_coords(a, b, xa, xb, pair_weights=v)  # noqa: E731
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = used_mb()
        r = {"pairs": p, "native_ms": median_ms(native, reps=args.reps), "native_mb": used_mb() - base}
        if not args.native_only:
            mid = used_mb()
            try:
                r["torch_ms"] = median_ms(old, reps=args.reps)
                r["torch_mb"] = used_mb() - mid
                got = old()
                r["max_abs_native_minus_torch"] = float(max((out[1] - got[1]).abs().max(), (out[2] - got[2]).abs().max()))
                r["width"] = int(sess.sensitivity(a, b, anc, w["thr"]).idx_a.shape[1]) if kind == "thr" else n
            except (RuntimeError, NotImplementedError) as e:  # (out of memory in the torch assembly)
                r["torch_error"] = str(e)[:200]
        res[case] = r
        sess.close()
        del out, v, xa, xb
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
