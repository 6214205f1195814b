"""DeviceSession.category_gradient_sum / weight_gradient_sum against the per-pair call plus torch's (g * v[:, None]).sum(0), on the
workload of DESIGN.md section 5 "Reduced parameter gradients": the two C2a clouds (bench.make_workload("c2a"): 10 k atoms, 10 categories,
the default weight function) and their first P anchor pairs.

  cat:P       the category form at the workload's 10 categories
  cat64:P     the category form with the atoms' categories redrawn from 64
  wf:P        the weight form (one function)

Both paths on one session, warm: 3 warm-up calls, the median of --reps timed calls (host wall time around calls that return complete;
min and max next to it).  Device memory: (total - free) of hipMemGetInfo after each path's timed calls -- the library's grow-only blocks
and torch's cached peak both stay allocated, so the growth over the state before is the path's footprint; the reduced path runs first.
--new-only: the reduced calls alone (for a kernel trace of their own).  Prints one JSON line."""
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


def median_ms(fn, warm=3, reps=10):
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
    ap.add_argument("--cases", default="cat:1000000,wf:1000000,cat64:1000000")
    ap.add_argument("--new-only", action="store_true")
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    w = bench.make_workload("c2a", 0, 1_000_000)
    res = {}
    for case in args.cases.split(","):
        kind, p = case.split(":")
        p = int(p)
        n_cat = 64 if kind == "cat64" else w["C"]
        lchd = lh.LoCoHD([f"c{i}" for i in range(n_cat)], lh.WeightFunction(*w["wf"]))
        cat_a, cat_b = w["cat_a"], w["cat_b"]
        if kind == "cat64":
            rng = np.random.default_rng(64)
            cat_a, cat_b = rng.integers(0, 64, len(cat_a)).astype(np.int32), rng.integers(0, 64, len(cat_b)).astype(np.int32)
        sess = DeviceSession(lchd)
        a, b = sess.upload(w["xyz_a"], cat_a), sess.upload(w["xyz_b"], cat_b)
        anc = torch.from_numpy(np.ascontiguousarray(w["pairs"][:p])).cuda()
        v = torch.rand(p, dtype=torch.float64, device="cuda") - 0.5
        if kind == "wf":
            width = 1 + int(lh.api.weight_gradient_width([lchd.w_func]))
            new = lambda: sess.weight_gradient_sum(a, b, anc, w["thr"], v).grad[0]  # noqa: E731
            old = lambda: (sess.weight_gradient(a, b, anc, w["thr"]).grad * v[:, None]).sum(0)  # noqa: E731
        else:
            width = n_cat
            new = lambda: sess.category_gradient_sum(a, b, anc, w["thr"], v)  # noqa: E731
            old = lambda: (sess.category_gradient(a, b, anc, w["thr"]) * v[:, None]).sum(0)  # noqa: E731
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = used_mb()
        r = {"pairs": p, "row_doubles": width, "rows_mb": p * width * 8 / 2 ** 20, "new_ms": median_ms(new, reps=args.reps),
             "new_mb": used_mb() - base}
        if not args.new_only:
            mid = used_mb()
            r["old_ms"] = median_ms(old, reps=args.reps)
            r["old_mb"] = used_mb() - mid
            per_pair = (lambda: sess.weight_gradient(a, b, anc, w["thr"])) if kind == "wf" else (lambda: sess.category_gradient(a, b, anc, w["thr"]))
            r["per_pair_call_ms"] = median_ms(per_pair, reps=args.reps)
            got, ref = new(), old()
            r["max_abs_new_minus_old"] = float((got - ref).abs().max())
            r["max_abs_sum"] = float(ref.abs().max())
        res[case] = r
        sess.close()
        del anc, v
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
