"""The cost of a radial call and of a sensitivity call at the sizes of profiles/r20/attribution_cost.py and
profiles/r21/category_gradient_cost.py: the benchmark's default cloud (bench.make_workload("c2a"): two 10^4-atom clouds, 10 categories,
threshold 10 A) under uniform[3, 10], the first 10^5 pairs of its list, default mode.  Per variant 5 warm-up calls, then 30 timed
calls, each timed on the host between two device synchronisations (the whole call: lists, pair records and the kernel).  Radial with 8 bins under
Hellinger 2 (unit weights) and under Kolmogorov-Smirnov (the generic instantiation); sensitivities under Hellinger 2 and
Kullback-Leibler 1e-3.  Usage: python profiles/r22/radial_sensitivity_cost.py OUT.json"""
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

import bench  # noqa: E402
import loco_hd_amd as lh  # noqa: E402
from loco_hd_amd.device import DeviceSession  # noqa: E402

WARMUP, CALLS, PAIRS = 5, 30, 100_000
EDGES8 = list(np.linspace(0.0, 10.0, 8)) + [float("inf")]


def main(out_path):
    w = bench.make_workload("c2a", 0, PAIRS)
    cats = [f"c{k}" for k in range(w["C"])]
    rows = {}
    for label, sd in (("hellinger 2", ("Hellinger", [2.0])), ("ks", ("Kolmogorov-Smirnov", [])), ("kl 1e-3", ("Kullback-Leibler", [1e-3]))):
        sess = DeviceSession(lh.LoCoHD(cats, lh.WeightFunction("uniform", [3.0, 10.0]), statistical_distance=lh.StatisticalDistance(*sd)))
        try:
            torch = sess.torch
            a, b = sess.upload(w["xyz_a"], w["cat_a"]), sess.upload(w["xyz_b"], w["cat_b"])
            anc = torch.from_numpy(w["pairs"][:PAIRS]).cuda()
            variants = {}
            if label != "kl 1e-3":
                variants["radial K=8"] = lambda: sess.radial(a, b, anc, w["thr"], EDGES8)
            if label != "ks":
                variants["sensitivity"] = lambda: sess.sensitivity(a, b, anc, w["thr"])
            for name, call in variants.items():
                for _ in range(WARMUP):
                    call()
                ms = []
                for _ in range(CALLS):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    call()
                    torch.cuda.synchronize()
                    ms.append((time.perf_counter() - t0) * 1e3)
                key = f"{name}, {label}"
                rows[key] = dict(median=float(np.median(ms)), min=float(min(ms)), max=float(max(ms)))
                print(key, f"{np.median(ms):.4f} [{min(ms):.4f}, {max(ms):.4f}]", flush=True)
        finally:
            sess.close()
    Path(out_path).write_text(json.dumps(dict(pairs=PAIRS, warmup=WARMUP, calls=CALLS, categories=w["C"], ms=rows), indent=1))


if __name__ == "__main__":
    main(sys.argv[1])
