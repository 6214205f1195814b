"""The cost of a weight-gradient call against the sensitivity call and the scoring call on the same pairs (DESIGN section 5,
"Weight-function gradients").

Workload: the benchmark's default cloud (bench.make_workload("c2a"): two 10^4-atom clouds, 10 categories, threshold 10 A), the first 10^5
pairs of its list, default mode; and the dense rows of the first 2 048 atoms of both clouds.  Per variant 5 warm-up calls, then 30 timed
calls; the figures are the entries of DeviceSession.last_ms() (event timing on the context's stream; "sweep": pair records + list build +
k_sensitivity / k_weight_gradient, or the sweep kernels of a scoring call) and their sum.  The sensitivity call runs at the row width
its first call reports.  Usage: python profiles/r23/weight_gradient_cost.py OUT.json"""
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

import bench  # noqa: E402
import loco_hd_amd as lh  # noqa: E402
from loco_hd_amd.device import DeviceSession  # noqa: E402

WARMUP, CALLS, PAIRS, DENSE = 5, 30, 100_000, 2048
CASES = (("hellinger 2, uniform [3, 10]", ("Hellinger", [2.0]), ("uniform", [3.0, 10.0])),
         ("hellinger 2, hyper_exp (4 parameters)", ("Hellinger", [2.0]), ("hyper_exp", [1.0, 0.5, 0.2, 0.05])),
         ("hellinger 2, kumaraswamy", ("Hellinger", [2.0]), ("kumaraswamy", [2.0, 11.0, 2.0, 3.0])),
         ("kl 1e-3, uniform [3, 10]", ("Kullback-Leibler", [1e-3]), ("uniform", [3.0, 10.0])))


def timed(sess, call, rows, key):
    for _ in range(WARMUP):
        call()
    ms = {}
    for _ in range(CALLS):
        call()
        t = dict(sess.last_ms())
        t["total"] = float(sum(v for v in t.values() if isinstance(v, (int, float))))
        for ph, v in t.items():
            if isinstance(v, (int, float)):
                ms.setdefault(ph, []).append(float(v))
    rows[key] = {ph: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v))) for ph, v in ms.items()}
    print(key, {ph: f"{np.median(v):.4f} [{min(v):.4f}, {max(v):.4f}]" for ph, v in ms.items() if ph in ("sweep", "env", "total")}, flush=True)


def main(out_path):
    w = bench.make_workload("c2a", 0, PAIRS)
    cats = [f"c{k}" for k in range(w["C"])]
    rows = {}
    for label, sd, wf in CASES:
        sess = DeviceSession(lh.LoCoHD(cats, lh.WeightFunction(*wf), statistical_distance=lh.StatisticalDistance(*sd)))
        try:
            torch = sess.torch
            sess.enable_timing(True)
            a, b = sess.upload(w["xyz_a"], w["cat_a"]), sess.upload(w["xyz_b"], w["cat_b"])
            anc = torch.from_numpy(w["pairs"][:PAIRS]).cuda()
            width = int(sess.sensitivity(a, b, anc, w["thr"]).idx_a.shape[1])
            out = torch.empty(PAIRS * (1 + len(wf[1])), dtype=torch.float64, device="cuda")
            timed(sess, lambda: sess.from_primitives(a, b, anc, w["thr"]), rows, f"score, {label}")
            timed(sess, lambda: sess.sensitivity(a, b, anc, w["thr"], width=width), rows, f"sensitivity (width {width}), {label}")
            timed(sess, lambda: sess.weight_gradient(a, b, anc, w["thr"], out=out), rows, f"weight_gradient, {label}")
            da, db = sess.upload(w["xyz_a"][:DENSE], w["cat_a"][:DENSE]), sess.upload(w["xyz_b"][:DENSE], w["cat_b"][:DENSE])
            timed(sess, lambda: sess.sensitivity_coords(da, db), rows, f"sensitivity_coords {DENSE}, {label}")
            timed(sess, lambda: sess.weight_gradient_coords(da, db), rows, f"weight_gradient_coords {DENSE}, {label}")
        finally:
            sess.close()
    Path(out_path).write_text(json.dumps(dict(pairs=PAIRS, dense=DENSE, warmup=WARMUP, calls=CALLS, categories=w["C"], ms=rows), indent=1))


if __name__ == "__main__":
    main(sys.argv[1])
