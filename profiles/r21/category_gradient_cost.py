"""The cost of a category-gradient call against the attribution call and the scoring call on the same pairs (DESIGN section 5,
"Category-weight gradients").

Workload: the benchmark's default cloud (bench.make_workload("c2a"): two 10^4-atom clouds, 10 categories, threshold 10 A) under
uniform[3, 10], the first 10^5 pairs of its list, default mode.  Per variant 5 warm-up calls, then 30 timed calls; the figures are the
"sweep" entry of DeviceSession.last_ms() (event timing on the context's stream: pair records + sweep kernels / attribution kernel /
category-gradient kernel) and the "env" entry next to it.  Hellinger 2 with unit and with drawn weights, Hellinger 3.5 and
Kullback-Leibler 1e-3 (no attribution there).  Usage: python profiles/r21/category_gradient_cost.py OUT.json"""
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

import bench  # noqa: E402
import loco_hd_amd as lh  # noqa: E402
from loco_hd_amd.device import DeviceSession  # noqa: E402

WARMUP, CALLS, PAIRS = 5, 30, 100_000


def main(out_path):
    w = bench.make_workload("c2a", 0, PAIRS)
    cats = [f"c{k}" for k in range(w["C"])]
    drawn = list(np.random.default_rng(3).uniform(0.3, 3.0, w["C"]))
    rows = {}
    for label, sd, weights in (("hellinger 2, unit weights", ("Hellinger", [2.0]), None), ("hellinger 2, drawn weights", ("Hellinger", [2.0]), drawn),
                               ("hellinger 3.5, drawn weights", ("Hellinger", [3.5]), drawn), ("kl 1e-3, drawn weights", ("Kullback-Leibler", [1e-3]), drawn)):
        sess = DeviceSession(lh.LoCoHD(cats, lh.WeightFunction("uniform", [3.0, 10.0]), category_weights=weights,
                                       statistical_distance=lh.StatisticalDistance(*sd)))
        try:
            torch = sess.torch
            sess.enable_timing(True)
            a, b = sess.upload(w["xyz_a"], w["cat_a"]), sess.upload(w["xyz_b"], w["cat_b"])
            anc = torch.from_numpy(w["pairs"][:PAIRS]).cuda()
            variants = {"score": lambda: sess.from_primitives(a, b, anc, w["thr"]),
                        "category_gradient": lambda: sess.category_gradient(a, b, anc, w["thr"])}
            if sd[0] == "Hellinger":
                variants["attribution"] = lambda: sess.attribution(a, b, anc, w["thr"])
            for name, call in variants.items():
                for _ in range(WARMUP):
                    call()
                ms = {"sweep": [], "env": []}
                for _ in range(CALLS):
                    call()
                    t = sess.last_ms()
                    for ph in ms:
                        ms[ph].append(t[ph])
                key = f"{name}, {label}"
                rows[key] = {ph: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v))) for ph, v in ms.items()}
                print(key, {ph: f"{np.median(v):.4f} [{min(v):.4f}, {max(v):.4f}]" for ph, v in ms.items()}, flush=True)
            g = sess.category_gradient(a, b, anc, w["thr"]).cpu().numpy()
            euler = float(np.max(np.abs((g * (1.0 if weights is None else np.asarray(weights))).sum(1))))
            rows[f"max |sum_c w_c G_c|, {label}"] = euler
            print(f"max |sum_c w_c G_c| = {euler:.3g}", flush=True)
        finally:
            sess.close()
    Path(out_path).write_text(json.dumps(dict(pairs=PAIRS, warmup=WARMUP, calls=CALLS, categories=w["C"], ms=rows), indent=1))


if __name__ == "__main__":
    main(sys.argv[1])
