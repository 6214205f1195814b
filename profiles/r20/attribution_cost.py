"""The cost of an attribution call against the scoring call and the radial call on the same pairs ("Score attribution").

Workload: the benchmark's default cloud (bench.make_workload("c2a"): two 10^4-atom clouds, 10 categories, threshold 10 A) under
uniform[3, 10], the first 10^5 pairs of its list.  Per variant 5 warm-up calls, then 30 timed calls; the figures are the "sweep" entry of
DeviceSession.last_ms() (event timing on the context's stream: pair records + sweep kernels / radial kernel / attribution kernel) and
the "env" entry next to it.  Exponent 2 (the default distance) and exponent 3.5 (the general-exponent kernel) in deterministic and in
default mode.  Usage: python profiles/r20/attribution_cost.py OUT.json"""
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
EDGES8 = list(np.linspace(0.0, 10.0, 8)) + [float("inf")]


def main(out_path):
    w = bench.make_workload("c2a", 0, PAIRS)
    cats = [f"c{k}" for k in range(w["C"])]
    rows = {}
    for e in (2.0, 3.5):
        for det in (True, False):
            sess = DeviceSession(lh.LoCoHD(cats, lh.WeightFunction("uniform", [3.0, 10.0]), statistical_distance=lh.StatisticalDistance("Hellinger", [e]),
                                           deterministic=det))
            try:
                torch = sess.torch
                sess.enable_timing(True)
                a, b = sess.upload(w["xyz_a"], w["cat_a"]), sess.upload(w["xyz_b"], w["cat_b"])
                anc = torch.from_numpy(w["pairs"][:PAIRS]).cuda()
                variants = {
                    "score": lambda: sess.from_primitives(a, b, anc, w["thr"]),
                    "radial K=8": lambda: sess.radial(a, b, anc, w["thr"], EDGES8),
                    "attribution": lambda: sess.attribution(a, b, anc, w["thr"]),
                }
                for name, call in variants.items():
                    for _ in range(WARMUP):
                        call()
                    ms = {"sweep": [], "env": []}
                    for _ in range(CALLS):
                        call()
                        t = sess.last_ms()
                        for ph in ms:
                            ms[ph].append(t[ph])
                    key = f"{name}, exponent={e}, deterministic={det}"
                    rows[key] = {ph: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v))) for ph, v in ms.items()}
                    print(key, {ph: f"{np.median(v):.4f} [{min(v):.4f}, {max(v):.4f}]" for ph, v in ms.items()}, flush=True)
                score = sess.from_primitives(a, b, anc, w["thr"]).cpu().numpy()
                gap = float(np.max(np.abs(sess.attribution(a, b, anc, w["thr"]).cpu().numpy().sum(1) - score)))
                rows[f"max |row sum - score|, exponent={e}, deterministic={det}"] = gap
                print(f"max |row sum - score| = {gap:.3g}", flush=True)
            finally:
                sess.close()
    Path(out_path).write_text(json.dumps(dict(pairs=PAIRS, warmup=WARMUP, calls=CALLS, categories=w["C"], ms=rows), indent=1))


if __name__ == "__main__":
    main(sys.argv[1])
