"""The "sweep" phase of a radial call against the scoring sweep it stands in for ("Radial profiles").

Workload: the benchmark's default cloud (bench.make_workload("c2a"): two 10^4-atom clouds, 10 categories, threshold 10 A) under
uniform[3, 10], the first 10^5 pairs of its list.  Per variant 5 warm-up calls, then 30 timed calls; the figure is the "sweep" entry of
DeviceSession.last_ms() (event timing on the context's stream: pair records + sweep kernels, or pair records + radial kernel), the
"env" entry next to it.  Yardstick: from_primitives in deterministic mode.  Usage: python profiles/r18/radial_sweep.py OUT.json"""
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


def edges(k):
    return [0.0, float("inf")] if k == 1 else list(np.linspace(0.0, 10.0, k)) + [float("inf")]


def main(out_path):
    w = bench.make_workload("c2a", 0, PAIRS)
    cats = [f"c{k}" for k in range(w["C"])]
    rows = {}
    for det in (True, False):
        sess = DeviceSession(lh.LoCoHD(cats, lh.WeightFunction("uniform", [3.0, 10.0]), deterministic=det))
        try:
            torch = sess.torch
            sess.enable_timing(True)
            a, b = sess.upload(w["xyz_a"], w["cat_a"]), sess.upload(w["xyz_b"], w["cat_b"])
            anc = torch.from_numpy(w["pairs"][:PAIRS]).cuda()
            variants = {"score": lambda: sess.from_primitives(a, b, anc, w["thr"])}
            for k in (1, 8, 64):
                variants[f"radial K={k}"] = (lambda e: lambda: sess.radial(a, b, anc, w["thr"], e))(edges(k))
            for name, call in variants.items():
                for _ in range(WARMUP):
                    call()
                ms = {"sweep": [], "env": []}
                for _ in range(CALLS):
                    call()
                    t = sess.last_ms()
                    for ph in ms:
                        ms[ph].append(t[ph])
                rows[f"{name}, deterministic={det}"] = {ph: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v))) for ph, v in ms.items()}
                print(name, f"deterministic={det}", {ph: f"{np.median(v):.4f} [{min(v):.4f}, {max(v):.4f}]" for ph, v in ms.items()}, flush=True)
        finally:
            sess.close()
    base = rows["score, deterministic=True"]["sweep"]["median"]
    ratios = {k: rows[f"radial K={k}, deterministic=True"]["sweep"]["median"] / base for k in (1, 8, 64)}
    print("radial sweep / deterministic scoring sweep:", {k: round(v, 3) for k, v in ratios.items()})
    Path(out_path).write_text(json.dumps(dict(pairs=PAIRS, warmup=WARMUP, calls=CALLS, ms=rows, ratio_to_deterministic_sweep=ratios), indent=1))


if __name__ == "__main__":
    main(sys.argv[1])
