"""Dense ensemble call against the per-pair loop it replaces (python_codes/ensembles/compare_ensembles.py:277-296 of the
reference): M = 32 structures of one topology, 10 categories, uniform [3, 10], Hellinger-2.  For each n it times
  (a) the from_coords loop over all M (M - 1) / 2 = 496 pairs i < j,
  (b) one from_coords_ensemble call,
with host clocks around calls that return only after their device work has finished (both entry points copy the scores back),
after one warm-up of each.  (a) and (b) must agree within 1e-12.  One JSON line per size on stdout (and in --out).

    python profiles/ensemble_calls.py [--sizes 500,1000,3000,10000] [--out FILE]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))  # repository root


def ensemble(rng, m, n, n_cat):
    side = (n / 0.05) ** (1 / 3)
    base = rng.uniform(0.0, side, (n, 3))
    seq = [f"c{k}" for k in rng.integers(0, n_cat, n)]
    return seq, np.stack([base + rng.normal(0.0, 1.0, (n, 3)) for _ in range(m)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="500,1000,3000,10000")
    ap.add_argument("--structures", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3, help="timed repetitions of (b); (a) is timed once")
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-loop", action="store_true", help="time (b) only (for a kernel trace of the ensemble call)")
    args = ap.parse_args()
    import loco_hd_amd as lh

    m, n_cat = args.structures, 10
    lchd = lh.LoCoHD([f"c{k}" for k in range(n_cat)], lh.WeightFunction("uniform", [3.0, 10.0]))
    pairs = [(i, j) for i in range(m) for j in range(i + 1, m)]
    lines = []
    for n in [int(s) for s in args.sizes.split(",")]:
        rng = np.random.default_rng(n)
        seq, xs = ensemble(rng, m, n, n_cat)
        lchd.from_coords(seq, seq, xs[0], xs[1])  # warm-up: code objects, workspace, staging block
        lchd.from_coords_ensemble(seq, xs[:3])
        loop, t_loop = None, float("nan")
        if not args.skip_loop:
            t0 = time.perf_counter()
            loop = np.stack([np.asarray(lchd.from_coords(seq, seq, xs[i], xs[j])) for i, j in pairs])
            t_loop = time.perf_counter() - t0
        fused = lchd.from_coords_ensemble(seq, xs)  # warm-up at this size
        times = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fused = lchd.from_coords_ensemble(seq, xs)
            times.append(time.perf_counter() - t0)
        diff = float(np.max(np.abs(loop - fused))) if loop is not None else None
        assert diff is None or diff < 1e-12, (n, diff)
        t_ens = min(times)
        line = {"n": n, "structures": m, "pairs": len(pairs), "rows": len(pairs) * n, "loop_s": round(t_loop, 4),
                "ensemble_s": round(t_ens, 4), "ensemble_s_all": [round(t, 4) for t in times], "speedup": None if loop is None else round(t_loop / t_ens, 2),
                "max_abs_diff": diff, "mean_score": float(fused.mean())}
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
