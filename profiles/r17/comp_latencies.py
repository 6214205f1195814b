"""A/B of composition-call latencies, timed like profiles/call_latencies.py: LCHD_LIB selects the library.  Prints one JSON line."""
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent.parent))  # repository root
import loco_hd_amd as lh
from loco_hd_amd.device import DeviceSession


def timed(fn, reps, warm):
    """Every call timed on its own (the calls are synchronous): mean, median and max in ms."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    ts = np.asarray(ts) * 1e3
    return {"mean_ms": float(ts.mean()), "median_ms": float(np.median(ts)), "max_ms": float(ts.max())}


types = ["Cent", "AmideC", "OH", "Pos", "Neg", "Aro", "Ali", "Sulf"]
lchd = lh.LoCoHD(types, lh.WeightFunction("uniform", [3.0, 10.0]), lh.TagPairingRule({"accept_same": False}))
nn = 1000
rs = np.random.default_rng(0)
sd = (nn / 0.023) ** (1 / 3)
xa = rs.uniform(0, sd, (nn, 3))
ct = rs.integers(0, 8, nn).astype(np.int32)
tg = (np.arange(nn) // 3).astype(np.int32)
res = {}
s1 = DeviceSession(lchd)
ha = s1.upload(xa, ct, tg)
an = torch.arange(0, nn, 3, dtype=torch.int64, device="cuda")
o1 = torch.empty((len(an), len(types)), dtype=torch.float64, device="cuda")
res["dev_composition_1000_atoms"] = timed(lambda: s1.composition(ha, an, 10.0, out=o1), reps=200, warm=20)
s1.close()
prims = [lh.PrimitiveAtom(types[c], str(t), list(map(float, p))) for p, c, t in zip(xa, ct, tg)]
anh = list(range(0, nn, 3))
res["host_ptr_composition_1000_atoms"] = timed(lambda: lchd.composition_from_primitives(prims, anh, 10.0), reps=100, warm=20)
print(json.dumps(res))
