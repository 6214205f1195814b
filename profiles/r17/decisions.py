"""Decisions and bits of a seeded call sequence, call by call: LCHD_LIB selects the library, argv[1] names the dump (JSON lines).

Run it once per library, each run a fresh process; the two dumps of a host-only change must be byte-identical
(profiles/r17/ab_store_builder.md).  Scoring and composition calls alternate on one context per configuration: the host-array
entry points of a LoCoHD instance run on the context of the DeviceSession next to it.  After every call one line holds the SHA-256 of
the output bytes (or the error), the context's pass counters, lchd_ctx_last_store_bytes, lchd_ctx_last_dense_fused and
lchd_ctx_last_grid / _last_anchors / _last_sweep in full.  Random float coordinates throughout (no tied distances but the +inf
blocks)."""
import hashlib
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent.parent))  # repository root
import loco_hd_amd as lh
from loco_hd_amd import _native as N
from loco_hd_amd.device import DeviceSession

dump = open(sys.argv[1], "w")
rng = np.random.default_rng(20261019)
dev = torch.device("cuda", 0)


class Ctx:
    """One configuration: a LoCoHD instance and a DeviceSession that share one context."""

    def __init__(self, name, n_cat, w_func=None, **kw):
        self.name, self.n_cat = name, n_cat
        self.cats = [f"c{i}" for i in range(n_cat)]
        self.lchd = lh.LoCoHD(self.cats, w_func if w_func is not None else lh.WeightFunction("uniform", [3.0, 10.0]), **kw)
        self.sess = DeviceSession(self.lchd)
        self.lchd._ctx = self.sess._ctx
        self.n_calls = 0

    def record(self, label, fn):
        """fn() -> array-like or torch tensor; an exception is part of the record."""
        rec = {"ctx": self.name, "call": self.n_calls, "label": label}
        self.n_calls += 1
        try:
            out = fn()
            out = out.cpu().numpy() if isinstance(out, torch.Tensor) else np.asarray(out, dtype=np.float64)
            rec["sha256"] = hashlib.sha256(np.ascontiguousarray(out).tobytes()).hexdigest()
            rec["shape"] = list(out.shape)
            rec["first"] = [float(v).hex() for v in out.reshape(-1)[:4]]
        except Exception as e:  # noqa: BLE001 -- the class and the message are what is compared
            rec["error"] = f"{type(e).__name__}: {e}"
            rec["last_error"] = N.lib().lchd_last_error().decode(errors="replace")
        s = self.sess
        rec.update(s.pass_counts())
        rec["dense_fused"] = s.last_dense_fused()
        rec["grid"], rec["anchors"], rec["sweep"] = s.last_grid(), s.last_anchors(), s.last_sweep()
        dump.write(json.dumps(rec, sort_keys=True) + "\n")
        dump.flush()

    def close(self):
        self.lchd._ctx = None
        self.sess.close()


def cloud(n, density=0.023, n_cat=5):
    side = (n / density) ** (1 / 3)
    return rng.uniform(0, side, (n, 3)), rng.integers(0, n_cat, n).astype(np.int32)


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev)


def t32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


def prims(ctx, xyz, cat):
    return [lh.PrimitiveAtom(ctx.cats[c], "", list(map(float, p))) for p, c in zip(xyz, cat)]


def cell_for(side):  # a triclinic cell that holds a cube of edge `side`
    return np.array([[side, 0.0, 0.0], [0.21 * side, 1.1 * side, 0.0], [0.13 * side, -0.17 * side, 1.2 * side]])


def dmx_with_inf(x, rows):
    d = np.linalg.norm(x[:rows, None, :] - x[None, :, :], axis=2)
    d[rows // 3: rows // 2, x.shape[0] // 2:] = np.inf  # (every row keeps its 0: the anchor itself lies in the first half)
    return d


def main_sequence(c, deterministic):
    """The call families on one context of 5 categories; deterministic: one call of each family only."""
    s, L = c.sess, c.lchd
    tag = "det " if deterministic else ""
    xa, ca = cloud(1500)
    xb, cb = cloud(1500)
    a, b = s.upload(xa, ca), s.upload(xb, cb)
    small = t64(np.stack([np.arange(0, 300), np.arange(0, 300)], 1))
    c.record(tag + "small call", lambda: s.from_primitives(a, b, small, 10.0))
    anc300 = t64(rng.integers(0, 1500, 300))
    c.record(tag + "composition 300 anchors / 1500 atoms", lambda: s.composition(a, anc300, 10.0))
    big_a, cat_a = cloud(6000)
    big_b, cat_b = cloud(6000)
    A, B = s.upload(big_a, cat_a), s.upload(big_b, cat_b)
    p4097 = t64(np.stack([rng.integers(0, 6000, 4097), rng.integers(0, 6000, 4097)], 1))
    for k in range(1 if deterministic else 2):
        c.record(tag + f"4097 pairs #{k}", lambda: s.from_primitives(A, B, p4097, 10.0))
    if not deterministic:
        ii = t64(np.stack([np.arange(4500), np.arange(4500)], 1))
        for k in range(3):
            c.record(f"(i, i) x 4500 #{k}", lambda: s.from_primitives(A, B, ii, 10.0))
            if k == 1:
                c.record("composition between per-pair passes", lambda: s.composition(A, t64(np.arange(0, 6000, 7)), 10.0))
        m21 = t64(np.stack([np.arange(4500), np.arange(4500) % 150], 1))
        for k in range(3):
            c.record(f"many-to-one x 4500 #{k}", lambda: s.from_primitives(A, B, m21, 10.0))
    # one 900-atom cluster of radius 3 among 8000 sparse atoms: the cluster's environments overflow the default slots
    sparse = rng.uniform(0, 120.0, (8000, 3))
    v = rng.normal(size=(900, 3))
    sparse[:900] = 60.0 + 3.0 * rng.uniform(0, 1, (900, 1)) ** (1 / 3) * v / np.linalg.norm(v, axis=1, keepdims=True)
    ccat = rng.integers(0, 5, 8000).astype(np.int32)
    K1, K2 = s.upload(sparse, ccat), s.upload(sparse + rng.normal(scale=0.05, size=sparse.shape), ccat)
    sel = np.concatenate([np.arange(0, 40), rng.choice(np.arange(900, 8000), 2000, replace=False)])
    kp = t64(np.stack([sel, sel], 1))
    for k in range(1 if deterministic else 2):
        c.record(tag + f"900-atom cluster #{k}", lambda: s.from_primitives(K1, K2, kp, 10.0))
        c.record(tag + f"composition on the cluster #{k}", lambda: s.composition(K1, t64(sel), 10.0))
    # a frames buffer as the cloud
    fr = s.frames_buffer(a, 4)
    s.load_frames(fr, np.stack([xa + rng.normal(scale=0.3, size=xa.shape) for _ in range(3)]))
    fanc = t64(rng.integers(0, 3 * 1500, 400))
    c.record(tag + "composition on a frames buffer", lambda: s.composition(fr, fanc, 10.0))
    c.record(tag + "frames against frames", lambda: s.from_primitives(fr, fr, t64(np.stack([np.arange(0, 1500), np.arange(1500, 3000)], 1)), 10.0))
    # dense calls through the host arrays
    for n, with_cell in ((65, False), (1025, False), (1025, True)) if not deterministic else ((65, False),):
        x1, c1 = cloud(n)
        x2, c2 = cloud(n)
        kw = {"cell_a": cell_for((n / 0.023) ** (1 / 3))} if with_cell else {}
        c.record(tag + f"from_coords n = {n}{' cell_a' if with_cell else ''}",
                 lambda: L.from_coords([c.cats[i] for i in c1], [c.cats[i] for i in c2], x1, x2, **kw))
    for n in (2, 65, 1025) if not deterministic else (65,):
        x1, c1 = cloud(n)
        seq = [c.cats[i] for i in c1]
        c.record(tag + f"composition_coords n = {n}", lambda: L.composition_from_coords(seq, x1))
        c.record(tag + f"composition_coords n = {n} cell", lambda: L.composition_from_coords(seq, x1, cell=cell_for((n / 0.023) ** (1 / 3))))
        if n == 65:
            d1 = s.upload(x1, c1)
            c.record(tag + "composition_coords n = 65 device", lambda: s.composition_coords(d1))
    x1, c1 = cloud(200)
    x2, c2 = cloud(200)
    seq1, seq2 = [c.cats[i] for i in c1], [c.cats[i] for i in c2]
    c.record(tag + "from_dmxs +inf block", lambda: L.from_dmxs(seq1, seq2, dmx_with_inf(x1, 120), dmx_with_inf(x2, 120)))
    c.record(tag + "composition_dmx +inf block", lambda: L.composition_from_dmx(seq1, dmx_with_inf(x1, 120)))
    # periodic from_primitives and composition through the host wrappers
    xp, cp = cloud(400)
    side = (400 / 0.023) ** (1 / 3)
    pp = prims(c, xp, cp)
    pairs = [(int(i), int(j)) for i, j in zip(rng.integers(0, 400, 250), rng.integers(0, 400, 250))]
    c.record(tag + "periodic from_primitives box", lambda: L.from_primitives(pp, pp, pairs, 8.0, box_a=[side] * 3, box_b=[side] * 3))
    if deterministic:
        return
    c.record("periodic from_primitives cell", lambda: L.from_primitives(pp, pp, pairs, 8.0, cell_a=cell_for(side)))
    c.record("periodic composition box", lambda: L.composition_from_primitives(pp, [i for i, _ in pairs], 8.0, box=[side] * 3))
    c.record("host composition", lambda: L.composition_from_primitives(pp, [i for i, _ in pairs], 8.0))
    # failing calls: the error string is part of the dump
    c.record("anchor out of range (host wrapper)", lambda: L.from_primitives(pp, pp, pairs + [(400, 0)], 8.0, box_a=[side] * 3))
    bad = pp[:200] + [lh.PrimitiveAtom("not a category", "", list(map(float, xp[200])))] + pp[201:]
    c.record("unknown category (host wrapper)", lambda: L.from_primitives(bad, pp, pairs, 8.0, box_a=[side] * 3))
    c.record("unknown category (host composition)", lambda: L.composition_from_primitives(bad, [i for i, _ in pairs], 8.0, cell=cell_for(side)))
    img = s.periodic_images(a, [(1500 / 0.023) ** (1 / 3)] * 3, 6.0)
    c.record("threshold beyond the images' reach", lambda: s.from_primitives(img, b, small, 10.0))
    c.record("composition beyond the images' reach", lambda: s.composition(img, anc300, 10.0))
    c.record("small call after the failures", lambda: s.from_primitives(a, b, small, 10.0))


c5 = Ctx("5 categories", 5)
main_sequence(c5, False)
c5.sess.set_deterministic(True)
main_sequence(c5, True)
c5.close()

# weight-function dictionaries with a per-pair / per-anchor index
for n_wf in (2, 5):
    wfs = {f"w{k}": lh.WeightFunction("uniform", [1.0 + k, 8.0 + k]) for k in range(n_wf)}
    cd = Ctx(f"dictionary of {n_wf}", 5, wfs)
    xa, ca = cloud(1500)
    xb, cb = cloud(1500)
    a, b = cd.sess.upload(xa, ca), cd.sess.upload(xb, cb)
    pr = t64(np.stack([rng.integers(0, 1500, 2000), rng.integers(0, 1500, 2000)], 1))
    wi = t32(rng.integers(0, n_wf, 2000))
    for k in range(2):
        cd.record(f"dictionary call #{k}", lambda: cd.sess.from_primitives(a, b, pr, 10.0, wf_index=wi))
        cd.record(f"composition with an index #{k}", lambda: cd.sess.composition(a, pr[:300, 0].contiguous(), 10.0, wf_index=wi[:300].contiguous()))
    x1, c1 = cloud(65)
    cd.record("composition_coords with an index", lambda: cd.lchd.composition_from_coords([cd.cats[i] for i in c1], x1, [f"w{i % n_wf}" for i in range(65)]))
    cd.close()

c300 = Ctx("300 categories", 300)
xa, ca = cloud(1500, n_cat=300)
xb, cb = cloud(1500, n_cat=300)
a, b = c300.sess.upload(xa, ca), c300.sess.upload(xb, cb)
pr = t64(np.stack([rng.integers(0, 1500, 1200), rng.integers(0, 1500, 1200)], 1))
for k in range(2):
    c300.record(f"300 categories #{k}", lambda: c300.sess.from_primitives(a, b, pr, 10.0))
    c300.record(f"composition, 300 categories #{k}", lambda: c300.sess.composition(a, pr[:300, 1].contiguous(), 10.0))
x1, c1 = cloud(65, n_cat=300)
c300.record("composition_coords, 300 categories", lambda: c300.lchd.composition_from_coords([c300.cats[i] for i in c1], x1))
c300.close()
dump.close()
print("calls dumped to", sys.argv[1])
