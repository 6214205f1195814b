"""The per-lane category counts of the team sweeps' event loop (TeamTile::run, loco_hd_amd/csrc/lchd_team_tile.h) at the seams of
their packing.  With 9 .. 16 category slots a side's counts are 8-bit fields of two 64-bit words (a 32-bit seam between categories
3 | 4 and 11 | 12, a 64-bit seam between 7 | 8) plus 4-bit fields of what the lane's chunk has added; an event picks its count with a
byte permute over the selected word and adds to the 4-bit fields of side A and of both sides together.  That is integer work only, so
every list is scored by the team kernel and compared
  * with the CPU oracle (<= 1e-11), and
  * with the scores recorded by the library of the commit BEFORE this bookkeeping (np.array_equal;
    tests/golden/team_count_fields/<case>.npy -- scores only, the inputs are rebuilt here).

One cloud serves both sides (so a star paired with itself is a pair of IDENTICAL environments: H^2 = 0 at every event, the literal
difference-of-roots branch).  Stars as in test_gpu_team_sentinel.py: an anchor on a lattice site (sites 30 apart, threshold 10) and
one atom per radius k / 32, k in 33 .. 287, on the axis k % 3 -- all exact, no tie inside a list.

Stars, for every category c of the case's MONO list (12 categories: 0, 3, 4, 7, 8, 11 -- both neighbours of every 32-bit and 64-bit
seam; 16 categories: 0, 7, 8, 15; 8 categories: 0, 3, 4, 7):
  big<c>     254 points + the anchor, ALL of category c: the byte field of c reaches 255 next to empty neighbours
  par<c>     226 points (the radii from the 30th on) of category c: (big<c>, par<c>) has T = 480 events, chunks of 15, and its first 29
             events are all A's -- lane 0's 4-bit field of c reaches 15; (par<c>, par<c>) is an identical pair
  alt34, alt78, bl34, bl78   two categories alternating point by point across a seam (3 / 4 and 7 / 8; the 8-category case: 3 / 4 only),
             180 and 170 points
  f0 .. f5   random categories, 135 .. 235 points (they decide the form's rule on the device)

Cases: c12 (12 categories, 12 slots), c12ksm (the same, Kolmogorov-Smirnov), c16 (16 slots), c8 (8 slots: one count word per side).
"""
import numpy as np
import pytest
from golden_util import GOLD

from loco_hd_amd import _native as N

pytestmark = pytest.mark.gpu

GOLDEN = GOLD / "team_count_fields"
THR = 10.0
TOL = 1e-11
GRID = np.arange(33, 288)  # 255 radii k / 32
CASES = {
    "c12": dict(ncat=12, slots=12, mono=(0, 3, 4, 7, 8, 11), ksm=False),
    "c12ksm": dict(ncat=12, slots=12, mono=(0, 3, 4, 7, 8, 11), ksm=True),
    "c16": dict(ncat=16, slots=16, mono=(0, 7, 8, 15), ksm=False),
    "c8": dict(ncat=8, slots=8, mono=(0, 3, 4, 7), ksm=False),
}
ENV = {"LCHD_NO_INLINE_META": "1", "LCHD_TEAM_BATCH": "16", "LCHD_PRE_ROWS": "1"}

_clouds = {}


def cloud(case):
    """(xyz, categories, {star: anchor atom}, {star: points incl. the anchor}) -- by (ncat, mono): c12 and c12ksm share theirs"""
    cfg = CASES[case]
    key = (cfg["ncat"], cfg["mono"])
    if key in _clouds:
        return _clouds[key]
    ncat, mono = key
    rng = np.random.default_rng(2000 + ncat)
    stars = {}  # name -> (radii numerators, categories of the anchor + the points)
    for c in mono:
        stars[f"big{c}"] = (GRID[:254], np.full(255, c))
        stars[f"par{c}"] = (GRID[29:255], np.full(227, c))
    seams = [(3, 4)] + ([(7, 8)] if ncat > 8 else [])
    for lo, hi in seams:
        stars[f"alt{lo}{hi}"] = (GRID[:180], np.where(np.arange(181) % 2 == 0, lo, hi))
        stars[f"bl{lo}{hi}"] = (GRID[40:210], np.where(np.arange(171) % 2 == 0, hi, lo))
    for k in range(6):
        m = int(rng.integers(135, 236))
        stars[f"f{k}"] = (np.sort(rng.permutation(GRID)[:m]), rng.integers(0, ncat, m + 1))
    sites = 30.0 * np.stack(np.meshgrid(*[np.arange(3)] * 3, indexing="ij"), -1).reshape(-1, 3)
    assert len(stars) <= len(sites)
    xyz, cats, anchor, size, at = [], [], {}, {}, 0
    for (name, (ks, cs)), site in zip(stars.items(), sites):
        pts = np.tile(site, (len(ks), 1))
        pts[np.arange(len(ks)), ks % 3] += ks / 32.0
        xyz.append(np.concatenate([site[None], pts]))
        cats.append(cs)
        anchor[name], size[name] = at, len(ks) + 1
        at += len(ks) + 1
    _clouds[key] = (np.concatenate(xyz), np.concatenate(cats).astype(np.int32), anchor, size)
    return _clouds[key]


def name_list(case):
    cfg = CASES[case]
    mono = cfg["mono"]
    names = []
    for k, c in enumerate(mono):
        d = mono[(k + 1) % len(mono)]
        names += [(f"big{c}", f"par{c}"), (f"par{c}", f"big{c}"), (f"par{c}", f"par{c}"), (f"big{c}", f"par{d}"), (f"par{d}", f"big{c}"),
                  (f"big{c}", "f0"), ("f1", f"big{c}")]
    alts = [s for s in ("alt34", "bl34", "alt78", "bl78") if cfg["ncat"] > 8 or s.endswith("34")]
    names += [(a, b) for a in alts for b in alts] + [(a, "f2") for a in alts] + [("f3", a) for a in alts]
    names += [(f"f{a}", f"f{b}") for a in range(6) for b in range(6)]
    rng = np.random.default_rng(77 + cfg["ncat"])
    names = names + [names[k] for k in rng.permutation(len(names))]  # every pair twice, at other places of the batches
    return names


def build(mod, case):
    cfg, kw = CASES[case], {}
    if cfg["ksm"]:
        kw["statistical_distance"] = mod.StatisticalDistance("Kolmogorov-Smirnov", [])
    return mod.LoCoHD([f"c{i}" for i in range(cfg["ncat"])], mod.WeightFunction("hyper_exp", [1.0, 0.1]), **kw)


def pairs_of(case):
    _, _, anchor, size = cloud(case)
    names = name_list(case)
    pairs = np.asarray([[anchor[a], anchor[b]] for a, b in names], dtype=np.int64)
    return pairs, np.asarray([size[a] for a, _ in names]), np.asarray([size[b] for _, b in names])


def gpu_scores(lh, case, passes=2):
    """scores and last_sweep() records of `passes` calls of one session (the first lets the device pick the rule, the second is hinted)"""
    import torch
    from loco_hd_amd.device import DeviceSession

    xyz, cats, _, _ = cloud(case)
    pairs, _, _ = pairs_of(case)
    sess = DeviceSession(build(lh, case))
    a, b = sess.upload(xyz, cats), sess.upload(xyz, cats)
    d_pairs = torch.from_numpy(pairs).cuda()
    outs, swept = [], []
    for _ in range(passes):
        outs.append(sess.from_primitives(a, b, d_pairs, THR).cpu().numpy())
        swept.append(sess.last_sweep())
    sess.close()
    return outs, swept


@pytest.mark.parametrize("case", sorted(CASES))
def test_count_fields_keep_the_bits(case, oracle, monkeypatch):
    import loco_hd_amd as lh

    for k, v in ENV.items():
        monkeypatch.setenv(k, v)
    cfg = CASES[case]
    xyz, cats, _, _ = cloud(case)
    pairs, nA, nB = pairs_of(case)
    T = nA + nB - 2
    # the list is what the docstring says
    assert 100 <= len(pairs) <= 400 and max(nA.max(), nB.max()) == 255 and T.max() == 480
    assert np.count_nonzero(pairs[:, 0] == pairs[:, 1]) >= 2 * len(cfg["mono"])  # identical environments
    lo = build(oracle, case)
    lo.n_threads = 8
    zeros = np.zeros(len(xyz), dtype=np.int32)
    want, sizes = lo.from_arrays(xyz, cats, zeros, xyz, cats, zeros, pairs, THR, return_env_sizes=True)
    want = np.asarray(want)
    assert np.array_equal(np.asarray(sizes), np.stack([nA, nB], 1)), "the stars do not have their sizes"

    outs, swept = gpu_scores(lh, case)
    for rec in swept:
        print(rec)
        assert rec is not None and rec["families"] & N.SWEEP_TEAM480 and rec["rule"] == 2 and rec["slots"] == cfg["slots"], rec
        assert rec["team_mode"] == (2 if cfg["ksm"] else 0) and rec["pre"] == 1, rec
    assert swept[-1]["left"] == 0, swept[-1]
    golden = np.load(GOLDEN / f"{case}.npy")
    for k, got in enumerate(outs):
        err = float(np.max(np.abs(got - want)))
        differ = int(np.count_nonzero(got.view(np.uint64) != golden.view(np.uint64))) if got.shape == golden.shape else -1
        print(f"{case} pass {k}: {len(pairs)} pairs, max |gpu - oracle| = {err:.3e}, scores whose bits differ from the fixture: {differ}")
        assert err <= TOL
    same = pairs[:, 0] == pairs[:, 1]
    assert golden.dtype == np.float64
    for got in outs:
        assert (got[same] == 0.0).all()  # identical environments: exactly 0
        assert np.array_equal(got, golden)
