"""The team sweeps (k_sweep_duo, lchd_team_tile.h) keep their bits: float64 scores of seeded random clouds, recorded once on the commit
before the chunk-start counts and the event loop of the tile were rewritten in 32-bit arithmetic, must come back unchanged
(np.array_equal) and lie at the CPU oracle (<= 1e-11).

Random coordinates have no exact distance ties, so an environment's order -- and with it every rounding of the sweep -- does not depend
on the order atomics hand points out in.  Three team shapes through the unit-weight Hellinger-2 form, and one call each with category
weights (WGT) and with the Kolmogorov-Smirnov distance (KSM):

  h2_12   2 x 3000 atoms at 0.05 atoms/A^3, 10 categories: 12 category slots; pairs of ~310 merged events: two pairs per wavefront, tiles
          of at most 480 events
  h2_8    0.023 atoms/A^3, 8 categories: 8 slots, ~140 events per pair: four pairs per wavefront, tiles of at most 240 events
  h2_16   0.05 atoms/A^3, 16 categories: 16 slots, 480-event tiles
  wgt_12, ksm_12   the clouds of h2_12 (the weighted form has no prefix-count-row instantiation: wgt_12 covers the event loop only)

Which kernels sweep a pass is decided inside the library from the previous pass's pair statistics; DeviceSession.last_sweep() reports it,
and the test asserts it: the hinted passes ran the team kernel of the case's tile and nothing else but the companion -- which is left out
where every pair of the list fits the tile (all cases but h2_16) --, at the case's slot count, reading prefix-count rows (PRE) in the h2 and ksm cases and building the chunk-start counts per tile in the weighted one.  It also
asserts the pair statistics that decide (most pairs fit the shape's tile, and for the 480-event shapes most do not fit the 240-event
one).  profiles/r10/kernel_stats_team_sweep_bits.csv is a kernel trace of these five cases.

Behind the 20 000 random pairs every list carries pairs built for the ends of the chunk-start reads: small clusters far outside the box
give environments of 1, 2 and 3 points on either side (a lane's chunk then starts 0 .. 2 points behind a prefix-count row that is the
environment's last), and the pair with the most merged events a tile takes -- exactly 480 for the 480-event shapes, asserted below --
fills the staged buffer to its last entry.

The fixtures (tests/golden/team_sweep_bits/<case>.npy) hold the scores only; the inputs are rebuilt from the seeds here.
"""
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "team_sweep_bits"
THR = 10.0
N_ATOMS, N_RANDOM_PAIRS = 3000, 20_000
CLUSTERS = (1, 2, 3, 1, 2, 3)  # points per far-away cluster, on both sides

# case -> (seed, density, categories, form, merged events of the fullest tile the case must contain or None)
CASES = {
    "h2_12": (9101, 0.05, 10, "h2", 480),
    "h2_8": (9102, 0.023, 8, "h2", None),
    "h2_16": (9104, 0.05, 16, "h2", 480),
    "wgt_12": (9101, 0.05, 10, "wgt", 480),
    "ksm_12": (9101, 0.05, 10, "ksm", 480),
}
TILE_OF = {"h2_12": 480, "h2_8": 240, "h2_16": 480, "wgt_12": 480, "ksm_12": 480}


def env_sizes(xyz):
    """points within THR of every point, itself included (what the sweep merges of an environment is this minus the anchor)"""
    out = np.empty(len(xyz), dtype=np.int64)
    for s in range(0, len(xyz), 500):
        d = xyz[s:s + 500, None, :] - xyz[None, :, :]
        out[s:s + 500] = (np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) < THR).sum(1)
    return out


def make_case(name):
    """dict(xa, xb, ca, cb, pairs, n_cat, form, weights, T) -- T: merged events of every pair"""
    seed, density, n_cat, form, _ = CASES[name]
    rng = np.random.default_rng(seed)
    side = (N_ATOMS / density) ** (1.0 / 3.0)

    def cloud():
        box = rng.uniform(0.0, side, (N_ATOMS, 3))
        far = [np.array([side + 60.0 * (k + 1), 0.0, 0.0]) + rng.uniform(0.0, 3.0, (m, 3)) for k, m in enumerate(CLUSTERS)]
        return np.concatenate([box] + far)

    xa, xb = cloud(), cloud()
    n = len(xa)
    ca, cb = rng.integers(0, n_cat, n).astype(np.int32), rng.integers(0, n_cat, n).astype(np.int32)
    pairs = np.stack([rng.integers(0, N_ATOMS, N_RANDOM_PAIRS), rng.integers(0, N_ATOMS, N_RANDOM_PAIRS)], 1)
    na, nb = env_sizes(xa), env_sizes(xb)
    tiny = np.arange(N_ATOMS, n)
    some = rng.integers(0, N_ATOMS, len(tiny))
    extra = [(a, b) for a in tiny for b in tiny] + [(a, b) for a, b in zip(tiny, some)] + [(a, b) for a, b in zip(some, tiny)]
    # the fullest tile: the pair of box atoms with the most merged events the shape's tile takes (environments of at most 255 points)
    tile = TILE_OF[name]
    ok_a, ok_b = np.flatnonzero(na[:N_ATOMS] <= 255), np.flatnonzero(nb[:N_ATOMS] <= 255)
    tot = (na[ok_a, None] - 1) + (nb[None, ok_b] - 1)
    tot = np.where(tot <= tile, tot, -1)
    ia, ib = np.unravel_index(np.argmax(tot), tot.shape)
    extra.append((ok_a[ia], ok_b[ib]))  # (the list's last pair)
    pairs = np.ascontiguousarray(np.concatenate([pairs, np.asarray(extra, dtype=np.int64)]), dtype=np.int64)
    weights = None if form != "wgt" else list(0.5 + 0.25 * np.arange(n_cat))
    return dict(xa=xa, xb=xb, ca=ca, cb=cb, pairs=pairs, n_cat=n_cat, form=form, weights=weights,
                T=(na[pairs[:, 0]] - 1) + (nb[pairs[:, 1]] - 1), na=na, nb=nb)


def build(mod, case):
    cats = [f"c{i}" for i in range(case["n_cat"])]
    kw = {}
    if case["form"] == "wgt":
        kw["category_weights"] = case["weights"]
    if case["form"] == "ksm":
        kw["statistical_distance"] = mod.StatisticalDistance("Kolmogorov-Smirnov", [])
    return mod.LoCoHD(cats, mod.WeightFunction("hyper_exp", [1.0, 0.1]), **kw)


def gpu_scores(lh, case, passes=3):
    """the scores of `passes` consecutive calls of one session (the first picks its sweeps on the device, the later ones launch what the
    previous pass's pair statistics name: the team kernel of the majority's tile)"""
    import torch
    from loco_hd_amd.device import DeviceSession

    sess = DeviceSession(build(lh, case))
    a, b = sess.upload(case["xa"], case["ca"]), sess.upload(case["xb"], case["cb"])
    d_pairs = torch.from_numpy(case["pairs"]).cuda()
    outs, swept = [], []
    for _ in range(passes):
        outs.append(sess.from_primitives(a, b, d_pairs, THR).cpu().numpy())
        swept.append(sess.last_sweep())
    sess.close()
    return outs, swept


@pytest.mark.parametrize("name", sorted(CASES))
def test_team_sweep_scores_keep_their_bits(name, oracle):
    import loco_hd_amd as lh

    case = make_case(name)
    T, tile, full = case["T"], TILE_OF[name], CASES[name][4]
    # the shape really is the one the case is named for: most pairs fit the tile, and (480-event shapes) most do not fit the smaller one
    small = (T <= tile) & (case["na"][case["pairs"][:, 0]] <= 255) & (case["nb"][case["pairs"][:, 1]] <= 255)
    assert small.mean() > 0.9
    if tile == 480:
        assert (T <= 240).mean() < 0.5
    sizes_a, sizes_b = set(case["na"][case["pairs"][:, 0]].tolist()), set(case["nb"][case["pairs"][:, 1]].tolist())
    assert {1, 2, 3} <= sizes_a and {1, 2, 3} <= sizes_b  # environments of 1 .. 3 points, the anchor included
    if full is not None:
        assert T[-1] == full, f"the fullest pair has {T[-1]} merged events, not {full}"
    assert T[-1] <= tile and T[-1] >= tile - 40

    tag = np.zeros(len(case["xa"]), dtype=np.int32)
    want = np.asarray(build(oracle, case).from_arrays(case["xa"], case["ca"], tag, case["xb"], case["cb"], tag, case["pairs"], THR))
    from loco_hd_amd import _native as N

    outs, swept = gpu_scores(lh, case)
    form = CASES[name][3]
    team, rule = (N.SWEEP_TEAM480, 2) if tile == 480 else (N.SWEEP_TEAM240, 0)
    assert swept[0]["families"] == N.SWEEP_TEAM240 | N.SWEEP_INDIRECT | N.SWEEP_TEAM480 | N.SWEEP_PLAIN and swept[0]["forced"] == 0, swept[0]
    for rec in swept:  # (pass 1: every candidate launched, the device decides for the same rule)
        assert rec["rule"] == rule and rec["slots"] == {8: 8, 10: 12, 16: 16}[case["n_cat"]], rec
        assert rec["team_mode"] == {"h2": 0, "wgt": 1, "ksm": 2}[form] and rec["pre"] == (0 if form == "wgt" else 1), rec
    for rec in swept[1:]:
        left = int(np.count_nonzero(~small))  # pairs beyond the tile: with none in the previous pass the companion is not launched
        assert rec["families"] == (team | N.SWEEP_INDIRECT if left else team) and rec["forced"] == 1 and rec["small_rule"] == rule, rec
        assert rec["left"] == left and rec["left_listing"] == (1 if left else 0) and rec["companion_left_out"] == (0 if left else 1), rec
        assert not rec["repeated"], rec
    assert (name == "h2_16") == bool(np.count_nonzero(~small))
    golden = np.load(GOLDEN / f"{name}.npy")
    for k, got in enumerate(outs):
        err = float(np.max(np.abs(got - want)))
        same = int(np.count_nonzero(got.view(np.uint64) != golden.view(np.uint64)))
        print(f"{name} pass {k}: max |gpu - oracle| = {err:.3e}, scores whose bits differ from the fixture: {same} of {got.size}")
        assert err <= 1e-11
    assert golden.dtype == np.float64 and golden.shape == outs[-1].shape
    # the hinted launch set (what a session runs from its second call on) gives the recorded bits
    assert np.array_equal(outs[-1], golden)
    assert np.array_equal(outs[1], golden)
