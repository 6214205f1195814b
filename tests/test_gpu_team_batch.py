"""The team sweeps (k_sweep_duo, loco_hd_amd/csrc/lchd_sweep_team.hip) take a BATCH of consecutive pairs per wavefront, rank the batch by
chunk length inside the wavefront and sweep the pairs of rank TEAMS q + team in iteration q.  What can go wrong: the seams of a batch, the
pair index that travels with the rank (a score stored at another pair's place), pairs of different kinds in one batch, a wavefront that
takes several batches.  A pair's score must not depend on which pair shares its wavefront.

Star clouds as in test_gpu_sweep_dispatch.py (rebuilt here): star i is an anchor on a lattice site (sites 3 thresholds apart) with m_i
further atoms at radius (0.05 .. 0.95) x threshold around it, so its environment has exactly m_i + 1 points.  Two pairs of clouds: the
"240" clouds hold 33 sizes of 1 .. 121 points (every pair of them has at most 240 merged events: the four-team form, 16 lanes per pair),
the "480" clouds 33 sizes of 122 .. 241 points (242 .. 480 events, environments of at most 255 points: the two-team form, 32 lanes), both
a few extra sizes for the mixed batches.  All 33 x 33 size pairs have distinct scores (asserted), so a score at the wrong place fails.
The oracle scores every distinct pair once per configuration; the lists index into that table.

LCHD_TEAM_BATCH forces the batch size the library uses for long lists (kTeamBatch240 / kTeamBatch480, lchd_kernels.hip) onto these short ones, LCHD_NO_INLINE_META
the record pass + team sweep onto lists of at most 4096 pairs; the default batch of a short list (one iteration's pairs) runs too."""
import numpy as np
import pytest

from loco_hd_amd import _native as N

pytestmark = pytest.mark.gpu

THR = 10.0
TIGHT = 1e-11
SENTINEL = -7.0
K_BATCH = {240: 32, 480: 16}   # kTeamBatch240 / kTeamBatch480
WAVES = 4             # kSweepWaves
GRID_CAP = 8192       # kTeamGridCap
RANGE = {240: np.unique(np.linspace(1, 121, 33).astype(int)), 480: np.unique(np.linspace(122, 241, 33).astype(int))}
EXTRA = {240: (2, 122, 256), 480: (1, 2, 242, 256)}
TEAMS = {240: 4, 480: 2}
FAMILY = {240: N.SWEEP_TEAM240, 480: N.SWEEP_TEAM480}
RULE = {240: 0, 480: 2}
assert all(len(r) == 33 for r in RANGE.values())

_clouds = {}


def star_cloud(form, seed):
    """(xyz, {size: anchor atom index})"""
    if (form, seed) not in _clouds:
        rng = np.random.default_rng(seed)
        sizes = list(RANGE[form]) + list(EXTRA[form])
        sites = np.stack(np.meshgrid(*[np.arange(4) * 3.0 * THR] * 3, indexing="ij"), -1).reshape(-1, 3)
        sites = sites[rng.permutation(len(sites))[:len(sizes)]]
        xyz, anchor, at = [], {}, 0
        for size, site in zip(sizes, sites):
            u = rng.normal(size=(size - 1, 3))
            r = rng.uniform(0.05 * THR, 0.95 * THR, size - 1)
            xyz.append(np.concatenate([site[None], site + u / np.linalg.norm(u, axis=1, keepdims=True) * r[:, None]]))
            anchor[int(size)] = at
            at += size
        _clouds[(form, seed)] = (np.concatenate(xyz), anchor)
    return _clouds[(form, seed)]


# id -> (categories, form, environment, configuration, what last_sweep() must show)
CONFIGS = {
    "h2_8_240": (8, 240, {"LCHD_PRE_ROWS": "1"}, {}, dict(slots=8, pre=1, team_mode=0)),
    "h2_8_240_rows_off": (8, 240, {"LCHD_PRE_ROWS": "-1"}, {}, dict(slots=8, pre=0, team_mode=0)),
    "h2_12_480": (12, 480, {"LCHD_PRE_ROWS": "1"}, {}, dict(slots=12, pre=1, team_mode=0)),
    "h2_12_480_rows_off": (12, 480, {"LCHD_PRE_ROWS": "-1"}, {}, dict(slots=12, pre=0, team_mode=0)),
    "h2_16_480": (16, 480, {"LCHD_PRE_ROWS": "1"}, {}, dict(slots=16, pre=1, team_mode=0)),
    "weights_12_480": (12, 480, {}, dict(weights=True), dict(slots=12, pre=0, team_mode=1)),
    "weights_8_240": (8, 240, {}, dict(weights=True), dict(slots=8, pre=0, team_mode=1)),
    "ksm_12_480": (12, 480, {}, dict(sd=("Kolmogorov-Smirnov", [])), dict(slots=12, team_mode=2)),
    "ksm_8_240": (8, 240, {}, dict(sd=("Kolmogorov-Smirnov", [])), dict(slots=8, team_mode=2)),
    "dict_12_480": (12, 480, {}, dict(wf_dict=True), dict(slots=12, team_mode=0)),
    "dict_8_240": (8, 240, {}, dict(wf_dict=True), dict(slots=8, team_mode=0)),
}


def build(mod, ncat, cfg):
    kw = {}
    if cfg.get("weights"):
        kw["category_weights"] = list(0.5 + 0.25 * np.arange(ncat))
    if "sd" in cfg:
        kw["statistical_distance"] = mod.StatisticalDistance(*cfg["sd"])
    wf = mod.WeightFunction("hyper_exp", [1.0, 0.1])
    if cfg.get("wf_dict"):
        wf = {"h": wf, "u": mod.WeightFunction("uniform", [1.0, 9.0])}
    return mod.LoCoHD([f"c{i}" for i in range(ncat)], wf, **kw)


class Bench:
    """one configuration on one pair of clouds: the oracle's score of every size pair (per weight function), a session of the library"""

    def __init__(self, name, oracle, monkeypatch, batch=None):
        import loco_hd_amd as lh
        from loco_hd_amd.device import DeviceSession

        self.ncat, self.form, env, self.cfg, self.show = CONFIGS[name]
        batch = K_BATCH[self.form] if batch is None else batch
        self.batch = batch or K_BATCH[self.form]
        self.hooked = batch  # 0: the library's own choice
        monkeypatch.setenv("LCHD_NO_INLINE_META", "1")
        if batch:
            monkeypatch.setenv("LCHD_TEAM_BATCH", str(batch))
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        (self.xa, self.anchor_a), (self.xb, self.anchor_b) = star_cloud(self.form, 5100 + self.form), star_cloud(self.form, 5200 + self.form)
        rng = np.random.default_rng(600 + self.ncat)
        self.ca = rng.integers(0, self.ncat, len(self.xa)).astype(np.int32)
        self.cb = rng.integers(0, self.ncat, len(self.xb)).astype(np.int32)
        self.sizes_all = [int(s) for s in list(RANGE[self.form]) + list(EXTRA[self.form])]
        self.lo = build(oracle, self.ncat, self.cfg)
        self.lo.n_threads = 8
        self.lchd = build(lh, self.ncat, self.cfg)
        self.names = list(self.lchd.w_func) if self.cfg.get("wf_dict") else None
        self.sess = DeviceSession(self.lchd)
        self.a, self.b = self.sess.upload(self.xa, self.ca), self.sess.upload(self.xb, self.cb)
        self._table = {}

    def anchors_of(self, sizes):
        return np.stack([[self.anchor_a[int(a)] for a in sizes[:, 0]], [self.anchor_b[int(b)] for b in sizes[:, 1]]], 1).astype(np.int64)

    def wf_index_of(self, n):
        """the weight function of pair p of a list: p % 2 (a dictionary's per-pair index follows the pair, not the lane)"""
        return None if self.names is None else (np.arange(n) % 2).astype(np.int32)

    def table(self, w):
        """oracle score of EVERY size pair under weight function w of the dictionary (0 without one): [size index A][size index B]"""
        if w not in self._table:
            s = np.asarray(self.sizes_all)
            grid = np.stack(np.meshgrid(s, s, indexing="ij"), -1).reshape(-1, 2)
            pairs, tag = self.anchors_of(grid), np.zeros(len(self.xa), dtype=np.int32)
            wfs = idx = None
            if self.names:
                wfs, idx = self.lo._wfs([self.names[w]] * len(pairs), len(pairs))
            want, got_sizes = self.lo.from_arrays(self.xa, self.ca, tag, self.xb, self.cb, np.zeros(len(self.xb), dtype=np.int32), pairs, THR,
                                                  wfs=wfs, wf_idx=idx, return_env_sizes=True)
            assert np.array_equal(np.asarray(got_sizes), grid), "the stars do not have the sizes of the table"
            self._table[w] = np.asarray(want).reshape(len(s), len(s))
        return self._table[w]

    def want(self, sizes):
        pos = {s: k for k, s in enumerate(self.sizes_all)}
        ia, ib = np.asarray([pos[int(a)] for a in sizes[:, 0]]), np.asarray([pos[int(b)] for b in sizes[:, 1]])
        if self.names is None:
            return self.table(0)[ia, ib]
        return np.where(np.arange(len(sizes)) % 2 == 0, self.table(0)[ia, ib], self.table(1)[ia, ib])

    def score(self, pairs, wf_index=None, expect_error=None):
        import torch

        import loco_hd_amd as lh

        out = torch.full((len(pairs),), SENTINEL, dtype=torch.float64, device="cuda")
        wfi = None if wf_index is None else torch.from_numpy(np.ascontiguousarray(wf_index)).cuda()
        if expect_error:
            with pytest.raises(lh.PanicException):
                self.sess.from_primitives(self.a, self.b, torch.from_numpy(np.ascontiguousarray(pairs)).cuda(), THR, out=out, wf_index=wfi)
        else:
            self.sess.from_primitives(self.a, self.b, torch.from_numpy(np.ascontiguousarray(pairs)).cuda(), THR, out=out, wf_index=wfi)
        return out.cpu().numpy()

    def assert_team_ran(self, n_pairs, batch=None):
        """the record of the last call: this form's team kernel in force, launched with the batch the hook (or `batch`) names, one
        batch per wavefront up to the cap"""
        seen = self.sess.last_sweep()
        assert seen is not None and seen["families"] & FAMILY[self.form] and seen["rule"] == RULE[self.form], seen
        assert {k: seen[k] for k in self.show} == self.show, seen
        kb = batch or self.hooked
        assert kb and seen[f"team_batch{self.form}"] == kb, (kb, seen)
        assert seen[f"team_grid{self.form}"] == min(-(-(-(-n_pairs // kb)) // WAVES), GRID_CAP), (n_pairs, seen)

    def in_range_list(self, n, seed=77):
        """n pairs over the 33 x 33 in-range size pairs, a seeded permutation (repeated beyond 1089)"""
        r = RANGE[self.form]
        grid = np.stack(np.meshgrid(r, r, indexing="ij"), -1).reshape(-1, 2)
        rng = np.random.default_rng(seed)
        reps = -(-n // len(grid))
        return np.concatenate([grid[rng.permutation(len(grid))] for _ in range(reps)])[:n]


def seam_lengths(form, batch):
    kb = batch or TEAMS[form]
    return sorted({1, 2, max(TEAMS[form] - 1, 1), kb - 1, kb, kb + 1, 2 * kb + 1, 4 * WAVES * kb + 3} - {0})


@pytest.mark.parametrize("name", list(CONFIGS))
def test_batch_seams(name, oracle, monkeypatch):
    """lists that end just before, at and just behind a batch's end, one that gives four workgroups' wavefronts a batch each and three
    pairs more; every pair has a score of its own"""
    bench = Bench(name, oracle, monkeypatch)
    longest = 4 * WAVES * bench.batch + 3
    sizes = bench.in_range_list(longest)
    want = bench.want(sizes)
    if bench.names is None:
        assert len(np.unique(want)) == len(want), "every pair of the list has a score of its own"
    pairs = bench.anchors_of(sizes)
    for n in seam_lengths(bench.form, bench.batch):
        got = bench.score(pairs[:n], bench.wf_index_of(n))
        bench.assert_team_ran(n)
        err = float(np.max(np.abs(got - want[:n])))
        print(f"{name}: {n} pairs, max |gpu - oracle| = {err:.3e}")
        assert not np.isnan(got).any() and not (got == SENTINEL).any()
        assert err <= TIGHT, (n, err)
    bench.sess.close()


@pytest.mark.parametrize("batch", [0, 16, 32, 64])
@pytest.mark.parametrize("name", ["h2_8_240", "h2_12_480"])
def test_other_batch_sizes(name, batch, oracle, monkeypatch):
    """the batch a short list gets by default (one iteration's pairs: 0 = no hook), and the other sizes the hook can set"""
    bench = Bench(name, oracle, monkeypatch, batch=batch)
    lengths = seam_lengths(bench.form, batch)
    sizes = bench.in_range_list(lengths[-1])
    want, pairs = bench.want(sizes), bench.anchors_of(sizes)
    for n in lengths:
        got = bench.score(pairs[:n])
        bench.assert_team_ran(n, batch=batch or TEAMS[bench.form])  # (no hook: a list this short gets one iteration's pairs)
        err = float(np.max(np.abs(got - want[:n])))
        print(f"{name} batch {batch}: {n} pairs, max |gpu - oracle| = {err:.3e}")
        assert err <= TIGHT, (n, err)
    bench.sess.close()


def mixed_list(bench, batches=3):
    """per 32 pairs (one batch under LCHD_TEAM_BATCH=32): three pairs without events, two with one event, 23 at the tile's limit, two one event over it (the companion's),
    one with an environment of 256 points (no 8-bit counts), one with an anchor out of range -- in a seeded order per batch.  Seven keys
    of 0 (an odd number), two of 1: ranked, a pair without events shares an iteration with unswept ones, a one-event pair with a zero
    and the other with a pair of 15 trips.  -> (sizes with (0, 0) for the bad pair, anchors, is_bad)"""
    form = bench.form
    lim = 121 if form == 240 else 241
    kinds = [(1, 1)] * 3 + [(1, 2), (2, 1)] + [(lim, lim)] * 23 + [(lim, lim + 1), (lim + 1, lim)] + [(256, 1)] + [(0, 0)]
    assert len(kinds) == 32
    rng = np.random.default_rng(31)
    sizes = np.concatenate([np.asarray(kinds)[rng.permutation(32)] for _ in range(batches)])
    bad = sizes[:, 0] == 0
    anchors = np.empty((len(sizes), 2), dtype=np.int64)
    anchors[~bad] = bench.anchors_of(sizes[~bad])
    anchors[bad] = [len(bench.xa), bench.anchor_b[1]]
    return sizes, anchors, bad


@pytest.mark.parametrize("name", list(CONFIGS))
def test_mixed_batch(name, oracle, monkeypatch):
    bench = Bench(name, oracle, monkeypatch, batch=32)  # (both forms: the 32 pairs of mixed_list are ONE batch)
    sizes, anchors, bad = mixed_list(bench)
    good = np.flatnonzero(~bad)
    # without the unusable pairs first: the call stands, and the record shows the team kernel of this form in force
    want = bench.want(sizes[good])
    got = bench.score(anchors[good], bench.wf_index_of(len(good)))
    bench.assert_team_ran(len(good))
    err = float(np.max(np.abs(got - want)))
    print(f"{name}: mixed batches without unusable pairs, max |gpu - oracle| = {err:.3e}")
    assert not np.isnan(got).any() and not (got == SENTINEL).any() and err <= TIGHT
    # with them: the call fails like the reference, NaN stands at those pairs and nowhere else
    wfi = bench.wf_index_of(len(sizes))
    want = np.full(len(sizes), np.nan)
    if bench.names is None:
        want[good] = bench.want(sizes[good])
    else:  # (the weight function follows the pair's place in THIS list)
        pos = {s: k for k, s in enumerate(bench.sizes_all)}
        for p in good:
            want[p] = bench.table(int(wfi[p]))[pos[int(sizes[p, 0])], pos[int(sizes[p, 1])]]
    got = bench.score(anchors, wfi, expect_error=True)
    assert np.array_equal(np.isnan(got), bad) and not (got == SENTINEL).any()
    err = float(np.max(np.abs(got[good] - want[good])))
    print(f"{name}: mixed batches, max |gpu - oracle| = {err:.3e}")
    assert err <= TIGHT
    bench.sess.close()


@pytest.mark.parametrize("name", ["h2_8_240", "h2_12_480", "dict_12_480"])
def test_partner_independence(name, oracle, monkeypatch):
    """a pair's bits do not depend on the pairs it shares a batch or an iteration with"""
    bench = Bench(name, oracle, monkeypatch)
    n = 4 * WAVES * bench.batch + 3
    pairs = bench.anchors_of(bench.in_range_list(n))
    wfi = bench.wf_index_of(n)
    first = bench.score(pairs, wfi)
    bench.assert_team_ran(n)
    assert np.array_equal(first, bench.score(pairs, wfi)), "two calls on the same list"
    perm = np.random.default_rng(5).permutation(n)
    for name_, order in (("reversed", np.arange(n)[::-1]), ("shuffled", perm)):
        got = bench.score(pairs[order], None if wfi is None else wfi[order])
        back = np.empty_like(got)
        back[order] = got
        assert np.array_equal(back, first), name_
    bench.sess.close()


@pytest.mark.parametrize("name", ["h2_8_240", "h2_12_480"])
def test_several_batches_per_wavefront(name, oracle, monkeypatch):
    """a list longer than GRID_CAP workgroups x WAVES wavefronts x K_BATCH pairs: the grid-stride loop over batches runs more than once
    in some wavefronts (no hook: a list of this length gets the form's K_BATCH by itself)"""
    bench = Bench(name, oracle, monkeypatch, batch=0)
    kb = K_BATCH[bench.form]
    n = GRID_CAP * WAVES * kb + 3 * WAVES * kb + 5
    sizes = bench.in_range_list(n)
    pairs = bench.anchors_of(sizes)
    got = bench.score(pairs)
    bench.assert_team_ran(n, batch=kb)
    assert bench.sess.last_sweep()[f"team_grid{bench.form}"] == GRID_CAP
    assert not np.isnan(got).any() and not (got == SENTINEL).any()
    sample = np.random.default_rng(9).choice(n, 20_000, replace=False)
    sample = np.concatenate([sample, np.arange(n - 3 * WAVES * kb - 5, n)])  # ... and the batches of the second trip
    err = float(np.max(np.abs(got[sample] - bench.want(sizes[sample]))))
    print(f"{name}: {n} pairs, max |gpu - oracle| over {len(sample)} = {err:.3e}")
    assert err <= TIGHT
    half = n // 2
    assert np.array_equal(got, np.concatenate([bench.score(pairs[:half]), bench.score(pairs[half:])])), "the list in two halves"
    bench.sess.close()


SHORT_BLOCKS, SHORT_CAP = 32768, 4096   # kTeamShortBlocks, kTeamShortCap


@pytest.mark.parametrize("name", ["h2_8_240", "h2_12_480"])
def test_short_and_long_launches(name, oracle, monkeypatch):
    """the library's own choice on both sides of its limit: a launch of at most SHORT_BLOCKS workgroups' worth of pairs (one iteration's
    pairs per wavefront) keeps one iteration's pairs per trip and SHORT_CAP workgroups, one pair more gets the form's batch; the scores
    of the common pairs are the same bits, and the oracle's"""
    bench = Bench(name, oracle, monkeypatch, batch=0)
    teams, kb = TEAMS[bench.form], K_BATCH[bench.form]
    limit = SHORT_BLOCKS * WAVES * teams
    sizes = bench.in_range_list(limit + 1)
    pairs = bench.anchors_of(sizes)
    short = bench.score(pairs[:limit])
    seen = bench.sess.last_sweep()
    assert (seen[f"team_batch{bench.form}"], seen[f"team_grid{bench.form}"]) == (teams, SHORT_CAP), seen
    long = bench.score(pairs)
    bench.assert_team_ran(limit + 1, batch=kb)
    assert np.array_equal(long[:limit], short)
    sample = np.concatenate([np.random.default_rng(11).choice(limit, 20_000, replace=False), [limit]])
    err = float(np.max(np.abs(long[sample] - bench.want(sizes[sample]))))
    print(f"{name}: {limit} / {limit + 1} pairs, max |gpu - oracle| over {len(sample)} = {err:.3e}")
    assert err <= TIGHT
    bench.sess.close()
