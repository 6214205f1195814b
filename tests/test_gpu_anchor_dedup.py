"""Every thresholded call de-duplicates its anchors in loco_hd_amd/csrc/lchd_prologue.hip: which atoms are anchors, which environment
slot each gets, how many unique anchors a side has.  Five paths are chosen by size, with index arithmetic at every seam -- bit-set
words of 32 atoms, scan chunks of 4096 words, chunks of 2^18 atoms -- and a wrong slot is silent: the pair reads another anchor's
environment and gets a plausible score.  Each case here puts anchors ON a seam, ASSERTS through DeviceSession.last_anchors() which path
ran and how many unique anchors the device counted, and compares the scores with the CPU oracle and the environment sizes with a
brute-force count (d^2 < thr^2, d^2 summed in x, y, z order, for the anchors only).

Clouds are uniform at about 20 neighbours inside the threshold: every environment stays far below the 512-point slots, so no overflow
pass replaces the record (subset_passes is asserted unchanged).  The oracle scores the DISTINCT pairs of a list; for a cloud of more than
20 000 atoms it is given the atoms inside the anchors' environments only (the same environments, point for point: the brute-force
neighbour search that counts them selects them)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TIGHT = 1e-11
CATS = ["A", "B", "C", "D", "E"]
WF = ("hyper_exp", [1.0, 0.3])
THR = 4.0
DENSITY = 20.0 / (4.0 / 3.0 * np.pi * THR ** 3)
SHARED, FUSED, SCAN, CHUNKED, PER_PAIR = 0, 1, 2, 3, 4  # lchd_ctx_last_anchors modes
PER_STRUCT_BUILD = 2                                    # lchd_ctx_last_grid build code
# the seams, as literals (tests/test_anchor_dedup_host.py holds them against the constants of lchd_prologue.hip)
FUSED_ATOMS = 4096     # fits_struct_path: a single structure of at most 4096 atoms takes the one-workgroup builds (kStructCellsMax cells)
FUSED_PAIRS = 65536    # kFusedPairsMax
STAGE_ATOMS = 131072   # scan_wg_1024 stages 4096 words of 32 atoms per step
CHUNK_ATOMS = 262144   # kPrepScanAtoms = 1 << 18 (k_prep_scatter: chunk of atom i = i >> 18)
DUP_SAMPLE = 131072    # kDupSampleAbove: longer per-pair lists count every 16th pair
FUSED_SIDE = 31.9      # 15 cells of 2.0 per axis: 4096 atoms in at most 4096 cells (about 33 neighbours)
BIG = 20000            # atoms above which the oracle gets the anchors' environments only / a stale pass touches words, not atoms


@pytest.fixture(scope="module")
def lh():
    import loco_hd_amd

    return loco_hd_amd


# ---- inputs -------------------------------------------------------------------------------------------------------------------
class Cloud:
    """Uniform random points and categories: one structure of `sizes` atoms or a batch of len(sizes) structures in one box."""

    def __init__(self, seed, sizes, side=None):
        rng = np.random.default_rng(seed)
        self.sizes = [sizes] if isinstance(sizes, int) else list(sizes)
        self.n = int(sum(self.sizes))
        if side is None:  # (up to 64 atoms: all inside one threshold or so)
            side = 4.5 if self.sizes[0] <= 64 else (self.sizes[0] / DENSITY) ** (1.0 / 3.0)
        self.xyz = rng.uniform(0.0, side, (self.n, 3))
        self.cat = rng.integers(0, len(CATS), self.n).astype(np.int32)
        self.sid = np.repeat(np.arange(len(self.sizes)), self.sizes)
        self.offsets = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        self._order = None
        self._env = {}

    def env(self, i):
        """Atoms of the environment of atom i (itself included), ascending: same structure, d^2 < thr^2 with d^2 summed in x, y, z order."""
        i = int(i)
        if i not in self._env:
            if self._order is None:
                self._order = np.argsort(self.xyz[:, 0], kind="stable")
                self._xs = self.xyz[self._order, 0]
            p = self.xyz[i]
            cand = self._order[np.searchsorted(self._xs, p[0] - THR, "left"):np.searchsorted(self._xs, p[0] + THR, "right")]
            d = self.xyz[cand] - p
            d2 = d[:, 0] * d[:, 0]
            d2 = d2 + d[:, 1] * d[:, 1]
            d2 = d2 + d[:, 2] * d[:, 2]
            self._env[i] = np.sort(cand[(d2 < np.float64(THR) * np.float64(THR)) & (self.sid[cand] == self.sid[i])])
        return self._env[i]

    def structures(self):
        return [(self.xyz[a:b], self.cat[a:b]) for a, b in zip(self.offsets[:-1], self.offsets[1:])]


_clouds = {}


def cloud(seed, sizes, side=None):
    key = (seed, tuple(sizes) if not isinstance(sizes, int) else sizes, side)
    if key not in _clouds:
        _clouds[key] = Cloud(seed, sizes, side)
    return _clouds[key]


def column(rng, n, seams, n_pairs, allowed=None):
    """An anchor column of n_pairs entries: the seams that exist in a structure of n atoms, then random atoms (of `allowed`)."""
    head = [int(s) for s in dict.fromkeys(seams) if 0 <= s < n][:n_pairs]
    fill = rng.integers(0, n, n_pairs - len(head)) if allowed is None else rng.choice(allowed, n_pairs - len(head))
    return np.concatenate([np.asarray(head, dtype=np.int64), fill.astype(np.int64)])


def word_seams(n):
    return [0, 31, 32, 63, 64, n - 33, n - 32, n - 1]


def seam_pairs(seed, a, b, seams_a, seams_b, n_pairs=300, allowed_a=None, allowed_b=None):
    rng = np.random.default_rng(seed)
    return np.stack([column(rng, a.n, seams_a, n_pairs, allowed_a), column(rng, b.n, seams_b, n_pairs, allowed_b)], 1)


def flood_pairs(a, b):
    """Every atom of both sides an anchor; clouds of more than BIG atoms: one anchor in every 32-atom word."""
    def col(c):
        if c.n <= BIG:
            return np.arange(c.n, dtype=np.int64)
        w = np.arange((c.n + 31) // 32, dtype=np.int64)
        return np.minimum(32 * w + (7 * w) % 32, c.n - 1)
    ca, cb = col(a), col(b)
    k = np.arange(max(len(ca), len(cb)))
    return np.stack([ca[k % len(ca)], cb[k % len(cb)]], 1)


# ---- reference ----------------------------------------------------------------------------------------------------------------
def reference(oracle, a, b, pairs, hollow_ok=False):
    """Oracle scores and brute-force environment sizes of a pair list, with the conditions that keep a case from being hollow (they
    hold on the oracle alone).  hollow_ok: structures of one or two atoms -- scores only."""
    uniq, inv = np.unique(pairs, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    lo = oracle.LoCoHD(CATS, oracle.WeightFunction(*WF))
    want_u = np.empty(len(uniq))
    combos = np.stack([a.sid[uniq[:, 0]], b.sid[uniq[:, 1]]], 1)
    for ka, kb in np.unique(combos, axis=0):  # (the oracle scores one structure pair per call)
        rows = np.flatnonzero((combos[:, 0] == ka) & (combos[:, 1] == kb))
        local = []
        sides = []
        for c, k, col in ((a, ka, 0), (b, kb, 1)):
            if c.n > BIG:  # the atoms of the anchors' environments, in index order
                keep = np.unique(np.concatenate([c.env(i) for i in np.unique(uniq[rows, col])]))
            else:
                keep = np.arange(c.offsets[k], c.offsets[k + 1])
            sides.append((c.xyz[keep], c.cat[keep], np.zeros(len(keep), np.int32)))
            local.append(np.searchsorted(keep, uniq[rows, col]))
        want_u[rows] = np.asarray(lo.from_arrays(*sides[0], *sides[1], np.stack(local, 1), THR))
    n_a = np.array([len(a.env(i)) for i in pairs[:, 0]])
    n_b = np.array([len(b.env(i)) for i in pairs[:, 1]])
    assert np.all(np.isfinite(want_u))
    if not hollow_ok:
        assert np.mean(np.concatenate([n_a, n_b])) >= 10.0
        s = np.sort(want_u)
        gap = np.full(len(s), np.inf)
        if len(s) > 1:
            gap[1:] = np.minimum(gap[1:], np.diff(s))
            gap[:-1] = np.minimum(gap[:-1], np.diff(s))
        assert np.mean(gap > 1e-9) >= 0.9  # a swapped slot changes the score of (almost) every pair
    return {"want": want_u[inv], "sizes": n_a + n_b}


def expected_unique(pairs, modes):
    if modes[1] == SHARED:
        return [len(np.unique(pairs)), 0]
    return [len(np.unique(pairs[:, 0])), len(pairs) if modes[1] == PER_PAIR else len(np.unique(pairs[:, 1]))]


def expected_repeats(pairs):
    """What a per-pair pass counts: the pairs whose side-B anchor an earlier pair had used; above DUP_SAMPLE pairs every 16th pair only."""
    col = pairs[:, 1] if len(pairs) <= DUP_SAMPLE else pairs[::16, 1]
    return (len(col) - len(np.unique(col))) * (1 if len(pairs) <= DUP_SAMPLE else 16)


class Session:
    def __init__(self, lh, monkeypatch, per_pair=None):
        from loco_hd_amd.device import DeviceSession

        if per_pair is None:
            monkeypatch.delenv("LCHD_PER_PAIR", raising=False)
        else:
            monkeypatch.setenv("LCHD_PER_PAIR", per_pair)  # (the hooks are read when the context is created)
        self.sess = DeviceSession(lh.LoCoHD(CATS, lh.WeightFunction(*WF)))
        monkeypatch.delenv("LCHD_PER_PAIR", raising=False)
        self.handles = {}

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.sess.close()

    def handle(self, c):
        if id(c) not in self.handles:
            if len(c.sizes) == 1:
                self.handles[id(c)] = self.sess.upload(c.xyz, c.cat)
            else:
                self.handles[id(c)], offsets = self.sess.upload_batch(c.structures())
                assert np.array_equal(offsets, c.offsets)
        return self.handles[id(c)]

    def score(self, a, b, pairs, modes, ref=None, label=""):
        """One call; asserts a. the modes, b. the unique counts (and the repeat count of a per-pair side B) and, given a reference,
        c. the scores and d. the environment points."""
        import torch

        sess = self.sess
        before = sess.pass_counts()
        got = sess.from_primitives(self.handle(a), self.handle(b), torch.from_numpy(np.ascontiguousarray(pairs)).cuda(), THR).cpu().numpy()
        rec, points = sess.last_anchors(), sess.last_env_points()
        print(label, len(pairs), "pairs", rec, "env points", points, "passes", sess.pass_counts()["passes"] - before["passes"])
        assert sess.pass_counts()["subset_passes"] == before["subset_passes"]
        assert rec is not None
        assert [r["mode"] for r in rec] == list(modes)
        assert [r["n_unique"] for r in rec] == expected_unique(pairs, modes)
        assert [r["n_repeated"] for r in rec] == [-1, expected_repeats(pairs) if modes[1] == PER_PAIR else -1]
        if ref is not None:
            assert np.array_equal(np.isfinite(got), np.isfinite(ref["want"]))
            assert np.max(np.abs(got - ref["want"])) < TIGHT
            assert points == int(np.sum(ref["sizes"]))
        return got


# ---- fused ----------------------------------------------------------------------------------------------------------------------
def fused_cloud(seed, n):
    return cloud(seed, n, FUSED_SIDE if n > 64 else None)


FUSED_SIZES = [(1, 2), (2, 1), (31, 32), (32, 33), (33, 31), (4095, 4096), (4096, 4095)]


def fused_list(kind, a, b):
    rng = np.random.default_rng(5)
    if kind == "seams":
        return seam_pairs(11, a, b, word_seams(a.n), word_seams(b.n))
    if kind == "every_atom":
        k = np.arange(max(a.n, b.n), dtype=np.int64)
        return np.stack([k % a.n, rng.permutation(k) % b.n], 1)
    if kind == "one_atom":  # one side-A atom in every pair
        return np.stack([np.full(min(b.n, 300), min(5, a.n - 1), dtype=np.int64), rng.permutation(b.n)[:300].astype(np.int64)], 1)
    if kind == "descending":
        p = seam_pairs(12, a, b, word_seams(a.n), word_seams(b.n))
        return np.stack([np.sort(p[:, 0])[::-1], np.sort(p[:, 1])[::-1]], 1)
    raise KeyError(kind)


@pytest.mark.parametrize("kind", ["seams", "every_atom", "one_atom", "descending"])
@pytest.mark.parametrize("na,nb", FUSED_SIZES, ids=[f"{x}x{y}" for x, y in FUSED_SIZES])
def test_fused_word_seams(lh, oracle, monkeypatch, na, nb, kind):
    """nw = (n + 31) >> 5 words, thread nw - 1 writes the total, the atom loop clamps its index to n - 1."""
    a, b = fused_cloud(1, na), fused_cloud(2, nb)
    pairs = fused_list(kind, a, b)
    ref = reference(oracle, a, b, pairs, hollow_ok=min(na, nb) <= 2)
    with Session(lh, monkeypatch) as s:
        assert s.sess.last_anchors() is None  # (before the first call)
        s.score(a, b, pairs, (FUSED, FUSED), ref, f"fused {na}x{nb} {kind}")


def test_fused_pair_count_limits(lh, oracle, monkeypatch):
    """1 pair, kFusedPairsMax pairs (fused), one more (both sides through the per-structure build and the one-workgroup scan)."""
    a, b = fused_cloud(1, FUSED_ATOMS - 1), fused_cloud(2, FUSED_ATOMS)
    pairs = seam_pairs(13, a, b, word_seams(a.n), word_seams(b.n), FUSED_PAIRS + 1)
    pairs[-1] = (a.n - 1, 0)
    ref = reference(oracle, a, b, pairs)
    cut = lambda m: {"want": ref["want"][:m], "sizes": ref["sizes"][:m]}
    with Session(lh, monkeypatch) as s:
        s.score(a, b, pairs[:1], (FUSED, FUSED), cut(1), "one pair")
        s.score(a, b, pairs[:FUSED_PAIRS], (FUSED, FUSED), cut(FUSED_PAIRS), "65536 pairs")
        assert [g["build"] for g in s.sess.last_grid()] == [FUSED, FUSED]
        s.score(a, b, pairs, (SCAN, SCAN), ref, "65537 pairs")
        assert [g["build"] for g in s.sess.last_grid()] == [PER_STRUCT_BUILD, PER_STRUCT_BUILD]
        s.score(a, b, pairs[:FUSED_PAIRS], (FUSED, FUSED), cut(FUSED_PAIRS), "65536 pairs again")


# ---- one-workgroup scan, chunked, shared, batches --------------------------------------------------------------------------------
C18 = CHUNK_ATOMS
N3 = 3 * C18 + 5  # two full chunks and a partial one of five atoms
# name -> (cloud A, cloud B or None for "one object on both sides", seams A, seams B, modes, random fill of A / B restricted to atoms below)
GENERAL = {
    # the first size off the fused path
    "scan_4097": (lambda: fused_cloud(3, FUSED_ATOMS + 1), lambda: fused_cloud(2, FUSED_ATOMS - 1), word_seams(4097), word_seams(4095), (SCAN, SCAN), None, None),
    # nw = 4096 and 4097 words: the chunk seam of scan_wg_1024 and its carry
    "scan_stage_seam": (lambda: cloud(4, STAGE_ATOMS), lambda: cloud(5, STAGE_ATOMS + 1), [131039, 131040, 131071, 0], [131039, 131040, 131071, 131072, 0],
                        (SCAN, SCAN), None, None),
    # the largest one-workgroup side; a side whose size is no multiple of 32 with its last atom an anchor
    "scan_2p18": (lambda: cloud(6, C18), lambda: cloud(7, 100003), [262112, 262143, 0], [100002, 99999, 99968, 99967], (SCAN, SCAN), None, None),
    # one atom beyond: two chunks, the second of one atom; `big` is decided by either side, so the 3000-atom side is chunked too
    "chunked_2p18_plus_1": (lambda: cloud(8, C18 + 1), lambda: cloud(9, 3000), [262143, 262144, 262112, 0], word_seams(3000), (CHUNKED, CHUNKED), None, None),
    "small_vs_chunked": (lambda: cloud(9, 3000), lambda: cloud(8, C18 + 1), word_seams(3000), [262143, 262144, 262112, 0], (CHUNKED, CHUNKED), None, None),
    # chunks 1 and 2 without an anchor: the only anchors beyond 2^18 - 1 are the five atoms of the last, partial chunk
    "chunked_empty_chunks": (lambda: cloud(10, N3), lambda: cloud(11, 200000), [C18 - 1, C18 - 2, C18 - 32, 3 * C18, 3 * C18 + 1, N3 - 1, 0], word_seams(200000),
                             (CHUNKED, CHUNKED), C18, None),
    "scan_sized_vs_chunked": (lambda: cloud(11, 200000), lambda: cloud(10, N3), word_seams(200000), [C18 - 1, C18, 2 * C18 - 1, 2 * C18, 3 * C18 - 1, 3 * C18, N3 - 1, 0],
                              (CHUNKED, CHUNKED), None, None),
    "chunked_vs_itself": (lambda: cloud(10, N3), None, [C18 - 1, C18, 2 * C18, 3 * C18 - 1, N3 - 1], [0, C18 + 31, C18 + 32, 2 * C18 - 1, 3 * C18, N3 - 2],
                          (CHUNKED, SHARED), None, None),
    "scan_vs_itself": (lambda: cloud(4, STAGE_ATOMS), None, [131039, 131071, 0], [131040, 31, 32], (SCAN, SHARED), None, None),
}


def batch_seams(c):
    return [int(v) for k in range(len(c.sizes)) for v in (c.offsets[k], c.offsets[k + 1] - 1)]


# both sides on the per-structure build: the flags are zeroed by that launch's spare workgroups (1024 threads up to 16 structures in
# all, 512 above); a batch against a structure of more than 4096 atoms: one memset
BATCHES = {
    "batch_8_8": (lambda: cloud(20, [500] * 8), lambda: cloud(21, [500] * 8)),
    "batch_9_9": (lambda: cloud(22, [500] * 9), lambda: cloud(23, [500] * 9)),
    "batch_vs_single": (lambda: cloud(20, [500] * 8), lambda: cloud(24, 5000)),
}


def general_case(name):
    if name in BATCHES:
        a, b = (f() for f in BATCHES[name])
        return a, b, batch_seams(a), batch_seams(b) if len(b.sizes) > 1 else word_seams(b.n), (SCAN, SCAN), None, None
    mk_a, mk_b, seams_a, seams_b, modes, below_a, below_b = GENERAL[name]
    a = mk_a()
    return a, (a if mk_b is None else mk_b()), seams_a, seams_b, modes, below_a, below_b


def general_list(seed, name, n_pairs=300):
    a, b, seams_a, seams_b, modes, below_a, below_b = general_case(name)
    pairs = seam_pairs(seed, a, b, seams_a, seams_b, n_pairs, None if below_a is None else np.arange(below_a), None if below_b is None else np.arange(below_b))
    return a, b, pairs, modes


@pytest.mark.parametrize("name", list(GENERAL) + list(BATCHES))
def test_seams_of_the_flag_paths(lh, oracle, monkeypatch, name):
    a, b, pairs, modes = general_list(31, name)
    if name == "chunked_empty_chunks":
        assert not np.any((pairs[:, 0] >= C18) & (pairs[:, 0] < 3 * C18)) and np.sum(pairs[:, 0] >= 3 * C18) == 3
    ref = reference(oracle, a, b, pairs)
    with Session(lh, monkeypatch) as s:
        s.score(a, b, pairs, modes, ref, name)
        if name in BATCHES:
            assert s.sess.last_grid()[0]["build"] == PER_STRUCT_BUILD


# ---- stale flags ----------------------------------------------------------------------------------------------------------------
STALE = ["fused", "scan_stage_seam", "chunked_2p18_plus_1", "chunked_vs_itself", "batch_8_8", "batch_9_9", "batch_vs_single"]


@pytest.mark.parametrize("name", STALE)
def test_a_pass_behind_one_that_left_many_flags_set(lh, oracle, monkeypatch, name):
    """A pass that flags every atom (large clouds: an atom of every 32-atom word), then 50 pairs on the same clouds; then a pass on other,
    larger clouds -- the workspace is carved elsewhere -- and 50 other pairs."""
    if name == "fused":
        a, b, modes = fused_cloud(1, FUSED_ATOMS - 1), fused_cloud(2, FUSED_ATOMS), (FUSED, FUSED)
        small = [seam_pairs(seed, a, b, word_seams(a.n), word_seams(b.n), 50) for seed in (41, 42)]
    else:
        a, b, _, modes = general_list(41, name, 50)
        small = [general_list(seed, name, 50)[2] for seed in (41, 42)]
    other_a, other_b = cloud(50, a.n + 7001), cloud(51, b.n + 9001)
    refs = [reference(oracle, a, b, p) for p in small]
    with Session(lh, monkeypatch) as s:
        s.score(a, b, flood_pairs(a, b), modes, None, name + " flood")
        s.score(a, b, small[0], modes, refs[0], name + " 50 pairs")
        flood = flood_pairs(other_a, other_b)
        big = other_a.n > C18 or other_b.n > C18
        s.score(other_a, other_b, flood, (CHUNKED, CHUNKED) if big else (SCAN, SCAN), None, name + " other clouds")
        s.score(a, b, small[1], modes, refs[1], name + " 50 other pairs")


# ---- per pair -------------------------------------------------------------------------------------------------------------------
PER_PAIR_INPUTS = {
    "fused_sized": (lambda: fused_cloud(60, 3000), lambda: fused_cloud(61, 2500), FUSED),
    "per_structure": (lambda: cloud(20, [500] * 8), lambda: cloud(21, [500] * 8), SCAN),
    "general_sized": (lambda: cloud(62, 5000), lambda: cloud(63, 6000), SCAN),
}


def repeating_pairs(seed, a, b, n_pairs):
    """Side-B anchors: half of the list distinct, the other half drawn from 40 atoms."""
    rng = np.random.default_rng(seed)
    col_b = np.concatenate([rng.permutation(b.n)[:n_pairs // 2], rng.choice(rng.permutation(b.n)[:40], n_pairs - n_pairs // 2)])
    return np.stack([rng.integers(0, a.n, n_pairs), rng.permutation(col_b)], 1).astype(np.int64)


@pytest.mark.parametrize("name", list(PER_PAIR_INPUTS))
def test_forced_per_pair_counts(lh, oracle, monkeypatch, name):
    """LCHD_PER_PAIR=1: slot p belongs to pair p, the repeats are counted through a bit set in side B's flag region -- exactly, and the
    same number on every pass, whatever the passes before left in that region."""
    mk_a, mk_b, mode_a = PER_PAIR_INPUTS[name]
    a, b = mk_a(), mk_b()
    pairs = repeating_pairs(70, a, b, 300)
    assert expected_repeats(pairs) > 100
    ref = reference(oracle, a, b, pairs)
    with Session(lh, monkeypatch, "-1") as s:
        regular = [s.score(a, b, pairs, (mode_a, mode_a), ref, name + " regular") for _ in range(3)]
    with Session(lh, monkeypatch, "1") as s:
        forced = [s.score(a, b, pairs, (mode_a, PER_PAIR), ref, name + " per pair") for _ in range(3)]
        for f, r in zip(forced, regular):
            assert np.array_equal(f, r)  # the same environments, the same sweeps: the same bits
        s.score(a, b, flood_pairs(a, b), (mode_a, PER_PAIR), None, name + " flood")
        s.score(a, b, pairs[:50], (mode_a, PER_PAIR), reference(oracle, a, b, pairs[:50]), name + " 50 pairs")
        if name == "general_sized":  # above kDupSampleAbove pairs every 16th pair is counted, and the count scaled
            base = repeating_pairs(71, a, b, 2048)
            long_list = np.concatenate([np.tile(base, (DUP_SAMPLE // 2048, 1)), base[:16]])
            assert len(long_list) == DUP_SAMPLE + 16 and expected_repeats(long_list) % 16 == 0 and expected_repeats(long_list) > 0
            s.score(a, b, long_list, (mode_a, PER_PAIR), reference(oracle, a, b, long_list), name + " 2^17 + 16 pairs")
            s.score(a, b, pairs, (mode_a, PER_PAIR), ref, name + " per pair again")


def test_unforced_per_pair_sequence(lh, oracle, monkeypatch):
    """No hook: a regular pass on an (i, i) list finds every side-B anchor unique, the next pass gives every pair its own slot; a list
    that repeats a third of its side-B anchors is counted exactly by that mode, and the pass after it is a regular one again."""
    a, b = cloud(64, 5003), cloud(65, 5000)
    n = b.n
    once = np.stack([np.arange(n), np.arange(n)], 1).astype(np.int64)
    third = np.stack([np.arange(n), np.concatenate([np.arange(n - n // 3), np.arange(n // 3)])], 1).astype(np.int64)
    ref_once, ref_third = reference(oracle, a, b, once), reference(oracle, a, b, third)
    with Session(lh, monkeypatch) as s:
        first = s.score(a, b, once, (SCAN, SCAN), ref_once, "regular")
        assert s.sess.pass_counts()["per_pair_passes"] == 0
        assert np.array_equal(s.score(a, b, once, (SCAN, PER_PAIR), ref_once, "used once"), first)
        assert expected_repeats(third) == n // 3
        s.score(a, b, third, (SCAN, PER_PAIR), ref_third, "a third repeats")
        assert s.sess.pass_counts()["per_pair_passes"] == 2
        s.score(a, b, third, (SCAN, SCAN), ref_third, "regular again")
        assert s.sess.pass_counts()["per_pair_passes"] == 2


# ---- out-of-range anchors ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [FUSED, SCAN, CHUNKED, PER_PAIR])
def test_out_of_range_anchor_leaves_no_record(lh, oracle, monkeypatch, mode):
    """The validated-input path (a status flag, the reference's index panic): index n and index -1, once in each column."""
    import torch

    a, b = {FUSED: (fused_cloud(1, 4095), fused_cloud(2, 4096)), SCAN: (cloud(62, 5000), cloud(63, 6000)),
            CHUNKED: (cloud(8, C18 + 1), cloud(9, 3000)), PER_PAIR: (fused_cloud(60, 3000), fused_cloud(61, 2500))}[mode]
    good = seam_pairs(81, a, b, word_seams(a.n), word_seams(b.n), 200)
    ref = reference(oracle, a, b, good)
    modes = (FUSED, PER_PAIR) if mode == PER_PAIR else (mode, mode)
    with Session(lh, monkeypatch, "1" if mode == PER_PAIR else None) as s:
        for col, value in ((0, a.n), (0, -1), (1, b.n), (1, -1)):
            s.score(a, b, good, modes, ref, "in range")
            bad = good.copy()
            bad[117, col] = value
            with pytest.raises(lh.PanicException):
                s.sess.from_primitives(s.handle(a), s.handle(b), torch.from_numpy(bad).cuda(), THR)
            assert s.sess.last_anchors() is None and s.sess.last_grid() is None
        s.score(a, b, good, modes, ref, "the session keeps working")
