"""Which kernel sorts the dense rows of from_dmxs / from_coords / the dense ensembles (plan_dense, loco_hd_amd/csrc/lchd_dense_plan.h) is
read back through lchd_ctx_last_dense and ASSERTED here against literal expectations, one case each side of every row-length and
category-width limit of the three launchers, on the default path and with LCHD_NO_DENSE_FUSED.  Every case also compares the scores with
the CPU oracle (1e-11), fills `out` with a sentinel beforehand and looks for survivors, and calls twice and requires equal bits; where
both paths run they agree within 1e-13.  tests/test_dense_plan.py holds the planner itself against the kernels' template parameters."""
import ctypes as C

import numpy as np
import pytest

from dense_plan_util import BIG32K, BIG64K, HUGE128K, ROWS, fused, rows, rows2, side
from dense_rows_util import oracle_rows

pytestmark = pytest.mark.gpu

TIGHT = 1e-11
PATHS_AGREE = 1e-13
SENTINEL = -7.25  # no score: LoCoHD lies in [0, 1]
NAMES = [f"c{i}" for i in range(300)]
WF = ("hyper_exp", [1.0, 0.1])
ONCE = dict(attempts=1, canon=False, n_bitonic=0)


@pytest.fixture(scope="module")
def lh():
    import loco_hd_amd

    return loco_hd_amd


def make(lh, n_cat, **kw):
    return lh.LoCoHD(NAMES[:n_cat], lh.WeightFunction(*WF), **kw)


def record(lchd):
    from loco_hd_amd.device import last_dense_of

    return last_dense_of(lchd._context())


def check_record(lchd, want):
    got = record(lchd)
    assert got is not None
    assert {k: got[k] for k in want} == want, got


def call_dmxs(lchd, cat_a, cat_b, rows_a, rows_b):
    """lchd_from_dmxs (lchd_from_dmxs_ragged for rows of unequal length) into a sentinel-filled `out`, twice: equal bits, no survivor."""
    from loco_hd_amd import _native as N

    lens_a, lens_b = [len(r) for r in rows_a], [len(r) for r in rows_b]
    ragged = len(set(lens_a)) > 1 or len(set(lens_b)) > 1
    ma, mb = np.zeros((len(rows_a), max(lens_a))), np.zeros((len(rows_b), max(lens_b)))
    for m, rws in ((ma, rows_a), (mb, rows_b)):
        for k, r in enumerate(rws):
            m[k, : len(r)] = r
    ca, cb = np.ascontiguousarray(cat_a, dtype=np.int32), np.ascontiguousarray(cat_b, dtype=np.int32)
    cfg, keep = lchd._config()
    outs = []
    for _ in range(2):
        out = np.full(len(rows_a), SENTINEL)
        if ragged:
            la, lb = np.asarray(lens_a, dtype=np.int32), np.asarray(lens_b, dtype=np.int32)
            N.check(N.lib().lchd_from_dmxs_ragged(lchd._context(), C.byref(cfg), N.ip(ca), ca.size, N.ip(cb), cb.size, N.dp(ma), ma.shape[0],
                                                  ma.shape[1], N.ip(la), N.dp(mb), mb.shape[0], mb.shape[1], N.ip(lb), None, N.dp(out)))
        else:
            N.check(N.lib().lchd_from_dmxs(lchd._context(), C.byref(cfg), N.ip(ca), ca.size, N.ip(cb), cb.size, N.dp(ma), ma.shape[0],
                                           ma.shape[1], N.dp(mb), mb.shape[0], mb.shape[1], None, N.dp(out)))
        assert not np.any(out == SENTINEL) and np.all(np.isfinite(out))
        outs.append(out)
    assert np.array_equal(outs[0], outs[1])  # same call, same bits
    return outs[0]


def call_coords(lchd, cat_a, cat_b, xa, xb):
    from loco_hd_amd import _native as N

    ca, cb = np.ascontiguousarray(cat_a, dtype=np.int32), np.ascontiguousarray(cat_b, dtype=np.int32)
    xa, xb = np.ascontiguousarray(xa, dtype=np.float64), np.ascontiguousarray(xb, dtype=np.float64)
    cfg, keep = lchd._config()
    outs = []
    for _ in range(2):
        out = np.full(len(xa), SENTINEL)
        N.check(N.lib().lchd_from_coords(lchd._context(), C.byref(cfg), N.ip(ca), ca.size, N.ip(cb), cb.size, N.dp(xa), len(xa), N.dp(xb),
                                         len(xb), None, N.dp(out)))
        assert not np.any(out == SENTINEL) and np.all(np.isfinite(out))
        outs.append(out)
    assert np.array_equal(outs[0], outs[1])
    return outs[0]


def given_row(rng, n):
    """an exact 0, then n - 1 distinct distances in random order"""
    return np.concatenate([[0.0], rng.permutation(np.linspace(0.5, 60.0, n - 1)) if n > 1 else []])


def given_rows(rng, n, n_rows=3, inf_tail=True):
    rws = [given_row(rng, n) for _ in range(n_rows)]
    if inf_tail and n >= 8:
        rws[1][-3:] = np.inf  # python_codes/ensembles/compare_ensembles.py:261-263
    return rws


def names_of(cats):
    return [NAMES[k] for k in cats]


class Oracle:
    """the CPU oracle's scores of given rows, computed once per input"""

    def __init__(self, oracle, n_cat):
        self.lo = oracle.LoCoHD(NAMES[:n_cat], oracle.WeightFunction(*WF))

    def __call__(self, cat_a, cat_b, rows_a, rows_b):
        return oracle_rows(self.lo, names_of(cat_a), names_of(cat_b), rows_a, rows_b)


# ---- given rows: every length of the table, each side of each limit --------------------------------------------------------------
# length -> (record on the default path, record with LCHD_NO_DENSE_FUSED); 10 categories, Hellinger-2, unit weights
GIVEN = {
    1: (rows2(64, 16, 1, 64),) * 2,
    64: (rows2(64, 16, 1, 64),) * 2,
    65: (rows2(64, 16, 1, 128),) * 2,
    1024: (rows2(64, 16, 1, 1024),) * 2,
    1025: (fused(segs=3), rows2(256, 16, 1, 2048)),
    4096: (fused(segs=4), rows2(256, 16, 1, 4096)),
    4097: (fused(segs=4), rows2(1024, 8, 1, 8192)),
    8192: (fused(segs=6), rows2(1024, 8, 1, 8192)),
    8193: (fused(segs=6), rows2(1024, 10, 1, 16384)),
    10240: (fused(segs=6), rows2(1024, 10, 1, 16384)),
    10241: (fused(segs=6), rows2(1024, 16, 1, 16384)),
    16384: (fused(segs=9), rows2(1024, 16, 1, 16384)),
    16385: (fused(segs=9), rows2(1024, 12, 2, 16384)),
    20480: (fused(segs=10), rows2(1024, 12, 2, 16384)),
    20481: (rows(BIG32K),) * 2,
    65535: (rows(BIG64K),) * 2,
    65536: (rows(BIG64K),) * 2,
    65537: (rows(HUGE128K),) * 2,
}


@pytest.mark.parametrize("n", sorted(GIVEN))
def test_given_rows_each_side_of_every_length_limit(lh, oracle, monkeypatch, n):
    rng = np.random.default_rng(9000 + n)
    n_cat = 10
    cat_a, cat_b = rng.integers(0, n_cat, n), rng.integers(0, n_cat, n)
    ra, rb = given_rows(rng, n), given_rows(rng, n, inf_tail=False)
    want = Oracle(oracle, n_cat)(cat_a, cat_b, ra, rb)
    default = make(lh, n_cat)
    got = call_dmxs(default, cat_a, cat_b, ra, rb)
    check_record(default, {**GIVEN[n][0], **ONCE})
    print(f"n = {n}: default path, max |hip - oracle| = {np.max(np.abs(got - want)):.3e}")
    assert np.max(np.abs(got - want)) < TIGHT
    monkeypatch.setenv("LCHD_NO_DENSE_FUSED", "1")
    plain = make(lh, n_cat)
    old = call_dmxs(plain, cat_a, cat_b, ra, rb)
    check_record(plain, {**GIVEN[n][1], **ONCE})
    print(f"n = {n}: LCHD_NO_DENSE_FUSED, max |hip - oracle| = {np.max(np.abs(old - want)):.3e}, |paths| = {np.max(np.abs(old - got)):.3e}")
    assert np.max(np.abs(old - want)) < TIGHT
    assert np.max(np.abs(old - got)) < PATHS_AGREE


@pytest.mark.parametrize("n,want_side", [(1024, side(64, 0, 2048, 1024, 2)), (1025, side(1024, 0, 2048, 2048, 2)),
                                         (8192, side(1024, 0, 2048, 8192, 2)), (8193, side(1024, 1, 16384, 16384, 2))])
def test_given_rows_sixteen_bit_categories(lh, oracle, n, want_side):
    rng = np.random.default_rng(9300 + n)
    n_cat = 300
    cat_a, cat_b = rng.integers(0, n_cat, n), rng.integers(0, n_cat, n)
    cat_a[:2], cat_b[:2] = (299, 256), (255, 299)  # ids on both sides of the 8-bit limit are there
    ra, rb = given_rows(rng, n), given_rows(rng, n, inf_tail=False)
    lchd = make(lh, n_cat)
    got = call_dmxs(lchd, cat_a, cat_b, ra, rb)
    check_record(lchd, {**rows(want_side), **ONCE})
    want = Oracle(oracle, n_cat)(cat_a, cat_b, ra, rb)
    print(f"n = {n}, 300 categories: max |hip - oracle| = {np.max(np.abs(got - want)):.3e}")
    assert np.max(np.abs(got - want)) < TIGHT


# ---- unequal and ragged widths ---------------------------------------------------------------------------------------------------
SHORT16K = side(1024, 0, 2048, 16384)
UNEQUAL = [
    ((20480, 16384), fused(segs=10), rows(BIG32K, SHORT16K)),
    ((16385, 16384), fused(segs=9), rows(BIG32K, SHORT16K)),
    ((1025, 1), fused(segs=3), rows2(256, 16, 1, 2048)),
    ((20481, 1024), rows(BIG32K, side(64, 0, 2048, 1024)), rows(BIG32K, side(64, 0, 2048, 1024))),
]


@pytest.mark.parametrize("widths,want_default,want_plain", UNEQUAL, ids=[f"{a}x{b}" for (a, b), _, _ in UNEQUAL])
def test_unequal_widths(lh, oracle, monkeypatch, widths, want_default, want_plain):
    na, nb = widths
    rng = np.random.default_rng(9500 + na + nb)
    n_cat = 10
    cat_a, cat_b = rng.integers(0, n_cat, na), rng.integers(0, n_cat, nb)
    ra, rb = given_rows(rng, na), given_rows(rng, nb, inf_tail=False)
    want = Oracle(oracle, n_cat)(cat_a, cat_b, ra, rb)
    default = make(lh, n_cat)
    got = call_dmxs(default, cat_a, cat_b, ra, rb)
    check_record(default, {**want_default, **ONCE})
    assert np.max(np.abs(got - want)) < TIGHT
    monkeypatch.setenv("LCHD_NO_DENSE_FUSED", "1")
    plain = make(lh, n_cat)
    old = call_dmxs(plain, cat_a, cat_b, ra, rb)
    check_record(plain, {**want_plain, **ONCE})
    assert np.max(np.abs(old - want)) < TIGHT
    assert np.max(np.abs(old - got)) < PATHS_AGREE


def test_ragged_rows_longest_16385_shortest_1(lh, oracle, monkeypatch):
    """Rows of their own lengths (utils.rs:25-39): the longest has 16385 points, the shortest one.  A two-segment launch of k_env_rows2
    has one segment count for every row, so ragged rows beyond 16384 points go to k_env_rows."""
    rng = np.random.default_rng(9600)
    n_cat, n = 10, 16385
    cat = rng.integers(0, n_cat, n)
    ra = [given_row(rng, k) for k in (n, 1, 5000, 16384)]
    rb = [given_row(rng, k) for k in (1, n, n, 1025)]
    want = Oracle(oracle, n_cat)(cat, cat, ra, rb)
    default = make(lh, n_cat)
    got = call_dmxs(default, cat, cat, ra, rb)
    check_record(default, {**fused(segs=9), **ONCE})
    assert np.max(np.abs(got - want)) < TIGHT
    monkeypatch.setenv("LCHD_NO_DENSE_FUSED", "1")
    plain = make(lh, n_cat)
    old = call_dmxs(plain, cat, cat, ra, rb)
    check_record(plain, {**rows(BIG32K), **ONCE})
    assert np.max(np.abs(old - want)) < TIGHT
    assert np.max(np.abs(old - got)) < PATHS_AGREE


# ---- coordinates: rows = n ---------------------------------------------------------------------------------------------------------
def dist_row(x, i):
    d = x[i] - x
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])  # utils.rs:1-8 order


def coords_case(rng, n, n_cat):
    box = (n / 0.05) ** (1 / 3)
    return (rng.integers(0, n_cat, n), rng.uniform(0.0, box, (n, 3))), (rng.integers(0, n_cat, n), rng.uniform(0.0, box, (n, 3)))


def sampled_rows(rng, n):
    """rows 0, n - 1, 8 random ones and both sides of the fused kernel's 512-workgroup row stride"""
    return sorted({0, 511, 512, 513, n - 1} | set(rng.integers(0, n, 8).tolist()))


# n -> (record on the default path, record with LCHD_NO_DENSE_FUSED or None: the default path only)
COORDS = {
    1024: (rows2(64, 16, 1, 1024), rows2(64, 16, 1, 1024)),
    1025: (fused(dmx=0, segs=3), rows2(256, 16, 1, 2048)),
    4096: (fused(dmx=0, segs=4), rows2(256, 16, 1, 4096)),
    4097: (fused(dmx=0, segs=4), rows2(1024, 8, 1, 8192)),
    8192: (fused(dmx=0, segs=6), rows2(1024, 8, 1, 8192)),
    8193: (fused(dmx=0, segs=6), rows2(1024, 10, 1, 16384)),
    10240: (fused(dmx=0, segs=6), rows2(1024, 10, 1, 16384)),
    10241: (fused(dmx=0, segs=6), rows2(1024, 16, 1, 16384)),
    16384: (fused(dmx=0, segs=9), None),
    16385: (fused(dmx=0, segs=9), None),
    20480: (fused(dmx=0, segs=10), None),
    20481: (rows(BIG32K), None),
}


@pytest.mark.parametrize("n", sorted(COORDS))
def test_coordinates_each_side_of_every_length_limit(lh, oracle, monkeypatch, n):
    rng = np.random.default_rng(9700 + n)
    n_cat = 10
    (cat_a, xa), (cat_b, xb) = coords_case(rng, n, n_cat)
    sample = sampled_rows(rng, n)
    want = Oracle(oracle, n_cat)(cat_a, cat_b, [dist_row(xa, i) for i in sample], [dist_row(xb, i) for i in sample])
    default = make(lh, n_cat)
    got = call_coords(default, cat_a, cat_b, xa, xb)
    check_record(default, {**COORDS[n][0], **ONCE})
    print(f"n = {n}: default path, max |hip - oracle| = {np.max(np.abs(got[sample] - want)):.3e}")
    assert np.max(np.abs(got[sample] - want)) < TIGHT
    if COORDS[n][1] is None:
        return
    monkeypatch.setenv("LCHD_NO_DENSE_FUSED", "1")
    plain = make(lh, n_cat)
    old = call_coords(plain, cat_a, cat_b, xa, xb)
    check_record(plain, {**COORDS[n][1], **ONCE})
    assert np.max(np.abs(old[sample] - want)) < TIGHT
    assert np.max(np.abs(old - got)) < PATHS_AGREE


# ---- the bucket limit ------------------------------------------------------------------------------------------------------------
def tie_rows(n, ties, n_rows=3):
    """n equally spaced distances per row (every sort bucket holds one or two points); row 1 of side A has `ties` entries set to ONE
    value.  The tied points share a category, so their order cannot change a bit of the score."""
    base = np.arange(n, dtype=float) * 0.125
    ra, rb = [base.copy() for _ in range(n_rows)], [base.copy() for _ in range(n_rows)]
    lo = n // 3
    ra[1][lo:lo + ties] = base[lo]
    rng = np.random.default_rng(n + ties)
    cat_a, cat_b = rng.integers(0, 10, n), rng.integers(0, 10, n)
    cat_a[lo:lo + ties] = 3
    return cat_a, cat_b, ra, rb


@pytest.mark.parametrize("hook,want", [(None, rows2(64, 16, 1, 512)), ("LCHD_OLD_ROWS", rows(side(64, 0, 2048, 512)))])
@pytest.mark.parametrize("ties,bitonic", [(0, 0), (65, 1), (64, None)])
def test_bucket_limit_of_the_row_sorts(lh, oracle, monkeypatch, hook, want, ties, bitonic):
    """A bucket of more than kRowBucketLimit = 64 points sends its row to the bitonic network, in k_env_rows2 and (LCHD_OLD_ROWS) in
    k_env_rows: 65 equal distances must, one row, counted once; 64 need not (a neighbour may share the bucket): scores only."""
    if hook:
        monkeypatch.setenv(hook, "1")
    cat_a, cat_b, ra, rb = tie_rows(300, ties)
    lchd = make(lh, 10)
    got = call_dmxs(lchd, cat_a, cat_b, ra, rb)
    check_record(lchd, {**want, "attempts": 1, "canon": False})
    if bitonic is not None:
        assert record(lchd)["n_bitonic"] == bitonic
    assert np.max(np.abs(got - Oracle(oracle, 10)(cat_a, cat_b, ra, rb))) < TIGHT


def test_bucket_limit_defeats_the_fused_kernel(lh, oracle):
    """The same 65 ties in a 2000-point row: the fused kernel has no fallback for an overfull bucket, reports the row and the call is
    repeated; the repeat runs k_env_rows, whose bitonic network takes the row."""
    cat_a, cat_b, ra, rb = tie_rows(2000, 65)
    lchd = make(lh, 10)
    got = call_dmxs(lchd, cat_a, cat_b, ra, rb)
    check_record(lchd, {**rows(side(256, 0, 2048, 2048)), "attempts": 2, "canon": False, "n_bitonic": 1})
    assert np.max(np.abs(got - Oracle(oracle, 10)(cat_a, cat_b, ra, rb))) < TIGHT


def test_bucket_limit_defeats_the_two_segment_sort(lh, oracle, monkeypatch):
    """... and in a 17000-point row with LCHD_NO_DENSE_FUSED: k_env_rows2<1024, 12, 2> gives up, the repeat sorts the keys in the store."""
    monkeypatch.setenv("LCHD_NO_DENSE_FUSED", "1")
    cat_a, cat_b, ra, rb = tie_rows(17000, 65)
    lchd = make(lh, 10)
    got = call_dmxs(lchd, cat_a, cat_b, ra, rb)
    check_record(lchd, {**rows(BIG32K), "attempts": 2, "canon": False})
    assert record(lchd)["path"] == ROWS and record(lchd)["n_bitonic"] >= 1
    assert np.max(np.abs(got - Oracle(oracle, 10)(cat_a, cat_b, ra, rb))) < TIGHT


# ---- deterministic mode ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,want", [(3000, rows2(256, 16, 1, 4096)), (16385, rows2(1024, 12, 2, 16384)), (20481, rows(BIG32K))])
def test_deterministic_mode_runs_canon_on_every_path(lh, oracle, n, want):
    """Deterministic mode never takes the fused kernel; behind either row sort the tie-canonicalisation kernel runs.  Every distance
    occurs twice here, with different categories: two contexts give the same bits."""
    rng = np.random.default_rng(9800 + n)
    n_cat = 10
    cat_a, cat_b = rng.integers(0, n_cat, n), rng.integers(0, n_cat, n)

    def doubled():
        half = np.linspace(0.5, 60.0, n // 2)
        return np.concatenate([[0.0], rng.permutation(np.concatenate([half, half[: n - 1 - len(half)]]))])

    ra, rb = [doubled() for _ in range(3)], [doubled() for _ in range(3)]
    first, second = make(lh, n_cat, deterministic=True), make(lh, n_cat, deterministic=True)
    got = call_dmxs(first, cat_a, cat_b, ra, rb)
    check_record(first, {**want, "attempts": 1, "canon": True, "n_bitonic": 0})
    again = call_dmxs(second, cat_a, cat_b, ra, rb)
    check_record(second, {**want, "attempts": 1, "canon": True, "n_bitonic": 0})
    assert np.array_equal(got, again)
    assert np.max(np.abs(got - Oracle(oracle, n_cat)(cat_a, cat_b, ra, rb))) < TIGHT


# ---- the dense ensemble ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,want", [(16384, rows2(1024, 16, 1, 16384)), (16385, rows(BIG32K))])
def test_ensemble_of_two_structures(lh, oracle, n, want):
    """An ensemble call cannot be repeated: k_env_rows2 up to its one-segment limit, k_env_rows beyond.  Deterministic mode: the scores
    are the bits of from_coords on the same two structures (tests/test_gpu_ensemble.py)."""
    import torch

    from loco_hd_amd.device import DeviceSession

    rng = np.random.default_rng(9900 + n)
    n_cat = 10
    (cat, xa), (_, xb) = coords_case(rng, n, n_cat)
    sess = DeviceSession(make(lh, n_cat, deterministic=True))
    try:
        batch, _ = sess.upload_batch([(xa, cat), (xb, cat)])
        outs = []
        for _ in range(2):
            out = torch.full((1, n), SENTINEL, dtype=torch.float64, device="cuda")
            sess.from_coords_ensemble(batch, out=out)
            outs.append(out.cpu().numpy()[0])
        assert np.array_equal(outs[0], outs[1]) and not np.any(outs[0] == SENTINEL)
        got = sess.last_dense()
        assert {k: got[k] for k in want} == want and (got["attempts"], got["canon"], got["n_bitonic"]) == (1, True, 0), got
        a, b = sess.upload(xa, cat), sess.upload(xb, cat)
        pair = torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda")
        sess.from_coords(a, b, out=pair)
        assert np.array_equal(pair.cpu().numpy(), outs[0])
    finally:
        sess.close()
    sample = [0, 511, n - 1]
    ref = Oracle(oracle, n_cat)(cat, cat, [dist_row(xa, i) for i in sample], [dist_row(xb, i) for i in sample])
    assert np.max(np.abs(outs[0][sample] - ref)) < TIGHT
