"""The determinism contract of LoCoHD(..., deterministic=True) (lchd_ctx_set_deterministic) on inputs full of exact distance ties.

In deterministic mode an environment's stored (key, category) sequence is a function of the multiset of (distance, category) of its
points, its first point included (several points at distance 0 are ordered like any other tie).  k_env_canon makes it so: it sorts the categories
inside every run of equal keys, whatever order the cell lists' atomics, the row sorts' LDS atomics or the bitonic networks left them in.
Repeating a call ("run 20 times, same bits") only checks that contract when the atomics happen to complete in another order; PERMUTING
THE POINTS checks it every time: a permutation moves every point to another thread / cell-list slot / bucket position, so a tie run the
canon misses shows up as a bit difference.  So:

- from_primitives (host API and DeviceSession): points of both clouds permuted, anchor pairs remapped -> the same bits;
- from_coords: one permutation pi of both structures -> out'[k] == out[pi[k]] bit for bit;
- from_dmxs (square): rows and columns permuted jointly -> the same bits, permuted; one row longer than 20 480 points: columns permuted;
- from_dmxs (ragged: a column permutation does not keep the prefixes): the same bits across calls and contexts.

The tie shapes: integer-lattice coordinates; every point four times, with categories that overlap between the two structures
(zero-distance ties at the anchor: position 0 of an environment is whichever of them the sort placed first, and the sums of square
roots over them round differently in another order); matrix rows with groups of 0.0 and -0.0 entries; rows of length 2
that are both zeros; +inf runs of 63, 64, 65, 128, 129 and ~2 000 entries, one that starts at position 1 and ends at the row's last
entry; finite runs of hundreds of entries that cross 64-lane chunk boundaries; a uniform weight function whose threshold lies far
beyond x_max (the F = 1 tail: runs of ~2 000 equal CDF keys in from_primitives environments).  Category counts 7, 40 (8-bit ids,
k_sweep_wide), 255, 256 (the first with 16-bit ids), 300 and 600 (HUGE).

Every case is also checked against the CPU oracle (<= 1e-11, in deterministic and in default mode) and on a sample of pairs against
tests/integral_form.py (the score from its definition, long double: relative error <= 1e-12)."""
import itertools

import numpy as np
import pytest

import integral_form as iform

pytestmark = pytest.mark.gpu

TIGHT = 1e-11
IFORM_TOL = 1e-12
CATS = [7, 40, 255, 256, 300, 600]


@pytest.fixture(scope="module")
def lh():
    import loco_hd_amd

    return loco_hd_amd


def names(n_cat):
    return [f"c{i}" for i in range(n_cat)]


def pooled(rng, n_groups, n_cat, size=4):
    """Categories of n_groups groups of `size` points for two structures: both draw a group's categories from the same pair of
    categories, so the groups' category counts overlap and differ (3 + 1 against 2 + 2, ...).  Sums of sqrt(a_c * b_c) over such
    groups are irrational: the order in which the sweep meets the group's points shows in the last bits."""
    pool = np.stack([rng.choice(n_cat, 2, replace=False) for _ in range(n_groups)])
    pick = lambda: np.take_along_axis(pool, rng.integers(0, 2, (n_groups, size)), 1).reshape(-1).astype(np.int32)
    return pick(), pick()


def lattice_groups(rng, m, n_cat):
    """m^3 integer-lattice points, each of them four times (zero-distance ties at every anchor), the same coordinates for both
    structures, categories from pooled(); in a random order."""
    g = np.array(list(itertools.product(range(m), repeat=3)), dtype=float)
    ca, cb = pooled(rng, len(g), n_cat)
    p = rng.permutation(4 * len(g))
    return np.repeat(g, 4, axis=0)[p], ca[p], cb[p]


def inverse(p):
    inv = np.empty_like(p)
    inv[p] = np.arange(len(p))
    return inv


def assert_iform(got, want):
    want = np.asarray(want)
    assert np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))) < IFORM_TOL


def oracle_rows(o, sa, sb, rows_a, rows_b):
    """The oracle's from_anchors on every row pair, each row sorted the reference's way (a stable sort, utils.rs:25-39; row r
    is sorted with the prefix of seq it covers)."""
    def srt(seq, row):
        row = np.asarray(row, dtype=float) + 0.0
        k = np.argsort(row, kind="stable")
        return [seq[i] for i in k], row[k].tolist()

    out = []
    for a, b in zip(rows_a, rows_b):
        (qa, ea), (qb, eb) = srt(sa, a), srt(sb, b)
        out.append(o.from_anchors(qa, qb, ea, eb))
    return np.asarray(out)


# ---- from_primitives ---------------------------------------------------------------------------------------------------------
# hyper_exp within 3.2: ~460 points per environment, dozens of ties per distance shell; uniform [1, 2] within 5.0: ~2 000 points,
# every one beyond x_max = 2 at F = 1 (one run of equal CDF keys of nearly the whole environment)
PRIM_CASES = {"lattice": (("hyper_exp", [1.0, 0.3]), 3.2, 10, 400), "f1_tail": (("uniform", [1.0, 2.0]), 5.0, 11, 48)}


@pytest.mark.parametrize("case", list(PRIM_CASES))
@pytest.mark.parametrize("api", ["host", "session"])
@pytest.mark.parametrize("n_cat", CATS)
def test_from_primitives_is_invariant_under_point_permutation(lh, oracle, n_cat, api, case):
    import torch
    from loco_hd_amd import _native as N
    from loco_hd_amd.device import DeviceSession, last_sweep_of

    wf, thr, m, n_pairs = PRIM_CASES[case]
    rng = np.random.default_rng(7000 + n_cat + (1 if api == "host" else 0) + (2 if case == "f1_tail" else 0))
    cats = names(n_cat)
    xa, ca, cb = lattice_groups(rng, m, n_cat)
    xb = xa
    pairs = np.stack([rng.integers(0, len(xa), n_pairs), rng.integers(0, len(xb), n_pairs)], 1).astype(np.int64)
    pa, pb = rng.permutation(len(xa)), rng.permutation(len(xb))
    pairs_p = np.stack([inverse(pa)[pairs[:, 0]], inverse(pb)[pairs[:, 1]]], 1).astype(np.int64)

    def run(det, xa, ca, xb, cb, pairs):
        lchd = lh.LoCoHD(cats, lh.WeightFunction(*wf), deterministic=det)
        if api == "host":
            prim = lambda x, c: [lh.PrimitiveAtom(cats[k], "", p) for k, p in zip(c, x)]
            out = np.asarray(lchd.from_primitives(prim(xa, ca), prim(xb, cb), [tuple(p) for p in pairs.tolist()], thr))
            swept = last_sweep_of(lchd._ctx)
        else:
            sess = DeviceSession(lchd)
            a, b = sess.upload(xa, ca), sess.upload(xb, cb)
            out = sess.from_primitives(a, b, torch.from_numpy(pairs).cuda(), thr).cpu().numpy()
            swept = sess.last_sweep()
            sess.close()
        if det:  # ONE family whatever the call looks like: the plain sweep with global-memory tables (beyond 32 categories: the wide one)
            assert swept is not None and swept["families"] == (N.SWEEP_PLAIN if n_cat <= 32 else N.SWEEP_WIDE), swept
            assert swept["forced"] == 0 and swept["rule"] == -1 and (n_cat > 32 or swept["ldstab"] == 0), swept
        return out

    got = run(True, xa, ca, xb, cb, pairs)
    assert np.array_equal(run(True, xa[pa], ca[pa], xb[pb], cb[pb], pairs_p), got)
    tz = np.zeros(len(xa), dtype=np.int32)
    want = np.asarray(oracle.LoCoHD(cats, oracle.WeightFunction(*wf), n_of_threads=8).from_arrays(xa, ca, tz, xb, cb, tz, pairs, thr))
    assert np.max(np.abs(got - want)) < TIGHT
    assert np.max(np.abs(run(False, xa, ca, xb, cb, pairs) - want)) < TIGHT
    k = slice(0, 6)
    assert_iform(got[k], iform.from_primitives(ca, xa, None, cb, xb, None, pairs[k], thr, n_cat, wf))


def test_deterministic_300_categories_independent_of_batch_and_context(lh, oracle):
    """test_gpu_configs.py's batch / history check at 300 categories (16-bit ids, k_sweep_wide<CAT16>) on lattice groups: the same
    probe pairs alone and inside a large call, in two fresh contexts, give the same bits."""
    rng = np.random.default_rng(300300)
    n_cat = 300
    cats = names(n_cat)
    wf = ("hyper_exp", [1.0, 0.3])
    xa, ca, cb = lattice_groups(rng, 9, n_cat)
    xb = xa
    prim = lambda x, c: [lh.PrimitiveAtom(cats[k], "", p) for k, p in zip(c, x)]
    la, lb = prim(xa, ca), prim(xb, cb)
    probes = [(int(i), int(j)) for i, j in zip(rng.integers(0, len(xa), 40), rng.integers(0, len(xb), 40))]
    big = [(int(i), int(j)) for i, j in zip(rng.integers(0, len(xa), 6000), rng.integers(0, len(xb), 6000))]
    big[2500:2540] = probes
    outs = []
    for _ in range(2):
        det = lh.LoCoHD(cats, lh.WeightFunction(*wf), deterministic=True)
        outs.append(np.asarray(det.from_primitives(la, lb, probes, 3.5)))
        outs.append(np.asarray(det.from_primitives(la, lb, big, 3.5))[2500:2540])
    for o in outs[1:]:
        assert np.array_equal(o, outs[0])
    tz = np.zeros(len(xa), dtype=np.int32)
    want = np.asarray(oracle.LoCoHD(cats, oracle.WeightFunction(*wf), n_of_threads=8).from_arrays(xa, ca, tz, xb, cb, tz, np.asarray(probes), 3.5))
    assert np.max(np.abs(outs[0] - want)) < TIGHT


# ---- from_coords ---------------------------------------------------------------------------------------------------------------
ROW_KERNELS = [(n, old) for n in CATS for old in (False, True) if not (old and n > 255)]  # (16-bit ids: k_env_rows only)


@pytest.mark.parametrize("n_cat,old_rows", ROW_KERNELS)
def test_from_coords_is_invariant_under_point_permutation(lh, oracle, monkeypatch, n_cat, old_rows):
    """216 lattice points, each four times: every row holds four points at distance 0 (the anchor and its copies) -- position 0 of
    a sorted row is one of them -- and dozens of ties per distance shell."""
    if old_rows:
        monkeypatch.setenv("LCHD_OLD_ROWS", "1")  # k_env_rows instead of k_env_rows2 (read when the context is created)
    rng = np.random.default_rng(8000 + n_cat + old_rows)
    cats = names(n_cat)
    wf = ("hyper_exp", [1.0, 0.3])
    xa, ca, cb = lattice_groups(rng, 6, n_cat)
    xb = xa
    sa, sb = [cats[k] for k in ca], [cats[k] for k in cb]
    det = lh.LoCoHD(cats, lh.WeightFunction(*wf), deterministic=True)
    got = np.asarray(det.from_coords(sa, sb, xa, xb))
    p = rng.permutation(len(xa))
    got_p = np.asarray(lh.LoCoHD(cats, lh.WeightFunction(*wf), deterministic=True).from_coords([sa[i] for i in p], [sb[i] for i in p], xa[p], xb[p]))
    assert np.array_equal(got_p, got[p])
    want = np.asarray(oracle.LoCoHD(cats, oracle.WeightFunction(*wf), n_of_threads=8).from_coords(sa, sb, xa, xb))
    assert np.max(np.abs(got - want)) < TIGHT
    assert np.max(np.abs(np.asarray(lh.LoCoHD(cats, lh.WeightFunction(*wf)).from_coords(sa, sb, xa, xb)) - want)) < TIGHT
    rows = rng.choice(len(xa), 8, replace=False)
    assert_iform(got[rows], [iform.score(ca, np.sqrt(iform._sqdist(xa[r], xa)), cb, np.sqrt(iform._sqdist(xb[r], xb)), n_cat, wf) for r in rows])


# ---- from_dmxs -----------------------------------------------------------------------------------------------------------------
INF_RUNS = [63, 64, 65, 128, 129, 2000]


def tie_matrix(rng, n):
    """n x n, points in groups of four (columns 4g .. 4g + 3): 0.0 or -0.0 between the members of a group, six distance levels
    elsewhere (runs of ~n / 6 equal entries per row, across 64-lane chunk boundaries), +inf runs of every length of INF_RUNS, and
    one row of nothing but +inf after its diagonal zero (a run from position 1 to the row's last entry)."""
    d = rng.integers(1, 7, (n, n)).astype(float)
    group = np.arange(n) // 4
    same = group[:, None] == group[None, :]
    d[same] = np.where(rng.integers(0, 2, int(same.sum())) == 1, -0.0, 0.0)
    rows = rng.permutation(n)
    for r, length in zip(rows, INF_RUNS * 3):
        cols = rng.permutation(np.nonzero(~same[r])[0])[:length]
        d[r, cols] = np.inf
    full = rows[len(INF_RUNS) * 3]
    d[full] = np.inf
    d[full, full] = 0.0
    return d


@pytest.mark.parametrize("n_cat,old_rows", ROW_KERNELS)
def test_from_dmxs_square_is_invariant_under_joint_row_and_column_permutation(lh, oracle, monkeypatch, n_cat, old_rows):
    if old_rows:
        monkeypatch.setenv("LCHD_OLD_ROWS", "1")
    rng = np.random.default_rng(9000 + n_cat + old_rows)
    cats = names(n_cat)
    wf = ("hyper_exp", [1.0, 0.5])
    n = 2052
    da, db = tie_matrix(rng, n), tie_matrix(rng, n)
    ga, gb = pooled(rng, n // 4, n_cat)
    sa, sb = [cats[k] for k in ga], [cats[k] for k in gb]
    got = np.asarray(lh.LoCoHD(cats, lh.WeightFunction(*wf), deterministic=True).from_dmxs(sa, sb, da, db))
    p = rng.permutation(n)
    got_p = lh.LoCoHD(cats, lh.WeightFunction(*wf), deterministic=True).from_dmxs([sa[i] for i in p], [sb[i] for i in p],
                                                                                    da[p][:, p], db[p][:, p])
    assert np.array_equal(np.asarray(got_p), got[p])
    # the oracle on the rows with +inf runs and a sample of the rest (rows are independent)
    rows = np.unique(np.concatenate([np.where(np.isinf(da).any(1) | np.isinf(db).any(1))[0], rng.choice(n, 48, replace=False)]))
    want = np.asarray(oracle.LoCoHD(cats, oracle.WeightFunction(*wf), n_of_threads=8).from_dmxs(sa, sb, da[rows], db[rows]))
    assert np.max(np.abs(got[rows] - want)) < TIGHT
    assert np.max(np.abs(np.asarray(lh.LoCoHD(cats, lh.WeightFunction(*wf)).from_dmxs(sa, sb, da, db))[rows] - want)) < TIGHT
    ia, ib = np.asarray([cats.index(s) for s in sa]), np.asarray([cats.index(s) for s in sb])
    sample = np.concatenate([rows[:12], rows[-12:]])
    assert_iform(got[sample], [iform.score(ia, da[r], ib, db[r], n_cat, wf) for r in sample])


@pytest.mark.parametrize("n_cat", CATS)
def test_from_dmxs_rows_of_two_zeros(lh, oracle, n_cat):
    """Rows of length 2 that are both zeros (0.0 / -0.0): the whole environment is one run of equal keys from position 0.  Swapping
    the two columns (and their categories) gives the same bits."""
    rng = np.random.default_rng(9500 + n_cat)
    cats = names(n_cat)
    wf = ("hyper_exp", [1.0, 0.5])
    rows = 512
    za = np.where(rng.integers(0, 2, (rows, 2)) == 1, -0.0, 0.0)
    zb = np.where(rng.integers(0, 2, (rows, 2)) == 1, -0.0, 0.0)
    c = rng.choice(n_cat, 4, replace=False)
    sa, sb = [cats[c[0]], cats[c[1]]], [cats[c[2]], cats[c[3]]]
    det = lh.LoCoHD(cats, lh.WeightFunction(*wf), deterministic=True)
    got = np.asarray(det.from_dmxs(sa, sb, za, zb))
    assert np.array_equal(np.asarray(det.from_dmxs(sa[::-1], sb[::-1], za[:, ::-1].copy(), zb[:, ::-1].copy())), got)
    want = np.asarray(oracle.LoCoHD(cats, oracle.WeightFunction(*wf)).from_dmxs(sa, sb, za, zb))
    assert np.max(np.abs(got - want)) < TIGHT
    assert_iform(got[:4], [iform.score(c[:2], za[r], c[2:], zb[r], n_cat, wf) for r in range(4)])


@pytest.mark.parametrize("n_cat", CATS)
def test_from_dmxs_ragged_rows_give_the_same_bits_across_calls_and_contexts(lh, oracle, n_cat):
    rng = np.random.default_rng(9700 + n_cat)
    cats = names(n_cat)
    wf = ("hyper_exp", [1.0, 0.5])
    lens = [2, 3, 64, 65, 66, 129, 130, 1500] + rng.integers(2, 1500, 56).tolist()
    width = max(lens)

    def rows():
        out = []
        for k, length in enumerate(lens):
            r = rng.integers(1, 7, length).astype(float)
            r[0] = 0.0
            if length == 2 or k % 3 == 0:
                r[1] = -0.0 if k % 2 else 0.0  # (length 2: both zeros)
            n_inf = min(length - 2, [63, 64, 65, 128, 129, 1000][k % 6])
            if n_inf > 0:
                r[2 + rng.permutation(length - 2)[:n_inf]] = np.inf
            out.append(rng.permutation(r).tolist())
        return out

    ra, rb = rows(), rows()
    sa, sb = rng.choice(cats, width).tolist(), rng.choice(cats, width).tolist()
    got = [np.asarray(lh.LoCoHD(cats, lh.WeightFunction(*wf), deterministic=True).from_dmxs(sa, sb, ra, rb)) for _ in range(2)]
    det = lh.LoCoHD(cats, lh.WeightFunction(*wf), deterministic=True)
    got += [np.asarray(det.from_dmxs(sa, sb, ra, rb)) for _ in range(2)]
    for g in got[1:]:
        assert np.array_equal(g, got[0])
    o = oracle.LoCoHD(cats, oracle.WeightFunction(*wf))
    want = oracle_rows(o, sa, sb, ra, rb)
    assert np.max(np.abs(got[0] - want)) < TIGHT
    assert np.max(np.abs(np.asarray(lh.LoCoHD(cats, lh.WeightFunction(*wf)).from_dmxs(sa, sb, ra, rb)) - want)) < TIGHT
    ia, ib = np.asarray([cats.index(s) for s in sa]), np.asarray([cats.index(s) for s in sb])
    assert_iform(got[0][:12], [iform.score(ia[:len(a)], a, ib[:len(b)], b, n_cat, wf) for a, b in zip(ra[:12], rb[:12])])


def long_rows(rng, n_rows, n, n_inf):
    """n_rows x n: 0.0, -0.0, 0.0, -0.0 in columns 0 .. 3, six distance levels and n_inf +inf entries in the others."""
    d = rng.integers(1, 7, (n_rows, n)).astype(float)
    d[:, :4] = [0.0, -0.0, 0.0, -0.0]
    for r in range(n_rows):
        d[r, 4 + rng.permutation(n - 4)[:n_inf]] = np.inf
    return d


@pytest.mark.parametrize("n_cat,n,n_inf,n_rows", [(40, 21000, 2000, 3), (300, 20500, 20000, 2), (300, 40000, 2000, 1)])
def test_from_dmxs_long_rows_are_invariant_under_column_permutation(lh, oracle, n_cat, n, n_inf, n_rows):
    """Rows longer than 20 480 points (8-bit ids: keys sorted in global memory); rows of 20 500 points with 16-bit ids of which
    20 000 are +inf (one run of equal keys that the wavefront counts in two levels); a row of 40 000 points with 16-bit ids (a store
    stride of 65 536: still the 16-bit-id sweep, not the 64-bit-count one).  Permuting the columns and their categories gives the
    same bits."""
    rng = np.random.default_rng(9900 + n_cat + n_inf)
    cats = names(n_cat)
    wf = ("hyper_exp", [1.0, 0.5])
    da, db = long_rows(rng, n_rows, n, n_inf), long_rows(rng, n_rows, n, n_inf)
    sa, sb = rng.choice(cats, n).tolist(), rng.choice(cats, n).tolist()
    ga, gb = pooled(rng, 1, n_cat)  # (the zero columns: categories that overlap)
    sa[:4], sb[:4] = [cats[k] for k in ga], [cats[k] for k in gb]
    got = np.asarray(lh.LoCoHD(cats, lh.WeightFunction(*wf), deterministic=True).from_dmxs(sa, sb, da, db))
    p = rng.permutation(n)
    got_p = lh.LoCoHD(cats, lh.WeightFunction(*wf), deterministic=True).from_dmxs([sa[i] for i in p], [sb[i] for i in p],
                                                                                    da[:, p].copy(), db[:, p].copy())
    assert np.array_equal(np.asarray(got_p), got)
    o = oracle.LoCoHD(cats, oracle.WeightFunction(*wf))
    want = oracle_rows(o, sa, sb, da, db)
    assert np.max(np.abs(got - want)) < TIGHT
    assert np.max(np.abs(np.asarray(lh.LoCoHD(cats, lh.WeightFunction(*wf)).from_dmxs(sa, sb, da, db)) - want)) < TIGHT
    if n * n_cat <= 10_000_000:  # (the integral form holds n x C long doubles per side)
        ia, ib = np.asarray([cats.index(s) for s in sa]), np.asarray([cats.index(s) for s in sb])
        assert_iform(got, [iform.score(ia, a, ib, b, n_cat, wf) for a, b in zip(da, db)])
