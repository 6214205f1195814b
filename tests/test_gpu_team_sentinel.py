"""The ends of the two staged lists in the team sweeps (k_sweep_duo, loco_hd_amd/csrc/lchd_sweep_team.hip; TeamTile::run,
lchd_team_tile.h).  The event loop merges the lists with ONE compare of their heads; a list that has ended shows by the sentinel key
~0 behind its last point (sA[mA], sB[mB]), written by the staging.  The change is integer and address work only, so every list here
is scored by the team kernel of its form and compared
  * with the CPU oracle (<= 1e-13), and
  * with scores recorded by the library of the commit BEFORE the sentinels (np.array_equal; tests/golden/team_sentinel/<form>_<case>.npy
    -- scores only, the inputs are rebuilt here).

Stars: an anchor on a lattice site (sites 30 apart, threshold 10) and one atom per radius k / 32 on the axis k % 3 -- coordinates,
differences, squares and roots are all exact, so two stars that share a k have an exact tie ACROSS the lists, and no list has a tie
inside (deterministic mode launches no team kernel, and the stored order of ties inside a list is decided by atomics).  The radii
k = 33 .. 287 lie strictly inside `uniform`'s (1, 9); k = 288 is its upper bound and k = 304 lies beyond it: both get F = 1 = F(+inf),
the largest real key, and a star holds at most one of them.

Stars (the same ones on both sides, other categories):
  n0 .. n3      0 .. 3 points (the sentinel is the only entry of an empty list); n1 .. n3 share k = 160
  e<m>          m points: m = tile / 2 - 1, tile / 2, tile / 2 + 1 -- (e, e) pairs fill the buffer to tile and tile - 1 events with an
                even and an odd list A (pad widths 2 and 1)
  low, high     every key of `low` below every key of `high`: the lanes whose run ends exactly at a list's end
  tlo, thi      the last key of `tlo` is the first of `thi`: ties across the lists at their ends
  ia, ib        random stars that end in k = 304 and k = 288
  f0 .. f7      fillers of the form's typical size (they decide the form's rule on the device)
  big           254 points: (big, big) has 508 events, too long for either tile -- the companion sweep's

Cases, for both forms (8 categories / 240 events / teams of 16; 10 categories, 12 slots / 480 events / teams of 32):
  h2      the special pairs and fillers, hyper_exp            nopre   the same without prefix-count rows (the per-tile histogram)
  uni     uniform(1, 9): the last keys of ia, ib are F(+inf)  mixed   one list with pairs too long for the tile and unusable pairs
  dict    two weight functions, wf_index = p % 2              ksm     Kolmogorov-Smirnov
  wgt     category weights                                    c25     25 categories (28 slots: the counts in LDS bytes)
With more than 16 slots the library sweeps the short pairs with the 480-event kernel too: 240-c25 runs the 240 form's lists through
`k_sweep_duo<28, 32, 480>`.  A call with unusable pairs fails like the reference and leaves no sweep record: `mixed` first scores its
usable pairs alone (the record; a pair's bits do not depend on its partners), then the whole list twice.
"""
import numpy as np
import pytest
from golden_util import GOLD

from loco_hd_amd import _native as N

pytestmark = pytest.mark.gpu

GOLDEN = GOLD / "team_sentinel"
THR = 10.0
TIGHT = 1e-13
SENTINEL = -7.0
GRID = np.arange(33, 288)  # 255 radii k / 32 strictly inside (1, 9)
K_BOUND, K_BEYOND = 288, 304
FORMS = {
    240: dict(ncat=8, slots=8, batch=32, rule=0, family=N.SWEEP_TEAM240, tile=240, fill=(50, 110)),
    480: dict(ncat=10, slots=12, batch=16, rule=2, family=N.SWEEP_TEAM480, tile=480, fill=(135, 235)),
}
CASES = ("h2", "nopre", "uni", "mixed", "dict", "ksm", "wgt", "c25")


def star_keys(form):
    """name -> sorted radii numerators k"""
    half = form // 2
    rng = np.random.default_rng(1600 + form)
    pick = lambda m: np.sort(rng.permutation(GRID)[:m])
    keys = {"n0": GRID[:0], "n1": np.array([160]), "n2": np.array([100, 160]), "n3": np.array([160, 200, 260])}
    for m in (half - 1, half, half + 1):
        keys[f"e{m}"] = pick(m)
    keys["low"], keys["high"] = GRID[:half - 8], GRID[half - 8:2 * half - 17]
    keys["tlo"], keys["thi"] = GRID[10:half // 2 + 10], GRID[half // 2 + 9:half + 5]
    keys["ia"] = np.append(pick(half - 30), K_BEYOND)
    keys["ib"] = np.append(pick(half - 31), K_BOUND)
    lo, hi = FORMS[form]["fill"]
    for k in range(8):
        keys[f"f{k}"] = pick(int(rng.integers(lo, hi + 1)))
    keys["big"] = GRID[:254]
    return keys


_clouds = {}


def cloud(form, ncat, side):
    """(xyz, categories, {star: anchor atom}, {star: points incl. the anchor}) of side 0 (A) or 1 (B)"""
    if (form, ncat, side) not in _clouds:
        keys = star_keys(form)
        rng = np.random.default_rng(8800 + 10 * form + side)
        sites = 30.0 * np.stack(np.meshgrid(*[np.arange(3)] * 3, indexing="ij"), -1).reshape(-1, 3)
        sites = sites[rng.permutation(len(sites))[:len(keys)]]
        xyz, anchor, size, at = [], {}, {}, 0
        for (name, ks), site in zip(keys.items(), sites):
            pts = np.tile(site, (len(ks), 1))
            pts[np.arange(len(ks)), ks % 3] += ks / 32.0
            xyz.append(np.concatenate([site[None], pts]))
            anchor[name], size[name] = at, len(ks) + 1
            at += len(ks) + 1
        xyz = np.concatenate(xyz)
        cats = np.random.default_rng(8900 + 10 * form + side + ncat).integers(0, ncat, len(xyz)).astype(np.int32)
        _clouds[(form, ncat, side)] = (xyz, cats, anchor, size)
    return _clouds[(form, ncat, side)]


def special_pairs(form):
    half = form // 2
    tiny = ["n0", "n1", "n2", "n3"]
    e = [f"e{half - 1}", f"e{half}", f"e{half + 1}"]
    pairs = [(a, b) for a in tiny for b in tiny]
    pairs += [(a, b) for a in tiny for b in e[:2]] + [(a, b) for a in e[:2] for b in tiny]
    # tile events with an even and an odd list A, tile - 1 events with an even and an odd list A
    pairs += [(e[1], e[1]), (e[0], e[2]), (e[2], e[0]), (e[1], e[0]), (e[0], e[1])]
    pairs += [("low", "high"), ("high", "low"), ("tlo", "thi"), ("thi", "tlo"), ("low", "low"), ("tlo", "tlo")]
    pairs += [("ia", "ib"), ("ib", "ia"), ("ia", "ia"), ("ib", "ib"), ("ia", "n0"), ("n0", "ib"), ("ia", "high"), ("high", "ib")]
    return pairs


def name_list(form, case):
    """the list as (star of A, star of B, usable) -- `mixed`: pairs too long for the tile and unusable pairs inside the batches"""
    rng = np.random.default_rng(500 + form + CASES.index(case))
    core = special_pairs(form)
    fill = [(f"f{a}", f"f{b}") for a in range(8) for b in range(8)]
    names = [(a, b, True) for a, b in core + [fill[k] for k in rng.permutation(len(fill))] + fill[:len(core)]]
    if case == "mixed":
        names += [("big", "big", True), ("big", "f0", True), ("f1", "big", True)] * 3 + [("n1", "n1", False)] * 7
    names = [names[k] for k in rng.permutation(len(names))]
    return names


def config_of(form, case):
    ncat = 25 if case == "c25" else FORMS[form]["ncat"]
    return ncat, (28 if case == "c25" else FORMS[form]["slots"])


def kernel_of(form, case):
    """the form whose team kernel sweeps the case's lists"""
    return FORMS[480 if case == "c25" else form]


def build(mod, form, case):
    ncat, _ = config_of(form, case)
    wf, kw = mod.WeightFunction("hyper_exp", [1.0, 0.1]), {}
    if case == "uni":
        wf = mod.WeightFunction("uniform", [1.0, 9.0])
    if case == "dict":
        wf = {"h": wf, "u": mod.WeightFunction("uniform", [1.0, 9.0])}
    if case == "ksm":
        kw["statistical_distance"] = mod.StatisticalDistance("Kolmogorov-Smirnov", [])
    if case == "wgt":
        kw["category_weights"] = list(0.5 + 0.25 * np.arange(ncat))
    return mod.LoCoHD([f"c{i}" for i in range(ncat)], wf, **kw)


def make_list(form, case):
    """dict(pairs, ok, nA, nB, wf_index)"""
    ncat, _ = config_of(form, case)
    names = name_list(form, case)
    (xa, _, anchor_a, size_a), (_, _, anchor_b, size_b) = cloud(form, ncat, 0), cloud(form, ncat, 1)
    ok = np.asarray([u for _, _, u in names])
    pairs = np.asarray([[anchor_a[a] if u else len(xa), anchor_b[b]] for a, b, u in names], dtype=np.int64)  # unusable: no such atom
    nA, nB = np.asarray([size_a[a] for a, _, _ in names]), np.asarray([size_b[b] for _, b, _ in names])
    wfi = (np.arange(len(pairs)) % 2).astype(np.int32) if case == "dict" else None
    return dict(pairs=pairs, ok=ok, nA=nA, nB=nB, wf_index=wfi)


def environment(form, case):
    """the hooks of a case, as environment variables: the record pass + team sweep, the long lists' batch size on these short ones"""
    return {"LCHD_NO_INLINE_META": "1", "LCHD_TEAM_BATCH": str(FORMS[form]["batch"]), "LCHD_PRE_ROWS": "-1" if case == "nopre" else "1"}


def gpu_scores(lh, form, case, passes=2):
    """scores and last_sweep() records of `passes` calls of one session (the first lets the device pick the rule, the second is hinted)"""
    import torch
    from loco_hd_amd.device import DeviceSession

    ncat, _ = config_of(form, case)
    lst = make_list(form, case)
    (xa, ca, _, _), (xb, cb, _, _) = cloud(form, ncat, 0), cloud(form, ncat, 1)
    sess = DeviceSession(build(lh, form, case))
    a, b = sess.upload(xa, ca), sess.upload(xb, cb)
    d_pairs = torch.from_numpy(lst["pairs"]).cuda()
    wfi = None if lst["wf_index"] is None else torch.from_numpy(lst["wf_index"]).cuda()
    outs, swept, usable = [], [], None
    if not lst["ok"].all():  # the usable pairs alone first: a failing call leaves no record
        usable = sess.from_primitives(a, b, torch.from_numpy(lst["pairs"][lst["ok"]]).cuda(), THR).cpu().numpy()
        swept.append(sess.last_sweep())
    for _ in range(passes):
        out = torch.full((len(lst["pairs"]),), SENTINEL, dtype=torch.float64, device="cuda")
        if lst["ok"].all():
            sess.from_primitives(a, b, d_pairs, THR, out=out, wf_index=wfi)
            swept.append(sess.last_sweep())
        else:  # the call fails like the reference; NaN stands at the unusable pairs and nowhere else
            with pytest.raises(lh.PanicException):
                sess.from_primitives(a, b, d_pairs, THR, out=out, wf_index=wfi)
        outs.append(out.cpu().numpy())
    sess.close()
    return outs, swept, usable


def oracle_scores(orc, form, case):
    """the usable pairs' scores and environment sizes"""
    ncat, _ = config_of(form, case)
    lst = make_list(form, case)
    (xa, ca, _, _), (xb, cb, _, _) = cloud(form, ncat, 0), cloud(form, ncat, 1)
    lo = build(orc, form, case)
    lo.n_threads = 8
    pairs = lst["pairs"][lst["ok"]]
    wfs = idx = None
    if case == "dict":
        names = list(lo.w_func)
        wfs, idx = lo._wfs([names[k] for k in lst["wf_index"][lst["ok"]]], len(pairs))
    want, sizes = lo.from_arrays(xa, ca, np.zeros(len(xa), dtype=np.int32), xb, cb, np.zeros(len(xb), dtype=np.int32), pairs, THR,
                                 wfs=wfs, wf_idx=idx, return_env_sizes=True)
    return np.asarray(want), np.asarray(sizes)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("form", sorted(FORMS))
def test_list_ends_keep_the_bits(form, case, oracle, monkeypatch):
    import loco_hd_amd as lh

    for k, v in environment(form, case).items():
        monkeypatch.setenv(k, v)
    f, half, lst = FORMS[form], form // 2, make_list(form, case)
    ok, nA, nB, n = lst["ok"], lst["nA"], lst["nB"], len(lst["pairs"])
    T = nA + nB - 2
    # the list is what the docstring says
    assert 100 <= n <= 400 and max(nA.max(), nB.max()) <= 255
    fits = T <= form
    assert T[fits].max() == form and (ok.all() and fits.all()) == (case != "mixed")
    if form == 480:
        assert 2 * np.count_nonzero(T <= 240) < n
    have = set(zip((nA - 1).tolist(), (nB - 1).tolist()))
    assert {(a, b) for a in range(4) for b in range(4)} <= have
    assert {(half, half), (half - 1, half + 1), (half + 1, half - 1), (half, half - 1), (half - 1, half)} <= have
    want, sizes = oracle_scores(oracle, form, case)
    assert np.array_equal(sizes, np.stack([nA, nB], 1)[ok]), "the stars do not have their sizes"

    outs, swept, usable = gpu_scores(lh, form, case)
    _, slots = config_of(form, case)
    kf = kernel_of(form, case)
    for rec in swept:
        print(rec)
        assert rec is not None and rec["families"] & kf["family"] and rec["rule"] == kf["rule"] and rec["slots"] == slots, rec
        assert rec["team_mode"] == {"wgt": 1, "ksm": 2}.get(case, 0), rec
        assert rec["pre"] == (0 if case in ("nopre", "wgt", "c25") else 1), rec
        assert rec[f"team_batch{kf['tile']}"] == f["batch"], rec
    if case != "mixed":  # (the hinted pass; `mixed` has the record of a session's first call only)
        assert swept[-1]["forced"] == 1 and swept[-1]["left"] == 0, swept[-1]
    golden = np.load(GOLDEN / f"{form}_{case}.npy")
    if usable is not None:
        assert np.array_equal(usable, golden[ok])
    for k, got in enumerate(outs):
        err = float(np.max(np.abs(got[ok] - want)))
        differ = int(np.count_nonzero(got.view(np.uint64) != golden.view(np.uint64))) if got.shape == golden.shape else -1
        print(f"{form} {case} pass {k}: {n} pairs, max |gpu - oracle| = {err:.3e}, scores whose bits differ from the fixture: {differ}")
        assert np.array_equal(np.isnan(got), ~ok) and not (got == SENTINEL).any()
        assert err <= TIGHT
    assert golden.dtype == np.float64
    for got in outs:
        assert np.array_equal(got, golden, equal_nan=True)
