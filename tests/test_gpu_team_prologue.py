"""The per-tile work of the team sweeps AROUND the event loop (k_sweep_duo, loco_hd_amd/csrc/lchd_sweep_team.hip; merge_path,
lchd_kcommon.h): staging of the two lists into the team's buffer, the merge-path partition, the chunk-start counts.  It is integer and
address work only, so a rewrite of it must give the SAME BITS: every list here is scored by the team kernel of its form and compared
  * with the CPU oracle (<= 1e-11), and
  * with scores recorded by the library of the commit BEFORE the staging and the merge path were rewritten (np.array_equal;
    tests/golden/team_prologue/<form>_<list>.npy -- scores only, the inputs are rebuilt from the seeds here).

Star clouds as in test_gpu_team_batch.py: a star is an anchor on a lattice site (sites 3 thresholds apart) with n - 1 further atoms
inside the threshold, so its environment has exactly n points (asserted through the oracle's environment sizes).  Kinds of stars:
  rand   radii uniform in (lo, hi) x threshold
  comb   radii on a comb: tooth k of n at 0.5 + (2 k + phase) d -- two combs of phase 0 and 1 interleave point by point
  lat    atoms on the lattice 0.5 x (i, j, k) around the anchor, ONE per squared distance i^2 + j^2 + k^2: no tie inside a list, and
         between two such stars an exact tie across the lists wherever both hold the squared distance (all coordinates, differences and
         squares are exact).  Deterministic mode launches no team kernel (lchd_capi.hip), so these lists run in default mode, and ties
         INSIDE a list, whose stored order the environment kernels' atomics decide from run to run, are kept out of them.

Two forms: 8 categories / tiles of 240 events (four teams of 16 lanes), 10 categories (12 slots) / tiles of 480 events (two teams of 32).
With lim = tile / 2 + 1 two stars of lim points merge to exactly `tile` events: the staged buffer is used to its last entry; (lim - 1,
lim + 1), (lim - far, lim + far) -- far = 40 and 14: (227, 255) in the 480 form -- and their mirrors reach the limit with an odd and an even list A (the pad entry) and from either side.

Lists (LCHD_TEAM_BATCH forces the long lists' batch size onto these short ones, LCHD_NO_INLINE_META the record pass + team sweep):
  sizes     environments of 1 .. 6 points (the anchor alone, 1, 2, 3 .. points) against each other and against the stars at the limit, both
            ways round; the limit pairs; filler pairs of the form's typical size.  The list ends ONE pair behind a batch: a short last
            batch, in which one team has a pair and the others none.
  extremes  every key of A below every key of B and the reverse, the two combs both ways round (fully interleaved), fillers; ends five
            pairs behind a batch.
  ties      lattice stars against their twins of the other side (every key tied across the lists: A goes first), against another
            lattice star (some keys tied) and against random stars; prefix-count rows off (the per-tile histogram instantiation).
  dict      the sizes list under a dictionary of two weight functions, wf_index = p % 2.
"""
from pathlib import Path

import numpy as np
import pytest

from loco_hd_amd import _native as N

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "team_prologue"
THR = 10.0
TIGHT = 1e-11
SENTINEL = -7.0
FORMS = {
    240: dict(ncat=8, slots=8, teams=4, batch=32, rule=0, family=N.SWEEP_TEAM240),
    480: dict(ncat=10, slots=12, teams=2, batch=16, rule=2, family=N.SWEEP_TEAM480),
}
LISTS = ("sizes", "extremes", "ties", "dict")
N_FILL = 12


def lim_of(form):
    return form // 2 + 1


def far_of(form):
    """how far the lopsided limit pair (lim - far, lim + far) leans: the 480 form takes environments of at most 255 points"""
    return 40 if form == 240 else 14


def star_specs(form):
    """name -> (kind, points incl. the anchor, parameters); the same stars on both sides (other seeds)"""
    lim = lim_of(form)
    rng = np.random.default_rng(40 + form)
    specs = {f"s{n}": ("rand", n, (0.05, 0.95)) for n in range(1, 7)}
    for n in (lim - 1, lim, lim + 1, lim - far_of(form), lim + far_of(form)):
        specs[f"e{n}"] = ("rand", n, (0.05, 0.95))
    for k in range(N_FILL):
        specs[f"f{k}"] = ("rand", int(rng.integers(lim - 60, lim + 1)), (0.05, 0.95))
    specs["low"] = ("rand", lim - 20, (0.05, 0.45))
    specs["high"] = ("rand", lim - 19, (0.55, 0.95))
    specs["comb0"] = ("comb", lim - 10, 0)
    specs["comb1"] = ("comb", lim - 9, 1)
    specs["lat0"] = ("lat", lim - 10, 0)
    specs["lat1"] = ("lat", lim - 11, 1)
    return specs


def lattice_points(n, which, rng):
    """n lattice offsets 0.5 x (i, j, k), one per squared distance; star `which` of either side takes the same squared distances (a seeded
    choice among the sums of three squares up to 380: distances below 9.75), `rng` picks the representation"""
    g = np.stack(np.meshgrid(*[np.arange(-19, 20)] * 3, indexing="ij"), -1).reshape(-1, 3)
    d2 = (g * g).sum(1)
    values = np.unique(d2[(d2 > 0) & (d2 <= 380)])
    chosen = np.sort(np.random.default_rng(90 + which).permutation(values)[:n])
    return 0.5 * np.stack([g[rng.choice(np.flatnonzero(d2 == v))] for v in chosen]).astype(np.float64)


_clouds = {}


def cloud(form, side):
    """(xyz, categories, {star: anchor atom}, {star: points}) of side 0 (A) or 1 (B)"""
    if (form, side) not in _clouds:
        specs = star_specs(form)
        rng = np.random.default_rng(7000 + 10 * form + side)
        sites = np.stack(np.meshgrid(*[np.arange(5) * 3.0 * THR] * 3, indexing="ij"), -1).reshape(-1, 3)
        sites = sites[rng.permutation(len(sites))[:len(specs)]]
        xyz, anchor, size, at = [], {}, {}, 0
        for (name, (kind, n, par)), site in zip(specs.items(), sites):
            if kind == "lat":
                pts = site + lattice_points(n - 1, par, rng)  # (the two sides' stars of one name: the same distances, other directions)
            else:
                u = rng.normal(size=(n - 1, 3))
                u /= np.linalg.norm(u, axis=1, keepdims=True)
                if kind == "rand":
                    r = rng.uniform(par[0] * THR, par[1] * THR, n - 1)
                else:
                    r = 0.5 + (2.0 * np.arange(n - 1) + par) * (9.0 / (2 * n + 2))
                pts = site + u * r[:, None]
            xyz.append(np.concatenate([site[None], pts]))
            anchor[name], size[name] = at, n
            at += n
        xyz = np.concatenate(xyz)
        cats = rng.integers(0, FORMS[form]["ncat"], len(xyz)).astype(np.int32)
        _clouds[(form, side)] = (xyz, cats, anchor, size)
    return _clouds[(form, side)]


def name_list(form, which):
    """the list as (star of A, star of B) names"""
    lim, far, kb = lim_of(form), far_of(form), FORMS[form]["batch"]
    rng = np.random.default_rng(300 + form + LISTS.index(which))
    fill = [f"f{k}" for k in range(N_FILL)]
    small = [f"s{n}" for n in range(1, 7)]
    edge = [f"e{lim - 1}", f"e{lim}"]
    limit = [(f"e{lim}", f"e{lim}"), (f"e{lim - 1}", f"e{lim + 1}"), (f"e{lim + 1}", f"e{lim - 1}"),
             (f"e{lim - far}", f"e{lim + far}"), (f"e{lim + far}", f"e{lim - far}")]
    if which in ("sizes", "dict"):
        core = [(a, b) for a in small for b in small + edge] + [(a, b) for a in edge for b in small] + limit * 4
        tail = 1
    elif which == "extremes":
        core = [("low", "high"), ("high", "low"), ("comb0", "comb1"), ("comb1", "comb0"), ("comb0", "comb0"), ("low", "low")] * 8 + limit
        tail = 5
    else:
        core = ([("lat0", "lat0"), ("lat1", "lat1"), ("lat0", "lat1"), ("lat1", "lat0")] * 8 +
                [("lat0", f) for f in fill] + [(f, "lat1") for f in fill] + limit)
        tail = 3
    # fillers: most of the list (they decide the form's rule on the device), every (filler, filler) pair in a seeded order
    pairs_f = [(a, b) for a in fill for b in fill]
    n_fill = 24 * len(core)
    filler = [pairs_f[k] for k in np.concatenate([rng.permutation(len(pairs_f)) for _ in range(-(-n_fill // len(pairs_f)))])[:n_fill]]
    names = core + filler
    names = [names[k] for k in rng.permutation(len(names))]
    return names[:(len(names) // kb - 1) * kb + tail]  # the last batch: `tail` pairs


def make_list(form, which):
    """dict(pairs, nA, nB, wf_index)"""
    names = name_list(form, which)
    (_, _, anchor_a, size_a), (_, _, anchor_b, size_b) = cloud(form, 0), cloud(form, 1)
    pairs = np.asarray([[anchor_a[a], anchor_b[b]] for a, b in names], dtype=np.int64)
    nA, nB = np.asarray([size_a[a] for a, _ in names]), np.asarray([size_b[b] for _, b in names])
    wfi = (np.arange(len(pairs)) % 2).astype(np.int32) if which == "dict" else None
    return dict(pairs=pairs, nA=nA, nB=nB, wf_index=wfi)


def build(mod, form, which):
    wf = mod.WeightFunction("hyper_exp", [1.0, 0.1])
    if which == "dict":
        wf = {"h": wf, "u": mod.WeightFunction("uniform", [1.0, 9.0])}
    return mod.LoCoHD([f"c{i}" for i in range(FORMS[form]["ncat"])], wf)


def environment(form, which):
    """the hooks of a case, as environment variables"""
    env = {"LCHD_NO_INLINE_META": "1", "LCHD_TEAM_BATCH": str(FORMS[form]["batch"])}
    env["LCHD_PRE_ROWS"] = "-1" if which == "ties" else "1"
    return env


def gpu_scores(lh, form, which, passes=2):
    """scores and last_sweep() records of `passes` calls of one session (the first lets the device pick the rule, the second is hinted)"""
    import torch
    from loco_hd_amd.device import DeviceSession

    case = make_list(form, which)
    (xa, ca, _, _), (xb, cb, _, _) = cloud(form, 0), cloud(form, 1)
    sess = DeviceSession(build(lh, form, which))
    a, b = sess.upload(xa, ca), sess.upload(xb, cb)
    d_pairs = torch.from_numpy(case["pairs"]).cuda()
    wfi = None if case["wf_index"] is None else torch.from_numpy(case["wf_index"]).cuda()
    outs, swept = [], []
    for _ in range(passes):
        out = torch.full((len(case["pairs"]),), SENTINEL, dtype=torch.float64, device="cuda")
        sess.from_primitives(a, b, d_pairs, THR, out=out, wf_index=wfi)
        outs.append(out.cpu().numpy())
        swept.append(sess.last_sweep())
    sess.close()
    return outs, swept


def oracle_scores(orc, form, which):
    case = make_list(form, which)
    (xa, ca, _, _), (xb, cb, _, _) = cloud(form, 0), cloud(form, 1)
    lo = build(orc, form, which)
    lo.n_threads = 8
    wfs = idx = None
    if which == "dict":
        names = list(lo.w_func)
        wfs, idx = lo._wfs([names[k] for k in case["wf_index"]], len(case["pairs"]))
    want, sizes = lo.from_arrays(xa, ca, np.zeros(len(xa), dtype=np.int32), xb, cb, np.zeros(len(xb), dtype=np.int32), case["pairs"], THR,
                                 wfs=wfs, wf_idx=idx, return_env_sizes=True)
    return np.asarray(want), np.asarray(sizes)


@pytest.mark.parametrize("which", LISTS)
@pytest.mark.parametrize("form", sorted(FORMS))
def test_prologue_keeps_the_bits(form, which, oracle, monkeypatch):
    import loco_hd_amd as lh

    for k, v in environment(form, which).items():
        monkeypatch.setenv(k, v)
    f, lim, far, case = FORMS[form], lim_of(form), far_of(form), make_list(form, which)
    nA, nB, n = case["nA"], case["nB"], len(case["pairs"])
    T = nA + nB - 2
    # the list is what the docstring says: everything fits the form's tile, most pairs are the form's own, the last batch is short
    assert 1000 <= n <= 4096 and T.max() == form and max(nA.max(), nB.max()) <= 255
    assert n % f["batch"] in (1, 3, 5)
    if form == 480:
        assert 2 * np.count_nonzero(T <= 240) < n
    if which in ("sizes", "dict"):
        have = set(zip(nA.tolist(), nB.tolist()))
        assert {(a, b) for a in (1, 2, 3, 4) for b in (1, 2, 3, 4)} <= have
        assert {(lim, lim), (lim - 1, lim + 1), (lim + 1, lim - 1), (lim - far, lim + far), (lim + far, lim - far), (1, lim), (lim, 1), (2, lim - 1)} <= have
    want, sizes = oracle_scores(oracle, form, which)
    assert np.array_equal(sizes, np.stack([nA, nB], 1)), "the stars do not have their sizes"

    outs, swept = gpu_scores(lh, form, which)
    for rec in swept:
        assert rec is not None and rec["families"] & f["family"] and rec["rule"] == f["rule"] and rec["slots"] == f["slots"], rec
        assert rec["team_mode"] == 0 and rec["pre"] == (0 if which == "ties" else 1), rec
        assert rec[f"team_batch{form}"] == f["batch"], rec
    assert swept[-1]["forced"] == 1 and swept[-1]["left"] == 0, swept[-1]
    golden = np.load(GOLDEN / f"{form}_{which}.npy")
    for k, got in enumerate(outs):
        err = float(np.max(np.abs(got - want)))
        differ = int(np.count_nonzero(got.view(np.uint64) != golden.view(np.uint64))) if got.shape == golden.shape else -1
        print(f"{form} {which} pass {k}: {n} pairs, max |gpu - oracle| = {err:.3e}, scores whose bits differ from the fixture: {differ}")
        assert not np.isnan(got).any() and not (got == SENTINEL).any()
        assert err <= TIGHT
    assert golden.dtype == np.float64
    for got in outs:
        assert np.array_equal(got, golden)
