"""Which sweep kernels score a pass (plan_sweep / launch_sweep, loco_hd_amd/csrc/lchd_kernels.hip) is read back through
DeviceSession.last_sweep() and ASSERTED here, on inputs whose environment sizes are exact by construction, with pairs on both sides of
every limit of the dispatch: 240 / 241 merged events, 480 / 481 events, 255 / 256 points, and the majority tests 2 n >= P at their ties.

Star clouds: star i is an anchor atom on a lattice site (sites 3 thresholds apart) with m_i further atoms at radius (0.05 .. 0.95) x
threshold around it, so its environment has exactly m_i + 1 points whatever the cell grid or the strictness of the comparison; only star
centres are anchors.  A pair list is written as (n_A, n_B) pairs over the size table, so every count the record must show -- pairs of at
most 240 events, pairs of the 8-bit-count rule, the largest environment, the pairs left to the companion -- is computed here in numpy
from the table and never read back from the library.  The sizes themselves are checked against the CPU oracle's.

Every case holds the literal family set, instantiation and rule of each pass of one session (pass 1 has no hint, later passes launch what
the previous pass counted).  Every pass: the record equals the table, the counts equal numpy's, the scores lie within 1e-11 of the CPU
oracle, `out` was filled with a sentinel before the call and none survives.  Passes 2 and 3 agree bit for bit, pass 1 with them in the
unit-weight Hellinger-2 cases.  A last call per case appends one out-of-range anchor: it raises like the reference, NaN stands at that
pair and nowhere else (whichever family is in force writes it), and the session keeps no record of such a call.

A pair with an unusable anchor ends the call with an error before the record is kept, so the three recorded passes carry none;
test_unusable_pair_has_one_nan_writer puts such pairs into passes without a hint (every candidate kernel launched) and into a pass
whose companion was left out."""
import numpy as np
import pytest

from loco_hd_amd import _native as N

pytestmark = pytest.mark.gpu

THR = 10.0
TIGHT = 1e-11
SENTINEL = -7.0
SIZES = (1, 2, 3, 120, 121, 122, 123, 200, 226, 227, 228, 240, 241, 242, 243, 254, 255, 256, 257)  # points per environment, anchor included
T240, T480, C8, IND, PLAIN, INC, WIDE, INLINE = (N.SWEEP_TEAM240, N.SWEEP_TEAM480, N.SWEEP_C8, N.SWEEP_INDIRECT, N.SWEEP_PLAIN, N.SWEEP_INC,
                                                 N.SWEEP_WIDE, N.SWEEP_INLINE)

EDGE = [(121, 121), (121, 122), (122, 121), (1, 241), (241, 1), (1, 242), (242, 1),                      # 240 / 241 events
        (241, 241), (241, 242), (255, 227), (227, 255), (255, 228), (256, 226), (226, 256), (255, 255),   # 480 / 481 events,
        (256, 1), (1, 256), (257, 257),                                                                   # 255 / 256 points
        (1, 1), (1, 2), (3, 1)]                                                                           # tiny
SMALL, C8ONLY, LARGE = (120, 121), (200, 226), (256, 257)  # padding: 239 events; 424 events; beyond every small rule


def is_small(rule, na, nb):
    """pair_is_small (lchd_team_tile.h) on arrays"""
    if rule == 0:
        return na + nb - 2 <= 240
    c8 = np.maximum(na, nb) <= 255
    return c8 if rule == 1 else c8 & (na + nb - 2 <= 480)


def padded(*parts):
    """[(pair, count) | list of pairs ...] -> int64 [P][2] of (n_A, n_B)"""
    out = []
    for part in parts:
        out += [part[0]] * part[1] if isinstance(part, tuple) and isinstance(part[0], tuple) else list(part)
    return np.asarray(out, dtype=np.int64)


def tie_list(rule, k, pad_in):
    """EDGE + x pairs of pad_in + 2100 LARGE ones with 2 * (pairs of `rule`) == P - k"""
    e = np.asarray(EDGE)
    n_e, y = int(is_small(rule, e[:, 0], e[:, 1]).sum()), 2100
    x = len(EDGE) + y - k - 2 * n_e
    sizes = padded(EDGE, (pad_in, x), (LARGE, y))
    assert 2 * int(is_small(rule, sizes[:, 0], sizes[:, 1]).sum()) == len(sizes) - k
    return sizes


L_SMALL, L_C8, L_LARGE = padded(EDGE, (SMALL, 4200)), padded(EDGE, (C8ONLY, 4200)), padded(EDGE, (LARGE, 4200))
ALL_SMALL = padded([(1, 1), (1, 2), (3, 1), (121, 121), (1, 241), (241, 1)], (SMALL, 4200))            # every pair <= 240 events
ALL_C8 = padded([(1, 1), (241, 241), (255, 227), (227, 255), (121, 122), (1, 242)], (C8ONLY, 4200))    # every pair of rule 2, few of rule 0


_clouds = {}


def star_cloud(seed):
    """(xyz, {size: anchor atom index})"""
    if seed not in _clouds:
        rng = np.random.default_rng(seed)
        sites = np.stack(np.meshgrid(*[np.arange(3) * 3.0 * THR] * 3, indexing="ij"), -1).reshape(-1, 3)
        sites = sites[rng.permutation(len(sites))[:len(SIZES)]]
        xyz, anchor, at = [], {}, 0
        for size, site in zip(SIZES, sites):
            u = rng.normal(size=(size - 1, 3))
            r = rng.uniform(0.05 * THR, 0.95 * THR, size - 1)
            xyz.append(np.concatenate([site[None], site + u / np.linalg.norm(u, axis=1, keepdims=True) * r[:, None]]))
            anchor[size] = at
            at += size
        _clouds[seed] = (np.concatenate(xyz), anchor)
    return _clouds[seed]


XA, ANCHOR_A = star_cloud(4101)
XB, ANCHOR_B = star_cloud(4102)
assert len(XA) == len(XB) == sum(SIZES) < 4000


def anchors_of(sizes):
    return np.stack([[ANCHOR_A[a] for a in sizes[:, 0]], [ANCHOR_B[b] for b in sizes[:, 1]]], 1).astype(np.int64)


# ---- what a pass must show ---------------------------------------------------------------------------------------------------------
def no_hint_16(rule, **kw):   # up to 16 slots, no hint: both team rules, the companion, the plain sweep; the device decides
    return dict(families=T240 | IND | T480 | PLAIN, forced=0, small_rule=0, second_rule=2, c8_rule=2, left_listing=0, companion_left_out=0, rule=rule, **kw)


def no_hint_32(rule, **kw):   # 17 .. 32 slots, no hint: only the 480-event team form exists
    return dict(families=T480 | IND | PLAIN, forced=0, small_rule=2, second_rule=0, c8_rule=2, left_listing=0, companion_left_out=0, rule=rule, **kw)


def hint_duo(**kw):           # the previous pass had a majority of pairs of at most 240 events
    return dict(families=T240 | IND, forced=1, small_rule=0, second_rule=0, c8_rule=2, left_listing=1, companion_left_out=0, rule=0, **kw)


def hint_team480(**kw):       # ... of pairs of rule 2 (and, up to 16 slots, not of rule 0)
    return dict(families=T480 | IND, forced=1, small_rule=2, second_rule=0, c8_rule=2, left_listing=1, companion_left_out=0, rule=2, **kw)


def hint_plain(**kw):         # ... of neither
    return dict(families=PLAIN, forced=1, left_listing=0, companion_left_out=0, rule=-1, **kw)


def same_3(rec):
    return [rec, rec, rec]


H2 = dict(team_mode=0, plain_mode=0)
KSM = dict(sd=("Kolmogorov-Smirnov", []))
KL = dict(sd=("Kullback-Leibler", [1e-10]))
WEIGHTS = dict(weights=True)
DICT = dict(wf_dict=True)

# id -> dict(ncat, cfg, env, lists (one per pass), expect (one per pass), bitwise_1 (pass 1 must equal pass 2 bit for bit))
CASES = {}


def case(name, ncat, lists, expect, cfg=None, env=None, bitwise_1=False, passes=None):
    lists = lists if isinstance(lists, list) else [lists] * len(expect)
    assert name not in CASES and len(lists) == len(expect)
    CASES[name] = dict(ncat=ncat, lists=lists, expect=expect, cfg=cfg or {}, env=env or {}, bitwise_1=bitwise_1, passes=passes or [1] * len(expect))


for ncat, slots in ((8, 8), (12, 12), (16, 16)):  # a majority of pairs of at most 240 events
    case(f"h2_{ncat}_small", ncat, L_SMALL, [no_hint_16(0, slots=slots, pre=1, **H2)] + [hint_duo(slots=slots, pre=1, **H2)] * 2, bitwise_1=True)
case("h2_12_c8", 12, L_C8, [no_hint_16(2, slots=12, pre=1, **H2)] + [hint_team480(slots=12, pre=1, **H2)] * 2, bitwise_1=True)
case("h2_12_large", 12, L_LARGE, [no_hint_16(-1, slots=12, pre=1, **H2)] + [hint_plain(slots=12, pre=0, ldstab=1, **H2)] * 2, bitwise_1=True)
# exact ties of the majority tests: the device (pass 1) and the host (the hint of pass 2) must land on the same side
case("tie_duo_P", 12, tie_list(0, 0, SMALL), [no_hint_16(0, slots=12)] + [hint_duo()] * 2, bitwise_1=True)
# (two short of a majority under rule 0 -- but every such pair is one of rule 2 as well, and the edge pairs hold seven more of those)
case("tie_duo_P-2", 12, tie_list(0, 2, SMALL), [no_hint_16(2, slots=12)] + [hint_team480()] * 2, bitwise_1=True)
case("tie_c8_P", 12, tie_list(2, 0, C8ONLY), [no_hint_16(2, slots=12)] + [hint_team480()] * 2, bitwise_1=True)
case("tie_c8_P-2", 12, tie_list(2, 2, C8ONLY), [no_hint_16(-1, slots=12)] + [hint_plain()] * 2, bitwise_1=True)
for ncat, slots in ((17, 20), (20, 20), (24, 24), (28, 28), (32, 32)):  # only the 480-event team form; without it the one-pair 8-bit kernel
    case(f"h2_{ncat}", ncat, L_SMALL, [no_hint_32(2, slots=slots, pre=0, **H2)] + [hint_team480(slots=slots, pre=0, **H2)] * 2, bitwise_1=True)
    c8 = dict(small_rule=1, second_rule=0, c8_rule=1, companion_left_out=0, rule=1, slots=slots, pre=0, team_mode=0)
    case(f"h2_{ncat}_no_c8_team", ncat, L_SMALL,
         [dict(families=C8 | IND | PLAIN, forced=0, left_listing=0, **c8)] + [dict(families=C8 | IND, forced=1, left_listing=1, **c8)] * 2,
         env={"LCHD_NO_C8_TEAM": "1"})
for ncat in (12, 16):  # category weights: the weighted team forms (no prefix-count-row instantiation)
    w = dict(slots=ncat, pre=0, team_mode=1, plain_mode=1)
    case(f"weights_{ncat}", ncat, L_SMALL, [no_hint_16(0, **w)] + [hint_duo(**w)] * 2, cfg=WEIGHTS)
case("ksm_12", 12, L_SMALL, [no_hint_16(0, slots=12, pre=1, team_mode=2, plain_mode=2)] + [hint_duo(slots=12, pre=1, team_mode=2)] * 2, cfg=KSM)
# the distances without a team form: the incremental sweep, and the generic one where a weight-function dictionary names one per pair
for ncat, slots in ((10, 12), (24, 24)):
    case(f"kl_{ncat}", ncat, L_SMALL, same_3(dict(families=INC, slots=slots, forced=0, rule=-1, left_listing=0, companion_left_out=0)), cfg=KL)
    case(f"kl_{ncat}_dict", ncat, L_SMALL, same_3(dict(families=PLAIN, slots=slots, forced=0, rule=-1, plain_mode=2, ldstab=0)), cfg={**KL, **DICT})
case("hellinger_3", 10, L_SMALL, same_3(dict(families=PLAIN, slots=12, forced=0, rule=-1, plain_mode=2, ldstab=0)), cfg=dict(sd=("Hellinger", [3.0])))
case("wide_33", 33, L_SMALL, same_3(dict(families=WIDE, slots=0, forced=0, rule=-1, plain_mode=0, wide_long=0, left_listing=0, c8_rule=1)))  # (no 480-event team beyond 32 slots: n_c8 counts rule 1)
# 4096 pairs: one launch, no record pass, nothing counted; one pair more: the pipeline
case("pairs_4096", 12, L_SMALL[:4096], same_3(dict(families=INLINE, slots=12, rule=-1, forced=0, n_duo=-1, n_c8=-1, max_env=-1, left=-1)))
case("pairs_4097", 12, L_SMALL[:4097], [no_hint_16(0, slots=12)] + [hint_duo()] * 2, bitwise_1=True)
# the left-out companion: every pair of pass 1 was small, pass 2 leaves the companion out and stands; pass 3 brings ONE pair beyond the
# rule: the host must notice, repeat the pass with the companion (two passes for one call), and that pair's score must be right
case("left_out_240", 12, [ALL_SMALL, ALL_SMALL, padded(ALL_SMALL, [(122, 121)])],
     [no_hint_16(0, slots=12, repeated=False),
      dict(families=T240, forced=1, small_rule=0, left_listing=0, companion_left_out=1, rule=0, left=0, repeated=False),
      hint_duo(left=1, repeated=True)], passes=[1, 1, 2], bitwise_1=True)
case("left_out_480", 20, [ALL_C8, ALL_C8, padded(ALL_C8, [(255, 228)])],
     [no_hint_32(2, slots=20, repeated=False),
      dict(families=T480, forced=1, small_rule=2, c8_rule=2, left_listing=0, companion_left_out=1, rule=2, left=0, repeated=False),
      hint_team480(left=1, repeated=True)], passes=[1, 1, 2], bitwise_1=True)
# the hint follows the workload: small -> c8 -> large -> small -> small on one session; each pass runs what the PREVIOUS one counted
case("transitions", 12, [L_SMALL, L_C8, L_LARGE, L_SMALL, L_SMALL],
     [no_hint_16(0, slots=12), hint_duo(slots=12), hint_team480(slots=12), hint_plain(slots=12), hint_duo(slots=12)])


def build(mod, c):
    ncat, cfg = c["ncat"], c["cfg"]
    kw = {}
    if cfg.get("weights"):
        kw["category_weights"] = list(0.5 + 0.25 * np.arange(ncat))
    if "sd" in cfg:
        kw["statistical_distance"] = mod.StatisticalDistance(*cfg["sd"])
    wf = mod.WeightFunction("hyper_exp", [1.0, 0.1])
    if cfg.get("wf_dict"):
        wf = {"h": wf, "u": mod.WeightFunction("uniform", [1.0, 9.0])}
    return mod.LoCoHD([f"c{i}" for i in range(ncat)], wf, **kw)


def expected_counts(rec, sizes):
    """n_duo, n_c8, max_env, left of a recorded pass -- from the size table alone"""
    na, nb = sizes[:, 0], sizes[:, 1]
    rule = rec["rule"]
    return dict(n_duo=int(is_small(0, na, nb).sum()), n_c8=int(is_small(rec.get("c8_rule", 2), na, nb).sum()), max_env=int(sizes.max()),
                left=-1 if rule < 0 else int((~is_small(rule, na, nb)).sum()))


@pytest.mark.parametrize("name", list(CASES))
def test_sweep_dispatch(name, oracle, monkeypatch):
    import torch

    import loco_hd_amd as lh
    from loco_hd_amd.device import DeviceSession

    c = CASES[name]
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(500 + c["ncat"])
    ca, cb = rng.integers(0, c["ncat"], len(XA)).astype(np.int32), rng.integers(0, c["ncat"], len(XB)).astype(np.int32)
    tag = np.zeros(len(XA), dtype=np.int32)
    lo = build(oracle, c)
    lo.n_threads = 8
    lchd = build(lh, c)
    names = list(lchd.w_func) if c["cfg"].get("wf_dict") else None

    wants = {}

    def reference(sizes):
        """oracle scores of a list (computed once per distinct list of the case), its environment sizes checked against the table"""
        key = id(sizes)
        if key not in wants:
            pairs = anchors_of(sizes)
            wfs, idx, wf_index = None, None, None
            if names:
                keys = [names[p % 2] for p in range(len(pairs))]
                wfs, idx = lo._wfs(keys, len(pairs))
                wf_index = np.asarray([names.index(k) for k in keys], dtype=np.int32)
            want, got_sizes = lo.from_arrays(XA, ca, tag, XB, cb, tag, pairs, THR, wfs=wfs, wf_idx=idx, return_env_sizes=True)
            assert np.array_equal(np.asarray(got_sizes), sizes), "the stars do not have the sizes of the table"
            wants[key] = (pairs, np.asarray(want), wf_index)
        return wants[key]

    sess = DeviceSession(lchd)
    a, b = sess.upload(XA, ca), sess.upload(XB, cb)
    outs = []
    for k, (sizes, rec) in enumerate(zip(c["lists"], c["expect"])):
        pairs, want, wf_index = reference(sizes)
        assert len(pairs) > 4096 or name == "pairs_4096"
        out = torch.full((len(pairs),), SENTINEL, dtype=torch.float64, device="cuda")
        before = sess.pass_counts()["passes"]
        sess.from_primitives(a, b, torch.from_numpy(pairs).cuda(), THR, out=out, wf_index=None if wf_index is None else torch.from_numpy(wf_index).cuda())
        got, seen = out.cpu().numpy(), sess.last_sweep()
        assert seen is not None
        counts = expected_counts(rec, sizes)
        err = float(np.max(np.abs(got - want)))
        print(f"{name} pass {k + 1}: families {seen['families']:#x} slots {seen['slots']} rule {seen['rule']} n_duo {seen['n_duo']} n_c8 {seen['n_c8']} "
              f"left {seen['left']} of {len(pairs)} pairs; max |gpu - oracle| = {err:.3e}")
        assert {f: seen[f] for f in rec} == rec, (k + 1, seen)
        if seen["families"] != INLINE:
            assert {f: seen[f] for f in counts} == counts, (k + 1, seen)
        assert sess.pass_counts()["passes"] - before == c["passes"][k], k + 1
        assert not np.isnan(got).any() and not (got == SENTINEL).any()
        assert err <= TIGHT, (k + 1, err)
        outs.append((sizes, got))
    # the same list under the same hint: the same bits
    for k in range(1, len(outs) - 1):
        if outs[k][0] is outs[k + 1][0] and c["expect"][k] == c["expect"][k + 1]:
            assert np.array_equal(outs[k][1], outs[k + 1][1]), (k + 1, k + 2)
    if c["bitwise_1"]:
        assert np.array_equal(outs[0][1], outs[1][1])
    # one unusable pair (an anchor index one past the structure) in the last list: the call fails like the reference, NaN stands there and
    # only there -- some launched kernel must own the pair --, every other score is still right, and no record is kept of such a call
    sizes = c["lists"][-1]
    pairs, want, wf_index = reference(sizes)
    at = len(pairs) // 2
    bad = np.insert(pairs, at, [len(XA), 0], axis=0)
    bad_wf = None if wf_index is None else torch.from_numpy(np.insert(wf_index, at, 0)).cuda()
    out = torch.full((len(bad),), SENTINEL, dtype=torch.float64, device="cuda")
    with pytest.raises(lh.PanicException):
        sess.from_primitives(a, b, torch.from_numpy(bad).cuda(), THR, out=out, wf_index=bad_wf)
    got = out.cpu().numpy()
    assert np.isnan(got[at]) and not np.isnan(np.delete(got, at)).any() and not (got == SENTINEL).any()
    assert float(np.max(np.abs(np.delete(got, at) - want))) <= TIGHT
    assert sess.last_sweep() is None
    sess.close()


# The NaN writer of the passes the fourth call above does not reach: a pass WITHOUT a hint (every candidate launched; under the rule the
# device finds in force exactly one of them must own the unusable pair) and a pass whose companion was left out.
NAN_CASES = {
    "no_hint_rule_0": (12, {}, [L_SMALL]),
    "no_hint_rule_2": (12, {}, [L_C8]),
    "no_hint_plain": (12, {}, [L_LARGE]),
    "no_hint_rule_2_20_slots": (20, {}, [L_SMALL]),
    "no_hint_rule_1": (20, {"LCHD_NO_C8_TEAM": "1"}, [L_SMALL]),
    "no_hint_weights": (12, {}, [L_SMALL]),
    "no_hint_incremental": (10, {}, [L_SMALL]),
    "no_hint_wide": (33, {}, [L_SMALL]),
    "left_out_240": (12, {}, [ALL_SMALL, ALL_SMALL]),
    "left_out_480": (20, {}, [ALL_C8, ALL_C8]),
}
NAN_CFG = {"no_hint_weights": WEIGHTS, "no_hint_incremental": KL}


@pytest.mark.parametrize("name", list(NAN_CASES))
def test_unusable_pair_has_one_nan_writer(name, oracle, monkeypatch):
    import torch

    import loco_hd_amd as lh
    from loco_hd_amd.device import DeviceSession

    ncat, env, lists = NAN_CASES[name]
    c = dict(ncat=ncat, cfg=NAN_CFG.get(name, {}))
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(900 + ncat)
    ca, cb = rng.integers(0, ncat, len(XA)).astype(np.int32), rng.integers(0, ncat, len(XB)).astype(np.int32)
    tag = np.zeros(len(XA), dtype=np.int32)
    lo = build(oracle, c)
    lo.n_threads = 8
    sess = DeviceSession(build(lh, c))
    a, b = sess.upload(XA, ca), sess.upload(XB, cb)
    for sizes in lists[:-1]:  # the passes before: they set the hint ("every pair was small": the next pass leaves the companion out)
        sess.from_primitives(a, b, torch.from_numpy(anchors_of(sizes)).cuda(), THR)
        assert sess.last_sweep()["left"] == 0
    pairs = anchors_of(lists[-1])
    want = np.asarray(lo.from_arrays(XA, ca, tag, XB, cb, tag, pairs, THR))
    spots = [0, len(pairs) // 2, len(pairs)]  # first, in the middle, last: another workgroup and lane each
    bad = pairs
    for k, at in enumerate(spots):
        bad = np.insert(bad, at + k, [ANCHOR_A[1], len(XB)] if k == 1 else [len(XA), ANCHOR_B[1]], axis=0)
    at = np.asarray([s + k for k, s in enumerate(spots)])
    out = torch.full((len(bad),), SENTINEL, dtype=torch.float64, device="cuda")
    with pytest.raises(lh.PanicException):
        sess.from_primitives(a, b, torch.from_numpy(bad).cuda(), THR, out=out)
    got = out.cpu().numpy()
    assert np.isnan(got[at]).all() and not np.isnan(np.delete(got, at)).any() and not (got == SENTINEL).any()
    assert float(np.max(np.abs(np.delete(got, at) - want))) <= TIGHT
    assert sess.last_sweep() is None
    sess.close()


# The slot count of a pass -- which instantiation of the register-resident sweeps runs -- comes from one table per family (kSweepSlots /
# kIncSlots, lchd_device.h), read by the launchers and by the planner alike: for every category count of 1 .. 32 the slots the session
# records after a real call equal the slots lchd_plan_sweep returns for the same query, and the scores are the oracle's.  Two random clouds
# of 1500 atoms in a box of 20 units, threshold 8, anchors next to the centre: environments of a few hundred points (more than 255: no
# small-pair rule applies; at most 512: the LDS-table forms), so every pair spans more than one tile of 384 events and every lane's chunk
# holds several events.  64 pairs: the one-launch form of the default configuration, the regular pipeline with LCHD_NO_INLINE_META (the
# plain sweep does the work, both team forms and the companion are launched next to it) and the incremental sweep of Kullback-Leibler.
SLOT_FAMILIES = {
    "inline": (INLINE, {}, {}, 0),
    "plain": (PLAIN, {"LCHD_NO_INLINE_META": "1"}, {}, N.HOOK_NO_INLINE_META),
    "inc": (INC, {}, KL, 0),
}
SLOT_THR, SLOT_BOX, SLOT_ATOMS, SLOT_PAIRS = 8.0, 20.0, 1500, 64


@pytest.mark.parametrize("family", list(SLOT_FAMILIES))
def test_recorded_slots_are_the_planned_slots(family, oracle, monkeypatch):
    import ctypes as C

    import torch

    import loco_hd_amd as lh
    from loco_hd_amd.device import DeviceSession

    fam, env, cfg, hooks = SLOT_FAMILIES[family]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(7300)
    xa, xb = rng.uniform(0.0, SLOT_BOX, (SLOT_ATOMS, 3)), rng.uniform(0.0, SLOT_BOX, (SLOT_ATOMS, 3))
    near = [np.argsort(np.linalg.norm(x - SLOT_BOX / 2, axis=1))[:SLOT_PAIRS] for x in (xa, xb)]
    pairs = np.stack([near[0], near[1][::-1]], 1).astype(np.int64)
    ra, rb = rng.integers(0, 1 << 20, SLOT_ATOMS), rng.integers(0, 1 << 20, SLOT_ATOMS)
    tag = np.zeros(SLOT_ATOMS, dtype=np.int32)
    bad = []
    for ncat in range(1, 33):
        c = dict(ncat=ncat, cfg=cfg)
        ca, cb = (ra % ncat).astype(np.int32), (rb % ncat).astype(np.int32)
        lo = build(oracle, c)
        lo.n_threads = 8
        want, sizes = lo.from_arrays(xa, ca, tag, xb, cb, tag, pairs, SLOT_THR, return_env_sizes=True)
        want, sizes = np.asarray(want), np.asarray(sizes)
        assert sizes.min() > 255 and sizes.max() <= 512 and (sizes.sum(axis=1) - 2 > 384).all(), (sizes.min(), sizes.max())
        sess = DeviceSession(build(lh, c))
        out = torch.full((SLOT_PAIRS,), SENTINEL, dtype=torch.float64, device="cuda")
        sess.from_primitives(sess.upload(xa, ca), sess.upload(xb, cb), torch.from_numpy(pairs).cuda(), SLOT_THR, out=out)
        got, seen = out.cpu().numpy(), sess.last_sweep()
        sess.close()
        q = N.SweepQueryC(n_pairs=SLOT_PAIRS, n_categories=ncat, force_cmax=0, hellinger2=0 if cfg else 1, unit_weights=1, wf_pow=0,
                          sd_fast=1 if cfg else 0, has_wf_index=0, has_left_list=1, stride_a=512, stride_b=512, cdf_keys_a=1, cdf_keys_b=1,
                          pre_rows=0, hint_bits=0, hooks=hooks)
        plan = N.SweepPlanC()
        assert N.lib().lchd_plan_sweep(C.byref(q), C.byref(plan)) == 0
        err = float(np.max(np.abs(got - want)))
        print(f"{family} {ncat} categories: families {seen['families']:#x} (planned {plan.families:#x}) slots {seen['slots']} (planned {plan.slots}) "
              f"environments {sizes.min()} .. {sizes.max()} points; max |gpu - oracle| = {err:.3e}")
        ok = (seen["families"] & fam and seen["families"] == plan.families and seen["slots"] == plan.slots and seen["rule"] == -1
              and not np.isnan(got).any() and not (got == SENTINEL).any() and err <= TIGHT)
        if not ok:
            bad.append((ncat, seen["families"], plan.families, seen["slots"], plan.slots, err))
    assert not bad, bad
