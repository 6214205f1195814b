"""Which sweep kernels score a from_primitives pass is decided on the host by lchd_plan_sweep (plan_sweep, loco_hd_amd/csrc/
lchd_kernels.hip): a pure function of the configuration, the call's size and the previous pass's pair statistics.  Without a hint
every candidate family is launched and each kernel decides on the device (rule_in_force, lchd_sweep_common.h) whether a pair is its
own; with a hint the companion may be left out.  A pair is scored correctly only if EXACTLY ONE launched kernel claims it.

Here, without a GPU: (1) over the whole input grid, the claim predicates of the launched families -- written down below from the
kernels, not from the planner -- give every pair exactly one taker whatever the majority test says, and a left-out companion has no
work whenever the host's check lets the pass stand; (2) a literal table, one row each side of every limit of the dispatch."""
import ctypes as C
import itertools

import pytest

from loco_hd_amd import _native as N

INLINE, TEAM240, TEAM480, C8, INDIRECT, PLAIN, INC, WIDE = (N.SWEEP_INLINE, N.SWEEP_TEAM240, N.SWEEP_TEAM480, N.SWEEP_C8,
                                                              N.SWEEP_INDIRECT, N.SWEEP_PLAIN, N.SWEEP_INC, N.SWEEP_WIDE)
RULED = TEAM240 | TEAM480 | C8
H2U, H2W, GEN = 0, 1, 2  # lchd_sweep_plan::plain_mode
F_KEY, F_FAST, F_ANY = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    handle = C.CDLL(str(N.LIB_PATH))
    res, args = N._PROTOS["lchd_plan_sweep"]
    handle.lchd_plan_sweep.restype, handle.lchd_plan_sweep.argtypes = res, args
    return handle


DEFAULTS = dict(n_pairs=10**6, n_categories=10, force_cmax=0, hellinger2=1, unit_weights=1, wf_pow=0, sd_fast=0, has_wf_index=0,
                has_left_list=1, stride_a=512, stride_b=512, cdf_keys_a=1, cdf_keys_b=1, pre_rows=0, hint_bits=0, hooks=0)


def plan(lib, **kw):
    unknown = set(kw) - set(DEFAULTS)
    assert not unknown, unknown
    q, p = N.SweepQueryC(**{**DEFAULTS, **kw}), N.SweepPlanC()
    assert lib.lchd_plan_sweep(C.byref(q), C.byref(p)) == 0
    return p.as_dict()


# ---- the kernels' claims ---------------------------------------------------------------------------------------------------------
def pair_is_small(rule, na, nb):
    """pair_is_small, lchd_team_tile.h."""
    if rule == 0:
        return na + nb - 2 <= 240
    c8 = max(na, nb) <= 255
    return c8 if rule == 1 else (c8 and na + nb - 2 <= 480)


def rule_in_force(p, outcome):
    """rule_in_force, lchd_sweep_common.h.  outcome: 'first' (2 n_small >= P), 'second' (only 2 n_c8 >= P), 'neither'."""
    if p["forced"]:
        return p["small_rule"]
    if outcome == "first":
        return p["small_rule"]
    if outcome == "second" and p["second_rule"]:
        return p["second_rule"]
    return -1


def takers(p, outcome, na, nb, companion_too=True):
    """The launched families that write out[pair] for a pair with environments of na and nb points (0: unusable, the answer is NaN)."""
    usable = na > 0 and nb > 0
    if not usable:
        na = nb = 0  # (k_pair_meta records n = 0 on both sides)
    fam, forced, rule = p["families"], p["forced"], rule_in_force(p, outcome)
    duo_enabled = bool(fam & RULED)  # (SweepArgs::duo_enabled)
    out = []
    for f in (INLINE, WIDE, INC):  # no rule: every pair
        if fam & f:
            out.append(f)
    if fam & PLAIN:  # k_sweep, plain: steps back when a small-pair kernel was launched and a rule is in force
        if forced or not (duo_enabled and rule >= 0):
            out.append(PLAIN)
    for f, own in ((TEAM240, 0), (TEAM480, 2)):  # k_sweep_duo<.., RULE>: its rule in force (or a host-picked pass); NaN writer
        if fam & f and (forced or rule == own) and (not usable or pair_is_small(own, na, nb)):
            out.append(f)
    if fam & C8 and (forced or rule == 1) and (not usable or max(na, nb) <= 255):  # k_sweep<.., CNT8>
        out.append(C8)
    if fam & INDIRECT and companion_too and (forced or rule >= 0) and usable and not pair_is_small(rule, na, nb):  # k_sweep<.., INDIRECT>
        out.append(INDIRECT)
    return out


SIZES = (0, 1, 2, 120, 121, 122, 240, 241, 242, 255, 256, 480)
PLAN_KEY = ("families", "forced", "small_rule", "second_rule", "c8_rule", "companion_left_out")


def coverage_errors(p):
    """Every (nA, nB) of SIZES x SIZES must have exactly one taker under each outcome of the majority test; with the companion left
    out, every pair the host's check lets stand must have one without it."""
    bad = []
    for outcome in ("first", "second", "neither"):
        for na, nb in itertools.product(SIZES, SIZES):
            t = takers(p, outcome, na, nb)
            if p["companion_left_out"]:
                # the host repeats the pass unless EVERY pair is small under the rule it checks: n_c8 (counted under c8_rule) for
                # a nonzero small_rule, n_duo (rule 0) otherwise
                checked = p["c8_rule"] if p["small_rule"] else 0
                if na > 0 and nb > 0 and not pair_is_small(checked, na, nb):
                    continue  # such a pair forces the repetition
            if len(t) != 1:
                bad.append((outcome, na, nb, t))
    if p["companion_left_out"]:
        if not p["forced"] or p["families"] & INDIRECT or bin(p["families"] & RULED).count("1") != 1:
            bad.append(("left-out companion without one host-picked rule kernel",))
        if p["small_rule"] and p["small_rule"] != p["c8_rule"]:
            bad.append(("the host's check counts another rule than the kernel sweeps",))
    return bad


HOOKS = (0, N.HOOK_NO_DUO, N.HOOK_NO_COUNT8, N.HOOK_NO_C8_TEAM, N.HOOK_NO_INLINE_META, N.HOOK_FORCE_WIDE, N.HOOK_FORCE_GENERIC,
         N.HOOK_FORCE_BIGENV, N.HOOK_NO_SWEEP_HINT)
# distance classes: Hellinger-2, Kolmogorov-Smirnov, Kullback-Leibler (incremental form), Renyi (incremental form), anything else
DISTANCES = ((1, 0), (0, 3), (0, 1), (0, 2), (0, 0))


def test_every_pair_has_exactly_one_taker_for_every_input(lib):
    q, p = N.SweepQueryC(**DEFAULTS), N.SweepPlanC()
    qp, pp, call = C.byref(q), C.byref(p), lib.lchd_plan_sweep
    verdicts, n = {}, 0
    # (LCHD_FORCE_CMAX is the one hook with a value: 0, a slot ladder's top, the first width without a 240-event team, beyond 32)
    hook_grid = [(h, 0) for h in HOOKS] + [(0, 16), (0, 17), (0, 40)]
    for hooks, force_cmax in hook_grid:
        q.hooks, q.force_cmax = hooks, force_cmax
        for (q.hellinger2, q.sd_fast), q.unit_weights, q.has_wf_index in itertools.product(DISTANCES, (1, 0), (0, 1)):
            for q.n_pairs, stride, keyed in itertools.product((1, 4096, 4097, 10**6), (512, 513, 65535, 65536), (1, 0) if not hooks else (1,)):
                q.stride_a, q.stride_b = stride, 512  # (either side beyond a limit is enough)
                q.cdf_keys_a = q.cdf_keys_b = keyed
                for q.n_categories in range(1, 41):
                    for q.hint_bits in range(32):
                        assert call(qp, pp) == 0
                        n += 1
                        key = (p.families, p.forced, p.small_rule, p.second_rule, p.c8_rule, p.companion_left_out)
                        if key not in verdicts:
                            verdicts[key] = (coverage_errors(dict(zip(PLAN_KEY, key))), {f: getattr(q, f) for f, _ in q._fields_})
    failures = {k: v for k, v in verdicts.items() if v[0]}
    assert not failures, failures
    assert n > 10**6 and len(verdicts) >= 12  # (the grid was walked, and the planner is not a constant)
    # the claim predicates above are not vacuous: a plan that launches the plain family next to a host-picked team kernel, or a
    # forced team kernel whose companion answers to another rule, is caught
    assert coverage_errors(dict(families=TEAM240 | INDIRECT | PLAIN, forced=1, small_rule=0, second_rule=0, c8_rule=2, companion_left_out=0))
    assert coverage_errors(dict(families=TEAM240 | INDIRECT, forced=1, small_rule=2, second_rule=0, c8_rule=2, companion_left_out=0))
    assert coverage_errors(dict(families=TEAM240 | PLAIN, forced=0, small_rule=0, second_rule=0, c8_rule=2, companion_left_out=0))
    assert coverage_errors(dict(families=C8, forced=1, small_rule=1, second_rule=0, c8_rule=2, companion_left_out=1))


def test_either_side_beyond_a_stride_limit_counts(lib):
    for a, b in ((513, 512), (512, 513)):
        assert plan(lib, stride_a=a, stride_b=b)["families"] == PLAIN
    for a, b in ((65536, 512), (512, 65536)):
        assert plan(lib, stride_a=a, stride_b=b)["families"] == WIDE
    for ka, kb in ((0, 1), (1, 0)):
        assert plan(lib, cdf_keys_a=ka, cdf_keys_b=kb)["fmode"] == F_FAST


def test_bad_arguments_are_refused(lib):
    q, p = N.SweepQueryC(**DEFAULTS), N.SweepPlanC()
    assert lib.lchd_plan_sweep(None, C.byref(p)) != 0
    assert lib.lchd_plan_sweep(C.byref(q), None) != 0
    for field in ("n_pairs", "n_categories"):
        bad = N.SweepQueryC(**{**DEFAULTS, field: 0})
        assert lib.lchd_plan_sweep(C.byref(bad), C.byref(p)) != 0


# ---- one row each side of every limit --------------------------------------------------------------------------------------------
NO_HINT_16 = TEAM240 | INDIRECT | TEAM480 | PLAIN  # up to 16 slots without a hint: both team rules, the companion, the plain sweep
NO_HINT_32 = TEAM480 | INDIRECT | PLAIN            # 17 .. 32 slots: only the 480-event team form exists
KS, KL, RENYI = dict(hellinger2=0, sd_fast=3), dict(hellinger2=0, sd_fast=1), dict(hellinger2=0, sd_fast=2)
WEIGHTED = dict(unit_weights=0)
NO_C8_TEAM = dict(hooks=N.HOOK_NO_C8_TEAM)

EDGES = [
    # 4096 / 4097 pairs: the one-launch sweep against the record pass
    ("4096 pairs", dict(n_pairs=4096), dict(families=INLINE, slots=12, ldstab=1)),
    ("4097 pairs", dict(n_pairs=4097), dict(families=NO_HINT_16, slots=12, forced=0, small_rule=0, second_rule=2, c8_rule=2)),
    ("4096 pairs, hook", dict(n_pairs=4096, hooks=N.HOOK_NO_INLINE_META), dict(families=NO_HINT_16, slots=12)),
    ("4096 pairs, weights", dict(n_pairs=4096, **WEIGHTED), dict(families=NO_HINT_16, team_mode=1)),
    ("4096 pairs, 32 slots", dict(n_pairs=4096, n_categories=32), dict(families=INLINE, slots=32)),
    ("4096 pairs, 33 categories", dict(n_pairs=4096, n_categories=33), dict(families=WIDE, slots=0)),
    # 16 / 17 slots: the 240-event team exists / only the 480-event one
    ("16 slots", dict(n_categories=16), dict(families=NO_HINT_16, slots=16, small_rule=0, second_rule=2)),
    ("17 slots", dict(n_categories=17), dict(families=NO_HINT_32, slots=20, small_rule=2, second_rule=0, c8_rule=2)),
    ("17 slots by hook", dict(n_categories=5, force_cmax=17), dict(families=NO_HINT_32, slots=20, small_rule=2)),
    # 32 / 33: wide
    ("32 slots", dict(n_categories=32), dict(families=NO_HINT_32, slots=32)),
    ("33 categories", dict(n_categories=33), dict(families=WIDE, slots=0, plain_mode=H2U, wide_long=0, small_rule=0, second_rule=0, left_listing=0)),
    ("33 categories, weights", dict(n_categories=33, **WEIGHTED), dict(families=WIDE, plain_mode=H2W)),
    ("33 categories, Kolmogorov-Smirnov", dict(n_categories=33, **KS), dict(families=WIDE, plain_mode=GEN)),
    ("wide by hook", dict(hooks=N.HOOK_FORCE_WIDE), dict(families=WIDE, slots=0)),
    # stride 512 / 513 (the LDS tables) and 65535 / 65536 (the 64-bit-count form of the wide sweep)
    ("stride 512", dict(hint_bits=4), dict(families=PLAIN, ldstab=1, forced=1)),
    ("stride 513", dict(stride_a=513, stride_b=513), dict(families=PLAIN, ldstab=0, forced=0)),
    ("stride 513, small call", dict(stride_a=513, stride_b=513, n_pairs=4096), dict(families=PLAIN, ldstab=0)),
    ("stride 65535", dict(stride_a=65535, stride_b=65535), dict(families=PLAIN, ldstab=0, slots=12)),
    ("stride 65536", dict(stride_a=65536, stride_b=65536), dict(families=WIDE, slots=0, wide_long=1)),
    ("big environments by hook", dict(hooks=N.HOOK_FORCE_BIGENV), dict(families=PLAIN, ldstab=0)),
    # weighted and Kolmogorov-Smirnov team forms at 16 / 17
    ("weights, 16", dict(n_categories=16, **WEIGHTED), dict(families=NO_HINT_16, slots=16, team_mode=1, plain_mode=H2W, ldstab=1)),
    ("weights, 17", dict(n_categories=17, **WEIGHTED), dict(families=PLAIN, slots=20, plain_mode=H2W, ldstab=1)),
    ("Kolmogorov-Smirnov, 16", dict(n_categories=16, **KS), dict(families=NO_HINT_16, slots=16, team_mode=2, plain_mode=GEN, ldstab=0)),
    ("Kolmogorov-Smirnov, 17", dict(n_categories=17, **KS), dict(families=PLAIN, slots=20, plain_mode=GEN)),
    ("Kolmogorov-Smirnov, weights", dict(**KS, **WEIGHTED), dict(families=PLAIN, plain_mode=GEN)),
    ("weights without the 480-event team", dict(**WEIGHTED, **NO_C8_TEAM), dict(families=PLAIN, plain_mode=H2W)),
    # Kullback-Leibler / Renyi: the incremental sweep, the generic one with a weight-function index per pair
    ("KL", dict(**KL), dict(families=INC, slots=12, forced=0)),
    ("KL, wf_index", dict(**KL, has_wf_index=1), dict(families=PLAIN, plain_mode=GEN, ldstab=0)),
    ("Renyi", dict(**RENYI), dict(families=INC)),
    ("Renyi, wf_index", dict(**RENYI, has_wf_index=1), dict(families=PLAIN, plain_mode=GEN)),
    ("KL, weights", dict(**KL, **WEIGHTED), dict(families=PLAIN, plain_mode=GEN)),
    ("KL, stride 513", dict(**KL, stride_a=513, stride_b=513), dict(families=PLAIN, plain_mode=GEN)),
    ("KL, distance keys", dict(**KL, cdf_keys_a=0, cdf_keys_b=0), dict(families=PLAIN, plain_mode=GEN, fmode=F_FAST)),
    ("KL, small call", dict(**KL, n_pairs=100), dict(families=INC)),
    ("KL, 33 categories", dict(**KL, n_categories=33), dict(families=WIDE, plain_mode=GEN)),
    ("generic distance", dict(hellinger2=0), dict(families=PLAIN, plain_mode=GEN, ldstab=0)),
    ("generic by hook", dict(hooks=N.HOOK_FORCE_GENERIC), dict(families=PLAIN, plain_mode=GEN)),
    # F(t): keys, inline CDFs, any CDF
    ("distance keys", dict(cdf_keys_a=0, cdf_keys_b=0), dict(families=PLAIN, fmode=F_FAST, ldstab=1)),
    ("distance keys, pow", dict(cdf_keys_a=0, cdf_keys_b=0, wf_pow=1), dict(families=PLAIN, fmode=F_ANY)),
    ("distance keys, wide", dict(cdf_keys_a=0, cdf_keys_b=0, n_categories=33), dict(families=WIDE, fmode=F_ANY)),
    ("key sets of a dictionary", dict(cdf_keys_a=3, cdf_keys_b=3, has_wf_index=1), dict(families=NO_HINT_16, fmode=F_KEY)),
    # the hint states, up to 16 slots ...
    ("unknown", dict(hint_bits=0), dict(families=NO_HINT_16, forced=0, left_listing=0, companion_left_out=0)),
    ("bits without 'known'", dict(hint_bits=1 | 2 | 8 | 16), dict(families=NO_HINT_16, forced=0, left_listing=0, companion_left_out=0)),
    ("duo majority", dict(hint_bits=4 | 1), dict(families=TEAM240 | INDIRECT, forced=1, small_rule=0, second_rule=0, left_listing=1)),
    ("duo and c8 majority", dict(hint_bits=4 | 1 | 2), dict(families=TEAM240 | INDIRECT, forced=1, small_rule=0, left_listing=1)),
    ("c8 majority only", dict(hint_bits=4 | 2), dict(families=TEAM480 | INDIRECT, forced=1, small_rule=2, c8_rule=2, left_listing=1)),
    ("neither", dict(hint_bits=4), dict(families=PLAIN, forced=1, left_listing=0, companion_left_out=0)),
    ("all small", dict(hint_bits=4 | 1 | 2 | 8 | 16), dict(families=TEAM240, forced=1, small_rule=0, left_listing=0, companion_left_out=1)),
    ("all c8, duo minority", dict(hint_bits=4 | 2 | 16), dict(families=TEAM480, forced=1, small_rule=2, left_listing=0, companion_left_out=1)),
    ("all c8, duo majority", dict(hint_bits=4 | 1 | 2 | 16), dict(families=TEAM240 | INDIRECT, forced=1, small_rule=0, left_listing=1, companion_left_out=0)),
    ("duo majority, no list buffers", dict(hint_bits=4 | 1, has_left_list=0), dict(families=TEAM240 | INDIRECT, left_listing=0)),
    ("hint ignored by hook", dict(hint_bits=4 | 1 | 8, hooks=N.HOOK_NO_SWEEP_HINT), dict(families=NO_HINT_16, forced=0, companion_left_out=0)),
    ("no duo, unknown", dict(hooks=N.HOOK_NO_DUO), dict(families=PLAIN, forced=0)),
    ("no duo, c8 majority", dict(hooks=N.HOOK_NO_DUO, hint_bits=4 | 1 | 2), dict(families=TEAM480 | INDIRECT, forced=1, small_rule=2)),
    ("no count8, unknown", dict(hooks=N.HOOK_NO_COUNT8), dict(families=TEAM240 | INDIRECT | PLAIN, forced=0, second_rule=0)),
    ("no count8, c8 majority only", dict(hooks=N.HOOK_NO_COUNT8, hint_bits=4 | 2), dict(families=PLAIN, forced=1)),
    ("no c8 team, unknown", dict(**NO_C8_TEAM), dict(families=TEAM240 | INDIRECT | PLAIN, second_rule=0, c8_rule=1)),
    ("no c8 team, c8 majority only", dict(**NO_C8_TEAM, hint_bits=4 | 2), dict(families=C8 | INDIRECT, forced=1, small_rule=1, c8_rule=1, team_mode=0)),
    # ... and above
    ("20 slots, unknown", dict(n_categories=20), dict(families=NO_HINT_32, slots=20, forced=0, small_rule=2)),
    ("20 slots, duo majority only", dict(n_categories=20, hint_bits=4 | 1 | 8), dict(families=PLAIN, forced=1, companion_left_out=0)),
    ("20 slots, c8 majority", dict(n_categories=20, hint_bits=4 | 1 | 2), dict(families=TEAM480 | INDIRECT, forced=1, small_rule=2, left_listing=1)),
    ("20 slots, all c8", dict(n_categories=20, hint_bits=4 | 2 | 16), dict(families=TEAM480, forced=1, companion_left_out=1, left_listing=0)),
    ("20 slots, all duo says nothing", dict(n_categories=20, hint_bits=4 | 1 | 2 | 8), dict(families=TEAM480 | INDIRECT, companion_left_out=0)),
    ("20 slots, no c8 team", dict(n_categories=20, **NO_C8_TEAM), dict(families=C8 | INDIRECT | PLAIN, slots=20, small_rule=1, c8_rule=1, second_rule=0)),
    ("20 slots, no c8 team, all c8", dict(n_categories=20, **NO_C8_TEAM, hint_bits=4 | 2 | 16), dict(families=C8, small_rule=1, c8_rule=1, companion_left_out=1)),
    ("20 slots, no count8", dict(n_categories=20, hooks=N.HOOK_NO_COUNT8), dict(families=PLAIN)),
    ("40 slots by hook", dict(force_cmax=40), dict(families=C8 | INDIRECT | PLAIN, slots=32, small_rule=1, c8_rule=1)),
    # prefix-count rows: the PRE instantiations of the unweighted team kernels of up to 16 slots
    ("rows", dict(pre_rows=1), dict(families=NO_HINT_16, pre=1)),
    ("rows, Kolmogorov-Smirnov", dict(pre_rows=1, **KS), dict(families=NO_HINT_16, pre=1)),
    ("rows, weights", dict(pre_rows=1, **WEIGHTED), dict(families=NO_HINT_16, pre=0)),
    ("rows, 17 slots", dict(pre_rows=1, n_categories=17), dict(families=NO_HINT_32, pre=0)),
    ("rows, plain sweep only", dict(pre_rows=1, hint_bits=4), dict(families=PLAIN, pre=0)),
]
# the slot ladders: launch_team / launch_sweep_plain (8 / 12 / 16 / 20 / 24 / 28 / 32) and launch_sweep_inc (8 / 12 / 16 / 24 / 32)
for n_cat, slots, inc_slots in ((8, 8, 8), (9, 12, 12), (12, 12, 12), (13, 16, 16), (16, 16, 16), (17, 20, 24), (20, 20, 24), (21, 24, 24),
                                (24, 24, 24), (25, 28, 32), (28, 28, 32), (29, 32, 32), (32, 32, 32)):
    EDGES.append((f"team ladder, {n_cat}", dict(n_categories=n_cat), dict(families=NO_HINT_16 if n_cat <= 16 else NO_HINT_32, slots=slots)))
    EDGES.append((f"inline ladder, {n_cat}", dict(n_categories=n_cat, n_pairs=7), dict(families=INLINE, slots=slots)))
    EDGES.append((f"incremental ladder, {n_cat}", dict(n_categories=n_cat, **KL), dict(families=INC, slots=inc_slots)))


@pytest.mark.parametrize("name,query,want", EDGES, ids=[e[0] for e in EDGES])
def test_edge_table(lib, name, query, want):
    got = plan(lib, **query)
    assert {k: got[k] for k in want} == want, (name, got)
