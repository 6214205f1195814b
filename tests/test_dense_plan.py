"""Which kernel sorts the dense rows of from_coords / from_dmxs / the dense ensembles is decided on the host by lchd_plan_dense
(plan_dense, loco_hd_amd/csrc/lchd_dense_plan.h): a pure function of the row lengths, the category width, the configuration, the two
tuning hooks and the attempt number.  The launchers (launch_dense_fused, launch_env_rows2, launch_env_rows) switch on its answer.

Here, without a GPU: (1) a literal table, one row each side of every limit of the dispatch; (2) over the whole input grid, every
supported query gets exactly one path and the instantiation named for it fits the rows -- the fit conditions are written down below from
the kernels' template parameters and LDS layouts (lchd_env_rows.hip, lchd_dense_fused.hip), not from the planner."""
import ctypes as C
import itertools

import pytest

from dense_plan_util import BIG32K, BIG64K, FUSED, HUGE128K, ROWS, ROWS2, fused, rows, rows2, side
from loco_hd_amd import _native as N

OLD_ROWS, NO_FUSED = N.DENSE_HOOK_OLD_ROWS, N.DENSE_HOOK_NO_FUSED
M23 = 1 << 23


@pytest.fixture(scope="module")
def lib():
    handle = C.CDLL(str(N.LIB_PATH))
    res, args = N._PROTOS["lchd_plan_dense"]
    handle.lchd_plan_dense.restype, handle.lchd_plan_dense.argtypes = res, args
    return handle


DEFAULTS = dict(cols_a=2000, cols_b=2000, n_categories=10, hellinger2=1, unit_weights=1, cat16=0, given_rows=1, ragged=0, hooks=0,
                attempt=0, single_attempt=0, reserved=0)


def plan(lib, n=None, **kw):
    unknown = set(kw) - set(DEFAULTS)
    assert not unknown, unknown
    if n is not None:
        kw.update(cols_a=n, cols_b=n)
    kw.setdefault("cat16", int(kw.get("n_categories", DEFAULTS["n_categories"]) > 255))  # as the library sets it
    q, p = N.DenseQueryC(**{**DEFAULTS, **kw}), N.DensePlanC()
    assert lib.lchd_plan_dense(C.byref(q), C.byref(p)) == 0
    return p.as_dict()


# ---- one row each side of every limit --------------------------------------------------------------------------------------------
UNSUPPORTED = dict(path=0, unsupported=1)
NF, OLD = dict(hooks=NO_FUSED), dict(hooks=OLD_ROWS)

# scr_segs, by hand: S starts at ceil(total / 6144) and grows while total / S + 6 * floor(sqrt(4 * (total / S))) + 70 > 6144; S + 2, at most 16
EDGES = [
    # the default configuration (Hellinger-2, unit weights, 10 categories, given rows): fused for 1025 .. 20480 points
    ("1", dict(n=1), rows2(64, 16, 1, 64)),
    ("64", dict(n=64), rows2(64, 16, 1, 64)),
    ("65", dict(n=65), rows2(64, 16, 1, 128)),
    ("1024", dict(n=1024), rows2(64, 16, 1, 1024)),
    ("1025", dict(n=1025), fused(segs=3)),       # 2050 events: 1 segment fits (2050 + 6 * 90 + 70)
    ("4096", dict(n=4096), fused(segs=4)),       # 8192: 2 (4096 + 6 * 128 + 70 = 4934)
    ("4097", dict(n=4097), fused(segs=4)),
    ("8192", dict(n=8192), fused(segs=6)),       # 16384: 3 does not fit (5461 + 6 * 147 + 70 = 6413), 4 does
    ("8193", dict(n=8193), fused(segs=6)),
    ("10240", dict(n=10240), fused(segs=6)),     # 20480: 4 (5120 + 6 * 143 + 70 = 6048)
    ("10241", dict(n=10241), fused(segs=6)),
    ("16384", dict(n=16384), fused(segs=9)),     # 32768: 6 does not fit (6413), 7 does (4681 + 6 * 136 + 70 = 5567)
    ("16385", dict(n=16385), fused(segs=9)),
    ("20480", dict(n=20480), fused(segs=10)),    # 40960: 7 does not fit (5851 + 6 * 152 + 70 = 6833), 8 does (6048)
    ("20481", dict(n=20481), rows(BIG32K)),
    ("65535", dict(n=65535), rows(BIG64K)),
    ("65536", dict(n=65536), rows(BIG64K)),
    ("65537", dict(n=65537), rows(HUGE128K)),
    ("2^23", dict(n=M23), rows(side(1024, 1, 32768, M23))),
    ("2^23 + 1", dict(n=M23 + 1), UNSUPPORTED),
    ("0", dict(n=0), UNSUPPORTED),
    ("coordinates", dict(n=2000, given_rows=0), fused(dmx=0)),
    # LCHD_NO_DENSE_FUSED: the ladder of k_env_rows2
    ("no fused, 1024", dict(n=1024, **NF), rows2(64, 16, 1, 1024)),
    ("no fused, 1025", dict(n=1025, **NF), rows2(256, 16, 1, 2048)),
    ("no fused, 4096", dict(n=4096, **NF), rows2(256, 16, 1, 4096)),
    ("no fused, 4097", dict(n=4097, **NF), rows2(1024, 8, 1, 8192)),
    ("no fused, 8192", dict(n=8192, **NF), rows2(1024, 8, 1, 8192)),
    ("no fused, 8193", dict(n=8193, **NF), rows2(1024, 10, 1, 16384)),
    ("no fused, 10240", dict(n=10240, **NF), rows2(1024, 10, 1, 16384)),
    ("no fused, 10241", dict(n=10241, **NF), rows2(1024, 16, 1, 16384)),
    ("no fused, 16384", dict(n=16384, **NF), rows2(1024, 16, 1, 16384)),
    ("no fused, 16385", dict(n=16385, **NF), rows2(1024, 12, 2, 16384)),
    ("no fused, 20480", dict(n=20480, **NF), rows2(1024, 12, 2, 16384)),
    ("no fused, 20481", dict(n=20481, **NF), rows(BIG32K)),
    # LCHD_OLD_ROWS: the ladder of k_env_rows
    ("old rows, 1", dict(n=1, **OLD), rows(side(64, 0, 2048, 64))),
    ("old rows, 64", dict(n=64, **OLD), rows(side(64, 0, 2048, 64))),
    ("old rows, 65", dict(n=65, **OLD), rows(side(64, 0, 2048, 128))),
    ("old rows, 1024", dict(n=1024, **OLD), rows(side(64, 0, 2048, 1024))),
    ("old rows, 1025", dict(n=1025, **OLD), rows(side(256, 0, 2048, 2048))),
    ("old rows, 4096", dict(n=4096, **OLD), rows(side(256, 0, 2048, 4096))),
    ("old rows, 4097", dict(n=4097, **OLD), rows(side(1024, 0, 2048, 8192))),
    ("old rows, 8192", dict(n=8192, **OLD), rows(side(1024, 0, 2048, 8192))),
    ("old rows, 8193", dict(n=8193, **OLD), rows(side(1024, 0, 2048, 16384))),
    ("old rows, 16384", dict(n=16384, **OLD), rows(side(1024, 0, 2048, 16384))),
    ("old rows, 16385", dict(n=16385, **OLD), rows(BIG32K)),
    ("both hooks", dict(n=2000, hooks=OLD_ROWS | NO_FUSED), rows(side(256, 0, 2048, 2048))),
    # category slots of the fused kernel, the fused kernel's 16, the 8-bit ids' 255
    ("8 categories", dict(n_categories=8), fused(slots=8)),
    ("9 categories", dict(n_categories=9), fused(slots=12)),
    ("12 categories", dict(n_categories=12), fused(slots=12)),
    ("13 categories", dict(n_categories=13), fused(slots=16)),
    ("16 categories", dict(n_categories=16), fused(slots=16)),
    ("17 categories", dict(n_categories=17), rows2(256, 16, 1, 2048)),
    ("255 categories", dict(n_categories=255), rows2(256, 16, 1, 2048)),
    ("256 categories", dict(n_categories=256), rows(side(1024, 0, 2048, 2048, 2))),
    # 16-bit ids: two LDS instantiations (64 and 1024 threads), keys in the store beyond 8192 points, no rows beyond 65535
    ("cat16, 1024", dict(n=1024, n_categories=300), rows(side(64, 0, 2048, 1024, 2))),
    ("cat16, 1025", dict(n=1025, n_categories=300), rows(side(1024, 0, 2048, 2048, 2))),
    ("cat16, 8192", dict(n=8192, n_categories=300), rows(side(1024, 0, 2048, 8192, 2))),
    ("cat16, 8193", dict(n=8193, n_categories=300), rows(side(1024, 1, 16384, 16384, 2))),
    ("cat16, 65535", dict(n=65535, n_categories=300), rows(side(1024, 1, 16384, 65536, 2))),
    ("cat16, 65536", dict(n=65536, n_categories=300), UNSUPPORTED),
    # not the fused kernel's configuration
    ("category weights", dict(unit_weights=0), rows2(256, 16, 1, 2048)),
    ("another distance", dict(hellinger2=0), rows2(256, 16, 1, 2048)),
    # unequal widths: the longer side picks the path; two segments need both sides long
    ("20480 x 16384", dict(cols_a=20480, cols_b=16384), fused(segs=10)),  # 36864: 6 and 7 do not fit (7150, 6206), 8 does (4608 + 6 * 135 + 70)
    ("20480 x 16384, no fused", dict(cols_a=20480, cols_b=16384, **NF), rows(BIG32K, side(1024, 0, 2048, 16384))),
    ("16385 x 16384, no fused", dict(cols_a=16385, cols_b=16384, **NF), rows(BIG32K, side(1024, 0, 2048, 16384))),
    ("16384 x 16385, no fused", dict(cols_a=16384, cols_b=16385, **NF), rows(side(1024, 0, 2048, 16384), BIG32K)),
    ("16385 x 16386, no fused", dict(cols_a=16385, cols_b=16386, **NF), rows2(1024, 12, 2, 16384)),
    ("1025 x 1", dict(cols_a=1025, cols_b=1), fused(segs=3)),
    ("1025 x 1, no fused", dict(cols_a=1025, cols_b=1, **NF), rows2(256, 16, 1, 2048)),
    ("1 x 1025, no fused", dict(cols_a=1, cols_b=1025, **NF), rows2(256, 16, 1, 2048)),
    ("20481 x 1024", dict(cols_a=20481, cols_b=1024), rows(BIG32K, side(64, 0, 2048, 1024))),
    ("2000 x 0", dict(cols_a=2000, cols_b=0), UNSUPPORTED),
    # ragged rows may be short: no two-segment launch
    ("ragged, 16384", dict(n=16384, ragged=1, **NF), rows2(1024, 16, 1, 16384)),
    ("ragged, 16385", dict(n=16385, ragged=1, **NF), rows(BIG32K)),
    ("ragged, 16385, fused", dict(n=16385, ragged=1), fused(segs=9)),
    # the second attempt: the kernel that never gives up
    ("attempt 0", dict(n=2000, attempt=0), fused()),
    ("attempt 1", dict(n=2000, attempt=1), rows(side(256, 0, 2048, 2048))),
    ("attempt 0, two segments", dict(n=17000, attempt=0, **NF), rows2(1024, 12, 2, 16384)),
    ("attempt 1, two segments", dict(n=17000, attempt=1, **NF), rows(BIG32K)),
    # a call that cannot be repeated (the dense ensembles)
    ("single attempt, 2000", dict(n=2000, single_attempt=1), rows2(256, 16, 1, 2048)),
    ("single attempt, 16384", dict(n=16384, single_attempt=1), rows2(1024, 16, 1, 16384)),
    ("single attempt, 16385", dict(n=16385, single_attempt=1), rows(BIG32K)),
    ("single attempt, old rows", dict(n=16384, single_attempt=1, **OLD), rows(side(1024, 0, 2048, 16384))),
]


@pytest.mark.parametrize("name,query,want", EDGES, ids=[e[0] for e in EDGES])
def test_edge_table(lib, name, query, want):
    got = plan(lib, **query)
    assert {k: got[k] for k in want} == want, (name, got)


def test_bad_arguments_are_refused(lib):
    q, p = N.DenseQueryC(**DEFAULTS), N.DensePlanC()
    assert lib.lchd_plan_dense(None, C.byref(p)) != 0
    assert lib.lchd_plan_dense(C.byref(q), None) != 0
    for field, value in (("n_categories", 0), ("attempt", 2), ("attempt", -1), ("hooks", 4)):
        bad = N.DenseQueryC(**{**DEFAULTS, field: value})
        assert lib.lchd_plan_dense(C.byref(bad), C.byref(p)) != 0


# ---- what the kernels hold, from their template parameters -----------------------------------------------------------------------
LDS_DEFAULT = 64 * 1024   # dynamic LDS of a kernel nobody raised the limit of
LDS_CU = 160 * 1024       # gfx950
HIST_SMALL = (2048 + 1) * 4
# k_env_rows2<NT, EPT, NSEG>: the instantiations of lchd_env_rows.hip with the dynamic LDS init_env_rows_kernels allows each
ROWS2_INST = {(64, 16, 1): LDS_DEFAULT, (256, 16, 1): LDS_DEFAULT, (1024, 8, 1): 8192 * 9 + 16 + HIST_SMALL,
              (1024, 10, 1): 16384 * 9 + 16 + HIST_SMALL, (1024, 16, 1): 16384 * 9 + 16 + HIST_SMALL,
              (1024, 12, 2): 11776 * 9 + (8192 + 1) * 4}
ROW_LONG_EPT, ROW_SEG_CAP = 20, 11776  # kRowLongEpt, kRowSegCap: points per thread of a two-segment row, keys of one segment
# k_env_rows<NT, GLOBALKV, VT>: (NT, GLOBALKV, sizeof(VT)) -> allowed dynamic LDS
ROWS_INST = {(64, 0, 1): LDS_DEFAULT, (256, 0, 1): LDS_DEFAULT, (1024, 0, 1): 16384 * 9 + 16 + HIST_SMALL, (1024, 1, 1): (32768 + 1) * 4 + 16,
             (64, 0, 2): LDS_DEFAULT, (1024, 0, 2): 8192 * 10 + 16 + HIST_SMALL, (1024, 1, 2): (16384 + 1) * 4 + 16}
FUSED_SEG_CAP, FUSED_MAX_SEG = 6144, 16  # kCap, kMaxSeg of lchd_dense_fused.hip


def fit_errors(q, p):
    """q: the query's fields, p: the plan as a dict.  What is wrong with the plan, as a list of strings."""
    a, b, cat16 = q["cols_a"], q["cols_b"], bool(q["cat16"])
    longest, shortest = max(a, b), min(a, b)
    supported = shortest >= 1 and longest <= M23 and not (cat16 and longest > 65535)
    if not supported:
        return [] if p["unsupported"] == 1 and p["path"] == 0 else ["a query no kernel takes was given a path"]
    bad = []
    if p["unsupported"] or p["path"] not in (FUSED, ROWS2, ROWS):
        return ["a supported query without a path"]
    zero = {FUSED: ("nt", "ept", "seg", "n2"), ROWS2: ("fused_slots", "fused_dmx", "scr_segs"), ROWS: ("nt", "ept", "seg", "n2", "fused_slots", "fused_dmx", "scr_segs")}
    if any(p[k] for k in zero[p["path"]]) or (p["path"] != ROWS and any(v for s in p["rows"] for v in s.values())):
        bad.append("fields of another path are set")
    may_give_up = False
    if p["path"] == FUSED:
        # k_dense_fused<CMAX, DMX>: CMAX category slots of 8-bit ids, Hellinger-2 on unit weights only, rows of 1025 .. 20480 points
        may_give_up = True
        if p["fused_slots"] not in (8, 12, 16) or p["fused_slots"] < q["n_categories"]:
            bad.append("category slots")
        if cat16 or not q["hellinger2"] or not q["unit_weights"]:
            bad.append("not the fused kernel's configuration")
        if not 1024 < longest <= 20480:
            bad.append("row length outside the fused kernel's")
        if p["fused_dmx"] != q["given_rows"]:
            bad.append("row form")
        if not p["scr_segs"] <= FUSED_MAX_SEG or p["scr_segs"] * FUSED_SEG_CAP < a + b:
            bad.append("the scratch segments do not hold the row pair's events")
    elif p["path"] == ROWS2:
        inst = (p["nt"], p["ept"], p["seg"])
        if inst not in ROWS2_INST:
            return bad + ["no such instantiation of k_env_rows2"]
        if cat16:
            bad.append("k_env_rows2 has 8-bit categories only")
        n2 = p["n2"]
        if n2 & (n2 - 1) or not 64 <= n2 <= 16384:
            bad.append("key array")
        if p["seg"] == 1:
            if p["nt"] * p["ept"] < longest or n2 < longest:
                bad.append("the row does not fit the registers / the key array")
            if n2 * 9 + 16 + HIST_SMALL > ROWS2_INST[inst]:
                bad.append("LDS beyond what init_env_rows_kernels raised")
        else:
            may_give_up = True
            if p["nt"] * ROW_LONG_EPT < longest or 2 * ROW_SEG_CAP < longest or p["nt"] * p["ept"] < ROW_SEG_CAP:
                bad.append("the row does not fit two segments")
            if shortest <= 16384 or q["ragged"]:
                bad.append("a short row in a two-segment launch")
            if n2 != 16384:
                bad.append("key array of a two-segment launch")
    else:
        for cols, s in zip((a, b), p["rows"]):
            inst = (s["nt"], s["globalkv"], s["cat_bytes"])
            if inst not in ROWS_INST:
                bad.append("no such instantiation of k_env_rows")
                continue
            cap = s["cap"]
            if cap < cols or cap & (cap - 1) or cap > M23:
                bad.append("cap")
            if s["cat_bytes"] != (2 if cat16 else 1):
                bad.append("category width")
            lds = (s["buckets"] + 1) * 4 + 16 if s["globalkv"] else cap * (8 + s["cat_bytes"]) + 16 + (s["buckets"] + 1) * 4
            if lds > ROWS_INST[inst] or lds > LDS_CU:
                bad.append("LDS beyond what init_env_rows_kernels raised")
            if s["buckets"] not in (2048, 16384, 32768) or (not s["globalkv"] and s["buckets"] != 2048):
                bad.append("buckets")
    if may_give_up and (q["attempt"] > 0 or q["single_attempt"] or q["hooks"] & OLD_ROWS):
        bad.append("a kernel that may give up on a row where the call cannot be repeated")
    if p["path"] == FUSED and q["hooks"] & NO_FUSED:
        bad.append("the fused kernel against its hook")
    return bad


LENGTHS = (1, 64, 65, 1024, 1025, 4096, 4097, 8192, 8193, 10240, 10241, 16384, 16385, 20480, 20481, 65535, 65536, 65537, M23, M23 + 1)
LENGTHS_B = (0, 1, 1024, 1025, 8193, 16384, 16385, 20480, 20481, 65536, M23 + 1)
CATEGORIES = (1, 8, 9, 12, 13, 16, 17, 255, 256, 300)


def test_every_supported_query_gets_one_path_that_fits(lib):
    q, p = N.DenseQueryC(**DEFAULTS), N.DensePlanC()
    qp, pp, call = C.byref(q), C.byref(p), lib.lchd_plan_dense
    names = [f for f, _ in q._fields_]
    failures, paths, n = [], set(), 0
    for a in LENGTHS:
        for b in (a,) + LENGTHS_B:
            q.cols_a, q.cols_b = a, b
            for q.n_categories in CATEGORIES:
                q.cat16 = int(q.n_categories > 255)
                for q.hellinger2, q.unit_weights, q.given_rows, q.ragged in ((1, 1, 1, 0), (1, 1, 0, 0), (1, 1, 1, 1), (0, 1, 1, 0), (1, 0, 0, 0)):
                    for q.hooks, q.attempt, q.single_attempt in itertools.product(range(4), (0, 1), (0, 1)):
                        assert call(qp, pp) == 0
                        n += 1
                        got = p.as_dict()
                        paths.add((got["path"], got["nt"], got["ept"], got["seg"], got["fused_slots"], tuple(s["nt"] for s in got["rows"])))
                        errs = fit_errors({f: getattr(q, f) for f in names}, got)
                        if errs and len(failures) < 10:
                            failures.append((errs, {f: getattr(q, f) for f in names}, got))
    assert not failures, failures
    # the grid was walked and the planner is not a constant: unsupported, three fused slot widths, six instantiations of k_env_rows2 and
    # the three thread counts of k_env_rows at the least
    assert n > 10**5 and len(paths) >= 13
    # the fit conditions are not vacuous: a row one point beyond its instantiation, a short side in a two-segment launch, 16-bit ids
    # in the LDS of 8-bit ones and a fused kernel on the repeat are caught
    base = {**DEFAULTS, "hooks": NO_FUSED}
    assert fit_errors({**base, "cols_a": 10241, "cols_b": 10241}, plan(lib, n=10240, **NF))
    assert fit_errors({**base, "cols_a": 1025, "cols_b": 1025}, plan(lib, n=1024, **NF))
    assert fit_errors({**base, "cols_a": 17000, "cols_b": 16384}, plan(lib, n=17000, **NF))
    assert fit_errors({**DEFAULTS, "cols_a": 16384, "cols_b": 16384, "n_categories": 300, "cat16": 1, "hooks": OLD_ROWS}, plan(lib, n=16384, **OLD))
    assert fit_errors({**DEFAULTS, "attempt": 1}, plan(lib, n=2000))
    assert fit_errors({**DEFAULTS, "cols_a": 20481, "cols_b": 20481}, plan(lib, n=20480))
