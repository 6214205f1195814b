"""Literal expectations for lchd_dense_plan / DeviceSession.last_dense(): shared by tests/test_dense_plan.py (the planner alone) and
tests/test_gpu_dense_dispatch.py (the record of what ran)."""
from loco_hd_amd import _native as N

FUSED, ROWS2, ROWS = N.DENSE_FUSED, N.DENSE_ROWS2, N.DENSE_ROWS


def fused(slots=12, dmx=1, segs=None):
    """k_dense_fused<slots, dmx> with `segs` scratch segments per workgroup"""
    want = dict(path=FUSED, unsupported=0, fused_slots=slots, fused_dmx=dmx, nt=0, ept=0, seg=0, n2=0)
    if segs is not None:
        want["scr_segs"] = segs
    return want


def rows2(nt, ept, seg, n2):
    """k_env_rows2<nt, ept, seg> with a key array of n2 points"""
    return dict(path=ROWS2, unsupported=0, nt=nt, ept=ept, seg=seg, n2=n2, fused_slots=0, scr_segs=0)


def side(nt, globalkv, buckets, cap, cat_bytes=1):
    """k_env_rows<nt, globalkv, 8 * cat_bytes-bit ids> with `buckets` distance buckets on slots of `cap` points"""
    return dict(nt=nt, globalkv=globalkv, cat_bytes=cat_bytes, buckets=buckets, cap=cap)


def rows(a, b=None):
    return dict(path=ROWS, unsupported=0, nt=0, ept=0, seg=0, n2=0, fused_slots=0, scr_segs=0, rows=[a, b or a])


BIG32K, BIG64K, HUGE128K = side(1024, 1, 16384, 32768), side(1024, 1, 16384, 65536), side(1024, 1, 32768, 131072)
