"""Thread safety of the host side (no GPU): the process-wide string tables of PrimitiveAtom, the order in which its setters
invalidate the pack cache, the lazy creation of an instance's context / device group, and the pack / anchor caches of a LoCoHD
shared by threads.  The reference's LoCoHD is a Send + Sync pyclass whose drivers take &self (src/locohd.rs:42-55) and its
PrimitiveAtom holds plain strings: sharing either between threads is safe there and must be here."""
import random
import sys
import threading
import time
import uuid

import numpy as np
import pytest

import loco_hd_amd as lh
from loco_hd_amd import _native as N
from loco_hd_amd import api

JOIN_S = 30.0


def _fresh(prefix, n):
    u = uuid.uuid4().hex[:10]
    return [f"{prefix}-{u}-{k}" for k in range(n)]


def _run_threads(fns, timeout=JOIN_S):
    """Start one thread per callable, join them with a time limit, re-raise the first exception a thread raised."""
    errors = []

    def wrap(fn):
        def run():
            try:
                fn()
            except BaseException as e:  # noqa: BLE001 -- reported below
                errors.append(e)
        return run

    ts = [threading.Thread(target=wrap(f), daemon=True) for f in fns]
    for t in ts:
        t.start()
    deadline = time.monotonic() + timeout
    for t in ts:
        t.join(max(0.0, deadline - time.monotonic()))
    assert not any(t.is_alive() for t in ts), "a thread did not finish in time"
    if errors:
        raise errors[0]


class _BarrierStr(str):
    """A str whose hash meets the other thread on a shared barrier: both threads are inside the same intern step at once."""

    barrier = None

    def __hash__(self):
        b = _BarrierStr.barrier
        if b is not None:
            try:
                b.wait(0.5)
            except threading.BrokenBarrierError:
                pass
        return str.__hash__(self)

    def __eq__(self, other):
        return str.__eq__(self, other)


def _check_tables(types, tags):
    for n in types:
        assert api._TYPE_NAMES[api._TYPE_IDS[n]] == n, f"type {n!r} is filed under the id of {api._TYPE_NAMES[api._TYPE_IDS[n]]!r}"
    ids = [api._TAG_IDS[t] for t in tags]
    assert len(set(ids)) == len(ids), "two tags share one id"


def test_intern_types_race_deterministic():
    a, b = (_BarrierStr(s) for s in _fresh("thr-type", 2))
    atoms = {}
    _BarrierStr.barrier = threading.Barrier(2)
    try:
        _run_threads([lambda: atoms.__setitem__(0, lh.PrimitiveAtom(a, "", [0.0, 0.0, 0.0])),
                      lambda: atoms.__setitem__(1, lh.PrimitiveAtom(b, "", [1.0, 0.0, 0.0]))])
    finally:
        _BarrierStr.barrier = None
    _check_tables([a, b], [])
    for at in atoms.values():
        assert api._TYPE_NAMES[at._pid] == at.primitive_type


def test_intern_tags_race_deterministic():
    a, b = (_BarrierStr(s) for s in _fresh("thr-tag", 2))
    atoms = {}
    _BarrierStr.barrier = threading.Barrier(2)
    try:
        _run_threads([lambda: atoms.__setitem__(0, lh.PrimitiveAtom("C", a, [0.0, 0.0, 0.0])),
                      lambda: atoms.__setitem__(1, lh.PrimitiveAtom("C", b, [1.0, 0.0, 0.0]))])
    finally:
        _BarrierStr.barrier = None
    _check_tables([], [a, b])
    assert atoms[0]._tid != atoms[1]._tid
    assert atoms[0]._tid == api._TAG_IDS[a] and atoms[1]._tid == api._TAG_IDS[b]


def test_intern_setters_race_deterministic():
    """The setters intern through the same tables."""
    ta, tb = (_BarrierStr(s) for s in _fresh("thr-stype", 2))
    ga, gb = (_BarrierStr(s) for s in _fresh("thr-stag", 2))
    atoms = [lh.PrimitiveAtom("C", "", [0.0, 0.0, 0.0]), lh.PrimitiveAtom("C", "", [1.0, 0.0, 0.0])]

    def setter(at, t, g):
        def run():
            at.primitive_type = t
            at.tag = g
        return run

    _BarrierStr.barrier = threading.Barrier(2)
    try:
        _run_threads([setter(atoms[0], ta, ga), setter(atoms[1], tb, gb)])
    finally:
        _BarrierStr.barrier = None
    _check_tables([ta, tb], [ga, gb])
    assert atoms[0]._tid != atoms[1]._tid


def test_intern_stress_and_fast_packing():
    n_threads, rounds, width = 8, 60, 30
    names = [[_fresh(f"thr-st{t}r{r}", width) for r in range(rounds)] for t in range(n_threads)]
    tags = [[_fresh(f"thr-sg{t}r{r}", width) for r in range(rounds)] for t in range(n_threads)]
    made = [[] for _ in range(n_threads)]

    def worker(t):
        def run():
            for r in range(rounds):
                made[t].extend(lh.PrimitiveAtom(ty, tg, [float(k), 0.0, 0.0]) for k, (ty, tg) in enumerate(zip(names[t][r], tags[t][r])))
        return run

    old = sys.getswitchinterval()
    sys.setswitchinterval(1e-6)
    try:
        _run_threads([worker(t) for t in range(n_threads)])
    finally:
        sys.setswitchinterval(old)
    all_types = [n for per in names for r in per for n in r]
    all_tags = [n for per in tags for r in per for n in r]
    _check_tables(all_types, all_tags)
    atoms = [a for per in made for a in per]
    for at in atoms:
        assert api._TYPE_NAMES[at._pid] == at.primitive_type
        assert at._tid == api._TAG_IDS[at.tag]
    # the id gather of _fastpack.pack_atoms (through LoCoHD._type_map) against the string look-up of LoCoHD.pack, atom by atom
    sample = random.Random(5).sample(all_types, 2000)
    lchd = lh.LoCoHD(sample)
    fast = lchd._pack_global(atoms)
    slow = lchd.pack(atoms)
    assert np.array_equal(fast.cat, slow.cat)
    assert (fast.cat >= 0).sum() == len(sample)


def _one_shot_str(action):
    """A str whose first hash runs `action` (later hashes do nothing): it lands inside whichever step hashes it first."""
    state = {"fired": False}

    class S(str):
        def __hash__(self):
            if not state["fired"]:
                state["fired"] = True
                action()
            return str.__hash__(self)

        def __eq__(self, other):
            return str.__eq__(self, other)

    return S, state


def test_setter_pack_window_primitive_type():
    """A pack that runs while primitive_type is being set must not outlive the setter (stale category)."""
    lchd = lh.LoCoHD(["A", "B"])
    atoms = [lh.PrimitiveAtom("A", "", [0.0, 0.0, 0.0]), lh.PrimitiveAtom("A", "", [1.0, 0.0, 0.0])]
    S, state = _one_shot_str(lambda: lchd._packed_lists(atoms, atoms))
    atoms[0].primitive_type = S("B")
    assert state["fired"]
    pa, pb, _ = lchd._packed_lists(atoms, atoms)
    assert pa.cat.tolist() == [1, 0] and pb.cat.tolist() == [1, 0]


def test_setter_pack_window_tag():
    lchd = lh.LoCoHD(["A"])
    atoms = [lh.PrimitiveAtom("A", "t0", [0.0, 0.0, 0.0]), lh.PrimitiveAtom("A", "t0", [1.0, 0.0, 0.0])]
    new_tag = _fresh("thr-wtag", 1)[0]
    S, state = _one_shot_str(lambda: lchd._packed_lists(atoms, atoms))
    atoms[1].tag = S(new_tag)
    assert state["fired"]
    pa, _, interner = lchd._packed_lists(atoms, atoms)
    assert pa.tag.tolist() == [interner["t0"], interner[new_tag]]


class _FakeLib:
    """Stands in for libloco_hd_hip.so: counts handle creation; the create calls sleep so that every thread gets inside."""

    def __init__(self):
        self.lock = threading.Lock()
        self.creates = self.group_creates = self.destroys = self.group_destroys = self.set_det = 0
        self.next = 0x1000

    def _new_handle(self, out):
        with self.lock:
            self.next += 0x10
            out._obj.value = self.next

    def lchd_ctx_create(self, device, out):
        with self.lock:
            self.creates += 1
        time.sleep(0.05)
        self._new_handle(out)
        return 0

    def lchd_group_create(self, devs, n, out):
        with self.lock:
            self.group_creates += 1
        time.sleep(0.05)
        self._new_handle(out)
        return 0

    def lchd_config_validate(self, *a):
        return 0

    def lchd_wf_validate(self, *a):
        return 0

    def lchd_sd_validate(self, *a):
        return 0

    def lchd_ctx_set_deterministic(self, h, on):
        with self.lock:
            self.set_det += 1
        return 0

    def lchd_ctx_destroy(self, h):
        with self.lock:
            self.destroys += 1

    def lchd_group_destroy(self, h):
        with self.lock:
            self.group_destroys += 1

    def lchd_group_last_counts(self, h, out):
        return 0

    def lchd_last_error(self):
        return b"fake"


@pytest.mark.parametrize("kind", ["context", "device_group"])
def test_lazy_handle_created_once(monkeypatch, kind):
    fake = _FakeLib()
    monkeypatch.setattr(N, "_lib", fake)
    if kind == "context":
        lchd = lh.LoCoHD(["A", "B"], deterministic=True)
        get = lchd._context
    else:
        lchd = lh.LoCoHD(["A", "B"], devices=[0, 0])
        get = lchd._device_group
    n = 8
    barrier = threading.Barrier(n)
    got = [None] * n

    def worker(k):
        def run():
            barrier.wait(5.0)
            got[k] = get().value
        return run

    try:
        _run_threads([worker(k) for k in range(n)])
        created = fake.creates if kind == "context" else fake.group_creates
        assert created == 1, f"{created} handles were created for one instance"
        assert len(set(got)) == 1
        if kind == "context":
            assert fake.set_det == 1
    finally:
        lchd.__del__()  # while the fake is still in place: the handles are not real
    assert (fake.destroys if kind == "context" else fake.group_destroys) == 1


def test_pack_and_anchor_caches_shared_by_threads():
    rng = np.random.default_rng(11)
    cats = ["A", "B", "C", "D"]
    lchd = lh.LoCoHD(cats)
    n_lists = lchd._CACHE_ENTRIES + 5
    lists = [[lh.PrimitiveAtom(str(rng.choice(cats)), f"r{int(rng.integers(0, 5))}", rng.uniform(-5, 5, 3).tolist())
              for _ in range(int(rng.integers(5, 40)))] for _ in range(n_lists)]
    anchors = [[(int(i), int(j)) for i, j in rng.integers(0, 5, (int(rng.integers(1, 20)), 2))] for _ in range(n_lists)]
    fresh = lh.LoCoHD(cats)
    want = []
    for k in range(n_lists):
        pa, pb, interner = fresh._packed_lists(lists[k], lists[(k + 1) % n_lists])
        arr, idx = fresh._anchor_arrays(anchors[k])
        want.append((pa, pb, arr.copy(), idx))

    def worker(seed):
        def run():
            r = random.Random(seed)
            for _ in range(300):
                k = r.randrange(n_lists)
                pa, pb, _ = lchd._packed_lists(lists[k], lists[(k + 1) % n_lists])
                arr, idx = lchd._anchor_arrays(anchors[k])
                wa, wb, warr, widx = want[k]
                for got, exp in ((pa, wa), (pb, wb)):
                    assert np.array_equal(got.xyz, exp.xyz) and np.array_equal(got.cat, exp.cat) and np.array_equal(got.tag, exp.tag)
                assert np.array_equal(arr, warr) and idx is None and widx is None
        return run

    old = sys.getswitchinterval()
    sys.setswitchinterval(1e-6)
    try:
        _run_threads([worker(s) for s in range(8)], timeout=60.0)
    finally:
        sys.setswitchinterval(old)
    assert len(lchd._pack_cache) <= lchd._CACHE_ENTRIES
