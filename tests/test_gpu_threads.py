"""LoCoHD, device groups and DeviceSession shared by threads, on the GPU.

The reference's LoCoHD is a Send + Sync pyclass whose drivers take &self (src/locohd.rs:42-55): callers may score from a thread
pool with one instance.  Here the calls on one context (and one device group) are serialised by the C library; these tests run
many threads over shapes that move the context's carried-over state from call to call (sweep hint, environment capacity, side B
used once, leftover slots, second passes over overflowed environments) and compare every threaded result with the serial result
of the same process: bit for bit in deterministic mode, within the 1e-13 that history-dependent kernel choice may give otherwise
(test_gpu_fuzz.py).  Every serial result is checked once against the CPU oracle first.  Threads are joined with a time limit; a
thread still running then fails the test."""
import threading
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TIGHT = 1e-11
DEFAULT_SPREAD = 1e-13
JOIN_S = 100.0
CATS = [f"k{i}" for i in range(10)]


@pytest.fixture(scope="module")
def lh():
    import loco_hd_amd

    return loco_hd_amd


def _run_threads(fns, timeout=JOIN_S):
    errors = []

    def wrap(fn):
        def run():
            try:
                fn()
            except BaseException as e:  # noqa: BLE001 -- re-raised in the main thread
                errors.append(e)
        return run

    ts = [threading.Thread(target=wrap(f), daemon=True) for f in fns]
    for t in ts:
        t.start()
    deadline = time.monotonic() + timeout
    for t in ts:
        t.join(max(0.0, deadline - time.monotonic()))
    assert not any(t.is_alive() for t in ts), f"threads did not finish within {timeout} s"
    if errors:
        raise errors[0]


def _prims(mod, seq, xyz, tags=None):
    tags = [""] * len(seq) if tags is None else tags
    return [mod.PrimitiveAtom(s, t, c) for s, t, c in zip(seq, tags, xyz)]


def _sorted_env(seq, row):
    row = np.asarray(row, dtype=float)
    order = np.argsort(row, kind="stable")
    return [seq[k] for k in order], row[order].tolist()


def _clustered(rng, n_uniform, n_blob, cats):
    """A uniform cloud (~200 points within 10 A) with a dense blob whose environments overflow the 512-point slot."""
    side = (n_uniform / 0.05) ** (1 / 3)
    x = np.concatenate([rng.uniform(0, side, (n_uniform, 3)), side / 2 + rng.normal(0, 2.0, (n_blob, 3))])
    return rng.choice(cats, len(x)).tolist(), x


def _anchors_of_rows(o, seq, row_a, row_b):
    """from_dmxs row = from_anchors of both rows sorted with their prefix of seq (utils.rs:25-39)."""
    (sa, da), (sb, db) = _sorted_env(seq, row_a), _sorted_env(seq, row_b)
    return o.from_anchors(sa, sb, da, db)


class Case:
    """One call shape: run(lchd) -> float64 array; oracle(orc_lchd) -> the oracle's values at `rows` (None: every row)."""

    def __init__(self, name, run, oracle, rows=None):
        self.name, self.run, self.oracle, self.rows = name, run, oracle, rows


def _main_cases(lh, orc, rng):
    cases = []
    # from_primitives, ~2 000 pairs: the one-launch sweep of small calls (INLINE_META) in default mode
    sa, xa = rng.choice(CATS, 2000).tolist(), rng.uniform(0, 34, (2000, 3))
    sb, xb = rng.choice(CATS, 2000).tolist(), rng.uniform(0, 34, (2000, 3))
    ta = [f"r{i // 4}" for i in range(2000)]
    pa, pb = _prims(lh, sa, xa, ta), _prims(lh, sb, xb, ta)
    oa, ob = _prims(orc, sa, xa, ta), _prims(orc, sb, xb, ta)
    small = [(i, (7 * i) % 2000) for i in range(2000)]
    cases.append(Case("prims_small", lambda l: np.asarray(l.from_primitives(pa, pb, small, 9.0)),
                      lambda o: np.asarray(o.from_primitives(oa, ob, small, 9.0))))
    # from_primitives, 1.5e5 pairs; about 5 % of the anchors (fewer than the 1/8 that rescore_overflow_pairs takes) lie in or
    # next to a blob whose environments overflow the 512-point slot
    ca, ya = _clustered(rng, 20000, 800, CATS)
    cb, yb = _clustered(rng, 20000, 800, CATS)
    qa, qb = _prims(lh, ca, ya), _prims(lh, cb, yb)
    big = list(zip(rng.integers(0, len(ya), 150_000).tolist(), rng.integers(0, len(yb), 150_000).tolist()))
    sample = np.sort(rng.choice(len(big), 1500, replace=False))
    big_sample = [big[k] for k in sample]
    cases.append(Case("prims_big", lambda l: np.asarray(l.from_primitives(qa, qb, big, 10.0)),
                      lambda o: np.asarray(o.from_primitives(_prims(orc, ca, ya), _prims(orc, cb, yb), big_sample, 10.0)),
                      rows=sample))
    # from_coords: n = 1 500 (dense) and n = 300
    for n in (1500, 300):
        s1, s2 = rng.choice(CATS, n).tolist(), rng.choice(CATS, n).tolist()
        x1, x2 = rng.uniform(0, 25, (n, 3)), rng.uniform(0, 25, (n, 3))
        cases.append(Case(f"coords_{n}", lambda l, s1=s1, s2=s2, x1=x1, x2=x2: np.asarray(l.from_coords(s1, s2, x1, x2)),
                          lambda o, s1=s1, s2=s2, x1=x1, x2=x2: np.asarray(o.from_coords(s1, s2, x1, x2))))
    # ragged from_dmxs with +inf entries
    n = 260
    sq, xq = rng.choice(CATS, n).tolist(), rng.uniform(0, 20, (n, 3))
    full = np.sqrt(((xq[:, None, :] - xq[None, :, :]) ** 2).sum(-1))
    full2 = full * rng.uniform(0.9, 1.1, full.shape)
    np.fill_diagonal(full2, 0.0)
    lens = rng.integers(60, n + 1, 200)
    ra, rb = [], []
    for i in range(200):
        L = max(int(lens[i]), i + 1)
        r1, r2 = full[i, :L].copy(), full2[i, :n].copy()
        r1[rng.random(L) < 0.1] = np.inf
        r2[rng.random(n) < 0.1] = np.inf
        r1[i] = r2[i] = 0.0
        ra.append(r1.tolist())
        rb.append(r2.tolist())
    cases.append(Case("dmxs_ragged", lambda l: np.asarray(l.from_dmxs(sq, sq, ra, rb)),
                      lambda o: np.asarray([_anchors_of_rows(o, sq, ra[i], rb[i]) for i in range(200)])))
    # from_anchors
    la, lb = int(rng.integers(300, 500)), int(rng.integers(300, 500))
    da = np.concatenate([[0.0], np.sort(rng.uniform(0, 15, la - 1))]).tolist()
    db = np.concatenate([[0.0], np.sort(rng.uniform(0, 15, lb - 1))]).tolist()
    xa_, xb_ = rng.choice(CATS, la).tolist(), rng.choice(CATS, lb).tolist()
    cases.append(Case("anchors", lambda l: np.asarray([l.from_anchors(xa_, xb_, da, db)]),
                      lambda o: np.asarray([o.from_anchors(xa_, xb_, da, db)])))
    # from_coords_ensemble, M = 4, n = 500
    se = rng.choice(CATS, 500).tolist()
    xe = rng.uniform(0, 22, (500, 3))
    xs = np.stack([xe + rng.normal(0, 0.8, xe.shape) for _ in range(4)])
    pairs = [(i, j) for i in range(4) for j in range(i + 1, 4)]
    cases.append(Case("ensemble", lambda l: np.asarray(l.from_coords_ensemble(se, xs)).reshape(-1),
                      lambda o: np.concatenate([np.asarray(o.from_coords(se, se, xs[i], xs[j])) for i, j in pairs])))
    # from_primitives_batch: two structures, three jobs
    structs = [_prims(lh, sa[:600], xa[:600]), _prims(lh, sb[:500], xb[:500])]
    jobs = [(0, 1, [(i, i) for i in range(0, 500, 2)]), (1, 0, [(i, 599 - i) for i in range(0, 500, 3)]), (0, 0, [(i, i) for i in range(600)])]

    def batch_oracle(o):
        st = [_prims(orc, sa[:600], xa[:600]), _prims(orc, sb[:500], xb[:500])]
        return np.concatenate([np.asarray(o.from_primitives(st[a], st[b], pr, 8.0)) for a, b, pr in jobs])

    cases.append(Case("batch", lambda l: np.concatenate([np.asarray(r) for r in l.from_primitives_batch(structs, jobs, 8.0)]),
                      batch_oracle))
    return cases


def _make_main(mod, deterministic):
    wf = mod.WeightFunction("hyper_exp", [1.0, 0.15])
    if mod.__name__.startswith("loco_hd_amd"):
        return mod.LoCoHD(CATS, wf, deterministic=deterministic)
    return mod.LoCoHD(CATS, wf)


def _second_cases(lh, orc, rng):
    """300 categories, Kullback-Leibler with eps = 1e-10: the wide sweeps and (default mode) the incremental one."""
    cats = [f"w{i}" for i in range(300)]
    sa, xa = rng.choice(cats, 3000).tolist(), rng.uniform(0, 40, (3000, 3))
    sb, xb = rng.choice(cats, 3000).tolist(), rng.uniform(0, 40, (3000, 3))
    pa, pb = _prims(lh, sa, xa), _prims(lh, sb, xb)
    pairs = [(i, (i * 13) % 3000) for i in range(0, 3000, 2)]
    sc, xc = rng.choice(cats, 700).tolist(), rng.uniform(0, 20, (700, 3))
    xd = xc + rng.normal(0, 0.5, xc.shape)

    def make(mod):
        return mod.LoCoHD(cats, mod.WeightFunction("uniform", [2.0, 9.0]), statistical_distance=mod.StatisticalDistance("Kullback-Leibler", [1e-10]))

    cases = [Case("wide_prims", lambda l: np.asarray(l.from_primitives(pa, pb, pairs, 10.0)),
                  lambda o: np.asarray(o.from_primitives(_prims(orc, sa, xa), _prims(orc, sb, xb), pairs, 10.0))),
             Case("wide_coords", lambda l: np.asarray(l.from_coords(sc, sc, xc, xd)), lambda o: np.asarray(o.from_coords(sc, sc, xc, xd)))]
    return make, cases


def _third_cases(lh, orc, rng):
    """A weight-function dictionary with per-pair keys."""
    sa, xa = rng.choice(CATS, 1500).tolist(), rng.uniform(0, 30, (1500, 3))
    sb, xb = rng.choice(CATS, 1500).tolist(), rng.uniform(0, 30, (1500, 3))
    pa, pb = _prims(lh, sa, xa), _prims(lh, sb, xb)
    keys = ["a", "b", "c"]
    pairs = [(i, (i * 7) % 1500, keys[i % 3]) for i in range(1500)]
    s, x1 = rng.choice(CATS, 400).tolist(), rng.uniform(0, 18, (400, 3))
    x2 = x1 + rng.normal(0, 0.6, x1.shape)
    rowkeys = [keys[(i * 5) % 3] for i in range(400)]

    def make(mod, **kw):
        wfs = {"a": mod.WeightFunction("uniform", [3.0, 10.0]), "b": mod.WeightFunction("dagum", [2.0, 4.0, 1.5]),
               "c": mod.WeightFunction("kumaraswamy", [1.0, 9.0, 2.0, 3.0])}
        return mod.LoCoHD(CATS, wfs, **kw)

    cases = [Case("dict_prims", lambda l: np.asarray(l.from_primitives(pa, pb, pairs, 9.5)),
                  lambda o: np.asarray(o.from_primitives(_prims(orc, sa, xa), _prims(orc, sb, xb), pairs, 9.5))),
             Case("dict_coords", lambda l: np.asarray(l.from_coords(s, s, x1, x2, rowkeys)),
                  lambda o: np.asarray(o.from_coords(s, s, x1, x2, rowkeys)))]
    return make, cases


def _check_oracle(cases, ref, serial):
    for c in cases:
        got = serial[c.name] if c.rows is None else serial[c.name][c.rows]
        want = c.oracle(ref)
        assert got.shape == want.shape, c.name
        err = float(np.max(np.abs(got - want)))
        assert err <= TIGHT, f"{c.name}: |hip - oracle| = {err}"


def _worker(lchd, cases, serial, seed, calls, exact, bad=None):
    """Run `calls` calls in a seeded random order; every result must equal (or, exact=False, lie within 1e-13 of) serial."""
    def run():
        r = np.random.default_rng(seed)
        order = np.concatenate([r.permutation(len(cases)) for _ in range(-(-calls // len(cases)))])[:calls]
        for k, ci in enumerate(order):
            c = cases[int(ci)]
            if bad is not None and k % 3 == 0:
                bad()
            got = c.run(lchd)
            want = serial[c.name]
            if exact:
                assert got.tobytes() == want.tobytes(), f"{c.name}: threaded result differs from serial (call {k})"
            else:
                err = float(np.max(np.abs(got - want)))
                assert err <= DEFAULT_SPREAD, f"{c.name}: threaded result {err} from serial (call {k})"
    return run


@pytest.mark.parametrize("deterministic", [True, False], ids=["deterministic", "default"])
def test_shared_instances(lh, oracle, deterministic):
    rng = np.random.default_rng(2024)
    main_cases = _main_cases(lh, oracle, rng)
    make2, cases2 = _second_cases(lh, oracle, rng)
    make3, cases3 = _third_cases(lh, oracle, rng)
    main = _make_main(lh, deterministic)
    second = make2(lh)  # default mode: the incremental Kullback-Leibler sweep
    third = make3(lh, deterministic=True)
    serial = {}
    for lchd, cases in ((main, main_cases), (second, cases2), (third, cases3)):
        for c in cases:
            serial[c.name] = c.run(lchd)
    for c in main_cases:  # the serial values are right, and a second serial call repeats them
        again = c.run(main)
        if deterministic:
            assert again.tobytes() == serial[c.name].tobytes(), c.name
    _check_oracle(main_cases, _make_main(oracle, False), serial)
    _check_oracle(cases2, make2(oracle), serial)
    _check_oracle(cases3, make3(oracle), serial)
    lib, ctx = lh._native.lib(), main._context()
    subset_before = lib.lchd_ctx_subset_pass_count(ctx)
    assert subset_before > 0, "the 1.5e5-pair shape ran no second pass over overflowed environments"

    # one thread also makes calls with an out-of-range anchor: it gets its own PanicException every time
    sa = [lh.PrimitiveAtom("k0", "", [0.0, 0.0, 0.0]), lh.PrimitiveAtom("k1", "", [1.0, 0.0, 0.0])]
    with pytest.raises(lh.PanicException) as ei:
        main.from_primitives(sa, sa, [(0, 0), (5, 1)], 5.0)
    bad_msg = str(ei.value)
    assert "anchor index is outside its structure" in bad_msg
    bad_count = [0]

    def bad():
        try:
            main.from_primitives(sa, sa, [(0, 0), (5, 1)], 5.0)
        except lh.PanicException as e:
            assert str(e) == bad_msg
            bad_count[0] += 1
        else:
            raise AssertionError("an out-of-range anchor did not raise")

    workers = [_worker(main, main_cases, serial, 100 + t, 104, deterministic, bad=bad if t == 0 else None) for t in range(4)]
    workers += [_worker(second, cases2, serial, 200 + t, 40, False) for t in range(2)]
    workers += [_worker(third, cases3, serial, 300 + t, 40, True) for t in range(2)]
    _run_threads(workers)
    assert bad_count[0] == 35
    assert lib.lchd_ctx_subset_pass_count(ctx) > subset_before


def test_instance_per_thread(lh, oracle):
    """The documented way to score in parallel: one LoCoHD per thread."""
    rng = np.random.default_rng(77)
    cases = [c for c in _main_cases(lh, oracle, rng) if c.name in ("prims_small", "coords_300", "dmxs_ragged", "anchors", "ensemble")]
    ref = _make_main(lh, True)
    serial = {c.name: c.run(ref) for c in cases}
    _check_oracle(cases, _make_main(oracle, False), serial)
    own = [_make_main(lh, True) for _ in range(4)]
    _run_threads([_worker(own[t], cases, serial, 400 + t, 50, True) for t in range(4)])


def test_shared_device_group(lh, oracle):
    """One LoCoHD(devices=[0, 0]) used by three threads.  A group picks kernels per share (deterministic=True is refused for
    it), so threaded results are held to the 1e-13 of default mode against serial group calls."""
    rng = np.random.default_rng(91)
    sa, xa = rng.choice(CATS, 4000).tolist(), rng.uniform(0, 43, (4000, 3))
    sb, xb = rng.choice(CATS, 4000).tolist(), rng.uniform(0, 43, (4000, 3))
    pa, pb = _prims(lh, sa, xa), _prims(lh, sb, xb)
    p1 = [(i, (i * 11) % 4000) for i in range(4000)]
    p2 = list(zip(rng.integers(0, 4000, 30000).tolist(), rng.integers(0, 4000, 30000).tolist()))
    grp = lh.LoCoHD(CATS, lh.WeightFunction("hyper_exp", [1.0, 0.15]), devices=[0, 0])
    cases = [Case("g1", lambda l: np.asarray(l.from_primitives(pa, pb, p1, 9.0)), None),
             Case("g2", lambda l: np.asarray(l.from_primitives(pa, pb, p2, 9.0)), None)]
    serial = {c.name: c.run(grp) for c in cases}
    assert sum(grp.last_group_counts()) == len(p2) and min(grp.last_group_counts()) > 0
    orc = oracle.LoCoHD(CATS, oracle.WeightFunction("hyper_exp", [1.0, 0.15]))
    oa, ob = _prims(oracle, sa, xa), _prims(oracle, sb, xb)
    assert float(np.max(np.abs(serial["g1"] - np.asarray(orc.from_primitives(oa, ob, p1, 9.0))))) <= TIGHT
    assert float(np.max(np.abs(serial["g2"][:2000] - np.asarray(orc.from_primitives(oa, ob, p2[:2000], 9.0))))) <= TIGHT
    _run_threads([_worker(grp, cases, serial, 500 + t, 40, False) for t in range(3)])


def test_shared_device_session(lh, oracle):
    """Thread A: from_primitives_async + finish; thread B: from_coords on the same DeviceSession.  B's calls wait for A's finish:
    neither ever sees "asynchronous call has not been finished"."""
    import torch

    from loco_hd_amd.device import DeviceSession

    rng = np.random.default_rng(5)
    lchd = lh.LoCoHD(CATS, lh.WeightFunction("hyper_exp", [1.0, 0.15]))
    sess = DeviceSession(lchd)
    sess.set_deterministic(True)
    try:
        n = 3000
        ca, cb = rng.integers(0, 10, n).astype(np.int32), rng.integers(0, 10, n).astype(np.int32)
        xa, xb = rng.uniform(0, 39, (n, 3)), rng.uniform(0, 39, (n, 3))
        ha, hb = sess.upload(xa, ca), sess.upload(xb, cb)
        m = 800
        hc, hd = sess.upload(xa[:m], ca[:m]), sess.upload(xb[:m], cb[:m])
        pairs = np.stack([rng.integers(0, n, 20000), rng.integers(0, n, 20000)], 1).astype(np.int64)
        anchors = torch.from_numpy(pairs).cuda()

        def prims_call():
            out = torch.empty(len(pairs), dtype=torch.float64, device="cuda")
            sess.from_primitives_async(ha, hb, anchors, 9.0, out)
            sess.finish()
            return out.cpu().numpy()

        def coords_call():
            return sess.from_coords(hc, hd).cpu().numpy()

        want_p, want_c = prims_call(), coords_call()
        orc = oracle.LoCoHD(CATS, oracle.WeightFunction("hyper_exp", [1.0, 0.15]))
        assert float(np.max(np.abs(want_p[:1500] - np.asarray(orc.from_arrays(xa, ca, np.zeros(n, np.int32), xb, cb, np.zeros(n, np.int32),
                                                                             pairs[:1500], 9.0))))) <= TIGHT
        seq_a, seq_b = [CATS[k] for k in ca[:m]], [CATS[k] for k in cb[:m]]
        assert float(np.max(np.abs(want_c - np.asarray(orc.from_coords(seq_a, seq_b, xa[:m], xb[:m]))))) <= TIGHT

        def loop(fn, want, reps):
            def run():
                for k in range(reps):
                    got = fn()
                    assert got.tobytes() == want.tobytes(), f"call {k} differs from serial"
            return run

        _run_threads([loop(prims_call, want_p, 150), loop(coords_call, want_c, 150)])
    finally:
        sess.close()
