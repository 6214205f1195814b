"""Stream ordering of the device API (DeviceSession, the *_dev / _async entry points, frames buffers) with delayed producers.

An ordering bug is invisible while the racing work is short.  Here the producer is held back: a long delay is put on the
stream, the write of the RIGHT data is queued behind it, and the buffer meanwhile holds OTHER, VALID data (in-range anchors,
finite coordinates with the same bounding box, in-range weight-function indices).  Code that does not wait scores the stale
data and disagrees with the oracle every time; nothing here can fault the device.

Every result is compared with the CPU oracle at 1e-11 and -- sessions in deterministic mode -- bit for bit with the same call
made on the default stream with complete, host-synchronised inputs (the `ref` fixture).

The delay is `torch.cuda._sleep(cycles)` (a chain of torch kernels if this torch has none), calibrated once per module with
events: at least 20 times the longest undelayed library call of the module (host enqueue to return), at least 10 ms, at most
200 ms.  `test_control_*` prove on the machine that the construct exposes a missing wait (torch only, no library call); if they
do not see the stale value the module fails.  Streams come from `Delay.streams`, which hands out only streams that the device is
seen to run side by side: two streams that share a hardware queue run in submission order, and a delay on one would hold the
other back as well, so that a missing wait between them could not show.  The calibrated cycles, the achieved delay and the undelayed call times are written
to profiles/r09/stream_delays.json.

The stream contract these tests enforce is written down in include/loco_hd_hip.h ("Streams") and INTEGRATION.md.
"""
import json
import os
import time
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
TIGHT = 1e-11
SENTINEL = -7.0  # (scores are >= 0)
THR = 8.0
MIN_DELAY_MS, MAX_DELAY_MS, CALL_FACTOR = 10.0, 200.0, 20.0


# ------------------------------------------------------------------------------------------------------------------------
# the delay
# ------------------------------------------------------------------------------------------------------------------------
class Delay:
    """Enqueue ~`ms` of idle GPU time on a torch stream."""

    def __init__(self, torch):
        self.torch = torch
        self.native = hasattr(torch.cuda, "_sleep")
        self._pad = torch.zeros(1 << 22, device="cuda")
        self.unit = 2_000_000 if self.native else 8  # cycles / kernels in a chain
        self.per_ms = None
        self.amount = None
        self.ms = None
        self.achieved_ms = None
        self.passed_over = 0

    def _enqueue(self, amount):
        if self.native:
            self.torch.cuda._sleep(int(amount))
        else:
            for _ in range(int(amount)):
                self._pad.add_(1.0)

    def _measure(self, amount):
        torch = self.torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        self._enqueue(amount)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def calibrate(self, target_ms):
        self._measure(self.unit)  # warm-up
        self.per_ms = max(self.unit / max(self._measure(self.unit), 1e-3), 1.0)
        self.ms = target_ms
        self.amount = int(np.ceil(target_ms * self.per_ms))
        self.achieved_ms = self._measure(self.amount)
        if self.achieved_ms < target_ms:  # clock moved between the two measurements: scale once more
            self.amount = int(np.ceil(self.amount * 1.25 * target_ms / max(self.achieved_ms, 1e-3)))
            self.achieved_ms = self._measure(self.amount)

    def on(self, stream):
        with self.torch.cuda.stream(stream):
            self._enqueue(self.amount)

    def _runs_beside(self, busy, other):
        """True if work queued on `other` completes while `busy` is held by a short delay (a tenth of the calibrated one)."""
        torch = self.torch
        torch.cuda.synchronize()
        done = torch.cuda.Event()
        with torch.cuda.stream(busy):
            self._enqueue(max(self.amount // 10, 1))
            done.record(busy)
        with torch.cuda.stream(other):
            self._pad[:64].add_(1.0)
        other.synchronize()
        beside = not done.query()
        busy.synchronize()
        return beside

    def streams(self, k):
        """k torch streams that the device runs side by side, each pair probed in both directions.  The runtime spreads its
        streams over a few hardware queues; two streams that share one run their work in submission order, and a delay on one
        would then hold the other back as well -- a missing wait between them could not show.  Such candidates are passed over
        (torch hands out its pooled streams in turn); if no set is found the test fails."""
        chosen = []
        for _ in range(32):
            cand = self.torch.cuda.Stream()
            if all(self._runs_beside(x, cand) and self._runs_beside(cand, x) for x in chosen):
                chosen.append(cand)
            else:
                self.passed_over += 1
                print(f"stream {cand.cuda_stream:#x} runs in submission order with an earlier one: passed over ({self.passed_over} so far)")
            if len(chosen) == k:
                return chosen
        pytest.fail(f"no {k} streams that run side by side among 32 candidates: a delay on one stream holds the others back")


# ------------------------------------------------------------------------------------------------------------------------
# data, configurations and the default-stream reference
# ------------------------------------------------------------------------------------------------------------------------
def _cloud(rng, n, n_cat, side):
    x = rng.uniform(0.0, side, (n, 3))
    x[0], x[1] = 0.0, side  # two fixed corners: every variant of a structure has the same bounding box
    return x, rng.integers(0, n_cat, n).astype(np.int32)


def _pairs(rng, n, p):
    return np.stack([rng.integers(0, n, p), rng.integers(0, n, p)], 1).astype(np.int64)


class Config:
    """One LoCoHD configuration with its data: clouds (xa, ca), (xb, cb), a second coordinate set xb2 for side B, anchor lists
    (real and stale) and, for a weight-function dictionary, per-pair / per-row function indices (real and stale)."""

    def __init__(self, name, seed, n_cat, w_func, n, n_small, p_big, p_small):
        rng = np.random.default_rng(seed)
        self.name, self.n, self.n_small = name, n, n_small
        self.cats = [f"c{i}" for i in range(n_cat)]
        self.w_func = w_func  # (name, params) or {key: (name, params)}
        side = (n / 0.04) ** (1 / 3)
        self.xa, self.ca = _cloud(rng, n, n_cat, side)
        self.xb, self.cb = _cloud(rng, n, n_cat, side)
        self.xb2 = _cloud(rng, n, n_cat, side)[0]
        self.tag = np.zeros(n, dtype=np.int32)
        self.anc_big, self.anc_big_stale = _pairs(rng, n, p_big), _pairs(rng, n, p_big)
        self.anc_small, self.anc_small_stale = _pairs(rng, n_small, p_small), _pairs(rng, n_small, p_small)
        self.dict = isinstance(w_func, dict)
        nk = len(w_func) if self.dict else 1

        def wf(k):
            return rng.integers(0, nk, k).astype(np.int32) if self.dict else None

        self.wf_big, self.wf_big_stale = wf(p_big), wf(p_big)
        self.wf_small, self.wf_small_stale = wf(p_small), wf(p_small)
        self.wf_rows, self.wf_rows_small = wf(n), wf(n_small)
        # ensemble: M structures of n_ens atoms of one topology
        self.m, self.n_ens = 5, 160
        self.ens_cat = rng.integers(0, n_cat, self.n_ens).astype(np.int32)
        self.ens_x = rng.uniform(0.0, 18.0, (self.m, self.n_ens, 3))
        self.ens_pairs = np.array([[0, 1], [3, 2], [4, 4], [1, 4], [2, 0], [3, 1]], dtype=np.int32)
        self.ens_pairs_stale = np.array([[4, 0], [1, 1], [2, 3], [0, 3], [4, 2], [0, 0]], dtype=np.int32)
        self.wf_ens = wf(self.n_ens)

    def make(self, mod, **kw):
        def one(spec):
            return mod.WeightFunction(spec[0], list(spec[1]))

        w = {k: one(v) for k, v in self.w_func.items()} if self.dict else one(self.w_func)
        return mod.LoCoHD(self.cats, w, **kw)

    def keys(self, idx):
        names = list(self.w_func)
        return None if idx is None else [names[i] for i in idx]


def _configs():
    return {
        "A": Config("A", 1, 7, ("hyper_exp", [1.0, 0.15]), n=1200, n_small=300, p_big=6000, p_small=200),
        "W": Config("W", 2, 300, ("hyper_exp", [1.0, 0.12]), n=1100, n_small=300, p_big=5000, p_small=200),  # > 255 categories
        "D": Config("D", 3, 6, {"near": ("uniform", [1.0, 6.0]), "far": ("hyper_exp", [1.0, 0.2])}, n=1100, n_small=300, p_big=5000,
                    p_small=200),
    }


CALLS = ("prims_small", "prims_big", "coords_small", "coords_big", "ensemble")


class Bench:
    """A session with one configuration's structures uploaded; `call(kind, ...)` runs one of CALLS and returns a CUDA tensor."""

    def __init__(self, env, cfg, deterministic):
        self.env, self.cfg, torch = env, cfg, env.torch
        self.lchd = cfg.make(env.lh, deterministic=deterministic)
        self.sess = env.DeviceSession(self.lchd)
        s, c = self.sess, cfg
        k = c.n_small
        self.a, self.b = s.upload(c.xa, c.ca), s.upload(c.xb, c.cb)
        self.a_s, self.b_s = s.upload(c.xa[:k], c.ca[:k]), s.upload(c.xb[:k], c.cb[:k])
        self.batch, _ = s.upload_batch([(c.ens_x[i], c.ens_cat) for i in range(c.m)])
        torch.cuda.synchronize()

    def dev(self, arr):
        """A complete device copy of a host array (None passes through), made on the current stream and waited for."""
        if arr is None:
            return None
        t = self.env.torch.from_numpy(np.ascontiguousarray(arr)).cuda()
        self.env.torch.cuda.current_stream().synchronize()
        return t

    def inputs(self, kind, stale=False):
        """(anchors or pairs, wf_index) host arrays of a call kind."""
        c = self.cfg
        if kind == "prims_small":
            return (c.anc_small_stale, c.wf_small_stale) if stale else (c.anc_small, c.wf_small)
        if kind == "prims_big":
            return (c.anc_big_stale, c.wf_big_stale) if stale else (c.anc_big, c.wf_big)
        if kind == "coords_small":
            return None, c.wf_rows_small
        if kind == "coords_big":
            return None, c.wf_rows
        return (c.ens_pairs_stale if stale else c.ens_pairs), c.wf_ens

    def call(self, kind, first=None, wf=None, out=None, use_async=False):
        s = self.sess
        if first is None and wf is None:
            h_first, h_wf = self.inputs(kind)
            first, wf = self.dev(h_first), self.dev(h_wf)
        if kind in ("prims_small", "prims_big"):
            a, b = (self.a_s, self.b_s) if kind == "prims_small" else (self.a, self.b)
            if use_async:
                if out is None:
                    out = self.env.torch.empty(first.shape[0], dtype=self.env.torch.float64, device="cuda")
                s.from_primitives_async(a, b, first, THR, out, wf_index=wf)
                s.finish()
                return out
            return s.from_primitives(a, b, first, THR, out=out, wf_index=wf)
        if kind in ("coords_small", "coords_big"):
            a, b = (self.a_s, self.b_s) if kind == "coords_small" else (self.a, self.b)
            return s.from_coords(a, b, out=out, wf_index=wf)
        return s.from_coords_ensemble(self.batch, pairs=first, out=out, wf_index=wf)

    def close(self):
        self.sess.close()


def _oracle_of(orc, cfg, kind):
    c = cfg
    o = c.make(orc)
    k = c.n_small
    if kind in ("prims_small", "prims_big"):
        small = kind == "prims_small"
        xa, ca, xb, cb = (c.xa[:k], c.ca[:k], c.xb[:k], c.cb[:k]) if small else (c.xa, c.ca, c.xb, c.cb)
        anc, wf = (c.anc_small, c.wf_small) if small else (c.anc_big, c.wf_big)
        wfs, idx = o._wfs(c.keys(wf), len(anc))
        tag = np.zeros(len(xa), dtype=np.int32)
        return np.asarray(o.from_arrays(xa, ca, tag, xb, cb, tag, anc, THR, wfs=wfs, wf_idx=idx))
    if kind in ("coords_small", "coords_big"):
        small = kind == "coords_small"
        xa, ca, xb, cb = (c.xa[:k], c.ca[:k], c.xb[:k], c.cb[:k]) if small else (c.xa, c.ca, c.xb, c.cb)
        wf = c.wf_rows_small if small else c.wf_rows
        return np.asarray(o.from_coords([c.cats[i] for i in ca], [c.cats[i] for i in cb], xa, xb, c.keys(wf)))
    seq = [c.cats[i] for i in c.ens_cat]
    return np.asarray([o.from_coords(seq, seq, c.ens_x[i], c.ens_x[j], c.keys(c.wf_ens)) for i, j in c.ens_pairs])


@pytest.fixture(scope="module")
def env(oracle):
    import torch

    import loco_hd_amd as lh
    from loco_hd_amd.device import DeviceSession

    return SimpleNamespace(torch=torch, lh=lh, DeviceSession=DeviceSession, orc=oracle, cfgs=_configs(), call_ms={})


@pytest.fixture(scope="module")
def ref(env):
    """Every call kind of every configuration on the DEFAULT stream with complete inputs: deterministic mode (the bit pattern the
    stream tests must reproduce), checked against the oracle here; the undelayed call times feed the delay's calibration."""
    want, bits = {}, {}
    for name, cfg in env.cfgs.items():
        b = Bench(env, cfg, deterministic=True)
        for kind in CALLS:
            b.call(kind)  # warm-up (workspace growth, first launches)
            env.torch.cuda.synchronize()
            first, wf = (b.dev(x) for x in b.inputs(kind))
            t0 = time.perf_counter()
            got = b.call(kind, first, wf)
            env.call_ms[f"{name}.{kind}"] = (time.perf_counter() - t0) * 1e3
            env.torch.cuda.synchronize()
            bits[name, kind] = got.cpu().numpy().copy()
            want[name, kind] = _oracle_of(env.orc, cfg, kind).reshape(bits[name, kind].shape)
            err = float(np.max(np.abs(bits[name, kind] - want[name, kind])))
            assert err < TIGHT, (name, kind, err)
        if name == "A":  # the other library calls the module makes, undelayed (each once warm, once timed)
            from loco_hd_amd.dist import score_sharded

            anc = b.dev(cfg.anc_big)
            others = {
                "upload": lambda: b.sess.upload(cfg.xb, cfg.cb),
                "upload_batch": lambda: b.sess.upload_batch([(cfg.ens_x[i], cfg.ens_cat) for i in range(cfg.m)]),
                "set_coords": lambda: b.sess.set_coords(b.b, cfg.xb),
                "use_current_stream": lambda: b.sess.use_current_stream(),
                "second_session": lambda: Bench(env, env.cfgs["D"], deterministic=True).close(),
                "score_sharded": lambda: score_sharded(lambda sub: b.sess.from_primitives(b.a, b.b, sub, THR), anc, 1, 0, n_atoms_a=cfg.n,
                                                       session=b.sess),
            }
            for what, fn in others.items():
                fn()
                env.torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                env.call_ms[f"A.{what}"] = (time.perf_counter() - t0) * 1e3
                env.torch.cuda.synchronize()
        b.close()
    return SimpleNamespace(want=want, bits=bits)


@pytest.fixture(scope="module")
def frames(env, ref):
    """Trajectory data on configuration A's small structure: source atoms (two per primitive atom) of frame sets X, Y and a set
    with one NaN; their centroids as the library evaluates them (read back on the default stream); the scores of X and Y."""
    torch, cfg = env.torch, env.cfgs["A"]
    rng = np.random.default_rng(77)
    nt, nf = cfg.n_small, 3
    side = 20.0

    def sources():
        c = rng.uniform(0.0, side, (nf, nt, 3))
        c[:, 0], c[:, 1] = 0.0, side
        d = rng.uniform(-0.5, 0.5, (nf, nt, 3))
        d[:, :2] = 0.0
        return np.stack([c - d, c + d], 2).reshape(nf, 2 * nt, 3).astype(np.float32)

    topo = SimpleNamespace(src_start=np.arange(0, 2 * nt + 1, 2, dtype=np.int32), src_idx=np.arange(2 * nt, dtype=np.int32), n_atoms=2 * nt)
    lp = np.stack([rng.integers(0, nt, 400), rng.integers(0, nt, 400)], 1).astype(np.int64)
    anchors = np.concatenate([lp + np.array([0, f * nt]) for f in range(nf)]).astype(np.int64)
    ens_pairs = np.array([[0, 1], [2, 0], [1, 2]], dtype=np.int32)
    fr = SimpleNamespace(nt=nt, nf=nf, topo=topo, lp=lp, anchors=anchors, ens_pairs=ens_pairs, src={}, xyz={}, bits={}, ens_bits={},
                         x_ref=cfg.xa[:nt] * (side / cfg.xa[:nt].max()), cat=cfg.ca[:nt])
    b = Bench(env, cfg, deterministic=True)
    s = b.sess
    tmpl = s.upload(fr.x_ref, fr.cat)
    buf = s.frames_buffer(tmpl, nf)
    s.set_frame_sources(buf, topo)
    o = cfg.make(env.orc)
    seq = [cfg.cats[i] for i in fr.cat]
    tag = np.zeros(nt, dtype=np.int32)
    anc_d, ens_d = b.dev(anchors), b.dev(ens_pairs)
    for key in ("X", "Y"):
        fr.src[key] = sources()
        s.load_atom_frames(buf, fr.src[key])
        t0 = time.perf_counter()
        got = s.from_primitives(tmpl, buf, anc_d, THR)
        env.call_ms[f"frames.prims.{key}"] = (time.perf_counter() - t0) * 1e3
        fr.bits[key] = got.cpu().numpy().copy()
        fr.xyz[key] = s.coords_of(buf, nf * nt).reshape(nf, nt, 3)
        fr.ens_bits[key] = s.from_coords_ensemble(buf, pairs=ens_d).cpu().numpy().copy()
        want = np.concatenate([o.from_arrays(fr.x_ref, fr.cat, tag, fr.xyz[key][f], fr.cat, tag, lp, THR) for f in range(nf)])
        assert float(np.max(np.abs(fr.bits[key] - want))) < TIGHT
        want_e = np.asarray([o.from_coords(seq, seq, fr.xyz[key][i], fr.xyz[key][j]) for i, j in ens_pairs])
        assert float(np.max(np.abs(fr.ens_bits[key] - want_e))) < TIGHT
    assert not np.array_equal(fr.bits["X"], fr.bits["Y"])
    t0 = time.perf_counter()
    s.load_atom_frames(buf, fr.src["Y"])
    env.call_ms["frames.load_atom_frames"] = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s.load_frames(buf, fr.xyz["Y"])
    env.call_ms["frames.load_frames"] = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    src_dev = torch.from_numpy(fr.src["Y"]).cuda()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s.load_atom_frames_dev(buf, src_dev)
    env.call_ms["frames.load_atom_frames_dev"] = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s.coords_of(buf, nf * nt)
    env.call_ms["frames.coords_of"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    s.from_coords_ensemble(buf, pairs=ens_d)
    env.call_ms["frames.ensemble"] = (time.perf_counter() - t0) * 1e3
    # score_trajectory is many library calls (two buffers made, a load and a pass per chunk); timed as a whole, the longest of them
    # cannot be longer.  Eleven frames in chunks of two, as the test below runs it.
    traj = np.concatenate([fr.src["X"], fr.src["Y"], fr.src["X"], fr.src["Y"][:2]])
    for what, kw, data in (("score_trajectory", {}, np.concatenate([fr.xyz["X"], fr.xyz["Y"], fr.xyz["X"], fr.xyz["Y"][:2]])),
                           ("score_trajectory_topology", {"topology": _Topology(topo, nt)}, traj)):
        s.score_trajectory(tmpl, data, lp, THR, chunk=2, **kw)
        t0 = time.perf_counter()
        s.score_trajectory(tmpl, data, lp, THR, chunk=2, **kw)
        env.call_ms[f"frames.{what}"] = (time.perf_counter() - t0) * 1e3
    bad = fr.src["Y"].copy()
    bad[1, 2 * 17, 1] = np.nan
    fr.src["bad"] = bad
    xb = fr.xyz["Y"].copy()
    xb[1, 17, 1] = np.nan
    fr.xyz["bad"] = xb
    b.close()
    return fr


@pytest.fixture(scope="module")
def delay(env, ref, frames):
    """Calibrated after `ref` and `frames` have measured the undelayed calls."""
    d = Delay(env.torch)
    longest = max(env.call_ms.values())
    d.calibrate(min(MAX_DELAY_MS, max(MIN_DELAY_MS, CALL_FACTOR * longest)))
    record = {"sleep": "torch.cuda._sleep" if d.native else "chain of torch kernels", "amount": d.amount, "target_ms": d.ms,
              "achieved_ms": d.achieved_ms, "amount_per_ms": d.per_ms, "longest_undelayed_call_ms": longest,
              "capped_at_200_ms": bool(CALL_FACTOR * longest > MAX_DELAY_MS), "undelayed_call_ms": dict(sorted(env.call_ms.items())),
              "device": env.torch.cuda.get_device_name(0)}
    try:  # (a read-only checkout still runs the tests)
        out = ROOT / "profiles" / "r09"
        out.mkdir(parents=True, exist_ok=True)
        (out / "stream_delays.json").write_text(json.dumps(record, indent=1) + "\n")
    except OSError:
        pass
    print("stream delay:", json.dumps(record))
    assert d.achieved_ms >= d.ms, f"the delay does not delay: {d.achieved_ms} ms for a target of {d.ms} ms"
    env.delay = d
    return d


def _same(got, bits, want, what=""):
    """bit for bit the default-stream result, and the oracle's at 1e-11"""
    g = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    g = g.reshape(bits.shape)
    err = float(np.max(np.abs(g - want))) if want is not None else 0.0
    print(f"{what}: max |got - oracle| = {err:.3e}, differing bit patterns: {int(np.sum(g.view(np.uint64) != bits.view(np.uint64)))} of {g.size}")
    assert err < TIGHT, (what, err)
    assert np.array_equal(g.view(np.uint64), bits.view(np.uint64)), what


def _close_to(got, want, what=""):
    g = got.cpu().numpy().reshape(want.shape)
    err = float(np.max(np.abs(g - want)))
    print(f"{what}: max |got - oracle| = {err:.3e}")
    assert err < TIGHT, (what, err)


# ------------------------------------------------------------------------------------------------------------------------
# control: the construct exposes a missing wait (torch only)
# ------------------------------------------------------------------------------------------------------------------------
def test_control_read_without_event_sees_the_stale_value(env, delay):
    torch = env.torch
    s1, s2 = delay.streams(2)
    buf = torch.full((4096,), 1.0, device="cuda")
    new = torch.full((4096,), 2.0, device="cuda")
    seen = torch.zeros(4096, device="cuda")
    torch.cuda.synchronize()
    delay.on(s1)
    with torch.cuda.stream(s1):
        buf.copy_(new)
    with torch.cuda.stream(s2):
        seen.copy_(buf)  # no event between the streams
    s2.synchronize()
    stale = seen.cpu().numpy().copy()
    torch.cuda.synchronize()
    assert np.all(stale == 1.0), "a read that does not wait saw the delayed write: the delay does not delay"
    assert np.all(buf.cpu().numpy() == 2.0)


def test_control_read_behind_an_event_sees_the_new_value(env, delay):
    torch = env.torch
    s1, s2 = delay.streams(2)
    buf = torch.full((4096,), 1.0, device="cuda")
    new = torch.full((4096,), 2.0, device="cuda")
    seen = torch.zeros(4096, device="cuda")
    torch.cuda.synchronize()
    delay.on(s1)
    with torch.cuda.stream(s1):
        buf.copy_(new)
        ev = torch.cuda.Event()
        ev.record(s1)
    with torch.cuda.stream(s2):
        s2.wait_event(ev)
        seen.copy_(buf)
    s2.synchronize()
    assert np.all(seen.cpu().numpy() == 2.0)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------------
# 1. a session on a non-default stream
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["created_on_stream", "moved_to_stream"])
@pytest.mark.parametrize("name", ["A", "W", "D"])
def test_session_on_a_side_stream(env, ref, delay, name, how):
    torch = env.torch
    s = delay.streams(1)[0]
    if how == "created_on_stream":
        with torch.cuda.stream(s):
            b = Bench(env, env.cfgs[name], deterministic=True)
    else:
        b = Bench(env, env.cfgs[name], deterministic=True)
        with torch.cuda.stream(s):
            b.sess.use_current_stream()
    try:
        with torch.cuda.stream(s):
            for kind in CALLS:
                got = b.call(kind)  # (the library call returns with d_out complete: no torch synchronise before the read-back)
                _same(got, ref.bits[name, kind], ref.want[name, kind], f"{name}.{kind}")
            for kind in ("prims_small", "prims_big"):
                _same(b.call(kind, use_async=True), ref.bits[name, kind], ref.want[name, kind], f"{name}.{kind} async")
    finally:
        b.close()


@pytest.mark.parametrize("no_inline_meta", [False, True])
def test_default_kernel_selection_on_a_side_stream(env, ref, delay, monkeypatch, no_inline_meta):
    """Not deterministic: the one-launch small path, the regular pipeline (LCHD_NO_INLINE_META) and the fused dense kernel."""
    torch = env.torch
    if no_inline_meta:
        # (the library has no counter that tells the one-launch path from the regular pipeline; what can be checked is that it
        #  still reads a hook of this name)
        from loco_hd_amd import _native as N

        assert b"LCHD_NO_INLINE_META" in Path(N.LIB_PATH).read_bytes()
        monkeypatch.setenv("LCHD_NO_INLINE_META", "1")
    s = delay.streams(1)[0]
    with torch.cuda.stream(s):
        b = Bench(env, env.cfgs["A"], deterministic=False)
        try:
            for rep in range(2):
                for kind in CALLS:
                    first, wf = (b.dev(x) for x in b.inputs(kind))
                    out = None
                    if rep:  # the second round behind a delay, into a sentinel-filled output
                        p = ref.bits["A", kind].size
                        out = torch.empty(p, dtype=torch.float64, device="cuda")
                        delay.on(s)
                        out.fill_(SENTINEL)
                    got = b.call(kind, first, wf, out=out)
                    _close_to(got, ref.want["A", kind], f"A.{kind} default mode, round {rep}")
                    if kind == "coords_big":
                        assert b.sess.last_dense_fused()
                    if kind == "coords_small":
                        assert not b.sess.last_dense_fused()
        finally:
            b.close()


# ------------------------------------------------------------------------------------------------------------------------
# 2. delayed producers on the session's stream
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_async", [False, True])
@pytest.mark.parametrize("name", ["A", "D"])
def test_inputs_written_behind_a_delay_on_the_session_stream(env, ref, delay, name, use_async):
    torch = env.torch
    s = delay.streams(1)[0]
    with torch.cuda.stream(s):
        b = Bench(env, env.cfgs[name], deterministic=True)
        try:
            kinds = ("prims_small", "prims_big") if use_async else ("prims_small", "prims_big", "coords_big", "ensemble")
            for kind in kinds:
                real = [b.dev(x) for x in b.inputs(kind)]
                held = [b.dev(x) for x in b.inputs(kind, stale=True)]  # what the buffers hold while the delay runs
                if kind == "coords_big" and held[1] is not None:
                    held[1] = b.dev(1 - b.inputs(kind)[1])
                if kind == "ensemble" and held[1] is not None:
                    held[1] = b.dev(1 - b.inputs(kind)[1])
                out = torch.zeros(ref.bits[name, kind].size, dtype=torch.float64, device="cuda")
                torch.cuda.synchronize()
                delay.on(s)
                for h, r in zip(held, real):
                    if h is not None:
                        h.copy_(r)  # the right inputs, written by a torch kernel behind the delay
                out.fill_(SENTINEL)
                if use_async:
                    a, bb = (b.a_s, b.b_s) if kind == "prims_small" else (b.a, b.b)
                    b.sess.from_primitives_async(a, bb, held[0], THR, out, wf_index=held[1])
                    b.sess.finish()
                    got = out
                else:
                    got = b.call(kind, held[0], held[1], out=out)
                g = got.cpu().numpy()
                assert not np.any(g == SENTINEL), f"{kind}: the sentinel written before the call survived in {int(np.sum(g == SENTINEL))} slots"
                _same(got, ref.bits[name, kind], ref.want[name, kind], f"{name}.{kind} delayed producers")
        finally:
            b.close()


# ------------------------------------------------------------------------------------------------------------------------
# 2b. the profile calls: anchors, weight-function indices and the coordinates of side B behind a delay
# ------------------------------------------------------------------------------------------------------------------------
PROFILE_CALLS = ("radial", "radial_coords", "composition", "composition_coords")
PROFILE_EDGES = [0.0, 2.0, 3.0, 4.5, 6.0, 7.25, float("inf")]  # (a host list: read before the call returns)


def _dense(x):
    d = x[:, None, :] - x[None, :, :]
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def _profile_inputs(cfg, kind, stale=False):
    """(anchors, wf_index) host arrays of a profile call on the small structures: pairs for radial, side-B atoms for composition."""
    if kind in ("radial", "composition"):
        anc, wf = (cfg.anc_small_stale, cfg.wf_small_stale) if stale else (cfg.anc_small, cfg.wf_small)
        return (anc if kind == "radial" else np.ascontiguousarray(anc[:, 1])), wf
    wf = cfg.wf_rows_small
    return None, (wf if wf is None or not stale else 1 - wf)


def _profile_call(b, kind, first, wf, out=None):
    s = b.sess
    if kind == "radial":
        return s.radial(b.a_s, b.b_s, first, THR, PROFILE_EDGES, out=out, wf_index=wf)
    if kind == "radial_coords":
        return s.radial_coords(b.a_s, b.b_s, PROFILE_EDGES, out=out, wf_index=wf)
    if kind == "composition":
        return s.composition(b.b_s, first, THR, out=out, wf_index=wf)
    return s.composition_coords(b.b_s, out=out, wf_index=wf)


def _profile_expected(env, name, kind):
    """radial_util / composition_util on the RIGHT data: side B at its second coordinate set.  Computed once per (configuration, call)."""
    import composition_util as cu
    import radial_util as ru

    cache = env.__dict__.setdefault("profile_want", {})
    if (name, kind) not in cache:
        c = env.cfgs[name]
        k, n_cat = c.n_small, len(c.cats)
        xa, ca, xb, cb = c.xa[:k], c.ca[:k], c.xb2[:k], c.cb[:k]
        anc, wf = _profile_inputs(c, kind)
        specs = list(c.w_func.values()) if c.dict else [c.w_func]
        per_item = [specs[i] for i in wf] if c.dict else None
        if kind == "radial":
            want = ru.from_primitives(ca, xa, None, cb, xb, None, anc, THR, n_cat, per_item if c.dict else specs[0], PROFILE_EDGES)
        elif kind == "radial_coords":
            da, db = _dense(xa), _dense(xb)
            want = np.asarray([ru.profile(ca, da[r], cb, db[r], n_cat, per_item[r] if c.dict else specs[0], PROFILE_EDGES) for r in range(k)])
        else:
            fns = [env.orc.WeightFunction(sp[0], list(sp[1])) for sp in specs]
            cdfs = [lambda x, f=f: np.asarray(f.integral_vec(np.asarray(x, dtype=np.float64).tolist())) for f in fns]
            per_cdf = [cdfs[i] for i in wf] if c.dict else cdfs[0]
            if kind == "composition":
                want = cu.profiles_of_cloud(xb, cb, np.zeros(k, dtype=np.int32), anc, THR, np.ones(n_cat), per_cdf)
            else:
                want = cu.profiles_of_rows(_dense(xb), cb, np.ones(n_cat), per_cdf)
        cache[name, kind] = want
    return cache[name, kind]


def _profile_bits(env, name, kind):
    """The same call on the DEFAULT stream with complete, host-synchronised inputs, deterministic mode: the bit pattern to reproduce."""
    cache = env.__dict__.setdefault("profile_bits", {})
    if (name, kind) not in cache:
        cfg = env.cfgs[name]
        b = Bench(env, cfg, deterministic=True)
        try:
            b.sess.set_coords(b.b_s, cfg.xb2[:cfg.n_small])
            env.torch.cuda.synchronize()
            first, wf = (b.dev(x) for x in _profile_inputs(cfg, kind))
            got = _profile_call(b, kind, first, wf).cpu().numpy().copy()
        finally:
            b.close()
        want = _profile_expected(env, name, kind)
        assert got.shape == want.shape and float(np.max(np.abs(got - want))) < TIGHT, (name, kind)
        cache[name, kind] = got
    return cache[name, kind]


@pytest.mark.parametrize("kind", PROFILE_CALLS)
@pytest.mark.parametrize("name", ["A", "D"])
def test_profile_inputs_written_behind_a_delay_on_the_session_stream(env, ref, delay, name, kind):
    torch, cfg = env.torch, env.cfgs[name]
    bits, want = _profile_bits(env, name, kind), _profile_expected(env, name, kind)
    s = delay.streams(1)[0]
    with torch.cuda.stream(s):
        b = Bench(env, cfg, deterministic=True)  # (side B of the small structures holds xb: the stale coordinates, the same bounding box)
        try:
            real = [b.dev(x) for x in _profile_inputs(cfg, kind)]
            held = [b.dev(x) for x in _profile_inputs(cfg, kind, stale=True)]  # what the buffers hold while the delay runs
            out = torch.zeros(bits.shape, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            delay.on(s)
            for h, r in zip(held, real):
                if h is not None:
                    h.copy_(r)  # the right inputs, written by a torch kernel behind the delay
            b.sess.set_coords(b.b_s, cfg.xb2[:cfg.n_small])  # the right coordinates of side B, queued behind the delay
            out.fill_(SENTINEL)
            got = _profile_call(b, kind, held[0], held[1], out=out)
            g = got.cpu().numpy()
            assert not np.any(g == SENTINEL), f"{kind}: the sentinel written before the call survived in {int(np.sum(g == SENTINEL))} slots"
            _same(got, bits, want, f"{name}.{kind} delayed producers")
        finally:
            b.close()


@pytest.mark.parametrize("how", ["created_on_stream", "moved_to_stream"])
def test_radial_session_on_a_side_stream(env, ref, delay, how):
    torch, cfg = env.torch, env.cfgs["A"]
    kinds = ("radial", "radial_coords")
    bits = {kind: _profile_bits(env, "A", kind) for kind in kinds}  # (on the default stream: before this test leaves it)
    s = delay.streams(1)[0]
    if how == "created_on_stream":
        with torch.cuda.stream(s):
            b = Bench(env, cfg, deterministic=True)
    else:
        b = Bench(env, cfg, deterministic=True)
        with torch.cuda.stream(s):
            b.sess.use_current_stream()
    try:
        with torch.cuda.stream(s):
            b.sess.set_coords(b.b_s, cfg.xb2[:cfg.n_small])
            for kind in kinds:
                first, wf = (b.dev(x) for x in _profile_inputs(cfg, kind))
                got = _profile_call(b, kind, first, wf)  # (the library call returns with d_out complete: no torch synchronise before the read-back)
                _same(got, bits[kind], _profile_expected(env, "A", kind), f"A.{kind} on a side stream")
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------------------------------
# 3. upload, then score without a pause
# ------------------------------------------------------------------------------------------------------------------------
def test_upload_and_set_coords_on_a_delayed_stream(env, ref, delay):
    torch, cfg = env.torch, env.cfgs["A"]
    s, s2 = delay.streams(2)
    with torch.cuda.stream(s):
        b = Bench(env, cfg, deterministic=True)
        try:
            sess = b.sess
            anc = b.dev(cfg.anc_big)
            # the reference of the second coordinate set: a cloud of its own, complete before the call
            b2 = sess.upload(cfg.xb2, cfg.cb)
            torch.cuda.synchronize()
            bits2 = sess.from_primitives(b.a, b2, anc, THR).cpu().numpy().copy()
            tag = np.zeros(cfg.n, dtype=np.int32)
            want2 = np.asarray(cfg.make(env.orc).from_arrays(cfg.xa, cfg.ca, tag, cfg.xb2, cfg.cb, tag, cfg.anc_big, THR))
            assert float(np.max(np.abs(bits2 - want2))) < TIGHT
            assert not np.array_equal(bits2, ref.bits["A", "prims_big"])
            # set_coords: b.b holds xb; behind a delay it gets xb2, and is scored at once
            delay.on(s)
            sess.set_coords(b.b, cfg.xb2)
            _same(sess.from_primitives(b.a, b.b, anc, THR), bits2, want2, "set_coords on a delayed stream")
            # upload / upload_batch while the stream is delayed
            delay.on(s)
            fresh = sess.upload(cfg.xb, cfg.cb)
            _same(sess.from_primitives(b.a, fresh, anc, THR), ref.bits["A", "prims_big"], ref.want["A", "prims_big"], "upload on a delayed stream")
            delay.on(s)
            batch, _ = sess.upload_batch([(cfg.ens_x[i], cfg.ens_cat) for i in range(cfg.m)])
            _same(sess.from_coords_ensemble(batch, pairs=b.dev(cfg.ens_pairs)), ref.bits["A", "ensemble"], ref.want["A", "ensemble"],
                  "upload_batch on a delayed stream")
            # set_config after a stream switch: a second session, another configuration, the same (delayed) stream
            with torch.cuda.stream(s2):
                sess.use_current_stream()
                delay.on(s2)
                other = Bench(env, env.cfgs["D"], deterministic=True)
                try:
                    for kind in ("prims_big", "coords_small"):
                        _same(other.call(kind), ref.bits["D", kind], ref.want["D", kind], f"D.{kind} second session on the stream")
                    _same(b.call("prims_small"), ref.bits["A", "prims_small"], ref.want["A", "prims_small"], "first session after the switch")
                finally:
                    other.close()
        finally:
            b.close()


# ------------------------------------------------------------------------------------------------------------------------
# 4. switching streams between calls
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deterministic", [True, False])
def test_alternating_between_two_streams(env, ref, delay, deterministic):
    """One session, calls of different shapes, every call on the OTHER stream: the session is moved first, then the stream it
    now sits on is held by a delay behind which a torch kernel writes the real pair list over a stale one and a sentinel into
    `out`.  A library step left on the stream the session came from (idle by then) would read the stale list."""
    torch = env.torch
    streams = delay.streams(2)
    b = Bench(env, env.cfgs["A"], deterministic=deterministic)
    try:
        order = ["prims_small", "prims_big", "coords_small", "prims_big", "ensemble", "prims_small", "coords_big", "prims_big", "prims_small"]
        before = b.sess.pass_counts()["passes"]
        for i, kind in enumerate(order):
            s = streams[i % 2]
            with torch.cuda.stream(s):
                real = [b.dev(x) for x in b.inputs(kind)]
                held = [b.dev(x) for x in b.inputs(kind, stale=True)]
                out = torch.zeros(ref.bits["A", kind].size, dtype=torch.float64, device="cuda")
                torch.cuda.synchronize()
                b.sess.use_current_stream()  # (waits for the stream it leaves)
                delay.on(s)
                for h, r in zip(held, real):
                    if h is not None:
                        h.copy_(r)
                out.fill_(SENTINEL)
                got = b.call(kind, held[0], held[1], out=out)
                assert not bool((got == SENTINEL).any()), f"call {i} ({kind}): the sentinel survived"
                if deterministic:
                    _same(got, ref.bits["A", kind], ref.want["A", kind], f"call {i} ({kind}) on stream {i % 2}")
                else:
                    _close_to(got, ref.want["A", kind], f"call {i} ({kind}) on stream {i % 2}")
        counts = b.sess.pass_counts()
        print("pass counts after the run:", counts)
        assert counts["passes"] - before >= sum(k.startswith("prims") for k in order)  # every from_primitives call ran on this context
    finally:
        torch.cuda.synchronize()
        b.close()


def test_stream_switch_is_refused_while_a_pass_is_pending(env, ref, delay):
    torch = env.torch
    s1, s2 = delay.streams(2)
    with torch.cuda.stream(s1):
        b = Bench(env, env.cfgs["A"], deterministic=True)
    try:
        with torch.cuda.stream(s1):
            anc = b.dev(env.cfgs["A"].anc_big)
            out = torch.empty(anc.shape[0], dtype=torch.float64, device="cuda")
            delay.on(s1)
            b.sess.from_primitives_async(b.a, b.b, anc, THR, out)
        with torch.cuda.stream(s2):
            with pytest.raises(ValueError, match="asynchronous call has not been finished"):
                b.sess.use_current_stream()
        b.sess.finish()
        _same(out, ref.bits["A", "prims_big"], ref.want["A", "prims_big"], "pending pass after the refused switch")
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------------------------------
# 5. frames hand-off
# ------------------------------------------------------------------------------------------------------------------------
LOADERS = ("load_frames", "load_atom_frames", "load_atom_frames_dev")


class FramesRig:
    """A deterministic session on its own stream with the template structure, two frames buffers and a copy stream."""

    def __init__(self, env, fr, n_bufs=2):
        torch = env.torch
        self.env, self.fr, self.torch = env, fr, torch
        self.s, self.cs = env.delay.streams(2)
        with torch.cuda.stream(self.s):
            self.b = Bench(env, env.cfgs["A"], deterministic=True)
            self.sess = self.b.sess
            self.tmpl = self.sess.upload(fr.x_ref, fr.cat)
            self.bufs = [self.sess.frames_buffer(self.tmpl, fr.nf) for _ in range(n_bufs)]
            for buf in self.bufs:
                self.sess.set_frame_sources(buf, fr.topo)
            self.anc = self.b.dev(fr.anchors)
            self.ens = self.b.dev(fr.ens_pairs)
        self.src_dev = {k: torch.from_numpy(fr.src[k]).cuda() for k in fr.src}
        self.held = [torch.from_numpy(fr.src["X"]).cuda() for _ in range(2)]  # device source blocks a producer overwrites
        torch.cuda.synchronize()

    def load(self, loader, buf, key, produce_late=False, slot=0):
        """Load frame set `key` on the copy stream.  load_atom_frames_dev with produce_late: the float32 source tensor holds X and
        gets `key`'s atoms from a torch kernel queued on the copy stream (behind whatever delays it)."""
        fr, sess = self.fr, self.sess
        if loader == "load_frames":
            sess.load_frames(buf, fr.xyz[key], stream=self.cs)
        elif loader == "load_atom_frames":
            sess.load_atom_frames(buf, fr.src[key], stream=self.cs)
        elif produce_late:
            with self.torch.cuda.stream(self.cs):
                self.held[slot].copy_(self.src_dev[key])
            sess.load_atom_frames_dev(buf, self.held[slot], stream=self.cs)
        else:
            sess.load_atom_frames_dev(buf, self.src_dev[key], stream=self.cs)

    def score(self, buf, out=None):
        with self.torch.cuda.stream(self.s):
            return self.sess.from_primitives(self.tmpl, buf, self.anc, THR, out=out)

    def close(self):
        self.torch.cuda.synchronize()
        self.b.close()


def _frames_want(env, fr, key):
    cfg = env.cfgs["A"]
    o = cfg.make(env.orc)
    tag = np.zeros(fr.nt, dtype=np.int32)
    return np.concatenate([o.from_arrays(fr.x_ref, fr.cat, tag, fr.xyz[key][f], fr.cat, tag, fr.lp, THR) for f in range(fr.nf)])


@pytest.fixture(scope="module")
def frames_want(env, frames):
    seq = [env.cfgs["A"].cats[i] for i in frames.cat]
    o = env.cfgs["A"].make(env.orc)
    ens = {k: np.asarray([o.from_coords(seq, seq, frames.xyz[k][i], frames.xyz[k][j]) for i, j in frames.ens_pairs]) for k in ("X", "Y")}
    return SimpleNamespace(prims={k: _frames_want(env, frames, k) for k in ("X", "Y")}, ens=ens)


@pytest.mark.parametrize("loader", LOADERS)
def test_load_returns_while_the_copy_stream_is_held(env, frames, delay, loader):
    """A load only queues its work: behind a delay on the copy stream the call returns long before the delay has run out, with
    an event recorded behind the load still pending (the overlap score_trajectory is built on), and the session's stream is not
    held either.  It also shows that the delay really holds THIS loader's work back in the hand-off tests below."""
    torch = env.torch
    rig = FramesRig(env, frames)
    try:
        rig.load(loader, rig.bufs[0], "X")
        torch.cuda.synchronize()
        delay.on(rig.cs)
        t0 = time.perf_counter()
        rig.load(loader, rig.bufs[0], "Y", produce_late=True)
        host_ms = (time.perf_counter() - t0) * 1e3
        behind = torch.cuda.Event()
        behind.record(rig.cs)
        pending = not behind.query()
        with torch.cuda.stream(rig.s):  # the session's stream runs on meanwhile
            probe = torch.zeros(64, device="cuda").add_(1.0)
        rig.s.synchronize()
        still_pending = not behind.query()
        print(f"{loader}: the load returned after {host_ms:.3f} ms behind a delay of {delay.ms:.1f} ms; pending at return: {pending}, "
              f"after work on the session's stream: {still_pending}")
        assert pending and still_pending, "the copy stream had drained when the load returned: the delay did not hold the load back"
        assert host_ms < 0.5 * delay.ms, (host_ms, delay.ms)  # (a call that waited for the stream would take the whole delay)
        assert float(probe.sum()) == 64.0
    finally:
        rig.close()


@pytest.mark.parametrize("loader", LOADERS)
def test_pass_waits_for_a_load_on_a_delayed_copy_stream(env, frames, frames_want, delay, loader):
    """The buffer holds X, Y is loaded behind a delay on the copy stream, the pass follows at once and scores Y.  Two waits of the
    library stand between the load and the pass's kernels: the host waits for the load's event before it plans the pass (the
    frames' bounding box comes back with it), and the pass's stream waits for the same event.  The second is belt and braces
    while the first exists: a build without the stream wait alone passes this test, a build without both scores X."""
    rig = FramesRig(env, frames)
    try:
        rig.load(loader, rig.bufs[0], "X")
        _same(rig.score(rig.bufs[0]), frames.bits["X"], frames_want.prims["X"], f"{loader}: X")
        delay.on(rig.cs)
        rig.load(loader, rig.bufs[0], "Y", produce_late=True)
        _same(rig.score(rig.bufs[0]), frames.bits["Y"], frames_want.prims["Y"], f"{loader}: Y behind the delay")
    finally:
        rig.close()


@pytest.mark.parametrize("loader", LOADERS)
def test_two_loads_back_to_back_on_a_delayed_copy_stream(env, frames, frames_want, delay, loader):
    """X then Y into one buffer with no pass in between.  The end state is Y (coordinates and scores) whether or not the second load
    waits for the first -- both copies would then carry Y --, so the end state alone cannot guard the wait for the pinned staging
    block.  What guards it (the two loaders that stage host memory): the first load, held behind the delay, must be COMPLETE when
    the second load's call returns -- an event recorded on the copy stream right behind the first load has fired, and the call
    took at least half of the delay it had to sit out."""
    rig = FramesRig(env, frames)
    try:
        rig.load(loader, rig.bufs[0], "Y")
        rig.torch.cuda.synchronize()
        delay.on(rig.cs)
        rig.load(loader, rig.bufs[0], "X", produce_late=True, slot=0)
        first_done = rig.torch.cuda.Event()
        first_done.record(rig.cs)
        t0 = time.perf_counter()
        rig.load(loader, rig.bufs[0], "Y", produce_late=True, slot=1)
        waited_ms = (time.perf_counter() - t0) * 1e3
        time.sleep(0.001)  # (the marker sits right behind the load's own event: a millisecond of grace against a 10+ ms delay)
        fired = first_done.query()
        print(f"{loader}: second load returned after {waited_ms:.3f} ms (delay {delay.ms:.1f} ms), first load complete by then: {fired}")
        if loader != "load_atom_frames_dev":  # (no staging block there: nothing to wait for)
            assert fired, "the second load returned while the first still had to read the staging block"
            assert waited_ms >= 0.5 * delay.ms, (waited_ms, delay.ms)
        _same(rig.score(rig.bufs[0]), frames.bits["Y"], frames_want.prims["Y"], f"{loader}: X then Y")
        got = rig.sess.coords_of(rig.bufs[0], frames.nf * frames.nt).reshape(frames.nf, frames.nt, 3)
        assert np.array_equal(got, frames.xyz["Y"])
        # and the other way round, on the same buffer
        delay.on(rig.cs)
        rig.load(loader, rig.bufs[0], "Y", produce_late=True, slot=0)
        rig.load(loader, rig.bufs[0], "X", produce_late=True, slot=1)
        got = rig.sess.coords_of(rig.bufs[0], frames.nf * frames.nt).reshape(frames.nf, frames.nt, 3)
        assert np.array_equal(got, frames.xyz["X"])
        _same(rig.score(rig.bufs[0]), frames.bits["X"], frames_want.prims["X"], f"{loader}: Y then X")
    finally:
        rig.close()


@pytest.mark.parametrize("loader", LOADERS)
def test_reload_of_a_buffer_a_pass_is_using(env, frames, frames_want, delay, loader):
    """A pass on buffer 0 is pending behind a delay on the session's stream; buffer 1 may be loaded meanwhile, buffer 0 may not
    (the refusal is what protects the frames the pass reads); after finish() buffer 0 is reloaded on the copy stream and scored
    again: new scores, the first output untouched.  The library also makes every load's stream wait for the event of the last
    pass that read the buffer; finish() has waited for that pass on the host by the time a load is accepted, so that stream wait
    cannot be observed through this API (a build without it passes) -- this test checks the refusal and the end state."""
    torch = env.torch
    rig = FramesRig(env, frames)
    try:
        sess = rig.sess
        rig.load(loader, rig.bufs[0], "X")
        out0 = torch.full((frames.anchors.shape[0],), SENTINEL, dtype=torch.float64, device="cuda")
        out1 = torch.full((frames.anchors.shape[0],), SENTINEL, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        delay.on(rig.s)
        with torch.cuda.stream(rig.s):
            sess.from_primitives_async(rig.tmpl, rig.bufs[0], rig.anc, THR, out0)
        rig.load(loader, rig.bufs[1], "Y")  # the other buffer: allowed while the pass is pending
        with pytest.raises(ValueError, match="in use by an unfinished asynchronous call"):
            rig.load(loader, rig.bufs[0], "Y")
        sess.finish()
        first = out0.cpu().numpy().copy()
        _same(first, frames.bits["X"], frames_want.prims["X"], f"{loader}: first pass")
        delay.on(rig.cs)
        rig.load(loader, rig.bufs[0], "Y", produce_late=True)
        _same(rig.score(rig.bufs[0], out=out1), frames.bits["Y"], frames_want.prims["Y"], f"{loader}: second pass on the reloaded buffer")
        assert np.array_equal(out0.cpu().numpy(), first), "the first pass's output changed"
        _same(rig.score(rig.bufs[1]), frames.bits["Y"], frames_want.prims["Y"], f"{loader}: the buffer loaded during the first pass")
    finally:
        rig.close()


@pytest.mark.parametrize("loader", LOADERS)
def test_ensemble_on_a_buffer_loaded_on_a_delayed_copy_stream(env, frames, frames_want, delay, loader):
    """The host's wait for the load's event (taken when the frames' bounding box is fetched) is the only wait between the load and
    the ensemble's kernels: a build without it scores X."""
    rig = FramesRig(env, frames)
    try:
        rig.load(loader, rig.bufs[0], "X")
        rig.torch.cuda.synchronize()
        delay.on(rig.cs)
        rig.load(loader, rig.bufs[0], "Y", produce_late=True)
        with rig.torch.cuda.stream(rig.s):
            got = rig.sess.from_coords_ensemble(rig.bufs[0], pairs=rig.ens)
        _same(got, frames.ens_bits["Y"], frames_want.ens["Y"], f"{loader}: ensemble of Y")
    finally:
        rig.close()


@pytest.mark.parametrize("loader", LOADERS)
def test_non_finite_frame_loaded_on_a_delayed_stream_is_reported(env, frames, frames_want, delay, loader):
    rig = FramesRig(env, frames)
    try:
        rig.load(loader, rig.bufs[0], "X")
        rig.torch.cuda.synchronize()
        delay.on(rig.cs)
        rig.load(loader, rig.bufs[0], "bad", produce_late=True)
        with pytest.raises(ValueError, match="non-finite coordinate in a trajectory frame"):
            rig.score(rig.bufs[0])
        delay.on(rig.cs)
        rig.load(loader, rig.bufs[0], "bad", produce_late=True)
        with pytest.raises(ValueError, match="non-finite coordinate in a trajectory frame"):
            with rig.torch.cuda.stream(rig.s):
                rig.sess.from_coords_ensemble(rig.bufs[0], pairs=rig.ens)
        rig.load(loader, rig.bufs[0], "Y", produce_late=True)
        _same(rig.score(rig.bufs[0]), frames.bits["Y"], frames_want.prims["Y"], f"{loader}: after the refused frames")
    finally:
        rig.close()


@pytest.mark.parametrize("with_topology", [False, True])
def test_score_trajectory_on_a_side_stream(env, frames, delay, with_topology):
    """Eleven frames in chunks of two (six passes, five buffer swaps): bit for bit the per-frame single calls."""
    torch, cfg = env.torch, env.cfgs["A"]
    rng = np.random.default_rng(5)
    nt, nf = frames.nt, 11
    src = np.concatenate([frames.src["X"], frames.src["Y"], frames.src["X"][::-1], frames.src["Y"][:2]])[:nf]
    src = (src + rng.uniform(-0.2, 0.2, (nf, 1, 3)).astype(np.float32)).astype(np.float32)
    s = delay.streams(1)[0]
    with torch.cuda.stream(s):
        b = Bench(env, cfg, deterministic=True)
        try:
            sess = b.sess
            tmpl = sess.upload(frames.x_ref, frames.cat)
            big = sess.frames_buffer(tmpl, nf)
            sess.set_frame_sources(big, frames.topo)
            sess.load_atom_frames(big, src)
            xyz = sess.coords_of(big, nf * nt).reshape(nf, nt, 3)  # the centroids as the library evaluates them
            one = sess.upload(xyz[0], frames.cat)
            lp = b.dev(frames.lp)
            single = []
            for f in range(nf):
                sess.set_coords(one, xyz[f])
                single.append(sess.from_primitives(tmpl, one, lp, THR).cpu().numpy().copy())
            single = np.stack(single)
            o = cfg.make(env.orc)
            tag = np.zeros(nt, dtype=np.int32)
            want = np.stack([o.from_arrays(frames.x_ref, frames.cat, tag, xyz[f], frames.cat, tag, frames.lp, THR) for f in range(nf)])
            delay.on(s)
            if with_topology:
                got = sess.score_trajectory(tmpl, src, frames.lp, THR, chunk=2, topology=_Topology(frames.topo, nt))
            else:
                got = sess.score_trajectory(tmpl, xyz, frames.lp, THR, chunk=2)
            _same(got, single, want, f"score_trajectory, topology={with_topology}")
        finally:
            b.close()


class _Topology:
    """What score_trajectory needs of a PrimitiveTopology: the CSR map, the number of source atoms, len() = primitive atoms."""

    def __init__(self, topo, n_primitive):
        self.src_start, self.src_idx, self.n_atoms, self._n = topo.src_start, topo.src_idx, topo.n_atoms, n_primitive

    def __len__(self):
        return self._n


# ------------------------------------------------------------------------------------------------------------------------
# 6. two sessions, two streams, one thread
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("delayed", [False, True])
def test_two_sessions_on_two_streams(env, ref, delay, delayed):
    torch = env.torch
    s1, s2 = delay.streams(2)
    with torch.cuda.stream(s1):
        b1 = Bench(env, env.cfgs["A"], deterministic=True)
    with torch.cuda.stream(s2):
        b2 = Bench(env, env.cfgs["D"], deterministic=True)
    try:
        for kind1, kind2 in (("prims_big", "prims_small"), ("prims_small", "prims_big"), ("prims_big", "prims_big")):
            with torch.cuda.stream(s1):
                i1 = [b1.dev(x) for x in b1.inputs(kind1)]
                o1 = torch.full((i1[0].shape[0],), SENTINEL, dtype=torch.float64, device="cuda")
            with torch.cuda.stream(s2):
                i2 = [b2.dev(x) for x in b2.inputs(kind2)]
                o2 = torch.full((i2[0].shape[0],), SENTINEL, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            if delayed:
                delay.on(s1)
            a1, bb1 = (b1.a_s, b1.b_s) if kind1 == "prims_small" else (b1.a, b1.b)
            a2, bb2 = (b2.a_s, b2.b_s) if kind2 == "prims_small" else (b2.a, b2.b)
            b1.sess.from_primitives_async(a1, bb1, i1[0], THR, o1, wf_index=i1[1])
            b2.sess.from_primitives_async(a2, bb2, i2[0], THR, o2, wf_index=i2[1])
            b2.sess.finish()  # the opposite order
            _same(o2, ref.bits["D", kind2], ref.want["D", kind2], f"D.{kind2} next to A.{kind1}")
            b1.sess.finish()
            _same(o1, ref.bits["A", kind1], ref.want["A", kind1], f"A.{kind1} next to D.{kind2}")
    finally:
        torch.cuda.synchronize()
        b1.close()
        b2.close()


# ------------------------------------------------------------------------------------------------------------------------
# 7. the sharded path
# ------------------------------------------------------------------------------------------------------------------------
def test_score_sharded_on_a_side_stream(env, ref, delay, monkeypatch):
    """score_sharded (plan on the context's side stream, selection and passes on the session's stream) in a world of one; the pair
    lists are complete when the plan is enqueued (that is the contract of lchd_shard_plan_dev)."""
    import torch.distributed as dist

    from loco_hd_amd.dist import score_sharded

    torch, cfg = env.torch, env.cfgs["A"]
    s = delay.streams(1)[0]
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", str(31100 + os.getpid() % 500))  # (a range no other test module uses)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        with torch.cuda.stream(s):
            b = Bench(env, cfg, deterministic=True)
            try:
                anc = b.dev(cfg.anc_big)
                rev = b.dev(cfg.anc_big[::-1].copy())
                fn = lambda sub: b.sess.from_primitives(b.a, b.b, sub, THR)
                for partition in ("anchor", "contiguous"):
                    full = score_sharded(fn, anc, 1, 0, n_atoms_a=cfg.n, session=b.sess, partition=partition, force_collective=True)
                    s.synchronize()
                    _same(full, ref.bits["A", "prims_big"], ref.want["A", "prims_big"], f"score_sharded, {partition}")
                    delay.on(s)  # the scoring stream is busy when the next plan is enqueued
                    full = score_sharded(fn, rev, 1, 0, n_atoms_a=cfg.n, session=b.sess, partition=partition, force_collective=True)
                    s.synchronize()
                    _same(full, ref.bits["A", "prims_big"][::-1].copy(), ref.want["A", "prims_big"][::-1].copy(), f"score_sharded reversed, {partition}")
            finally:
                torch.cuda.synchronize()
                b.close()
    finally:
        dist.destroy_process_group()


def test_next_shard_plan_waits_for_the_pending_selection(env, delay):
    """shard_sel_ev: a selection is queued behind a delay on the session's stream; the plan of ANOTHER list is enqueued at once on
    the context's side stream.  It must not overwrite the bin table the pending selection reads.  (Output buffers have room for
    the whole list, so a selection made with the wrong table would still write inside them.)"""
    import ctypes as C

    from loco_hd_amd import _native as N
    from loco_hd_amd.dist import shard_rule

    torch, cfg = env.torch, env.cfgs["A"]
    world, n = 2, cfg.n
    s = delay.streams(1)[0]
    with torch.cuda.stream(s):
        b = Bench(env, cfg, deterministic=True)
        try:
            p = cfg.anc_big.shape[0]
            skew = cfg.anc_big.copy()
            skew[:, 0] = (skew[:, 0].astype(np.float64) ** 2 / n).astype(np.int64)  # another histogram over the bins
            lists = [b.dev(cfg.anc_big), b.dev(skew)]
            sels = [torch.full((p, 2), -1, dtype=torch.int64, device="cuda") for _ in lists]
            idxs = [torch.full((p,), -1, dtype=torch.int64, device="cuda") for _ in lists]
            counts = [(C.c_int64 * world)() for _ in lists]
            torch.cuda.synchronize()
            lib, ctx = N.lib(), b.sess._ctx
            delay.on(s)
            for k, rank in ((0, 0), (1, 1)):
                N.check(lib.lchd_shard_plan_dev(ctx, C.c_void_p(lists[k].data_ptr()), p, n, n, world, counts[k]))
                N.check(lib.lchd_shard_select_dev(ctx, C.c_void_p(lists[k].data_ptr()), p, n, n, rank, C.c_void_p(sels[k].data_ptr()),
                                                  C.c_void_p(idxs[k].data_ptr())))
            s.synchronize()
            for k, rank in ((0, 0), (1, 1)):
                rank_of_pair, want_counts = shard_rule(lists[k], n, world, n)
                assert [int(v) for v in counts[k]] == want_counts
                want_idx = (rank_of_pair == rank).nonzero().reshape(-1)
                m = want_counts[rank]
                assert torch.equal(torch.sort(idxs[k][:m]).values, want_idx), f"list {k}"
                assert torch.equal(sels[k][:m], lists[k][idxs[k][:m]])
                assert bool((idxs[k][m:] == -1).all())
        finally:
            torch.cuda.synchronize()
            b.close()


# ------------------------------------------------------------------------------------------------------------------------
# 8. timing events on a non-default stream
# ------------------------------------------------------------------------------------------------------------------------
def test_timing_events_on_side_streams(env, ref, frames, delay):
    """The phases are consecutive intervals between events recorded inside the call; (1 + 1e-5): the elapsed times are float32."""
    torch, cfg = env.torch, env.cfgs["A"]
    rig = FramesRig(env, frames)
    try:
        sess, s = rig.sess, rig.s
        with torch.cuda.stream(s):
            anc = rig.b.dev(cfg.anc_big)
            sess.enable_timing(True)
            sess.from_primitives(rig.b.a, rig.b.b, anc, THR)  # (warm-up)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            got = sess.from_primitives(rig.b.a, rig.b.b, anc, THR)
            e1.record(s)
            e1.synchronize()
            span = e0.elapsed_time(e1)
            ms = sess.last_ms()
            print("phases:", ms, "span of the call on its stream:", span)
            assert all(np.isfinite(v) and v >= 0.0 for v in ms.values()), ms
            assert sum(ms.values()) <= span * (1 + 1e-5), (ms, span)
            _same(got, ref.bits["A", "prims_big"], ref.want["A", "prims_big"], "timed call")
        for loader in ("load_atom_frames", "load_atom_frames_dev"):
            c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            c0.record(rig.cs)
            rig.load(loader, rig.bufs[0], "Y")
            c1.record(rig.cs)
            c1.synchronize()
            span = c0.elapsed_time(c1)
            conv = sess.last_convert_ms(rig.bufs[0])
            print(loader, "conversion:", conv, "span of the load on the copy stream:", span)
            assert np.isfinite(conv) and 0.0 <= conv <= span * (1 + 1e-5), (loader, conv, span)
        sess.enable_timing(False)
    finally:
        rig.close()
