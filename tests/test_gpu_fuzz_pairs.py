"""The seeded whole-surface fuzz (tests/test_gpu_fuzz_surface.py) extended to score attribution, neighbour sensitivities / gradients and
cross-scoring / nearest: every case of fuzz_surface.draw with the axes tests/fuzz_pairs.py adds, through the host API and -- where the
case says so -- through DeviceSession and loco_hd_amd.autograd, against references that share no arithmetic with the library
(tests/attribution_util.py and tests/sensitivity_util.py in longdouble on reference environments, the CPU oracle for cross).
tests/test_fuzz_pairs_draw.py checks the axes and the references without a device; a failure here is reproduced by its seed.

A family that refuses the case as drawn (more than 64 categories, a non-Hellinger attribution, a periodic host sensitivity) must say so,
and is then given the fitted case of fuzz_pairs.pair_axes.  Bounds (none of them measured on the code under test):
    scores, attribution rows, cross entries   1e-10 * max(1, max |reference|) per case: the fuzz's existing bound
    g, per element                            1e-10 * max(1, w(d)), w(d) the longdouble density at the member: the error of w(d) (H- - H+)
                                              is w(d) times the rounding of two statistical distances of size O(10) at most
    gradients over the sampled pairs          1e-11 * max(1, sum |v g|): at most 40 pairs x 800 members = 3.2e4 unit-direction terms,
                                              3.2e4 x 1.1e-16 < 4e-12
The largest ratio of a deviation to its bound is printed per seed (DESIGN.md section 5 records the largest over the default seeds)."""
import os
import re
import time

import numpy as np
import pytest

import cross_util as cu
import fuzz_pairs as fq
import fuzz_surface as fs
import sensitivity_util as su
import test_gpu_fuzz_surface as scoring
from test_fuzz_profiles_draw import DEFAULT, GAP, NO_GAP

pytestmark = pytest.mark.gpu
N_SEEDS = int(os.environ.get("LCHD_FUZZ_SEEDS", "40"))  # a one-off campaign: LCHD_FUZZ_SEEDS=400 python -m pytest tests/test_gpu_fuzz_pairs.py


def tol(want):
    return 1e-10 * max(1.0, float(np.max(np.abs(want), initial=0.0)))


def per_kw(case):
    return {**scoring.side_kw(case.get("per_a"), "a"), **scoring.side_kw(case.get("per_b"), "b")}


def keyed(case, rows):
    """The anchor pairs `rows` of a prims case as from_primitives takes them."""
    return [case["pairs"][p] + ((case["keys"][p],) if case["multi"] else ()) for p in rows]


def take(full, ax, case):
    """The rows of a whole attribution result that the reference holds, in the order of its items."""
    if case["driver"] == "prims_batch":
        return np.concatenate([g[np.asarray(s, dtype=np.int64)] for g, s in zip(full, ax["sample"])])
    return full[ax["sample"]]


def trimmed(sens, rows):
    """The rows `rows` of a Sens / Sensitivity of arrays as a call on those pairs alone returns them: as wide as their longest list."""
    part = [np.asarray(f)[rows] for f in sens]
    k = int(max(np.max(part[1], initial=1), np.max(part[5], initial=1)))
    for f in part:
        assert f.ndim == 1 or np.all((f[:, k:] == 0) | (f[:, k:] == -1))  # only padding is cut
    return su.Sens(*[f if f.ndim == 1 else f[:, :k] for f in part])


# ---- the host API -----------------------------------------------------------------------------------------------------------------
def attribution_host(lh, lchd, case):
    """The whole result: an array (P, C), or a list of them for the jobs of a batch."""
    drv, keys = case["driver"], case.get("keys")
    if drv == "prims":
        pa, pb = scoring.prims_of(lh, case)
        return lchd.attribution_from_primitives(pa, pb, fs.anchor_pairs(case), case["thr"], **per_kw(case))
    if drv == "prims_batch":
        ps = [fs.prim_list(lh, *s) for s in case["structs"]]
        return [lchd.attribution_from_primitives(ps[a], ps[b], pairs, case["thr"]) if pairs else np.zeros((0, case["ncat"])) for a, b, pairs in case["jobs"]]
    if drv == "coords":
        return lchd.attribution_from_coords(case["sa"], case["sb"], case["xa"], case["xb"], keys, **per_kw(case))
    assert drv == "dmxs"
    return lchd.attribution_from_dmxs(case["sa"], case["sb"], case["da"], case["db"], keys)


def pair_calls(lh, case, ax, order=None):
    """[(prims a, prims b, anchor pairs, rows of the reference)] per host call on the SAMPLED pairs: one for a prims case, one per job of
    a batch.  order: a permutation of a prims case's sampled pairs."""
    if case["driver"] == "prims":
        pa, pb = scoring.prims_of(lh, case)
        rows = list(range(len(ax["sample"]))) if order is None else list(order)
        return [(pa, pb, keyed(case, [ax["sample"][r] for r in rows]), rows)]
    ps = [fs.prim_list(lh, *s) for s in case["structs"]]
    out, start = [], 0
    for (a, b, pairs), s in zip(case["jobs"], ax["sample"]):
        if s:
            out.append((ps[a], ps[b], [pairs[p] for p in s], list(range(start, start + len(s)))))
        start += len(s)
    return out


def sensitivity_host(lh, lchd, case, ax, order=None, **kw):
    return [(lchd.sensitivity_from_primitives(pa, pb, pairs, case["thr"], **kw), rows) for pa, pb, pairs, rows in pair_calls(lh, case, ax, order)]


def gradient_host(lh, lchd, case, ax):
    return [lchd.gradient_from_primitives(pa, pb, pairs, case["thr"], pair_weights=ax["pair_weights"][rows]) for pa, pb, pairs, rows in pair_calls(lh, case, ax)]


def cross_sides(lh, case, ax):
    """(prims a, {structure or None: prims b}) of an OPEN case for the host cross calls."""
    if case["driver"] == "prims":
        pa, pb = scoring.prims_of(lh, case)
        return pa, {None: pb}
    return fs.prim_list(lh, *case["structs"][0]), {s: fs.prim_list(lh, *case["structs"][s]) for s, _, _ in ax["cross"]["groups"]}


def cross_host(lh, lchd, case, ax, tile_rows):
    cx = ax["cross"]
    pa, sides = cross_sides(lh, case, ax)
    out = np.full((cx["na"], cx["nb"]), np.nan)
    for s, local, cols in cx["groups"]:
        out[:, cols] = lchd.cross_from_primitives(pa, sides[s], cx["anchors_a"], local, case["thr"], cx["key"], tile_rows=tile_rows)
    return out


def nearest_host(lh, lchd, case, ax, tile_rows):
    """[(Nearest, columns of the group in anchors_b, k)] per structure of side B, k clipped to the group."""
    cx = ax["cross"]
    pa, sides = cross_sides(lh, case, ax)
    return [(lchd.nearest_from_primitives(pa, sides[s], cx["anchors_a"], local, case["thr"], min(cx["k"], len(local)), cx["key"], tile_rows=tile_rows),
             cols, min(cx["k"], len(local))) for s, local, cols in cx["groups"]]


# ---- DeviceSession ----------------------------------------------------------------------------------------------------------------
class Uploaded:
    """A prims / prims_batch case in a DeviceSession of `lchd`: .sides (prims: two clouds, periodic sides as image clouds where
    `images`) or .batch / .offs, and the anchors / weight-function indices as tensors."""

    def __init__(self, lh, lchd, case, images=True):
        from loco_hd_amd.device import DeviceSession

        self.case, self.lchd, interner = case, lchd, {}
        if case["driver"] == "prims":
            packed = [lchd.pack(p, interner) for p in scoring.prims_of(lh, case)]
        else:
            packed = [lchd.pack(fs.prim_list(lh, *s), interner) for s in case["structs"]]
        self.packed = packed
        self.sess = sess = DeviceSession(lchd, interner=interner)
        self.torch = sess.torch
        self.dev = self.torch.device("cuda", sess.device)
        if case["driver"] == "prims":
            self.sides = []
            for pk, per in zip(packed, (case["per_a"], case["per_b"])):
                cl = sess.upload(pk.xyz, pk.cat, pk.tag)
                if per is not None and images:
                    cl = sess.periodic_images(cl, per[1], case["thr"]) if per[0] == "box" else sess.periodic_images(cl, reach=case["thr"], cell=per[1])
                self.sides.append(cl)
            self.offs = None
        else:
            self.batch, self.offs = sess.upload_batch([(pk.xyz, pk.cat, pk.tag) for pk in packed])

    def i64(self, x, shape):
        return self.torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.int64).reshape(shape))).to(self.dev)

    def wf(self, keys):
        idx = self.lchd._wf_indices(keys, len(keys)) if keys is not None else None
        return None if idx is None else self.torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int32)).to(self.dev)

    def pair_calls(self, ax, rows_of=None):
        """[(cloud a, cloud b, anchors tensor, wf_index tensor, structures (a, b) or None)] per call: every pair of a prims case or the
        sampled ones (rows_of = ax["sample"]), per job of a batch."""
        case = self.case
        if case["driver"] == "prims":
            rows = list(range(len(case["pairs"]))) if rows_of is None else rows_of
            keys = [case["keys"][p] for p in rows] if case["multi"] else None
            return [(self.sides[0], self.sides[1], self.i64([case["pairs"][p] for p in rows], (-1, 2)), self.wf(keys), None)]
        out = []
        for j, (a, b, pairs) in enumerate(case["jobs"]):
            rows = list(range(len(pairs))) if rows_of is None else rows_of[j]
            if rows:
                flat = np.asarray([pairs[p] for p in rows], dtype=np.int64).reshape(-1, 2) + np.asarray([self.offs[a], self.offs[b]], dtype=np.int64)
                out.append((self.batch, self.batch, self.i64(flat, (-1, 2)), None, (a, b)))
        return out

    def close(self):
        self.sess.close()


def attribution_session(lh, lchd, case):
    """attribution_host through DeviceSession.attribution / attribution_coords: periodic from_primitives sides as image clouds, a batch
    as one object with global indices."""
    if case["driver"] == "coords":
        from loco_hd_amd.device import DeviceSession

        sess = DeviceSession(lchd)
        try:
            torch = sess.torch
            a, b = sess.upload(case["xa"], lchd._cats(case["sa"])), sess.upload(case["xb"], lchd._cats(case["sb"]))
            idx = lchd._wf_indices(case.get("keys"), case["n"])
            wf = None if idx is None else torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int32)).to(torch.device("cuda", sess.device))
            return sess.attribution_coords(a, b, wf_index=wf, **per_kw(case)).cpu().numpy()
        finally:
            sess.close()
    up = Uploaded(lh, lchd, case)
    try:
        got = [up.sess.attribution(a, b, anc, case["thr"], wf_index=wf).cpu().numpy() for a, b, anc, wf, _ in up.pair_calls(None)]
        if case["driver"] == "prims":
            return got[0]
        it = iter(got)
        return [next(it) if pairs else np.zeros((0, case["ncat"])) for _, _, pairs in case["jobs"]]
    finally:
        up.close()


def sensitivity_session(lh, lchd, case, ax, host_gradients, autograd_check):
    """[(Sensitivity of arrays with LOCAL indices, rows)] as sensitivity_host returns them, through DeviceSession.sensitivity on the
    sampled pairs; a batch is one object: its idx are GLOBAL atom indices (include/loco_hd_hip.h), checked and made local here.
    DeviceSession.gradient and -- for an open prims case -- the autograd function are compared with the host gradients on the way."""
    up = Uploaded(lh, lchd, case)
    try:
        torch, sess = up.torch, up.sess
        out, start = [], 0
        for call, (a, b, anc, wf, structs) in enumerate(up.pair_calls(ax, ax["sample"])):
            rows = list(range(start, start + anc.shape[0]))
            start += anc.shape[0]
            dev = sess.sensitivity(a, b, anc, case["thr"], wf_index=wf)
            got = {name: getattr(dev, name).cpu().numpy() for name in dev._fields}
            v = torch.from_numpy(ax["pair_weights"][rows]).to(up.dev)
            if structs is None:
                xa, xb = (torch.from_numpy(np.ascontiguousarray(pk.xyz, dtype=np.float64).reshape(-1, 3)).to(up.dev) for pk in up.packed)
            else:
                xa = xb = torch.from_numpy(np.concatenate([np.asarray(pk.xyz, dtype=np.float64).reshape(-1, 3) for pk in up.packed])).to(up.dev)
            s_dev, ga, gb = sess.gradient(a, b, anc, case["thr"], xa, xb, pair_weights=v, wf_index=wf)
            s_host, ga_host, gb_host = host_gradients[call]
            ga, gb = ga.cpu().numpy(), gb.cpu().numpy()
            if structs is not None:  # global indices: the gradient of the whole batch, zero outside the job's two structures
                for name, off in (("idx_a", up.offs[structs[0]]), ("idx_b", up.offs[structs[1]])):
                    size = len(case["structs"][structs[0 if name == "idx_a" else 1]][0])
                    assert np.all((got[name] == -1) | ((got[name] >= off) & (got[name] < off + size))), "idx of a batch are global atom indices"
                    got[name] = np.where(got[name] >= 0, got[name] - off, -1).astype(np.int32)
                total = np.zeros_like(ga)
                total[up.offs[structs[0]]:up.offs[structs[0]] + len(ga_host)] += ga_host
                total[up.offs[structs[1]]:up.offs[structs[1]] + len(gb_host)] += gb_host
                assert np.max(np.abs(ga + gb - total), initial=0.0) <= 1e-11 * max(1.0, float(np.max(np.abs(total), initial=0.0)))
            else:
                scale = max(1.0, float(np.max(np.abs(ga_host), initial=0.0)), float(np.max(np.abs(gb_host), initial=0.0)))
                assert np.max(np.abs(ga - ga_host), initial=0.0) <= 1e-11 * scale and np.max(np.abs(gb - gb_host), initial=0.0) <= 1e-11 * scale
            assert np.max(np.abs(s_dev.cpu().numpy() - s_host), initial=0.0) <= tol(s_host)
            if structs is None and autograd_check is not None:
                autograd_check(up, anc, v, ga_host)
            out.append((type(dev)(**got), rows))
        return out
    finally:
        up.close()


def cross_session(lh, lchd, case, ax, tile_rows):
    """(cross matrix, Nearest of arrays at tile_rows, Nearest at 0) through DeviceSession.cross / nearest: periodic sides as image clouds,
    a batch as one object with global indices on both sides."""
    cx = ax["cross"]
    up = Uploaded(lh, lchd, case)
    try:
        sess = up.sess
        wf = None if cx["key"] is None else int(lchd._wf_indices([cx["key"]], 1)[0])
        if case["driver"] == "prims":
            a, b = up.sides
            anc_a, anc_b = up.i64(cx["anchors_a"], (-1,)), up.i64(cx["anchors_b"], (-1,))
        else:
            a = b = up.batch
            anc_a, anc_b = up.i64(np.asarray(cx["anchors_a"]) + up.offs[0], (-1,)), up.i64(cx["anchors_b"], (-1,))
        m = sess.cross(a, b, anc_a, anc_b, case["thr"], wf_index=wf, tile_rows=tile_rows).cpu().numpy()
        near = [sess.nearest(a, b, anc_a, anc_b, case["thr"], cx["k"], wf_index=wf, tile_rows=t) for t in (tile_rows, 0)]
        return m, [(n.scores.cpu().numpy(), n.cols.cpu().numpy()) for n in near]
    finally:
        up.close()


# ---- the test ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(N_SEEDS))
def test_random_configuration(oracle, seed, monkeypatch):
    import loco_hd_amd as lh

    # the hooks of tests/test_gpu_fuzz_surface.py on the same seed classes (read when a context is created)
    if seed % 2:
        monkeypatch.setenv("LCHD_NO_INLINE_META", "1")
    if seed % 4 == 3:
        monkeypatch.setenv("LCHD_PER_PAIR", "1")
    case = fs.draw(seed)
    if case.get("block"):
        monkeypatch.setenv("LCHD_ENSEMBLE_BLOCK", "2")
    ax = fq.pair_axes(case)
    drv, det, runs = case["driver"], case["det"], ax["runs"]
    session = case["entry"] == "session"
    what = (seed, drv, case["boundary"], "deterministic" if det else "default", case["entry"], case["ncat"], case["sd"], case["wfs"], ax["changed"])
    if not (any(runs.values()) or ax["ragged"]):
        assert drv in fs.ENSEMBLES  # ensembles have no call in these families
        return
    worst = {}

    def ratio(name, err, bound):
        r = float(np.max(np.asarray(err) / np.asarray(bound), initial=0.0))
        worst[name] = max(worst.get(name, 0.0), r)
        return r

    def close(got, want, name):
        assert got.shape == want.shape and np.all(np.isfinite(got)), what + (name,)
        r = ratio(name.split(",")[0], np.max(np.abs(got - want), initial=0.0), tol(want))
        assert r < 1.0, what + (name, r)

    # ---- the references, all on the host
    t0 = time.perf_counter()
    score_want, score_rows = fs.expected(case, oracle)
    fit_a, fit_s, fit_c = (ax["fit"].get(f) for f in fq.FAMILIES)
    if runs["attribution"]:
        att_want, _ = fq.attribution_reference(fit_a, ax)
        att_scores = fq.sampled_scores(fit_a, ax, oracle)
        att_gap = float(np.max(np.abs(fq.attribution_reference(fs.open_twin(fit_a), ax)[0] - att_want))) if fs.is_periodic(fit_a) else None
    if runs["sensitivity"]:
        sens_want = fq.sensitivity_reference(fit_s, ax)
        dens = fq.densities(fit_s, ax, sens_want)
        sens_scores = fq.sampled_scores(fit_s, ax, oracle)
        grad_want = fq.gradient_reference(fit_s, ax, sens_want)
    if runs["cross"]:
        cx = ax["cross"]
        cross_want = fq.cross_reference(fit_c, ax, oracle)
        images = session and drv == "prims" and fs.is_periodic(case)
        cross_images = fq.cross_reference(case, ax, oracle) if images else None
    t1 = time.perf_counter()

    lchd = fs.build(lh, case, deterministic=det)

    def scored(name):
        got = scoring.run_host(lh, lchd, case)
        parts = scoring.parts(got if score_rows is None else np.asarray(got)[..., score_rows])
        for g, w in zip(parts, scoring.parts(score_want)):
            assert g.shape == w.shape and np.all(np.isfinite(g)), what
            assert np.max(np.abs(g - w), initial=0.0) < tol(w), what + (name,)
        return got

    before = scored("the scoring call before the pair-family calls")

    # ---- 1. refusals as drawn
    if ax["ragged"]:
        with pytest.raises(ValueError, match=re.escape(fq.RAGGED_ATTRIBUTION)):
            lchd.attribution_from_dmxs(case["sa"], case["sb"], [r.tolist() for r in case["rows_a"]], [r.tolist() for r in case["rows_b"]], case["keys"])
    for family, call in (("attribution", lambda: attribution_host(lh, lchd, case)),
                         ("sensitivity", lambda: lchd.sensitivity_from_primitives(*pair_calls(lh, case, ax)[0][:3], case["thr"], **per_kw(case)))):
        if runs[family] and ax["refused"][family]:
            with pytest.raises(NotImplementedError, match="|".join(re.escape(r) for r in ax["refused"][family])):
                call()
    if ax["ragged"] or any(ax["refused"].get(f) for f in ("attribution", "sensitivity")):
        middle = scored("the scoring call after a refusal")
        assert not det or scoring.bits_equal(before, middle), what
    if ax["ragged"]:
        return

    # ---- 2. parity of the fitted case, host API
    if runs["attribution"]:
        l_att = fs.build(lh, fit_a, deterministic=det) if ax["changed"]["attribution"] else lchd
        att = attribution_host(lh, l_att, fit_a)
        got = take(att, ax, fit_a)
        close(got, att_want, "attribution, host")
        assert not np.any(np.signbit(got) & (got == 0.0)), what
        close(got.sum(1), att_scores, "attribution row sums, host")
    if runs["sensitivity"]:
        l_sens = fs.build(lh, fit_s, deterministic=det) if ax["changed"]["sensitivity"] else lchd
        host_scores = scoring.run_host(lh, l_sens, fit_s)
        flat_scores = np.concatenate([np.asarray(g)[s] for g, s in zip(host_scores, ax["sample"])]) if drv == "prims_batch" else np.asarray(host_scores)[ax["sample"]]
        close(flat_scores, sens_scores, "scores, from_primitives of the fitted case")

        def sensitivity_checked(results, name):
            for got, rows in results:
                want = trimmed(sens_want, rows)
                for f in ("count_a", "count_b", "idx_a", "idx_b", "dist_a", "dist_b"):
                    assert np.array_equal(getattr(got, f), getattr(want, f)), what + (name, f)
                close(got.scores, flat_scores[rows], f"scores, {name} vs from_primitives")
                close(got.scores, want.scores, f"scores, {name} vs the model")
                for g, w, d in ((got.g_a, want.g_a, dens[0]), (got.g_b, want.g_b, dens[1])):
                    assert np.all(np.isfinite(g)), what + (name,)
                    r = ratio("g", np.abs(g - w), 1e-10 * np.maximum(1.0, d[rows][:, :g.shape[1]]))
                    assert r < 1.0, what + (name, "g", r)

        sens = sensitivity_host(lh, l_sens, fit_s, ax)
        sensitivity_checked(sens, "host")
        grads = gradient_host(lh, l_sens, fit_s, ax)
        wants = [(None,) + grad_want] if drv == "prims" else grad_want
        assert len(grads) == len(wants) == len(sens)
        for (s, ga, gb), (_, wa, wb, size), (got, rows) in zip(grads, wants, sens):
            bound = 1e-11 * max(1.0, size)
            assert np.array_equal(s, got.scores) or not det, what
            assert ratio("gradient", max(np.max(np.abs(ga - wa), initial=0.0), np.max(np.abs(gb - wb), initial=0.0)), bound) < 1.0, what
            # translation invariance: every side's gradient sums to zero over its atoms
            assert ratio("gradient column sums", max(np.max(np.abs(ga.sum(0))), np.max(np.abs(gb.sum(0)))), bound) < 1.0, what
    if runs["cross"]:
        cross = {t: cross_host(lh, lchd, fit_c, ax, t) for t in sorted({cx["tile_rows"], 0})}
        for t, m in cross.items():
            close(m, cross_want, f"cross, host, tile_rows {t}")
        for t in sorted({cx["tile_rows"], 0}):
            for near, cols, k in nearest_host(lh, lchd, fit_c, ax, t):
                ratio("nearest", cu.accept(near.scores, near.cols, cross_want[:, cols], k, tol(cross_want)), tol(cross_want))
    t2 = time.perf_counter()
    print(f"seed {seed}: references {t1 - t0:.3f} s on the host, first library calls {t2 - t1:.3f} s")

    # ---- 3. deterministic seeds
    if det:
        if runs["attribution"]:
            assert scoring.bits_equal(att, attribution_host(lh, l_att, fit_a)), what
            if drv == "prims":
                perm = np.random.default_rng(seed).permutation(len(fit_a["pairs"]))
                moved = dict(fit_a, pairs=[fit_a["pairs"][k] for k in perm], keys=None if fit_a["keys"] is None else [fit_a["keys"][k] for k in perm])
                assert np.array_equal(attribution_host(lh, l_att, moved), att[perm]), what
        if runs["sensitivity"]:
            again = sensitivity_host(lh, l_sens, fit_s, ax)
            assert all(np.array_equal(p, q) for (x, _), (y, _) in zip(sens, again) for p, q in zip(x, y)), what
            if drv == "prims":
                perm = np.random.default_rng(seed).permutation(len(ax["sample"]))
                (moved, _), = sensitivity_host(lh, l_sens, fit_s, ax, order=perm, width=sens[0][0].idx_a.shape[1])
                assert all(np.array_equal(p, q[perm]) for p, q in zip(moved, sens[0][0])), what
        if runs["cross"]:
            assert np.array_equal(cross[0], cross_host(lh, lchd, fit_c, ax, 0)), what
            for t in sorted({cx["tile_rows"], 1, 5}):
                m = cross[t] if t in cross else cross_host(lh, lchd, fit_c, ax, t)
                assert np.array_equal(m, cross[0]), what + ("tile_rows", t)
            for t in sorted({cx["tile_rows"], 0}):
                for near, cols, k in nearest_host(lh, lchd, fit_c, ax, t):  # the (score, j) rule on the device's own matrix, ties included
                    want_scores, want_cols = cu.nearest(cross[0][:, cols], k)
                    assert np.array_equal(near.cols, want_cols) and np.array_equal(near.scores, want_scores), what + ("nearest", t)

    # ---- 4. the session path
    if session:
        if runs["attribution"]:
            s_att = attribution_session(lh, l_att, fit_a)
            got = take(s_att, ax, fit_a)
            close(got, att_want, "attribution, session")
            close(got.sum(1), att_scores, "attribution row sums, session")
            assert not det or scoring.bits_equal(s_att, att), what
        if runs["sensitivity"]:
            auto = None
            if drv == "prims" and not fs.is_periodic(case):
                def auto(up, anc, v, ga_host):
                    from loco_hd_amd.autograd import locohd_scores

                    if fit_s["multi"]:  # the function takes no weight-function index: every pair under the first function
                        first = [k for k in fit_s["wfs"] if int(l_sens._wf_indices([k], 1)[0]) == 0][0]
                        one = dict(fit_s, keys=[first] * len(fit_s["pairs"]))
                        _, ga_host, _ = gradient_host(lh, l_sens, one, ax)[0]
                    x = up.torch.from_numpy(np.asarray(up.packed[0].xyz, dtype=np.float64).reshape(-1, 3)).to(up.dev).requires_grad_(True)
                    scores = locohd_scores(up.sess, up.sides[1], x, up.packed[0].cat, up.packed[0].tag, anc, fit_s["thr"])
                    (scores * v).sum().backward()
                    err = np.max(np.abs(x.grad.cpu().numpy() - ga_host), initial=0.0)
                    assert ratio("autograd vs the host gradient", err, 1e-11 * max(1.0, float(np.max(np.abs(ga_host), initial=0.0)))) < 1.0, what
            s_sens = sensitivity_session(lh, l_sens, fit_s, ax, grads, auto)
            sensitivity_checked(s_sens, "session")
            if det:
                assert all(np.array_equal(p, q) for (x, _), (y, _) in zip(s_sens, sens) for p, q in zip(x, y)), what
        if runs["cross"]:
            s_case, s_want = (case, cross_images) if images else (fit_c, cross_want)
            m, near = cross_session(lh, lchd, s_case, ax, cx["tile_rows"])
            close(m, s_want, "cross, session")
            for scores, cols in near:
                ratio("nearest", cu.accept(scores, cols, s_want, cx["k"], tol(s_want)), tol(s_want))
            if det:
                want_scores, want_cols = cu.nearest(m, cx["k"])
                assert all(np.array_equal(s, want_scores) and np.array_equal(c, want_cols) for s, c in near), what
                assert images or np.array_equal(m, cross[0]), what
            # ---- 5. the open twin of a periodic session cross: a call that ignores its image clouds fails here
            if images:
                gap = float(np.max(np.abs(cross_images - cross_want)))
                if gap > GAP and (seed, "cross") not in NO_GAP:
                    diff = float(np.max(np.abs(m - cross[0])))
                    print(f"seed {seed}: cross, image clouds against open: reference {gap:.3e}, library {diff:.3e}")
                    assert diff > 0.5 * gap, what
                else:
                    assert seed not in DEFAULT or gap > GAP or (seed, "cross") in NO_GAP, what

    # ---- 5. the open twin of a periodic attribution
    if runs["attribution"] and att_gap is not None and att_gap > GAP and (seed, "attribution") not in NO_GAP:
        opened = take(attribution_host(lh, l_att, fs.open_twin(fit_a)), ax, fit_a)
        diff = float(np.max(np.abs(opened - take(att, ax, fit_a))))
        print(f"seed {seed}: attribution, periodic against open: reference {att_gap:.3e}, library {diff:.3e}")
        assert diff > 0.5 * att_gap, what

    # ---- non-interference
    after = scored("the scoring call after the pair-family calls")
    if det:
        assert scoring.bits_equal(before, after), what
    print(f"seed {seed}: largest deviation / bound:", {k: float(f"{v:.3g}") for k, v in sorted(worst.items())})
