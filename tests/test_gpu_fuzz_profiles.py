"""The seeded whole-surface fuzz (tests/test_gpu_fuzz_surface.py) extended to the radial and the composition profiles: every case of
fuzz_surface.draw, with the axes tests/fuzz_profiles.py adds (bin count, edge kind, sampled pairs / rows), through the host API and --
where the case says so -- through DeviceSession, against the longdouble restatements of tests/radial_util.py / tests/composition_util.py
on reference environments that share no periodic arithmetic with the library.  tests/test_fuzz_profiles_draw.py checks the axes and
the references without a device; a failure here is reproduced by its seed.

Exact zeros: the C header promises that a bin which does not overlap the weight function's support is exactly 0.0.  That is asserted
for every edge kind (bins with F(e_k) == F(e_{k+1}) in longdouble), and makes a `below` / `beyond` row of a uniform or Kumaraswamy
function all zeros.  Under a function with support everywhere (hyper_exp, Dagum) such a row is NOT zero by the definition the header
gives -- a `below` bin is H(anchors) * (F(e_{k+1}) - F(e_k)), a `beyond` bin the same with H of the whole environments -- so those
bins are compared with the reference like any other.  No bin is ever -0.0."""
import os
import re
import time

import numpy as np
import pytest

import fuzz_profiles as fp
import fuzz_surface as fs
import test_gpu_fuzz_surface as scoring
from integral_form import cdf
from test_fuzz_profiles_draw import DEFAULT, GAP, NO_GAP

pytestmark = pytest.mark.gpu
N_SEEDS = int(os.environ.get("LCHD_FUZZ_SEEDS", "40"))  # a one-off campaign: LCHD_FUZZ_SEEDS=400 python -m pytest tests/test_gpu_fuzz_profiles.py


def comp_kw(per):
    return {} if per is None else {per[0]: per[1]}


def take(full, ax, case):
    """The rows of a whole result that the references hold, in the order of fuzz_profiles.environments().items."""
    if case["driver"] == "prims_batch":
        return np.concatenate([g[np.asarray(s, dtype=np.int64)] for g, s in zip(full, ax["sample"])])
    if case["driver"] in fs.ENSEMBLES:
        return np.concatenate([g[ax["sample"]] for g in full])
    return full[ax["sample"]]


# ---- the host API -----------------------------------------------------------------------------------------------------------------
def radial_host(lh, lchd, case, ax):
    """The whole result: an array (P, K), or a list of them for the jobs of a batch."""
    drv, keys, e = case["driver"], case.get("keys"), ax["edges"]
    per = {**scoring.side_kw(case.get("per_a"), "a"), **scoring.side_kw(case.get("per_b"), "b")}
    if drv == "prims":
        pa, pb = scoring.prims_of(lh, case)
        return lchd.radial_from_primitives(pa, pb, fs.anchor_pairs(case), case["thr"], e, **per)
    if drv == "prims_batch":
        ps = [fs.prim_list(lh, *s) for s in case["structs"]]
        # (an empty pair list is the keyed variant of the reference's AnchorPairSpecifier: a ValueError under a single weight function,
        #  as in from_primitives; fuzz_surface.expected leaves the empty job out in the same way)
        return [lchd.radial_from_primitives(ps[a], ps[b], pairs, case["thr"], e) if pairs else np.zeros((0, ax["k"])) for a, b, pairs in case["jobs"]]
    if drv == "coords":
        return lchd.radial_from_coords(case["sa"], case["sb"], case["xa"], case["xb"], e, keys, **per)
    assert drv == "dmxs"
    return lchd.radial_from_dmxs(case["sa"], case["sb"], case["da"], case["db"], e, keys)


def composition_host(lh, lchd, case):
    """The whole tables: [side A, side B], or [structure 0, structure M - 1] of an ensemble."""
    drv, keys = case["driver"], case.get("keys")
    if drv == "prims":
        cols = np.asarray(case["pairs"]).reshape(-1, 2)
        return [lchd.composition_from_primitives(p, cols[:, k].tolist(), case["thr"], keys, **comp_kw(per))
                for k, (p, per) in enumerate(zip(scoring.prims_of(lh, case), (case["per_a"], case["per_b"])))]
    if drv == "coords":
        return [lchd.composition_from_coords(case["sa"], case["xa"], keys, **comp_kw(case["per_a"])),
                lchd.composition_from_coords(case["sb"], case["xb"], keys, **comp_kw(case["per_b"]))]
    if drv == "dmxs":
        return [lchd.composition_from_dmx(case["sa"], case["da"], keys), lchd.composition_from_dmx(case["sb"], case["db"], keys)]
    if drv == "coords_ensemble":
        return [lchd.composition_from_coords(case["seq"], case["xs"][k], keys, **comp_kw(fp._per_of(case, k))) for k in (0, case["m"] - 1)]
    assert drv == "dmxs_ensemble"
    return [lchd.composition_from_dmx(case["seq"], case["dmxs"][k], keys) for k in (0, case["m"] - 1)]


def composition_sampled(full, ax, case):
    """The tables as fuzz_profiles.composition_reference returns them: [side A, side B or None]."""
    if case["driver"] in fs.ENSEMBLES:
        return [take(full, ax, case), None]
    return [t[ax["sample"]] for t in full]


# ---- DeviceSession ----------------------------------------------------------------------------------------------------------------
def through_a_session(lh, lchd, case, ax):
    """(radial or None, composition tables or None): the calls of radial_host / composition_host through DeviceSession.radial,
    radial_coords, composition and composition_coords -- periodic from_primitives sides as periodic_images clouds, a batch as one
    object with global indices."""
    from loco_hd_amd.device import DeviceSession

    drv, e = case["driver"], ax["edges"]
    interner = {}
    if drv == "prims":
        packed = [lchd.pack(p, interner) for p in scoring.prims_of(lh, case)]
    elif drv == "prims_batch":
        packed = [lchd.pack(fs.prim_list(lh, *s), interner) for s in case["structs"]]
    sess = DeviceSession(lchd, interner=interner)
    try:
        torch = sess.torch
        dev = torch.device("cuda", sess.device)

        def wf_index(n):
            idx = lchd._wf_indices(case.get("keys"), n)
            return None if idx is None else torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int32)).to(dev)

        if drv == "prims":
            sides = []
            for pk, per in zip(packed, (case["per_a"], case["per_b"])):
                cl = sess.upload(pk.xyz, pk.cat, pk.tag)
                if per is not None:
                    cl = sess.periodic_images(cl, per[1], case["thr"]) if per[0] == "box" else sess.periodic_images(cl, reach=case["thr"], cell=per[1])
                sides.append(cl)
            anchors = torch.from_numpy(np.asarray(case["pairs"], dtype=np.int64).reshape(-1, 2)).to(dev)
            wf = wf_index(len(case["pairs"]))
            rad = sess.radial(sides[0], sides[1], anchors, case["thr"], e, wf_index=wf).cpu().numpy()
            comp = [sess.composition(sides[k], anchors[:, k].contiguous(), case["thr"], wf_index=wf).cpu().numpy() for k in (0, 1)]
            return rad, comp
        if drv == "prims_batch":
            batch, offs = sess.upload_batch([(pk.xyz, pk.cat, pk.tag) for pk in packed])
            out = []
            for a, b, pairs in case["jobs"]:
                if not pairs:
                    out.append(np.zeros((0, ax["k"])))
                    continue
                flat = np.asarray(pairs, dtype=np.int64).reshape(-1, 2) + np.asarray([offs[a], offs[b]], dtype=np.int64)
                out.append(sess.radial(batch, batch, torch.from_numpy(flat).to(dev), case["thr"], e).cpu().numpy())
            return out, None
        if drv == "coords":
            a, b = sess.upload(case["xa"], lchd._cats(case["sa"])), sess.upload(case["xb"], lchd._cats(case["sb"]))
            wf = wf_index(case["n"])
            per = {**scoring.side_kw(case["per_a"], "a"), **scoring.side_kw(case["per_b"], "b")}
            rad = sess.radial_coords(a, b, e, wf_index=wf, **per).cpu().numpy()
            comp = [sess.composition_coords(c, wf_index=wf, **comp_kw(p)).cpu().numpy() for c, p in ((a, case["per_a"]), (b, case["per_b"]))]
            return rad, comp
        assert drv == "coords_ensemble"
        cat, wf = lchd._cats(case["seq"]), wf_index(case["n"])
        return None, [sess.composition_coords(sess.upload(case["xs"][k], cat), wf_index=wf, **comp_kw(fp._per_of(case, k))).cpu().numpy()
                      for k in (0, case["m"] - 1)]
    finally:
        sess.close()


# ---- the checks -------------------------------------------------------------------------------------------------------------------
def flat_bins(case, ax):
    """[items][K] True where a bin does not overlap the support of the item's weight function: F(e_k) == F(e_{k+1}) in longdouble."""
    return np.asarray([np.diff(cdf(*fp._wf(case, it[1]), ax["edges"])) == 0 for it in fp.environments(case, ax).items])


def close(got, want, what):
    assert got.shape == want.shape, what
    assert np.all(np.isfinite(got)), what
    assert not np.any(np.signbit(got) & (got == 0.0)), what  # no -0.0
    err = float(np.max(np.abs(got - want), initial=0.0))
    assert err < 1e-10 * max(1.0, float(np.max(np.abs(want), initial=0.0))), what + (err,)
    return err


def same_bits(a, b):
    a, b = (x if isinstance(x, list) else [x] for x in (a, b))
    return len(a) == len(b) and all(p is None and q is None or np.array_equal(p, q) for p, q in zip(a, b))


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
    ax = fp.profile_axes(case)
    drv, det = case["driver"], case["det"]
    what = (seed, drv, case["boundary"], "deterministic" if det else "default", case["entry"], case["ncat"], ax["k"], ax["kind"], case["sd"], case["wfs"])
    periodic = fs.is_periodic(case)
    twin = fs.open_twin(case)

    # the references, all on the host
    t0 = time.perf_counter()
    score_want, score_rows = fs.expected(case, oracle)
    rad_want = fp.radial_reference(case, ax) if ax["radial"] else None
    sums = ax["radial"] and ax["kind"] in ("cover", "on_points")
    rad_scores = fp.oracle_scores(case, ax, oracle) if sums else None
    comp_want = fp.composition_reference(case, ax, oracle) if ax["composition"] else None
    rad_gap = comp_gap = None
    if periodic and sums:
        rad_gap = float(np.max(np.abs(fp.radial_reference(twin, ax).sum(1) - rad_want.sum(1))))
    if periodic and ax["composition"]:
        comp_gap = max(float(np.max(np.abs(a - b))) for a, b in zip(comp_want, fp.composition_reference(twin, ax, oracle)) if a is not None)
    t1 = time.perf_counter()

    lchd = fs.build(lh, case, deterministic=det)

    def scored(name):
        got = scoring.run_host(lh, lchd, case)
        parts = scoring.parts(got if score_rows is None else np.asarray(got)[..., score_rows])
        for g, w in zip(parts, scoring.parts(score_want)):
            assert g.shape == w.shape and np.all(np.isfinite(g)), what
            assert np.max(np.abs(g - w), initial=0.0) < 1e-10 * max(1.0, float(np.max(np.abs(w), initial=0.0))), what + (name,)
        return got

    before = scored("the scoring call before the profile calls")

    # 6. ragged rows
    if ax["ragged"]:
        ra, rb = [r.tolist() for r in case["rows_a"]], [r.tolist() for r in case["rows_b"]]
        with pytest.raises(ValueError, match=re.escape(fp.RAGGED_RADIAL)):
            lchd.radial_from_dmxs(case["sa"], case["sb"], ra, rb, ax["edges"], case["keys"])
        with pytest.raises(ValueError, match=re.escape(fp.RAGGED_COMPOSITION)):
            lchd.composition_from_dmx(case["sa"], ra, case["keys"])

    # 1. the oracle comparison
    def radial_checked(full, name):
        got = take(full, ax, case)
        err = close(got, rad_want, what + (name,))
        flat = flat_bins(case, ax)
        assert np.all(got[flat] == 0.0), what + (name, "a bin outside the support is not exactly 0.0")
        if ax["kind"] == "below" or ax["kind"] == "beyond":
            print(f"seed {seed}: {ax['kind']}, {int(flat.sum())} of {flat.size} bins outside the support")
        if sums:
            rows = got.sum(1)
            assert np.max(np.abs(rows - rad_scores), initial=0.0) < 1e-10 * max(1.0, float(np.max(np.abs(rad_scores), initial=0.0))), what + (name, "row sums")
        print(f"radial {name} vs the reference:", err, what[:8])

    def composition_checked(full, name):
        got = composition_sampled(full, ax, case)
        err = max(close(g, w, what + (name,)) for g, w in zip(got, comp_want) if w is not None)
        print(f"composition {name} vs the reference:", err, what[:6])

    rad = comp = None
    if ax["radial"]:
        rad = radial_host(lh, lchd, case, ax)
        radial_checked(rad, "host")
    if ax["composition"]:
        comp = composition_host(lh, lchd, case)
        composition_checked(comp, "host")
    t2 = time.perf_counter()
    print(f"seed {seed}: references {t1 - t0:.3f} s on the host, first library calls {t2 - t1:.3f} s")

    # 2. deterministic seeds
    if det:
        if ax["radial"]:
            assert same_bits(rad, radial_host(lh, lchd, case, ax)), what
        if ax["composition"]:
            assert same_bits(comp, composition_host(lh, lchd, case)), what
        if drv == "prims":
            perm = np.random.default_rng(seed).permutation(len(case["pairs"]))
            moved = dict(case, pairs=[case["pairs"][k] for k in perm], keys=None if case["keys"] is None else [case["keys"][k] for k in perm])
            assert np.array_equal(radial_host(lh, lchd, moved, ax), rad[perm]), what
            assert same_bits(composition_host(lh, lchd, moved), [t[perm] for t in comp]), what
            # an anchor listed once or three times
            for k, (prims, per) in enumerate(zip(scoring.prims_of(lh, case), (case["per_a"], case["per_b"]))):
                a = case["pairs"][0][k]
                key = None if case["keys"] is None else case["keys"][0]
                once = lchd.composition_from_primitives(prims, [a], case["thr"], None if key is None else [key], **comp_kw(per))
                thrice = lchd.composition_from_primitives(prims, [a] * 3, case["thr"], None if key is None else [key] * 3, **comp_kw(per))
                assert np.array_equal(thrice, np.repeat(once, 3, axis=0)) and np.array_equal(once[0], comp[k][0]), what

    # 3. the session path
    if case["entry"] == "session" and drv in fs.SESSION_DRIVERS:
        s_rad, s_comp = through_a_session(lh, lchd, case, ax)
        if s_rad is not None:
            radial_checked(s_rad, "session")
        if s_comp is not None:
            composition_checked(s_comp, "session")
        if det:  # (otherwise each result stands against the reference on its own)
            assert s_rad is None or same_bits(s_rad, rad), what
            assert s_comp is None or same_bits(s_comp, comp), what

    # 4. the open twin: a periodic keyword that a profile call ignores fails here
    for family, gap in (("radial", rad_gap), ("composition", comp_gap)):
        if gap is None or (seed, family) in NO_GAP or (seed not in DEFAULT and gap <= GAP):
            continue
        assert gap > GAP, what
        if family == "radial":
            diff = float(np.max(np.abs(take(radial_host(lh, lchd, twin, ax), ax, case).sum(1) - take(rad, ax, case).sum(1))))
        else:
            opened = composition_sampled(composition_host(lh, lchd, twin), ax, case)
            diff = max(float(np.max(np.abs(a - b))) for a, b in zip(opened, composition_sampled(comp, ax, case)) if a is not None)
        print(f"seed {seed}: {family}, periodic against open: reference {gap:.3e}, library {diff:.3e}")
        assert diff > 0.5 * gap, what + (family,)

    # 5. non-interference
    after = scored("the scoring call after the profile calls")
    if det:
        assert scoring.bits_equal(before, after), what
