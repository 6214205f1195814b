"""Seeded random configurations of the WHOLE API surface, HIP path vs CPU oracle: tests/test_gpu_fuzz.py extended to what the library
gained since (periodic boxes and cells, minimum-image rows, the two ensembles with blocking and excluded pairs, from_primitives_batch,
deterministic mode, 16-bit category ids, ragged from_dmxs, the DeviceSession entry points).  tests/fuzz_surface.py holds the draw
and the references, tests/test_fuzz_surface_draw.py checks them without a device; a failure here is reproduced by its seed."""
import os
import time

import numpy as np
import pytest

import fuzz_surface as fs

pytestmark = pytest.mark.gpu
N_SEEDS = int(os.environ.get("LCHD_FUZZ_SEEDS", "40"))  # a one-off campaign: LCHD_FUZZ_SEEDS=3000 python -m pytest tests/test_gpu_fuzz_surface.py
SAME = 1e-13  # between two device paths


def side_kw(per, side):
    return {} if per is None else {f"{per[0]}_{side}": per[1]}


def batch_kw(per):
    return {} if per is None else {"boxes" if per[0] == "box" else "cells": per[1]}


def prims_of(lh, case):
    return (fs.prim_list(lh, case["sa"], case["tags_a"], case["xa"]), fs.prim_list(lh, case["sb"], case["tags_b"], case["xb"]))


def run_host(lh, lchd, case):
    """The case through the host-pointer API: an array, or a list of arrays for a batch."""
    drv, keys = case["driver"], case.get("keys")
    if drv == "prims":
        pa, pb = prims_of(lh, case)
        return np.asarray(lchd.from_primitives(pa, pb, fs.anchor_pairs(case), case["thr"], **side_kw(case["per_a"], "a"), **side_kw(case["per_b"], "b")))
    if drv == "prims_batch":
        return [np.asarray(g) for g in lchd.from_primitives_batch([fs.prim_list(lh, *s) for s in case["structs"]], case["jobs"], case["thr"])]
    if drv == "coords":
        return np.asarray(lchd.from_coords(case["sa"], case["sb"], case["xa"], case["xb"], keys, **side_kw(case["per_a"], "a"), **side_kw(case["per_b"], "b")))
    if drv == "dmxs":
        return np.asarray(lchd.from_dmxs(case["sa"], case["sb"], case["da"], case["db"], keys))
    if drv == "dmxs_ragged":
        return np.asarray(lchd.from_dmxs(case["sa"], case["sb"], [r.tolist() for r in case["rows_a"]], [r.tolist() for r in case["rows_b"]], keys))
    if drv == "coords_ensemble":
        return lchd.from_coords_ensemble(case["seq"], case["xs"], case["spairs"], keys, case["excluded"], **batch_kw(case["per"]))
    return lchd.from_dmxs_ensemble(case["seq"], case["dmxs"], case["spairs"], keys)


def run_session(lh, lchd, case):
    """The same case through DeviceSession: upload / upload_batch, periodic_images, from_primitives / from_coords / from_coords_ensemble."""
    from loco_hd_amd.device import DeviceSession

    drv = case["driver"]
    interner = {}
    if drv == "prims":
        packed = [lchd.pack(p, interner) for p in prims_of(lh, case)]
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
            return sess.from_primitives(sides[0], sides[1], anchors, case["thr"], wf_index=wf_index(len(case["pairs"]))).cpu().numpy()
        if drv == "prims_batch":
            batch, offs = sess.upload_batch([(pk.xyz, pk.cat, pk.tag) for pk in packed])
            out = []
            for a, b, pairs in case["jobs"]:  # one pass per job on the one batch object
                if not pairs:
                    out.append(np.zeros(0))
                    continue
                flat = np.asarray(pairs, dtype=np.int64).reshape(-1, 2) + np.asarray([offs[a], offs[b]], dtype=np.int64)
                out.append(sess.from_primitives(batch, batch, torch.from_numpy(flat).to(dev), case["thr"]).cpu().numpy())
            return out
        if drv == "coords":
            a, b = sess.upload(case["xa"], lchd._cats(case["sa"])), sess.upload(case["xb"], lchd._cats(case["sb"]))
            return sess.from_coords(a, b, wf_index=wf_index(case["n"]), **side_kw(case["per_a"], "a"), **side_kw(case["per_b"], "b")).cpu().numpy()
        assert drv == "coords_ensemble"
        cat = lchd._cats(case["seq"])
        batch, _ = sess.upload_batch([(x, cat) for x in case["xs"]])
        pairs = None if case["spairs"] is None else torch.from_numpy(np.asarray(case["spairs"], dtype=np.int32).reshape(-1, 2)).to(dev)
        return sess.from_coords_ensemble(batch, pairs, wf_index=wf_index(case["n"]), excluded=case["excluded"], **batch_kw(case["per"])).cpu().numpy()
    finally:
        sess.close()


def parts(x):
    return x if isinstance(x, list) else [x]


def bits_equal(a, b):
    return len(parts(a)) == len(parts(b)) and all(np.array_equal(p, q) for p, q in zip(parts(a), parts(b)))


def worst(a, b):
    return max((float(np.max(np.abs(p - q), initial=0.0)) for p, q in zip(parts(a), parts(b))), default=0.0)


@pytest.mark.parametrize("seed", range(N_SEEDS))
def test_random_configuration(oracle, seed, monkeypatch):
    import loco_hd_amd as lh

    # the hooks of tests/test_gpu_fuzz.py on the same seed classes (read when a context is created): the regular pipeline on odd
    # seeds, side B without de-duplication on seeds 3 mod 4
    if seed % 2:
        monkeypatch.setenv("LCHD_NO_INLINE_META", "1")
    if seed % 4 == 3:
        monkeypatch.setenv("LCHD_PER_PAIR", "1")
    case = fs.draw(seed)
    if case.get("block"):
        monkeypatch.setenv("LCHD_ENSEMBLE_BLOCK", "2")
    drv, det = case["driver"], case["det"]
    what = (seed, drv, case["boundary"], "deterministic" if det else "default", case["entry"], case["ncat"], case["sd"], case["wfs"])

    t0 = time.perf_counter()
    want, rows = fs.expected(case, oracle)
    t1 = time.perf_counter()
    lchd = fs.build(lh, case, deterministic=det)
    got = run_host(lh, lchd, case)
    print(f"seed {seed}: reference {t1 - t0:.3f} s on the host, first library call {time.perf_counter() - t1:.3f} s")

    def sampled(x):
        return x if rows is None else np.asarray(x)[..., rows]

    def against_the_oracle(result, name):
        assert len(parts(result)) == len(parts(want))
        err = 0.0
        for g, w in zip(parts(sampled(result)), parts(want)):
            assert g.shape == w.shape, what
            assert np.all(np.isfinite(g)), what  # the reference is finite everywhere (test_fuzz_surface_draw.py)
            tol = 1e-10 * max(1.0, float(np.max(np.abs(w), initial=0.0)))
            err = max(err, float(np.max(np.abs(g - w), initial=0.0)))
            assert np.max(np.abs(g - w), initial=0.0) < tol, what
        print(name, "vs the oracle:", err, what[:6])

    against_the_oracle(got, "host")

    if det:
        assert bits_equal(got, run_host(lh, lchd, case)), what  # the same call twice
        if drv == "prims":  # a permuted pair list gives the permuted scores
            perm = np.random.default_rng(seed).permutation(len(case["pairs"]))
            moved = dict(case, pairs=[case["pairs"][k] for k in perm], keys=None if case["keys"] is None else [case["keys"][k] for k in perm])
            assert np.array_equal(run_host(lh, lchd, moved), got[perm]), what
        if drv in fs.ENSEMBLES:  # the per-pair calls, bit for bit
            keys = case["keys"]
            for p, (i, k) in enumerate(fs.structure_pairs(case)):
                if drv == "dmxs_ensemble":
                    one = lchd.from_dmxs(case["seq"], case["seq"], case["dmxs"][i], case["dmxs"][k], keys)
                elif case["excluded"] is None:
                    per = case["per"]
                    pi, pk = ((per[0], per[1][q]) if per is not None and np.ndim(per[1]) == 3 else per for q in (i, k))
                    one = lchd.from_coords(case["seq"], case["seq"], case["xs"][i], case["xs"][k], keys, **side_kw(pi, "a"), **side_kw(pk, "b"))
                elif case["per"] is None:  # excluded entries: from_dmxs on the open rows with +inf in them
                    mats = []
                    for x in (case["xs"][i], case["xs"][k]):
                        m = fs.norm3(x[:, None, :] - x[None, :, :])
                        for r, c in case["excluded"]:
                            m[r, c] = np.inf
                        mats.append(m)
                    one = lchd.from_dmxs(case["seq"], case["seq"], mats[0], mats[1], keys)
                else:  # (no per-pair call takes a periodic cell and excluded entries)
                    continue
                assert np.array_equal(got[p], np.asarray(one)), what + (p, i, k)
    elif drv == "prims":  # the same object again: later passes launch the sweep kernels the first pass's statistics suggest
        for _ in range(2):
            again = run_host(lh, lchd, case)
            assert np.all(np.isfinite(again)) and np.max(np.abs(again - got), initial=0.0) < SAME, what

    if case["entry"] == "session":
        through = run_session(lh, lchd, case)
        against_the_oracle(through, "session")
        if det:
            assert bits_equal(through, got), what
        else:
            assert worst(through, got) < SAME, what

    if fs.is_periodic(case):  # a periodic keyword that is silently ignored fails here
        opened = run_host(lh, lchd, fs.open_twin(case))
        assert worst(opened, got) > 1e-6, what
