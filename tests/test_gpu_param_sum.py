"""Reduced parameter gradients on the device (DeviceSession.category_gradient_sum / weight_gradient_sum and the LoCoHD host-array forms).

The expected value is always the model of tests/param_sum_util.py (one float64 product per term, the Python-integer exact accumulator,
one rounding) applied to the output of the existing per-pair call on the same session and inputs: the sums must equal it in every bit,
and the weight form's scores must equal the per-pair call's in every bit.  Random coordinates, no exact ties: default and deterministic
mode see the same lists."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import gradient_native_util as gn
import param_sum_util as ps

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
CATS5 = [f"c{k}" for k in range(5)]
UNI = ("uniform", [3.0, 10.0])
FAMILIES = {"uniform": [3.0, 10.0], "hyper_exp": [1.0, 0.5, 0.2, 0.05], "dagum": [4.0, 6.0, 1.5], "kumaraswamy": [2.0, 11.0, 2.0, 3.0]}
DISTANCES = {"h2": ("Hellinger", [2.0]), "h3.5": ("Hellinger", [3.5]), "ks": ("Kolmogorov-Smirnov", []), "kl": ("Kullback-Leibler", [1e-3]),
             "renyi": ("Renyi", [2.5, 1e-3])}
CW = [1.0, 0.5, 2.0, 1.5, 0.75]
THR = 10.0


def case(seed=7, n=40, n_pairs=12):
    rng = np.random.default_rng(seed)
    xa, xb = rng.uniform(0.0, 12.0, (n, 3)), rng.uniform(0.0, 12.0, (n, 3))
    ca, cb = rng.integers(0, 5, n).astype(np.int32), rng.integers(0, 5, n).astype(np.int32)
    return xa, xb, ca, cb, rng.integers(0, n, (n_pairs, 2))


def pair_weights(n, seed=3):
    """Mixed sign, one zero, scaled by 2^40 here and there so that columns cancel."""
    rng = np.random.default_rng(seed)
    v = rng.uniform(-1.0, 1.0, n) * np.where(rng.integers(0, 2, n) == 1, 2.0 ** 40, 1.0)
    v[n // 2] = 0.0
    return v


def locohd(sd=DISTANCES["h2"], wf=UNI, weights=None, **kw):
    import loco_hd_amd as lh

    w = {k: lh.WeightFunction(*v) for k, v in wf.items()} if isinstance(wf, dict) else lh.WeightFunction(*wf)
    return lh.LoCoHD(CATS5, w, category_weights=weights, statistical_distance=lh.StatisticalDistance(sd[0], sd[1]), **kw)


class Session:
    """One DeviceSession with the 40-atom case uploaded."""

    def __init__(self, host, data=None, n_pairs=12):
        import torch
        from loco_hd_amd.device import DeviceSession

        self.torch, self.data = torch, case(n_pairs=n_pairs) if data is None else data
        xa, xb, ca, cb, pairs = self.data
        self.sess = DeviceSession(host)
        self.a, self.b = self.sess.upload(xa, ca), self.sess.upload(xb, cb)
        self.anchors = torch.from_numpy(np.ascontiguousarray(pairs, dtype=np.int64)).cuda()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.sess.close()

    def dev(self, v, dtype=None):
        return None if v is None else self.torch.from_numpy(np.ascontiguousarray(v, dtype=dtype)).cuda()


def same(got, want, what=""):
    got, want = np.asarray(got.cpu() if hasattr(got, "cpu") else got), np.asarray(want)
    assert got.shape == want.shape, what
    assert gn.bits(got).tolist() == gn.bits(want).tolist(), what


def category_model(s, v=None, **kw):
    rows = s.sess.category_gradient(s.a, s.b, s.anchors, THR, **kw).cpu().numpy()
    out, flag = ps.param_sum(rows, v)
    assert flag == 0 and np.isfinite(rows).all() and np.any(rows != 0.0)
    return out[0]


def weight_model(s, v=None, wf_index=None, n_wf=1):
    rows = s.sess.weight_gradient(s.a, s.b, s.anchors, THR, wf_index=s.dev(wf_index, np.int32))
    grad = rows.grad.cpu().numpy()
    out, flag = ps.param_sum(grad, v, wf_index, n_wf)
    assert flag == 0 and np.isfinite(grad).all() and np.any(grad != 0.0)
    return rows.scores.cpu().numpy(), out


# ---- thresholded: tiles, weights, repeats, modes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
def test_category_sum_tiles_weights_repeat_and_modes(weighted):
    with Session(locohd(weights=CW)) as s:
        v = pair_weights(12) if weighted else None
        want = category_model(s, v)
        for tile in (0, 1, 5, 12, 100, 5):  # (5 twice: a repeated call)
            same(s.sess.category_gradient_sum(s.a, s.b, s.anchors, THR, s.dev(v), tile_pairs=tile), want, f"tile {tile}")
        s.sess.set_deterministic(True)
        same(category_model(s, v), want, "the per-pair rows of deterministic mode")
        for tile in (0, 5):
            same(s.sess.category_gradient_sum(s.a, s.b, s.anchors, THR, s.dev(v), tile_pairs=tile), want, f"deterministic, tile {tile}")


@pytest.mark.parametrize("weighted", [False, True])
def test_weight_sum_tiles_weights_repeat_and_modes(weighted):
    with Session(locohd()) as s:
        v = pair_weights(12) if weighted else None
        scores, want = weight_model(s, v)
        for tile in (0, 1, 5, 12, 100, 5):
            got = s.sess.weight_gradient_sum(s.a, s.b, s.anchors, THR, s.dev(v), tile_pairs=tile)
            assert tuple(got.grad.shape) == (1, 2)
            same(got.grad, want, f"tile {tile}")
            same(got.scores, scores, f"scores, tile {tile}")
        s.sess.set_deterministic(True)
        for tile in (0, 5):
            got = s.sess.weight_gradient_sum(s.a, s.b, s.anchors, THR, s.dev(v), tile_pairs=tile)
            same(got.grad, want, f"deterministic, tile {tile}")
            same(got.scores, scores, f"deterministic scores, tile {tile}")


# ---- distances and families ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dist", ["h2", "h3.5", "kl"])
def test_category_sum_distances(dist):
    with Session(locohd(DISTANCES[dist], weights=CW)) as s:
        v = pair_weights(12)
        same(s.sess.category_gradient_sum(s.a, s.b, s.anchors, THR, s.dev(v), tile_pairs=5), category_model(s, v), dist)


@pytest.mark.parametrize("dist,family", [(d, "uniform") for d in sorted(DISTANCES)] + [("h2", f) for f in sorted(FAMILIES) if f != "uniform"])
def test_weight_sum_distances_and_families(dist, family):
    with Session(locohd(DISTANCES[dist], (family, FAMILIES[family]))) as s:
        v = pair_weights(12)
        scores, want = weight_model(s, v)
        got = s.sess.weight_gradient_sum(s.a, s.b, s.anchors, THR, s.dev(v), tile_pairs=5)
        assert tuple(got.grad.shape) == (1, len(FAMILIES[family]))
        same(got.grad, want, f"{dist}, {family}")
        same(got.scores, scores, f"{dist}, {family}: scores")


def test_weight_sum_dictionary_buckets():
    with Session(locohd(wf=DICT)) as s:
        wf_index = np.asarray([p % 2 if p % 5 else 1 - p % 2 for p in range(12)], dtype=np.int32)
        v = pair_weights(12)
        scores, want = weight_model(s, v, wf_index, 2)
        for tile in (0, 5):
            got = s.sess.weight_gradient_sum(s.a, s.b, s.anchors, THR, s.dev(v), s.dev(wf_index), tile_pairs=tile)
            assert tuple(got.grad.shape) == (2, 4)
            same(got.grad, want, f"tile {tile}")
            same(got.scores, scores)
            grad = got.grad.cpu().numpy()
            assert np.all(grad[0, 2:] == 0.0) and not np.any(np.signbit(grad[0, 2:])) and np.any(grad[0, :2] != 0.0) and np.any(grad[1, 2:] != 0.0)
        rows = s.sess.weight_gradient(s.a, s.b, s.anchors, THR, wf_index=s.dev(wf_index)).grad.cpu().numpy()
        for f in range(2):  # each row: the model over its own pairs
            own = wf_index == f
            same(grad[f], ps.param_sum(rows[own], v[own])[0][0], f"function {f}")


def test_weight_sum_dictionary_without_an_index():
    """A dictionary and no wf_index: every pair is scored with function 0, as the per-pair call scores it; bucket 0 takes every pair."""
    with Session(locohd(wf=DICT)) as s:
        v = pair_weights(12)
        per = s.sess.weight_gradient(s.a, s.b, s.anchors, THR)
        rows = per.grad.cpu().numpy()
        assert rows.shape == (12, 4) and np.all(rows[:, 2:] == 0.0) and np.any(rows[:, :2] != 0.0)
        want = np.zeros((2, 4))
        want[0] = ps.param_sum(rows, v)[0][0]
        for tile in (0, 5):
            got = s.sess.weight_gradient_sum(s.a, s.b, s.anchors, THR, s.dev(v), tile_pairs=tile)
            assert tuple(got.grad.shape) == (2, 4)
            same(got.grad, want, f"tile {tile}")
            same(got.scores, per.scores.cpu().numpy())
        data = case(seed=11, n=24)
    with Session(locohd(wf=DICT), data) as s:  # ... and the dense form
        v = pair_weights(24)
        per = s.sess.weight_gradient_coords(s.a, s.b)
        want = np.zeros((2, 4))
        want[0] = ps.param_sum(per.grad.cpu().numpy(), v)[0][0]
        got = s.sess.weight_gradient_sum_coords(s.a, s.b, s.dev(v))
        same(got.grad, want, "dense")
        same(got.scores, per.scores.cpu().numpy())


# ---- dense --------------------------------------------------------------------------------------------------------------------------
def test_dense_forms():
    data = case(seed=11, n=24)
    with Session(locohd(weights=CW), data) as s:
        v = pair_weights(24)
        for kw in ({}, {"box_a": [30.0, 31.0, 32.0]}):
            rows = s.sess.category_gradient_coords(s.a, s.b, **kw).cpu().numpy()
            assert np.isfinite(rows).all()
            for w in (None, v):
                same(s.sess.category_gradient_sum_coords(s.a, s.b, s.dev(w), **kw), ps.param_sum(rows, w)[0][0], f"category, {kw}")
        rows = s.sess.weight_gradient_coords(s.a, s.b)
        got = s.sess.weight_gradient_sum_coords(s.a, s.b, s.dev(v))
        same(got.grad, ps.param_sum(rows.grad.cpu().numpy(), v)[0])
        same(got.scores, rows.scores.cpu().numpy())


# ---- a batch cloud on side B, global atom indices -----------------------------------------------------------------------------------
def test_batch_cloud():
    xa, xb, ca, cb, pairs = case()
    with Session(locohd(weights=CW)) as s:
        batch, offs = s.sess.upload_batch([(xb[:20], cb[:20]), (xb[20:], cb[20:])])
        assert offs.tolist() == [0, 20, 40]
        v = pair_weights(12)
        rows = s.sess.category_gradient(s.a, batch, s.anchors, THR).cpu().numpy()
        same(s.sess.category_gradient_sum(s.a, batch, s.anchors, THR, s.dev(v), tile_pairs=5), ps.param_sum(rows, v)[0][0])
        per = s.sess.weight_gradient(s.a, batch, s.anchors, THR)
        got = s.sess.weight_gradient_sum(s.a, batch, s.anchors, THR, s.dev(v), tile_pairs=5)
        same(got.grad, ps.param_sum(per.grad.cpu().numpy(), v)[0])
        same(got.scores, per.scores.cpu().numpy())
        assert np.any(rows != s.sess.category_gradient(s.a, s.b, s.anchors, THR).cpu().numpy())  # (two structures of 20 are not one of 40)


# ---- the stride loop and the multi-workgroup atomics: the grid cap lowered to 1 and 2 workgroups -------------------------------------
def big_case():
    xa, xb, ca, cb, _ = case()
    rng = np.random.default_rng(5)
    return xa, xb, ca, cb, rng.integers(0, 40, (1500, 2))


DICT = {"u": UNI, "k": ("kumaraswamy", FAMILIES["kumaraswamy"])}


def dict_index(n):
    return np.asarray([(p * 7 // 3) % 2 for p in range(n)], dtype=np.int32)


def hexes(a):
    return [float(x).hex() for x in np.asarray(a).reshape(-1)]


def child_main():
    """Run in a child process (the hook is read when the context is created): the category form, the weight form with one function and
    with a dictionary and an index, at tiles 0 and 700; sums as hex on stdout."""
    out = {}
    v, wf_index = pair_weights(1500), dict_index(1500)
    with Session(locohd(weights=CW), big_case()) as s:
        for tile in (0, 700):
            out[f"category {tile}"] = hexes(s.sess.category_gradient_sum(s.a, s.b, s.anchors, THR, s.dev(v), tile_pairs=tile).cpu().numpy())
            got = s.sess.weight_gradient_sum(s.a, s.b, s.anchors, THR, s.dev(v), tile_pairs=tile)
            out[f"weight {tile}"], out[f"scores {tile}"] = hexes(got.grad.cpu().numpy()), hexes(got.scores.cpu().numpy())
    with Session(locohd(wf=DICT), big_case()) as s:
        for tile in (0, 700):
            got = s.sess.weight_gradient_sum(s.a, s.b, s.anchors, THR, s.dev(v), s.dev(wf_index), tile_pairs=tile)
            out[f"dict {tile}"], out[f"dict scores {tile}"] = hexes(got.grad.cpu().numpy()), hexes(got.scores.cpu().numpy())
    print("RESULT " + json.dumps(out))


def unhex(res, key, shape):
    return np.asarray([float.fromhex(x) for x in res[key]]).reshape(shape)


def test_stride_loop_and_contention():
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(ROOT), str(ROOT / "tests")] + [p for p in [os.environ.get("PYTHONPATH")] if p]))
    code = "import test_gpu_param_sum as t; t.child_main()"
    procs = [subprocess.Popen([sys.executable, "-c", code], env=dict(env, LCHD_PARAM_SUM_BLOCKS=str(blocks)), cwd=str(ROOT),
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for blocks in (1, 2)]
    try:
        v, wf_index = pair_weights(1500), dict_index(1500)
        with Session(locohd(weights=CW), big_case()) as s:  # the default cap, and the model
            want_c = category_model(s, v)
            scores, want_w = weight_model(s, v)
            for tile in (0, 700):
                same(s.sess.category_gradient_sum(s.a, s.b, s.anchors, THR, s.dev(v), tile_pairs=tile), want_c, f"default cap, tile {tile}")
                got = s.sess.weight_gradient_sum(s.a, s.b, s.anchors, THR, s.dev(v), tile_pairs=tile)
                same(got.grad, want_w, f"default cap, tile {tile}")
                same(got.scores, scores)
        with Session(locohd(wf=DICT), big_case()) as s:  # the dictionary kernel: direct atomics from every wavefront
            dscores, want_d = weight_model(s, v, wf_index, 2)
            assert np.all(want_d[0, 2:] == 0.0) and np.any(want_d[1, 2:] != 0.0)
            for tile in (0, 700):
                got = s.sess.weight_gradient_sum(s.a, s.b, s.anchors, THR, s.dev(v), s.dev(wf_index), tile_pairs=tile)
                same(got.grad, want_d, f"dictionary, default cap, tile {tile}")
                same(got.scores, dscores)
        for blocks, proc in zip((1, 2), procs):
            stdout, stderr = proc.communicate(timeout=120)
            assert proc.returncode == 0, stderr[-2000:]
            res = json.loads([ln for ln in stdout.splitlines() if ln.startswith("RESULT ")][0][7:])
            for tile in (0, 700):
                what = f"{blocks} workgroups, tile {tile}"
                same(unhex(res, f"category {tile}", (5,)), want_c, what)
                same(unhex(res, f"weight {tile}", (1, 2)), want_w, what)
                same(unhex(res, f"scores {tile}", (1500,)), scores, what)
                same(unhex(res, f"dict {tile}", (2, 4)), want_d, "dictionary, " + what)
                same(unhex(res, f"dict scores {tile}", (1500,)), dscores, "dictionary, " + what)
    finally:
        for proc in procs:
            if proc.poll() is None:
                proc.kill()
            proc.communicate()


# ---- failures -----------------------------------------------------------------------------------------------------------------------
def test_runaway_weight():
    with Session(locohd(weights=CW)) as s:
        torch = s.torch
        rows = s.sess.category_gradient(s.a, s.b, s.anchors, THR).cpu().numpy()
        per = s.sess.weight_gradient(s.a, s.b, s.anchors, THR)
        v = np.ones(12)
        v[int(np.argmax(np.abs(rows[:, 0]) * np.abs(per.grad.cpu().numpy()[:, 0])))] = 1e300
        assert ps.param_sum(rows, v)[1] == 1 and ps.param_sum(per.grad.cpu().numpy(), v)[1] == 1
        with pytest.raises(ValueError, match=r"parameter gradient contribution not finite or >= 2\^63 \(pair weights\?\)"):
            s.sess.category_gradient_sum(s.a, s.b, s.anchors, THR, s.dev(v), tile_pairs=5)
        same(s.sess.category_gradient_sum(s.a, s.b, s.anchors, THR, tile_pairs=5), ps.param_sum(rows)[0][0], "the next call")
        out = (torch.full((12,), -1.0, dtype=torch.float64, device="cuda"), torch.empty((1, 2), dtype=torch.float64, device="cuda"))
        with pytest.raises(ValueError, match=r"parameter gradient contribution not finite or >= 2\^63 \(pair weights\?\)"):
            s.sess.weight_gradient_sum(s.a, s.b, s.anchors, THR, s.dev(v), tile_pairs=5, out=out)
        same(out[0], per.scores.cpu().numpy(), "the scores behind the failure")
        got = s.sess.weight_gradient_sum(s.a, s.b, s.anchors, THR, tile_pairs=5)
        same(got.grad, ps.param_sum(per.grad.cpu().numpy())[0], "the next call")
        for bad in (np.nan, np.inf):
            v[0] = bad
            with pytest.raises(ValueError, match="parameter gradient contribution"):
                s.sess.category_gradient_sum(s.a, s.b, s.anchors, THR, s.dev(v))
        same(s.sess.category_gradient_sum(s.a, s.b, s.anchors, THR), ps.param_sum(rows)[0][0], "after NaN and inf weights")


def test_bad_weight_function_index():
    specs = {"u": UNI, "k": ("kumaraswamy", FAMILIES["kumaraswamy"])}
    with Session(locohd(wf=specs)) as s:
        good = np.asarray([p % 2 for p in range(12)], dtype=np.int32)
        bad = good.copy()
        bad[7] = 2
        with pytest.raises(Exception) as per_pair:
            s.sess.weight_gradient(s.a, s.b, s.anchors, THR, wf_index=s.dev(bad))
        for tile in (0, 5):
            with pytest.raises(type(per_pair.value)) as reduced:
                s.sess.weight_gradient_sum(s.a, s.b, s.anchors, THR, wf_index=s.dev(bad), tile_pairs=tile)
            assert str(reduced.value) == str(per_pair.value)
        with pytest.raises(type(per_pair.value)):
            s.sess.category_gradient_sum(s.a, s.b, s.anchors, THR, wf_index=s.dev(bad), tile_pairs=5)
        scores, want = weight_model(s, None, good, 2)
        got = s.sess.weight_gradient_sum(s.a, s.b, s.anchors, THR, wf_index=s.dev(good), tile_pairs=5)
        same(got.grad, want, "the next call")
        same(got.scores, scores)


# ---- the host-array forms are the session forms ---------------------------------------------------------------------------------------
def test_host_array_forms():
    import loco_hd_amd as lh

    xa, xb, ca, cb, pairs = case()
    host = locohd(weights=CW)
    pa = [lh.PrimitiveAtom(CATS5[k], "x", list(x)) for k, x in zip(ca, xa)]
    pb = [lh.PrimitiveAtom(CATS5[k], "x", list(x)) for k, x in zip(cb, xb)]
    plist = [(int(i), int(j)) for i, j in pairs]
    seq_a, seq_b = [CATS5[k] for k in ca], [CATS5[k] for k in cb]
    v = pair_weights(12)
    box = [14.0, 15.0, 16.0]
    with Session(host) as s:
        same(host.category_gradient_sum_from_primitives(pa, pb, plist, THR, v, tile_pairs=5),
             s.sess.category_gradient_sum(s.a, s.b, s.anchors, THR, s.dev(v)).cpu().numpy())
        images = s.sess.periodic_images(s.a, box=box, reach=THR)
        want = s.sess.category_gradient_sum(images, s.b, s.anchors, THR, s.dev(v)).cpu().numpy()
        same(host.category_gradient_sum_from_primitives(pa, pb, plist, THR, v, box_a=box), want, "box_a")
        assert np.any(want != s.sess.category_gradient_sum(s.a, s.b, s.anchors, THR, s.dev(v)).cpu().numpy())
        got, ref = host.weight_gradient_sum_from_primitives(pa, pb, plist, THR, v), s.sess.weight_gradient_sum(s.a, s.b, s.anchors, THR, s.dev(v))
        assert isinstance(got, lh.WeightGradientSum)
        same(got.grad, ref.grad.cpu().numpy())
        same(got.scores, ref.scores.cpu().numpy())
        v40 = pair_weights(40)
        same(host.category_gradient_sum_from_coords(seq_a, seq_b, xa, xb, None, v40), s.sess.category_gradient_sum_coords(s.a, s.b, s.dev(v40)).cpu().numpy())
        got, ref = host.weight_gradient_sum_from_coords(seq_a, seq_b, xa, xb, None, v40), s.sess.weight_gradient_sum_coords(s.a, s.b, s.dev(v40))
        same(got.grad, ref.grad.cpu().numpy())
        same(got.scores, ref.scores.cpu().numpy())
