"""Cross-scoring on the device (LoCoHD.cross_from_primitives / nearest_from_primitives, DeviceSession.cross / nearest) against the CPU
oracle's from_primitives on the explicit pair list.  Clouds as in tests/test_gpu_attribution.py: 300 atoms in a box of edge 20, seven
categories, four tags, threshold 10.

Expected values never come from the library, with one stated exception: the ordering rule among exactly equal scores is checked on the
device's own deterministic cross matrix (test_exact_ties_and_order).  Bound: the project's parity bound, 1e-11 absolute."""
import numpy as np
import pytest

import cross_util as cu

pytestmark = pytest.mark.gpu

TOL = 1e-11
THR = 10.0
CATS7 = [f"c{k}" for k in range(7)]
UNI = ("uniform", [3.0, 10.0])
NA, NB = 37, 130


def _lh():
    import loco_hd_amd as lh

    return lh


class Cloud:
    def __init__(self, seed, n=300, edge=20.0, far=0):
        """far: that many extra atoms far outside the box, each alone within any threshold used here."""
        rng = np.random.default_rng(seed)
        self.xyz = np.concatenate([rng.uniform(0.0, edge, (n, 3)), 1000.0 + 100.0 * np.arange(3 * far).reshape(far, 3)])
        self.types = [CATS7[k] for k in rng.integers(0, 7, n + far)]
        self.tags = [f"t{k}" for k in rng.integers(0, 4, n + far)]

    def atoms(self, mod):
        return [mod.PrimitiveAtom(t, g, list(c)) for t, g, c in zip(self.types, self.tags, self.xyz)]


def _make(mod, wf=UNI, accept_same=True, weights=None, sd=("Hellinger", [2.0]), **kw):
    w = {k: mod.WeightFunction(*v) for k, v in wf.items()} if isinstance(wf, dict) else mod.WeightFunction(*wf)
    return mod.LoCoHD(CATS7, w, mod.TagPairingRule({"accept_same": accept_same}), category_weights=weights,
                      statistical_distance=mod.StatisticalDistance(*sd), **kw)


def _oracle_matrix(oracle, a, b, anchors_a, anchors_b, key=None, **cfg):
    """The oracle's from_primitives on the explicit pair list, as an (Na, Nb) matrix."""
    pairs = [(int(i), int(j)) + (() if key is None else (key,)) for i in anchors_a for j in anchors_b]
    s = _make(oracle, **cfg).from_primitives(a.atoms(oracle), b.atoms(oracle), pairs, THR)
    return np.asarray(s).reshape(len(anchors_a), len(anchors_b))


@pytest.fixture(scope="module")
def clouds():
    return Cloud(101), Cloud(102)


@pytest.fixture(scope="module")
def anchors():
    rng = np.random.default_rng(17)
    return rng.choice(300, NA, replace=False).tolist(), rng.choice(300, NB, replace=False).tolist()


@pytest.fixture(scope="module")
def S(oracle, clouds, anchors):
    """The reference matrix of the default configuration, computed once; the narrower nearest cases use its leading columns."""
    m = _oracle_matrix(oracle, *clouds, *anchors)
    m.setflags(write=False)
    return m


@pytest.fixture(scope="module")
def det(clouds):
    """One deterministic instance and the two atom lists for the default configuration."""
    lh = _lh()
    return _make(lh, deterministic=True), clouds[0].atoms(lh), clouds[1].atoms(lh)


# ---- 1. cross parity ----------------------------------------------------------------------------------------------------------------
def test_cross_parity_and_tiling(det, anchors, S):
    lchd, pa, pb = det
    got = {t: lchd.cross_from_primitives(pa, pb, anchors[0], anchors[1], THR, tile_rows=t) for t in (0, 1, 5, 37, 64)}
    for t, m in got.items():
        assert m.shape == (NA, NB) and m.dtype == np.float64
        err = float(np.max(np.abs(m - S)))
        print(f"tile_rows {t}: max |device - oracle| = {err:.3g}")
        assert err <= TOL
    for t, m in got.items():
        assert np.array_equal(m, got[0]), f"tile_rows {t} changed bits"


# ---- 2. nearest, width edges ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [1, 63, 64, 65, 130])
def test_nearest_width_edges(det, anchors, S, nb):
    lchd, pa, pb = det
    for k in sorted({1, min(3, nb), min(nb, 64)}):
        for t in (0, 5):
            got = lchd.nearest_from_primitives(pa, pb, anchors[0], anchors[1][:nb], THR, k, tile_rows=t)
            err = cu.accept(got.scores, got.cols, S[:, :nb], k, TOL)
            print(f"Nb {nb}, k {k}, tile_rows {t}: max |score - oracle| = {err:.3g}")


# ---- 3. exact ties and order ----------------------------------------------------------------------------------------------------------
def test_exact_ties_and_order(det):
    lchd, pa, pb = det
    rng = np.random.default_rng(5)
    base = rng.choice(300, 45, replace=False)
    anchors_b = rng.permutation(np.repeat(base, 3)).tolist()  # every column three times
    anchors_a = rng.permutation(np.repeat(rng.choice(300, 10, replace=False), 2)).tolist()  # every row twice
    m = lchd.cross_from_primitives(pa, pb, anchors_a, anchors_b, THR)
    for atom in base:
        same = [j for j, v in enumerate(anchors_b) if v == atom]
        assert len(same) == 3 and np.array_equal(m[:, same[0]], m[:, same[1]]) and np.array_equal(m[:, same[0]], m[:, same[2]])
    for atom in set(anchors_a):
        r0, r1 = [i for i, v in enumerate(anchors_a) if v == atom]
        assert np.array_equal(m[r0], m[r1])
    for k in (1, 4, 64):
        want_scores, want_cols = cu.nearest(m, k)
        if k >= 3:
            assert (want_scores[:, 0] == want_scores[:, 2]).all() and (np.diff(want_cols[:, :3], axis=1) > 0).all()  # ties in column order
        for t in (1, 7, 0):
            got = lchd.nearest_from_primitives(pa, pb, anchors_a, anchors_b, THR, k, tile_rows=t)
            assert got.cols.dtype == np.int32 and np.array_equal(got.cols, want_cols), f"k {k}, tile_rows {t}"
            assert np.array_equal(got.scores, want_scores), f"k {k}, tile_rows {t}"


# ---- 4. configurations reach the new path unchanged -----------------------------------------------------------------------------------
WFS = {"near": ("uniform", [0.0, 6.0]), "far": ("hyper_exp", [1.0, 0.5, 0.2, 0.05])}
CONFIGS = {
    "reject_same_tag": dict(accept_same=False),
    "category_weights": dict(weights=[1.0, 2.0, 0.5, 1.0, 1.5, 3.0, 0.25]),
    "kolmogorov_smirnov": dict(sd=("Kolmogorov-Smirnov", [])),
    "wf_dictionary": dict(wf=WFS),
}


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_configurations(oracle, clouds, anchors, name):
    lh, cfg = _lh(), CONFIGS[name]
    key = "far" if name == "wf_dictionary" else None
    aa, ab = anchors[0][:9], anchors[1][:70]
    want = _oracle_matrix(oracle, *clouds, aa, ab, key, **cfg)
    got = _make(lh, **cfg).cross_from_primitives(clouds[0].atoms(lh), clouds[1].atoms(lh), aa, ab, THR, key, tile_rows=4)
    err = float(np.max(np.abs(got - want)))
    print(f"{name}: max |device - oracle| = {err:.3g}")
    assert err <= TOL
    if key is not None:  # the key matters: the other function gives other scores
        other = _oracle_matrix(oracle, *clouds, aa, ab, "near", **cfg)
        assert float(np.max(np.abs(other - want))) > 1e-3


def test_an_environment_emptied_by_the_tag_rule(oracle, anchors):
    """The tag rule never rejects the anchor itself (src/locohd.rs:525), so the emptiest environment is the anchor alone: an atom with no
    neighbour within the threshold, or -- under accept_same=False -- one whose neighbours all carry its tag.  Both kinds on both
    sides, in the middle of the lists, against the oracle."""
    lh = _lh()
    a, b = Cloud(101, far=1), Cloud(102, far=1)
    for cl in (a, b):  # atom 0: every neighbour within the threshold gets its tag
        near = np.linalg.norm(cl.xyz - cl.xyz[0], axis=1) <= THR
        cl.tags = [cl.tags[0] if near[i] else t for i, t in enumerate(cl.tags)]
    aa = anchors[0][:3] + [300, 0] + anchors[0][3:6]
    ab = anchors[1][:40] + [0, 300] + anchors[1][40:70]
    want = _oracle_matrix(oracle, a, b, aa, ab, accept_same=False)
    lchd = _make(lh, accept_same=False)
    pa, pb = a.atoms(lh), b.atoms(lh)
    for t in (0, 3):
        got = lchd.cross_from_primitives(pa, pb, aa, ab, THR, tile_rows=t)
        err = float(np.max(np.abs(got - want)))
        print(f"anchors alone in their environments, tile_rows {t}: max |device - oracle| = {err:.3g}")
        assert err <= TOL
    near = lchd.nearest_from_primitives(pa, pb, aa, ab, THR, 5, tile_rows=3)
    cu.accept(near.scores, near.cols, want, 5, TOL)


def test_an_anchor_outside_its_structure(det, anchors):
    lchd, pa, pb = det
    lh = _lh()
    with pytest.raises(lh.PanicException):
        lchd.cross_from_primitives(pa, pb, anchors[0][:5] + [300], anchors[1][:5], THR, tile_rows=2)
    with pytest.raises(lh.PanicException):
        lchd.nearest_from_primitives(pa, pb, anchors[0][:5], anchors[1][:5] + [300], THR, 1)


# ---- 5. batches through the device session --------------------------------------------------------------------------------------------
def test_nearest_over_a_batch(oracle, clouds, anchors):
    import torch

    from loco_hd_amd.device import DeviceSession

    lh = _lh()
    lchd = _make(lh)
    a = clouds[0]
    structures = [Cloud(200 + s, n=100 + 20 * s) for s in range(3)]
    sess = DeviceSession(lchd)
    try:
        interner = {}
        pk_a = lchd.pack(a.atoms(lh), interner)
        packed = [lchd.pack(st.atoms(lh), interner) for st in structures]
        cl_a = sess.upload(pk_a.xyz, pk_a.cat, pk_a.tag)
        cl_b, offs = sess.upload_batch([(p.xyz, p.cat, p.tag) for p in packed])
        rng = np.random.default_rng(3)
        local = [rng.choice(len(st.xyz), 30, replace=False) for st in structures]  # 90 anchors of B over the three structures
        anchors_b = np.concatenate([offs[s] + local[s] for s in range(3)])
        aa = anchors[0][:11]
        dev = torch.device("cuda", sess.device)
        d_a, d_b = torch.tensor(aa, dtype=torch.int64, device=dev), torch.from_numpy(anchors_b).to(dev)
        want = np.concatenate([_oracle_matrix(oracle, a, structures[s], aa, local[s]) for s in range(3)], axis=1)
        m = sess.cross(cl_a, cl_b, d_a, d_b, THR, tile_rows=3)
        assert float(np.max(np.abs(m.cpu().numpy() - want))) <= TOL
        for t in (0, 4):
            got = sess.nearest(cl_a, cl_b, d_a, d_b, THR, 8, tile_rows=t)
            assert got.scores.is_cuda and got.cols.dtype == torch.int32
            err = cu.accept(got.scores.cpu().numpy(), got.cols.cpu().numpy(), want, 8, TOL)
            print(f"batch of three, tile_rows {t}: max |score - oracle| = {err:.3g}")
        out = lh.api.Nearest(torch.empty((11, 8), dtype=torch.float64, device=dev), torch.empty((11, 8), dtype=torch.int32, device=dev))
        assert sess.nearest(cl_a, cl_b, d_a, d_b, THR, 8, out=out).scores.data_ptr() == out.scores.data_ptr()
        cu.accept(out.scores.cpu().numpy(), out.cols.cpu().numpy(), want, 8, TOL)
        with pytest.raises(ValueError, match="k = 65"):
            sess.nearest(cl_a, cl_b, d_a, d_b, THR, 65)
    finally:
        sess.close()


# ---- 6. existing calls untouched ------------------------------------------------------------------------------------------------------
def test_from_primitives_is_bit_equal_around_the_new_calls(det, anchors):
    lchd, pa, pb = det
    rng = np.random.default_rng(9)
    pairs = [(int(i), int(j)) for i, j in rng.integers(0, 300, (40, 2))]
    before = np.asarray(lchd.from_primitives(pa, pb, pairs, THR))
    lchd.cross_from_primitives(pa, pb, anchors[0], anchors[1], THR, tile_rows=5)
    middle = np.asarray(lchd.from_primitives(pa, pb, pairs, THR))
    lchd.nearest_from_primitives(pa, pb, anchors[0], anchors[1], THR, 8)
    after = np.asarray(lchd.from_primitives(pa, pb, pairs, THR))
    assert np.array_equal(before, middle) and np.array_equal(before, after)
