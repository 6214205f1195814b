"""Local composition profiles on the device against the CPU oracle.

Every expected value comes from the total-variation identity  P_X = (F(inf) - F(0)) - score_TV(environment, lone anchor of category X)
evaluated by the unchanged oracle (from_primitives / from_dmxs with StatisticalDistance("Hellinger", [1.0])), or -- where a whole table
of many categories or long rows is needed -- from tests/composition_util.py, which tests/test_composition_model.py pins to that
identity.  Bound: the project's parity bound, 1e-11 absolute."""
import numpy as np
import pytest

import composition_util as cu
from min_image_util import brute_rows

pytestmark = pytest.mark.gpu

TOL = 1e-11
CATS7 = [f"c{k}" for k in range(7)]
HYPER = ("hyper_exp", [1.0, 0.2])


def _lh():
    import loco_hd_amd as lh

    return lh


def _cdf(spec):
    wf = _lh().WeightFunction(*spec)
    return lambda x: np.asarray(wf.integral_vec(x))


def _atoms(mod, types, tags, xyz):
    return [mod.PrimitiveAtom(t, g, list(c)) for t, g, c in zip(types, tags, xyz)]


def oracle_table(orc, cats, weights, w_func_spec, xyz, types, tags, anchors, thr, accept_same=True, keys=None, cat_subset=None):
    """(len(anchors), len(cat_subset or cats)) by the identity: one oracle from_primitives call per category X, side B a lone X atom."""
    if isinstance(w_func_spec, dict):
        wf = {k: orc.WeightFunction(*v) for k, v in w_func_spec.items()}
        span = np.asarray([np.diff(wf[k].integral_vec([0.0, np.inf]))[0] for k in keys])
    else:
        wf = orc.WeightFunction(*w_func_spec)
        span = np.diff(wf.integral_vec([0.0, np.inf]))[0]
    lchd = orc.LoCoHD(cats, wf, orc.TagPairingRule({"accept_same": accept_same}), category_weights=weights,
                      statistical_distance=orc.StatisticalDistance("Hellinger", [1.0]))
    prims = _atoms(orc, types, tags, xyz)
    pairs = [(int(a), 0) for a in anchors] if keys is None else [(int(a), 0, k) for a, k in zip(anchors, keys)]
    cols = []
    for x in (cats if cat_subset is None else cat_subset):
        lone = [orc.PrimitiveAtom(x, "lone", [0.0, 0.0, 0.0])]
        cols.append(span - np.asarray(lchd.from_primitives(prims, lone, pairs, thr)))
    return np.stack(cols, axis=1)


def _check(got, want, what):
    err = float(np.max(np.abs(np.asarray(got) - want)))
    print(f"{what}: max |device - oracle identity| = {err:.3g}")
    assert np.isfinite(np.asarray(got)).all()
    assert err <= TOL, what


class Cloud:
    def __init__(self, seed, n, edge, cats, n_tags=4):
        rng = np.random.default_rng(seed)
        self.xyz = rng.uniform(0.0, edge, (n, 3))
        self.types = [cats[k] for k in rng.integers(0, len(cats), n)]
        self.tags = [f"t{k}" for k in rng.integers(0, n_tags, n)]
        self.cats = cats
        self.cat_ids = np.asarray([cats.index(t) for t in self.types])
        self.atoms = _atoms(_lh(), self.types, self.tags, self.xyz)


@pytest.fixture(scope="module")
def cloud():
    return Cloud(11, 300, 20.0, CATS7)


@pytest.fixture(scope="module")
def anchors300():
    rng = np.random.default_rng(5)
    a = np.concatenate([np.arange(300), rng.integers(0, 300, 50)])  # every atom, 50 of them twice
    rng.shuffle(a)
    return a


# ---- thresholded ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accept_same", [True, False])
def test_random_cloud(oracle, cloud, anchors300, accept_same):
    lh = _lh()
    lchd = lh.LoCoHD(CATS7, lh.WeightFunction(*HYPER), lh.TagPairingRule({"accept_same": accept_same}))
    got = lchd.composition_from_primitives(cloud.atoms, anchors300, 10.0)
    assert got.shape == (350, 7)
    want = oracle_table(oracle, CATS7, None, HYPER, cloud.xyz, cloud.types, cloud.tags, anchors300, 10.0, accept_same)
    _check(got, want, f"random cloud, accept_same={accept_same}")
    assert np.max(np.abs(got.sum(axis=1) - 1.0)) <= TOL  # F(inf) - F(0) of a hyper_exp function


@pytest.mark.parametrize("n_functions", [2, 5])  # (up to four functions: key sets written next to k_env_group's; beyond: the same, one more set each)
def test_weight_function_dictionary(oracle, cloud, anchors300, n_functions):
    lh = _lh()
    specs = {"near": ("uniform", [0.0, 6.0]), "far": ("hyper_exp", [1.0, 0.1]), "dag": ("dagum", [4.0, 6.0, 1.5]),
             "kum": ("kumaraswamy", [2.0, 11.0, 2.0, 3.0]), "mid": ("uniform", [3.0, 10.0])}
    specs = {k: specs[k] for k in list(specs)[:n_functions]}
    keys = [list(specs)[(3 * int(a) + j) % n_functions] for j, a in enumerate(anchors300)]  # a repeated anchor gets different keys
    lchd = lh.LoCoHD(CATS7, {k: lh.WeightFunction(*v) for k, v in specs.items()})
    got = lchd.composition_from_primitives(cloud.atoms, anchors300, 10.0, keys)
    want = oracle_table(oracle, CATS7, None, specs, cloud.xyz, cloud.types, cloud.tags, anchors300, 10.0, keys=keys)
    _check(got, want, f"dictionary of {n_functions}")


def test_category_weights(oracle, cloud, anchors300):
    lh = _lh()
    w = [0.5, 2.0, 1.0, 3.25, 0.75, 1.5, 1.0]
    lchd = lh.LoCoHD(CATS7, lh.WeightFunction("uniform", [3.0, 10.0]), category_weights=w)
    got = lchd.composition_from_primitives(cloud.atoms, anchors300, 10.0)
    want = oracle_table(oracle, CATS7, w, ("uniform", [3.0, 10.0]), cloud.xyz, cloud.types, cloud.tags, anchors300, 10.0)
    _check(got, want, "category weights")


def _lattice():
    g = np.arange(7, dtype=np.float64)
    xyz = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)  # 1.0 A spacing: every distance ties many times
    rng = np.random.default_rng(3)
    types = [CATS7[k] for k in rng.integers(0, 7, len(xyz))]
    return xyz, types, ["t"] * len(xyz)


def test_lattice_cloud(oracle):
    lh = _lh()
    xyz, types, tags = _lattice()
    anchors = np.arange(len(xyz))
    lchd = lh.LoCoHD(CATS7, lh.WeightFunction(*HYPER))
    got = lchd.composition_from_primitives(_atoms(lh, types, tags, xyz), anchors, 4.0)
    _check(got, oracle_table(oracle, CATS7, None, HYPER, xyz, types, tags, anchors, 4.0), "lattice")


def test_isolated_atom(oracle, cloud):
    lh = _lh()
    xyz = np.vstack([cloud.xyz, [[500.0, 500.0, 500.0]]])
    types, tags = cloud.types + ["c4"], cloud.tags + ["t0"]
    lchd = lh.LoCoHD(CATS7, lh.WeightFunction("uniform", [3.0, 10.0]))
    got = lchd.composition_from_primitives(_atoms(lh, types, tags, xyz), [300, 0, 300], 10.0)
    want = np.zeros(7)
    want[4] = 1.0
    assert np.array_equal(got[0], want) and np.array_equal(got[2], want)  # a one-point environment: (F(inf) - F(0)) on its own category
    _check(got, oracle_table(oracle, CATS7, None, ("uniform", [3.0, 10.0]), xyz, types, tags, [300, 0, 300], 10.0), "isolated atom")


def test_environments_beyond_the_default_slots(oracle):
    """700 atoms inside a 9 A ball, threshold 12: environments of 400 .. 700 points exceed the 320- and 512-point slots of k_env_group;
    the pass is repeated with 1024-point slots through k_env_cells."""
    lh = _lh()
    rng = np.random.default_rng(17)
    v = rng.normal(size=(700, 3))
    xyz = v / np.linalg.norm(v, axis=1, keepdims=True) * 9.0 * rng.uniform(0.0, 1.0, (700, 1)) ** (1.0 / 3.0)
    types = [CATS7[k] for k in rng.integers(0, 7, 700)]
    tags = ["t"] * 700
    anchors = np.arange(700)
    lchd = lh.LoCoHD(CATS7, lh.WeightFunction(*HYPER))
    got = lchd.composition_from_primitives(_atoms(lh, types, tags, xyz), anchors, 12.0)
    _check(got, oracle_table(oracle, CATS7, None, HYPER, xyz, types, tags, anchors, 12.0), "700 atoms in a ball")


@pytest.mark.parametrize("n_cat", [300, 700])  # (16-bit category store; 700: two tiles of category accumulators)
def test_many_categories(oracle, n_cat):
    lh = _lh()
    cats = [f"k{k}" for k in range(n_cat)]
    cl = Cloud(23, 300, 20.0, cats)
    anchors = np.arange(300)
    w = np.random.default_rng(2).uniform(0.5, 2.0, n_cat)
    lchd = lh.LoCoHD(cats, lh.WeightFunction(*HYPER), category_weights=list(w))
    got = lchd.composition_from_primitives(cl.atoms, anchors, 10.0)
    assert got.shape == (300, n_cat)
    _check(got, cu.profiles_of_cloud(cl.xyz, cl.cat_ids, cl.tags, anchors, 10.0, w, _cdf(HYPER)), f"{n_cat} categories (restatement)")
    subset = [cl.types[0], cl.types[1], cats[255], cats[256], cats[n_cat - 1]]
    cols = [cats.index(s) for s in subset]
    want = oracle_table(oracle, cats, list(w), HYPER, cl.xyz, cl.types, cl.tags, anchors, 10.0, cat_subset=subset)
    _check(got[:, cols], want, f"{n_cat} categories (oracle identity)")


# ---- periodic ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["box", "cell"])
def test_periodic_against_the_replicated_cloud(oracle, kind):
    lh = _lh()
    rng = np.random.default_rng(29)
    n = 200
    cell = np.diag([18.0, 20.0, 22.0]) if kind == "box" else np.asarray([[19.0, 0.0, 0.0], [5.0, 20.0, 0.0], [-4.0, 6.0, 21.0]])
    xyz = rng.uniform(0.0, 1.0, (n, 3)) @ cell  # inside the cell: wrapping changes nothing
    types = [CATS7[k] for k in rng.integers(0, 7, n)]
    tags = [f"t{k}" for k in rng.integers(0, 3, n)]
    lchd = lh.LoCoHD(CATS7, lh.WeightFunction(*HYPER))
    kw = {"box": [18.0, 20.0, 22.0]} if kind == "box" else {"cell": cell}
    got = lchd.composition_from_primitives(_atoms(lh, types, tags, xyz), np.arange(n), 8.0, **kw)
    shifts = [(0, 0, 0)] + [s for s in np.ndindex(3, 3, 3) if s != (1, 1, 1)]
    big = np.vstack([xyz] + [xyz + (np.asarray(s, dtype=np.float64) - 1.0) @ cell for s in shifts[1:]])  # the originals first
    want = oracle_table(oracle, CATS7, None, HYPER, big, types * 27, tags * 27, np.arange(n), 8.0)
    _check(got, want, f"periodic {kind}")


def _dense_identity(orc, cats, weights, w_func_spec, seq, dmx_rows):
    """Rows of given distances against a lone X, through the oracle's from_dmxs: (rows, C)."""
    wf = orc.WeightFunction(*w_func_spec)
    span = np.diff(wf.integral_vec([0.0, np.inf]))[0]
    lchd = orc.LoCoHD(cats, wf, category_weights=weights, statistical_distance=orc.StatisticalDistance("Hellinger", [1.0]))
    lone = np.zeros((len(dmx_rows), 1))
    return np.stack([span - np.asarray(lchd.from_dmxs(seq, [x], dmx_rows, lone)) for x in cats], axis=1)


def test_coords_with_a_cell(oracle):
    lh = _lh()
    rng = np.random.default_rng(31)
    n = 90
    cell = np.asarray([[14.0, 0.0, 0.0], [6.0, 13.0, 0.0], [-3.0, 5.0, 12.0]])
    xyz = rng.uniform(-20.0, 30.0, (n, 3))  # not wrapped
    seq = [CATS7[k] for k in rng.integers(0, 7, n)]
    lchd = lh.LoCoHD(CATS7, lh.WeightFunction(*HYPER))
    got = lchd.composition_from_coords(seq, xyz, cell=cell)
    rows = np.asarray(brute_rows(xyz, range(n), cell))
    _check(got, _dense_identity(oracle, CATS7, None, HYPER, seq, rows), "from_coords in a cell")


# ---- dense ---------------------------------------------------------------------------------------------------------------------------
def _dist(xyz):
    d = xyz[:, None, :] - xyz[None, :, :]
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


@pytest.mark.parametrize("n", [2, 65, 1025])
def test_dense_rows(oracle, n):
    lh = _lh()
    rng = np.random.default_rng(n)
    xyz = rng.uniform(0.0, 30.0, (n, 3))
    seq = [CATS7[k] for k in rng.integers(0, 7, n)]
    w = [0.5, 2.0, 1.0, 3.25, 0.75, 1.5, 1.0]
    lchd = lh.LoCoHD(CATS7, lh.WeightFunction(*HYPER), category_weights=w)
    got = lchd.composition_from_coords(seq, xyz)
    assert got.shape == (n, 7)
    _check(got, _dense_identity(oracle, CATS7, w, HYPER, seq, _dist(xyz)), f"dense rows, n = {n}")


def test_dmx_with_an_infinite_block(oracle):
    lh = _lh()
    rng = np.random.default_rng(41)
    n = 65
    xyz = rng.uniform(0.0, 25.0, (n, 3))
    seq = [CATS7[k] for k in rng.integers(0, 7, n)]
    dmx = _dist(xyz)
    for r0 in range(0, n, 5):  # the homo-residue ban: the other atoms of a row's own residue count as +inf
        blk = slice(r0, min(r0 + 5, n))
        sub = dmx[blk, blk]
        sub[~np.eye(sub.shape[0], dtype=bool)] = np.inf
    specs = {"a": ("uniform", [3.0, 10.0]), "b": HYPER}
    keys = ["a" if r % 3 else "b" for r in range(n)]
    lchd = lh.LoCoHD(CATS7, {k: lh.WeightFunction(*v) for k, v in specs.items()})
    got = lchd.composition_from_dmx(seq, dmx, keys)
    want = np.empty((n, 7))
    for k, spec in specs.items():
        sel = [r for r in range(n) if keys[r] == k]
        want[sel] = _dense_identity(oracle, CATS7, None, spec, seq, dmx[sel])
    _check(got, want, "dmx with +inf blocks, per-row keys")


def test_long_rows(oracle):
    """16 500 atoms: rows beyond 16 384 points (keys sorted in the store), 258 chunks per row in the profile kernel."""
    lh = _lh()
    from loco_hd_amd.device import DeviceSession

    cats = ["A", "B", "C"]
    rng = np.random.default_rng(43)
    n = 16500
    xyz = rng.uniform(0.0, 60.0, (n, 3))
    cat = rng.integers(0, 3, n).astype(np.int32)
    lchd = lh.LoCoHD(cats, lh.WeightFunction(*HYPER))
    sess = DeviceSession(lchd)
    try:
        got = sess.composition_coords(sess.upload(xyz, cat)).cpu().numpy()
    finally:
        sess.close()
    assert got.shape == (n, 3) and np.isfinite(got).all()
    assert np.max(np.abs(got.sum(axis=1) - 1.0)) <= TOL
    rows = [0, 1, 4097, 9000, 16383, 16499]
    d = xyz[rows][:, None, :] - xyz[None, :, :]
    dm = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    _check(got[rows], cu.profiles_of_rows(dm, cat, np.ones(3), _cdf(HYPER)), "rows of 16 500 points (restatement)")
    # (one row through the oracle: its stable row sort takes seconds per row at this length)
    _check(got[rows[3:4]], _dense_identity(oracle, cats, None, HYPER, [cats[k] for k in cat], dm[3:4]), "a row of 16 500 points (oracle identity)")


# ---- device-resident -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def session_case():
    """Three structures of different sizes as a batch, their restated profiles, and a session on them."""
    lh = _lh()
    from loco_hd_amd.device import DeviceSession

    lchd = lh.LoCoHD(CATS7, lh.WeightFunction(*HYPER))
    sess = DeviceSession(lchd)
    clouds = [Cloud(50 + k, n, 18.0, CATS7) for k, n in enumerate((120, 200, 77))]
    tag_ids = {f"t{k}": k for k in range(4)}
    packed = [(c.xyz, c.cat_ids.astype(np.int32), np.asarray([tag_ids[t] for t in c.tags], dtype=np.int32)) for c in clouds]
    batch, offs = sess.upload_batch(packed)
    tables = [cu.profiles_of_cloud(c.xyz, c.cat_ids, c.tags, np.arange(len(c.xyz)), 9.0, np.ones(7), _cdf(HYPER)) for c in clouds]
    yield sess, clouds, packed, batch, offs, np.vstack(tables)
    sess.close()


def test_batch_of_three_structures(session_case):
    sess, clouds, packed, batch, offs, table = session_case
    torch = sess.torch
    rng = np.random.default_rng(61)
    anchors = rng.permutation(int(offs[-1]))[:300]
    got = sess.composition(batch, torch.from_numpy(anchors).cuda(), 9.0)
    assert tuple(got.shape) == (300, 7)
    _check(got.cpu().numpy(), table[anchors], "batch of three structures")


def test_out_tensor_and_frames_buffer(session_case):
    sess, clouds, packed, batch, offs, table = session_case
    torch = sess.torch
    c = clouds[0]
    n = len(c.xyz)
    tmpl = sess.upload(*packed[0])
    frames = sess.frames_buffer(tmpl, 3)
    rng = np.random.default_rng(67)
    xs = np.stack([c.xyz, c.xyz + rng.normal(0.0, 0.7, c.xyz.shape), c.xyz[::-1].copy()])
    sess.load_frames(frames, xs)
    anchors = torch.arange(3 * n, dtype=torch.int64, device="cuda")
    out = torch.full((3 * n, 7), -1.0, dtype=torch.float64, device="cuda")
    ret = sess.composition(frames, anchors, 9.0, out=out)
    assert ret is out
    want = np.vstack([cu.profiles_of_cloud(x, c.cat_ids, c.tags, np.arange(n), 9.0, np.ones(7), _cdf(HYPER)) for x in xs])
    _check(out.cpu().numpy(), want, "frames buffer, out=")


def test_producer_on_the_current_stream(session_case):
    """The anchors are written by a copy queued on the session's stream behind a delay: the call must read them in stream order."""
    sess, clouds, packed, batch, offs, table = session_case
    torch = sess.torch
    src = torch.from_numpy(np.random.default_rng(71).permutation(int(offs[-1]))[:256]).cuda()
    side = torch.cuda.Stream()
    try:
        with torch.cuda.stream(side):
            sess.use_current_stream()
            anchors = torch.zeros(256, dtype=torch.int64, device="cuda")
            side.synchronize()
            if hasattr(torch.cuda, "_sleep"):
                torch.cuda._sleep(40_000_000)  # some 20 ms
            anchors.copy_(src, non_blocking=True)
            got = sess.composition(batch, anchors, 9.0)
    finally:
        sess.use_current_stream()
    _check(got.cpu().numpy(), table[src.cpu().numpy()], "anchors produced on the stream")


# ---- determinism, state -------------------------------------------------------------------------------------------------------------
def test_deterministic_rows_do_not_depend_on_the_call(oracle):
    lh = _lh()
    xyz, types, tags = _lattice()
    atoms = _atoms(lh, types, tags, xyz)
    lchd = lh.LoCoHD(CATS7, lh.WeightFunction(*HYPER), deterministic=True)
    full = lchd.composition_from_primitives(atoms, np.arange(len(xyz)), 4.0)
    sub = np.random.default_rng(73).permutation(len(xyz))[:90]
    part = lchd.composition_from_primitives(atoms, sub, 4.0)
    assert np.array_equal(part, full[sub])  # identical bits
    # ... nor on earlier calls of the context
    lchd.composition_from_primitives(atoms, np.arange(20), 6.5)
    assert np.array_equal(lchd.composition_from_primitives(atoms, sub, 4.0), part)
    _check(full, oracle_table(oracle, CATS7, None, HYPER, xyz, types, tags, np.arange(len(xyz)), 4.0), "lattice, deterministic mode")


def test_scoring_is_unchanged_by_a_composition_call(cloud):
    lh = _lh()
    other = Cloud(12, 300, 20.0, CATS7)
    pairs = [(i, (7 * i) % 300) for i in range(300)]
    lchd = lh.LoCoHD(CATS7, lh.WeightFunction(*HYPER))
    before = [lchd.from_primitives(cloud.atoms, other.atoms, pairs, 10.0) for _ in range(2)][-1]  # (the second call: the hints have settled)
    lchd.composition_from_primitives(cloud.atoms, np.arange(300), 10.0)
    lchd.composition_from_coords(cloud.types[:64], cloud.xyz[:64])
    after = lchd.from_primitives(cloud.atoms, other.atoms, pairs, 10.0)
    assert np.array_equal(np.asarray(before), np.asarray(after))
