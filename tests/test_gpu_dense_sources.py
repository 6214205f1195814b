"""Every source of dense rows through every dense host pass, at the smallest shape that reaches it (the seams of RowSource / take_rows /
produce_rows / sort_rows in loco_hd_amd/csrc/lchd_capi.hip).  Sources: open coordinates, a cell on side A only, on side B only, on both
(one diagonal, one triclinic), given host rows, ragged rows with a shortest row of 1, device-resident clouds.  Passes: scoring on the
k_env_rows2, k_env_rows (LCHD_OLD_ROWS; 300 categories) and fused paths, composition, attribution, sensitivity, the ensemble.  A pass is
given the sources its API has: ragged rows are from_dmxs', a sensitivity call takes no cell.  Scores are held against the CPU oracle,
consumer tables against the model and with the tolerance of that consumer's own test file."""
import numpy as np
import pytest

import attribution_util as au
import dense_sensitivity_util as du
from dense_rows_util import oracle_rows
from min_image_util import brute_rows, min_image_matrix
from periodic_cell_util import CELLS
from test_gpu_attribution import TOL as TOL_ATTRIBUTION
from test_gpu_composition import TOL as TOL_COMPOSITION, _dense_identity
from test_gpu_dense_dispatch import TIGHT
from test_gpu_dense_periodic import SAME, matrix  # two device paths on the same rows; the minimum-image rows in the prescribed arithmetic
from test_gpu_sensitivity_dense import _compare

pytestmark = pytest.mark.gpu

NAMES = [f"c{i}" for i in range(300)]
HYP, UNI = ("hyper_exp", [1.0, 0.1]), ("uniform", [3.0, 10.0])
DICT = {"h": HYP, "u": UNI}
BOX = np.diag([9.0, 8.0, 10.0])
SKEW = CELLS["skewed"]
# source -> (cell of side A, cell of side B) for the calls on coordinates
CELL_SOURCES = {"open": (None, None), "cell-a": (SKEW, None), "cell-b": (None, BOX), "cells": (BOX, SKEW)}
# scoring shape -> (n, categories, environment hook, path of lchd_ctx_last_dense)
SCORING = {"rows2": (5, 5, None, "ROWS2"), "rows-hook": (5, 5, "LCHD_OLD_ROWS", "ROWS"), "rows-cat16": (5, 300, None, "ROWS"),
           "fused": (1025, 7, None, "FUSED")}


@pytest.fixture(scope="module")
def lh():
    import loco_hd_amd

    return loco_hd_amd


def wfs(mod, n_wf):
    return mod.WeightFunction(*HYP) if n_wf == 1 else {k: mod.WeightFunction(*v) for k, v in DICT.items()}


def structures(seed, n, n_cat):
    """Lattice-free random coordinates (no two distances of a row tie), a few cells wide; categories as indices."""
    rng = np.random.default_rng(seed)
    return (rng.uniform(-12.0, 21.0, (n, 3)), rng.integers(0, n_cat, n)), (rng.uniform(-12.0, 21.0, (n, 3)), rng.integers(0, n_cat, n))


def rows_of(x, cell, which):
    """Reference rows `which` of a structure: open (utils.rs:1-8 order), or by brute force over the shifts of the cell as given."""
    return [au.open_rows(x)[r] for r in which] if cell is None else brute_rows(x, which, cell)


def given(x, cell):
    """The whole matrix a *_from_dmxs call is handed in place of the coordinates: bit for bit the rows the device produces."""
    if cell is None:
        return du.coords_rows(x)
    if np.array_equal(cell, np.diag(np.diagonal(cell))):  # (a diagonal cell takes the orthorhombic producer's arithmetic)
        return min_image_matrix(x, box=np.diagonal(cell))
    return matrix(x, cell)


def keys_of(n, n_wf):
    return None if n_wf == 1 else [("h", "u")[r % 2] for r in range(n)]


def record(lchd):
    from loco_hd_amd.device import last_dense_of, last_sweep_of

    return last_dense_of(lchd._context()), last_sweep_of(lchd._context())


def check_path(lchd, path, deterministic=False):
    from loco_hd_amd import _native as N

    got = record(lchd)[0]
    assert got is not None and got["path"] == getattr(N, "DENSE_" + path) and (got["attempts"], got["canon"]) == (1, deterministic), got


# ---- scoring ------------------------------------------------------------------------------------------------------------------------
# (the fused kernel writes no store: the dictionary cases are the store paths')
@pytest.mark.parametrize("shape,n_wf", [(s, 1) for s in SCORING] + [(s, 2) for s in SCORING if s != "fused"])
def test_scoring_from_every_source(lh, oracle, monkeypatch, shape, n_wf):
    n, n_cat, hook, path = SCORING[shape]
    det_path = "ROWS2" if path == "FUSED" else path  # (deterministic mode never takes the fused kernel)
    if hook:
        monkeypatch.setenv(hook, "1")
    (xa, ca), (xb, cb) = structures(11, n, n_cat)
    sa, sb = [NAMES[k] for k in ca], [NAMES[k] for k in cb]
    keys = keys_of(n, n_wf)
    lchd, det = (lh.LoCoHD(NAMES[:n_cat], wfs(lh, n_wf), deterministic=d) for d in (False, True))
    orc = oracle.LoCoHD(NAMES[:n_cat], wfs(oracle, n_wf))
    which = list(range(n)) if n <= 5 else [0, 1, 511, 512, n - 1]
    okeys = None if keys is None else [keys[r] for r in which]
    for source, (cell_a, cell_b) in CELL_SOURCES.items():
        kw = {k: v for k, v in (("cell_a", cell_a), ("cell_b", cell_b)) if v is not None}
        got = np.asarray(lchd.from_coords(sa, sb, xa, xb, keys, **kw))
        check_path(lchd, path)
        want = oracle_rows(orc, sa, sb, rows_of(xa, cell_a, which), rows_of(xb, cell_b, which), okeys)
        err = float(np.max(np.abs(got[which] - want)))
        print(f"{shape}, {n_wf} wf, {source}: max |device - oracle| = {err:.3g}")
        assert got.shape == (n,) and np.all(np.isfinite(got)) and err <= TIGHT
        # deterministic mode: coordinates (in their cells) and the same rows given are one result, bit for bit
        by_coords = np.asarray(det.from_coords(sa, sb, xa, xb, keys, **kw))
        check_path(det, det_path, deterministic=True)
        by_rows = np.asarray(det.from_dmxs(sa, sb, given(xa, cell_a), given(xb, cell_b), keys))
        check_path(det, det_path, deterministic=True)
        print(f"{shape}, {n_wf} wf, {source}: coordinates vs given rows, max |difference| = {np.max(np.abs(by_coords - by_rows)):.3g}")
        assert by_coords.tobytes() == by_rows.tobytes(), source
        assert float(np.max(np.abs(by_coords - got))) <= SAME  # (two device paths on the same rows: test_gpu_dense_periodic.SAME)
    # ragged rows: row r has lens[r] entries (a prefix of the sequence), the shortest 1, the longest n; column 0 holds the row's 0
    rng = np.random.default_rng(12)
    lens = [1, n] + rng.integers(1, n + 1, n - 2).tolist()
    ragged_a = [np.concatenate([[0.0], rng.uniform(0.5, 30.0, m - 1)]) for m in lens]
    ragged_b = [np.concatenate([[0.0], rng.uniform(0.5, 30.0, m - 1)]) for m in reversed(lens)]
    got = np.asarray(lchd.from_dmxs(sa, sb, ragged_a, ragged_b, keys))
    check_path(lchd, path)
    want = oracle_rows(orc, sa, sb, [ragged_a[r] for r in which], [ragged_b[r] for r in which], okeys)
    print(f"{shape}, {n_wf} wf, ragged: max |device - oracle| = {np.max(np.abs(got[which] - want)):.3g}")
    assert float(np.max(np.abs(got[which] - want))) <= TIGHT


@pytest.mark.parametrize("shape", ["rows2", "fused"])
def test_device_resident_scoring_and_the_cells_time(lh, shape):
    """DeviceSession.from_coords is the host entry, open and periodic: bit for bit in deterministic mode (the k_env_rows2 shape), to the
    1e-13 of two device paths on the same rows on the fused path, which deterministic mode never takes.  With timing on, "cells" of
    last_ms is the row producers' time: positive after a periodic single-pair call, not after an open one."""
    from loco_hd_amd import _native as N
    from loco_hd_amd.device import DeviceSession

    n, n_cat, _, path = SCORING[shape]
    (xa, ca), (xb, cb) = structures(13, n, n_cat)
    sa, sb = [NAMES[k] for k in ca], [NAMES[k] for k in cb]
    lchd = lh.LoCoHD(NAMES[:n_cat], wfs(lh, 1), deterministic=path != "FUSED")
    host = {s: np.asarray(lchd.from_coords(sa, sb, xa, xb, **{k: v for k, v in (("cell_a", c[0]), ("cell_b", c[1])) if v is not None}))
            for s, c in CELL_SOURCES.items()}
    sess = DeviceSession(lchd)
    try:
        sess.enable_timing(True)
        a, b = sess.upload(xa, ca.astype(np.int32)), sess.upload(xb, cb.astype(np.int32))
        for source, (cell_a, cell_b) in CELL_SOURCES.items():
            got = sess.from_coords(a, b, cell_a=cell_a, cell_b=cell_b).cpu().numpy()
            if path == "FUSED":
                assert float(np.max(np.abs(got - host[source]))) <= SAME, source
            else:
                assert got.tobytes() == host[source].tobytes(), source
            rec, ms = sess.last_dense(), sess.last_ms()
            print(f"{shape}, device clouds, {source}: last_ms = {ms}")
            assert rec["path"] == getattr(N, "DENSE_" + path) and rec["attempts"] == 1
            assert (ms["cells"] > 0.0) == (source != "open"), (source, ms)
    finally:
        sess.close()


# ---- the consumers ------------------------------------------------------------------------------------------------------------------
def composition_model(oracle, n_cat, seq, rows, keys):
    cats = NAMES[:n_cat]
    if keys is None:
        return _dense_identity(oracle, cats, None, HYP, seq, rows)
    per_key = {k: _dense_identity(oracle, cats, None, DICT[k], seq, rows) for k in DICT}
    return np.stack([per_key[k][r] for r, k in enumerate(keys)])


@pytest.mark.parametrize("n_wf", [1, 2])
@pytest.mark.parametrize("consumer", ["composition", "attribution", "sensitivity"])
def test_consumers_from_every_source(lh, oracle, consumer, n_wf):
    """n = 5 (sensitivity: width 8).  A consumer call leaves lchd_ctx_last_dense and lchd_ctx_last_sweep as it found them."""
    from loco_hd_amd.device import DeviceSession

    n, n_cat = 5, 4
    (xa, ca), (xb, cb) = structures(17, n, n_cat)
    sa, sb = [NAMES[k] for k in ca], [NAMES[k] for k in cb]
    keys = keys_of(n, n_wf)
    spec = HYP if keys is None else [DICT[k] for k in keys]
    lchd = lh.LoCoHD(NAMES[:n_cat], wfs(lh, n_wf), deterministic=True)
    scores = np.asarray(lchd.from_coords(sa, sb, xa, xb, keys))  # a scoring call first: its records must survive the consumers
    before = record(lchd)
    assert before[0] is not None
    every = list(range(n))
    sources = CELL_SOURCES if consumer != "sensitivity" else {"open": (None, None)}
    for source, (cell_a, cell_b) in sources.items():
        ra, rb = np.asarray(rows_of(xa, cell_a, every)), np.asarray(rows_of(xb, cell_b, every))
        ga, gb = given(xa, cell_a), given(xb, cell_b)
        what = f"{consumer}, {n_wf} wf, {source}"
        if consumer == "composition":
            got = lchd.composition_from_coords(sa, xa, keys, cell=cell_a)
            by_rows = lchd.composition_from_dmx(sa, ga, keys)
            want, tol = composition_model(oracle, n_cat, sa, ra, keys), TOL_COMPOSITION
        elif consumer == "attribution":
            kw = {k: v for k, v in (("cell_a", cell_a), ("cell_b", cell_b)) if v is not None}
            got = lchd.attribution_from_coords(sa, sb, xa, xb, keys, **kw)
            by_rows = lchd.attribution_from_dmxs(sa, sb, ga, gb, keys)
            specs = [HYP] * n if keys is None else spec  # (the model takes one weight function: row by row)
            want = np.vstack([au.from_rows(ca, ra[r:r + 1], cb, rb[r:r + 1], n_cat, specs[r]) for r in range(n)])
            tol = TOL_ATTRIBUTION
        else:
            got = lchd.sensitivity_from_coords(sa, sb, xa, xb, keys, width=8)
            by_rows = lchd.sensitivity_from_dmxs(sa, sb, ga, gb, keys, width=8)
            _compare(got, du.from_dmxs(ca, ga, cb, gb, n_cat, spec, width=8), scores, what)
            for name in got._fields:
                assert getattr(got, name).tobytes() == getattr(by_rows, name).tobytes(), (what, name)
            continue
        err = float(np.max(np.abs(np.asarray(got) - want)))
        print(f"{what}: max |device - model| = {err:.3g}")
        assert np.isfinite(np.asarray(got)).all() and err <= tol, what
        assert np.asarray(got).tobytes() == np.asarray(by_rows).tobytes(), what  # (deterministic: coordinates and the same rows given)
    assert record(lchd) == before
    # device-resident clouds: the host entry's bits, and the session's records stand as well
    sess = DeviceSession(lchd)
    try:
        torch = sess.torch
        a, b = sess.upload(xa, ca.astype(np.int32)), sess.upload(xb, cb.astype(np.int32))
        wf = None if keys is None else torch.tensor([list(DICT).index(k) for k in keys], dtype=torch.int32, device="cuda")
        assert sess.from_coords(a, b, wf_index=wf).cpu().numpy().tobytes() == scores.tobytes()
        seen = sess.last_dense(), sess.last_sweep()
        if consumer == "composition":
            assert sess.composition_coords(a, wf_index=wf, cell=SKEW).cpu().numpy().tobytes() == lchd.composition_from_coords(sa, xa, keys, cell=SKEW).tobytes()
        elif consumer == "attribution":
            assert (sess.attribution_coords(a, b, wf_index=wf, cell_b=BOX).cpu().numpy().tobytes()
                    == lchd.attribution_from_coords(sa, sb, xa, xb, keys, cell_b=BOX).tobytes())
        else:
            dev, host = sess.sensitivity_coords(a, b, wf_index=wf, width=8), lchd.sensitivity_from_coords(sa, sb, xa, xb, keys, width=8)
            for name in dev._fields:
                assert getattr(dev, name).cpu().numpy().tobytes() == getattr(host, name).tobytes(), name
        assert (sess.last_dense(), sess.last_sweep()) == seen
    finally:
        sess.close()


# ---- the ensemble -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_wf", [1, 2])
def test_ensemble_from_every_source(lh, oracle, n_wf):
    """M = 3, n = 5: open, one cell for all structures, one per structure with one of them non-diagonal, given rows, a device batch."""
    from loco_hd_amd import _native as N
    from loco_hd_amd.device import DeviceSession

    m, n, n_cat = 3, 5, 4
    rng = np.random.default_rng(19)
    xs = rng.uniform(-12.0, 21.0, (m, n, 3))
    cat = rng.integers(0, n_cat, n)
    seq = [NAMES[k] for k in cat]
    keys = keys_of(n, n_wf)
    det = lh.LoCoHD(NAMES[:n_cat], wfs(lh, n_wf), deterministic=True)
    orc = oracle.LoCoHD(NAMES[:n_cat], wfs(oracle, n_wf))
    pairs = [(i, j) for i in range(m) for j in range(i + 1, m)]
    every = list(range(n))
    for source, cells in {"open": None, "one-cell": SKEW, "cell-each": np.stack([BOX, SKEW, 1.1 * BOX])}.items():
        cell_of = [None if cells is None else (cells if cells.ndim == 2 else cells[k]) for k in range(m)]
        got = det.from_coords_ensemble(seq, xs, None, keys, **({} if cells is None else {"cells": cells}))
        rec = record(det)[0]
        assert rec["path"] == N.DENSE_ROWS2 and (rec["attempts"], rec["canon"]) == (1, True), rec
        assert got.shape == (len(pairs), n)
        for p, (i, j) in enumerate(pairs):
            want = oracle_rows(orc, seq, seq, rows_of(xs[i], cell_of[i], every), rows_of(xs[j], cell_of[j], every), keys)
            err = float(np.max(np.abs(got[p] - want)))
            print(f"ensemble, {n_wf} wf, {source}, pair {i}-{j}: max |device - oracle| = {err:.3g}")
            assert err <= TIGHT
        by_rows = det.from_dmxs_ensemble(seq, np.stack([given(xs[k], cell_of[k]) for k in range(m)]), None, keys)
        assert record(det)[0]["path"] == N.DENSE_ROWS2
        assert got.tobytes() == by_rows.tobytes(), source
        sess = DeviceSession(det)
        try:
            batch, _ = sess.upload_batch([(x, cat.astype(np.int32)) for x in xs])
            wf = None if keys is None else sess.torch.tensor([list(DICT).index(k) for k in keys], dtype=sess.torch.int32, device="cuda")
            assert sess.from_coords_ensemble(batch, wf_index=wf, cells=cells).cpu().numpy().tobytes() == got.tobytes(), source
            assert sess.last_dense()["path"] == N.DENSE_ROWS2 and sess.last_dense()["attempts"] == 1
        finally:
            sess.close()
