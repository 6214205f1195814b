"""The model of the native periodic gradients and the strain derivative (tests/strain_native_util.py) pinned to its definition, and the
host path of loco_hd_amd/csrc/lchd_strain_sum.h replayed against it.  CPU only.

The lists are hand-sized: a few pairs, a few slots, every branch of the use rule.  The definition is evaluated with fractions.Fraction:
each float64 term (computed by the rule, one IEEE operation at a time) is cut to a multiple of 2^-192 toward zero, the cuts are summed
exactly, and the sum is rounded once.  The C program (tests/cabi_strain_sum.c) is built with AddressSanitizer and UBSan and run as a
child process; nothing sanitised is loaded into Python."""
import math
import shutil
import struct
import subprocess
from fractions import Fraction
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import gradient_native_util as gn
import strain_native_util as sn

ROOT = Path(__file__).resolve().parent.parent


def lists(seed, n_pairs, width, n_atoms, dense=False, scale=1.0):
    """Random lists with padding, a member at distance 0, a non-finite g and an anchor of its own image (idx[p][k] == idx[p][0])."""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, n_atoms, (n_pairs, width)).astype(np.int32)
    if dense:
        idx[:, 0] = np.arange(n_pairs) % n_atoms
    disp = rng.normal(0.0, 4.0, (n_pairs, width, 3)) * scale
    dist = np.sqrt((disp[..., 0] * disp[..., 0] + disp[..., 1] * disp[..., 1]) + disp[..., 2] * disp[..., 2])
    g = rng.normal(0.0, 0.1, (n_pairs, width)) * scale
    for p in range(n_pairs):
        count = int(rng.integers(1, width + 1))
        idx[p, count:], dist[p, count:], g[p, count:], disp[p, count:] = -1, 0.0, 0.0, 0.0
    if width > 2:
        dist[0, 1], disp[0, 1] = 0.0, 0.0
        g[0, 2] = np.inf
        if idx[0, 2] < 0:
            g[0, 2] = 0.0
        idx[n_pairs - 1, 1] = idx[n_pairs - 1, 0]
    disp[:, 0], dist[:, 0], g[:, 0] = 0.0, 0.0, 0.0
    return SimpleNamespace(idx=idx, dist=dist, g=g, disp=disp, v=rng.uniform(-2.0, 2.0, n_pairs))


CASES = [(1, 1, 1, 3, False), (2, 1, 2, 3, False), (3, 2, 3, 4, False), (4, 3, 5, 6, False), (5, 4, 8, 5, True), (6, 5, 5, 5, True),
         (7, 6, 4, 9, False), (8, 2, 9, 3, False), (9, 7, 3, 7, True), (10, 3, 12, 20, False), (11, 8, 6, 8, True), (12, 5, 7, 2, False)]


def by_definition(L, n_atoms, dense):
    """(grad, W, trace terms) with fractions.Fraction from the rule, slot by slot."""
    q = Fraction(1, 2 ** 192)
    grad = [[Fraction(0)] * 3 for _ in range(n_atoms)]
    w = {c: Fraction(0) for c in sn.COMPONENTS}
    diag = {0: [], 1: [], 2: []}
    for p in range(L.idx.shape[0]):
        a = p if dense else int(L.idx[p, 0])
        for k in range(1, L.idx.shape[1]):
            m, d, g = int(L.idx[p, k]), float(L.dist[p, k]), float(L.g[p, k])
            if m < 0 or not d > 0.0 or not math.isfinite(g):
                continue
            coef = np.float64(L.v[p]) * np.float64(g) / np.float64(d)
            step = [np.float64(coef) * np.float64(L.disp[p, k, c]) for c in range(3)]
            for c in range(3):
                t = int(Fraction(float(step[c])) / q) * q
                grad[m][c] += t
                grad[a][c] -= t
            for i, j in sn.COMPONENTS:
                term = float(np.float64(step[i]) * np.float64(L.disp[p, k, j]))
                w[(i, j)] += int(Fraction(term) / q) * q
                if i == j:
                    diag[i].append(term)
    to_double = lambda f: f.numerator / f.denominator  # noqa: E731  (int / int: correctly rounded)
    W = np.zeros((3, 3))
    for (i, j), f in w.items():
        W[i, j] = W[j, i] = to_double(f)
    return np.asarray([[to_double(f) for f in row] for row in grad]).reshape(n_atoms, 3), W, w, diag


@pytest.mark.parametrize("seed,n_pairs,width,n_atoms,dense", CASES)
def test_model_against_fractions(seed, n_pairs, width, n_atoms, dense):
    n_atoms = max(n_atoms, n_pairs) if dense else n_atoms
    L = lists(seed, n_pairs, width, n_atoms, dense)
    grad, W, flag = sn.side_result(L.idx, L.dist, L.g, L.disp, n_atoms, L.v, dense)
    want_grad, want_w, exact, diag = by_definition(L, n_atoms, dense)
    assert flag == 0
    assert np.array_equal(gn.bits(grad), gn.bits(want_grad))
    assert np.array_equal(gn.bits(W), gn.bits(want_w))
    assert np.array_equal(gn.bits(W), gn.bits(W.T))  # symmetric in every bit
    # trace W is the exact sum of the three diagonal term lists (each term cut at 2^-192, which no term here reaches below)
    q = Fraction(1, 2 ** 192)
    m, a, step, terms = sn.side_terms(L.idx, L.dist, L.g, L.disp, n_atoms, L.v, dense)
    totals, _ = sn.exact_totals(terms)
    assert len(m) == len(diag[0])
    assert [Fraction(t) * q for t in totals] == [exact[c] for c in sn.COMPONENTS]
    trace_exact = sum(int(Fraction(t) / q) * q for i in range(3) for t in diag[i])
    assert (totals[0] + totals[3] + totals[5]) * q == trace_exact
    trace = W[0, 0] + W[1, 1] + W[2, 2]
    assert abs(trace - float(trace_exact)) <= 4 * np.finfo(float).eps * sum(abs(W[i, i]) for i in range(3))


def test_out_of_range_term_raises_the_flag_and_adds_nothing():
    L = lists(3, 2, 3, 4)
    L.idx[:] = [[0, 1, 2], [1, 2, 3]]
    L.dist[:, 1:] = np.sqrt((L.disp[:, 1:] ** 2).sum(-1))
    L.g[:, 1:] = 0.25
    clean = sn.side_result(L.idx, L.dist, L.g, L.disp, 4, L.v)
    assert clean[2] == 0
    L.v[1] = 2.0 ** 70
    huge = sn.side_result(L.idx, L.dist, L.g, L.disp, 4, L.v)
    assert huge[2] == 1
    L.v[1] = np.nan
    assert sn.side_result(L.idx, L.dist, L.g, L.disp, 4, L.v)[2] == 1


def _slots(L, dense, n_atoms):
    rows = []
    for p in range(L.idx.shape[0]):
        for k in range(1, L.idx.shape[1]):
            if L.idx[p, k] >= 0 and L.dist[p, k] > 0.0 and math.isfinite(L.g[p, k]):
                rows.append((L.v[p], L.g[p, k], L.dist[p, k], *L.disp[p, k]))
    return rows


def test_c_header_replays_the_model_under_sanitizers(tmp_path):
    if shutil.which("gcc") is None:
        pytest.fail("gcc is needed to build the C client")
    exe, vec = tmp_path / "cabi_strain_sum", tmp_path / "slots.txt"
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-g", "-Wall", "-Wextra", "-pedantic", "-Werror", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", str(ROOT / "loco_hd_amd" / "csrc"),
                           str(ROOT / "tests" / "cabi_strain_sum.c"), "-o", str(exe)])
    table = []
    for seed, n_pairs, width, n_atoms, dense in CASES:
        L = lists(seed, n_pairs, width, max(n_atoms, n_pairs), dense)
        table.append(_slots(L, dense, n_atoms))
    big = lists(99, 40, 70, 50, scale=2.0 ** 20)  # 70 slots a row, terms up to 2^60: high limbs and carries across lanes
    table.append(_slots(big, False, 50))
    table.append([(2.0 ** 70, 1.0, 1.0, 1.0, 2.0, 3.0), (1.0, 0.5, 2.0, 1.0, -2.0, 0.5), (np.nan, 1.0, 1.0, 1.0, 1.0, 1.0)])  # out of range
    table.append([])
    hexbits = lambda v: f"{struct.unpack('<Q', struct.pack('<d', float(v)))[0]:x}"  # noqa: E731
    with open(vec, "w") as f:
        for rows in table:
            f.write(f"{len(rows)}\n")
            f.writelines(" ".join(hexbits(v) for v in row) + "\n" for row in rows)
    out = subprocess.run([str(exe), str(vec)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    lines = out.stdout.splitlines()
    assert len(lines) == len(table)
    for n, (rows, line) in enumerate(zip(table, lines)):
        arr = np.asarray(rows, dtype=np.float64).reshape(-1, 6)
        with np.errstate(over="ignore", invalid="ignore"):
            coef = (arr[:, 0] * arr[:, 1]) / arr[:, 2]
            step = coef[:, None] * arr[:, 3:]
            terms = np.stack([step[:, i] * arr[:, 3 + j] for i, j in sn.COMPONENTS], axis=1)
        sums = [gn.ExactSum() for _ in sn.COMPONENTS]
        for row in terms.tolist():
            for acc, s in zip(sums, row):
                acc.add(s)
        f = line.split()
        assert [int(x) for x in f[:48]] == [v for acc in sums for v in acc.limbs], n
        assert int(f[48]) == max(acc.flag for acc in sums), n
        want = sn.strain_from_totals([acc.total for acc in sums])
        assert [int(x, 16) for x in f[49:58]] == [int(b) for b in gn.bits(want).reshape(-1)], n
