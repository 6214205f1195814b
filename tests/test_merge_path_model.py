"""profiles/merge_path_model.py: the fixed-trip, branch-free merge-path search of the team tiles (merge_path_fixed, lchd_kcommon.h) against
the plain bisection (merge_path) -- the same partition for every diagonal of every input, ties included (A goes first), with every read
inside the lists (asserted in the model)."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "profiles"))
import merge_path_model as M  # noqa: E402


def brute(A, B, d):
    """entries of A among the first d of the stable merge, A first on ties"""
    keys = np.concatenate([A, B])
    from_a = np.concatenate([np.ones(len(A), bool), np.zeros(len(B), bool)])
    order = np.lexsort((~from_a, keys))  # by key, A before B at equal keys
    return int(from_a[order][:d].sum())


def check(A, B, extra=0):
    A, B = np.sort(np.asarray(A, dtype=np.uint64)), np.sort(np.asarray(B, dtype=np.uint64))
    wmax = min(len(A), len(B)) + extra
    for d in range(len(A) + len(B) + 1):
        want, _ = M.plain(A, B, d)
        got, trips = M.fixed(A, B, d, wmax)
        assert got == want == brute(A, B, d), (len(A), len(B), d)
        assert trips == M.fixed_trips(wmax) <= 9


@pytest.mark.parametrize("seed", range(6))
def test_random_and_tied_keys(seed):
    rng = np.random.default_rng(seed)
    for _ in range(40):
        mA, mB = (int(x) for x in rng.integers(0, 60, 2))
        spread = int(rng.choice([1, 3, 20, 10**6]))  # (1: every key tied)
        check(rng.integers(0, spread, mA), rng.integers(0, spread, mB), extra=int(rng.integers(0, 40)))


def test_extremes_and_limits():
    check([], [])
    check([], [5])
    check([5], [])
    check([5], [5])
    check(np.arange(100), np.arange(100) + 1000)          # every key of A below every key of B
    check(np.arange(100) + 1000, np.arange(100))          # and the reverse
    check(2 * np.arange(120), 2 * np.arange(120) + 1)     # fully interleaved
    check(np.arange(120), np.arange(120))                 # exact ties across the lists
    check(np.full(254, 7), np.full(226, 7))               # a 480-event tile of one key
    check(np.arange(240), [])
    rng = np.random.default_rng(1)
    check(rng.integers(0, 50, 255), rng.integers(0, 50, 225), extra=30)


def test_team_diagonals_cover_the_tile():
    for mA, mB, tl in ((0, 0, 32), (1, 0, 16), (170, 173, 32), (254, 226, 32), (120, 120, 16)):
        d1 = M.team_diagonals(mA, mB, tl)
        assert len(d1) == tl and d1[-1] == mA + mB and all(a <= b for a, b in zip(d1, d1[1:]))
