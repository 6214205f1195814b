"""A Python-integer model of the reduced parameter-gradient calls (test infrastructure, CPU only).

The rule of include/loco_hd_hip.h ("reduced parameter gradients") in numpy float64 -- one IEEE multiplication per term -- followed by
the accumulator of tests/gradient_native_util.py (truncation toward zero at 2^-192, integer sums, one rounding):

    use      = !isnan(row[p][0])
    term_k   = v_p * row[p][k]
    acc[b][k] += term_k ;  out[b][k] = round(acc[b][k])            b = bucket[p] (0 without buckets)
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

import gradient_native_util as gn

MESSAGE = "parameter gradient contribution not finite or >= 2^63 (pair weights?)"


def terms(rows, weights=None):
    """(usable row indices [M], terms [M][W]) in float64."""
    rows = np.asarray(rows, dtype=np.float64)
    rows = rows.reshape(len(rows), -1)
    v = np.ones(len(rows)) if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
    assert len(v) == len(rows)
    use = np.nonzero(~np.isnan(rows[:, 0]))[0] if rows.shape[1] else np.zeros(0, dtype=np.int64)
    with np.errstate(over="ignore", invalid="ignore"):
        return use, v[use, None] * rows[use]


def param_sum(rows, weights=None, bucket=None, n_buckets=1):
    """(out [n_buckets][W] float64, flag): the model of a reduced call on the rows of the per-pair call."""
    rows = np.asarray(rows, dtype=np.float64)
    rows = rows.reshape(len(rows), -1)
    width = rows.shape[1]
    use, t = terms(rows, weights)
    b = np.zeros(len(rows), dtype=np.int64) if bucket is None else np.asarray(bucket, dtype=np.int64).reshape(-1)
    total = [[0] * width for _ in range(n_buckets)]
    flag = 0
    for p, row in zip(use.tolist(), t.tolist()):
        for k, s in enumerate(row):
            q = gn.quantize(s)
            if q is None:
                flag |= 1
                continue
            total[b[p]][k] += q
    return np.asarray([[gn.round_total(x) for x in r] for r in total], dtype=np.float64).reshape(n_buckets, width), flag


def param_sum_fraction(rows, weights=None, bucket=None, n_buckets=1):
    """The same from the definition with fractions.Fraction: every in-range term cut toward zero to a multiple of 2^-192, the exact
    rational sum, one rounding (Fraction -> float is correctly rounded)."""
    rows = np.asarray(rows, dtype=np.float64)
    rows = rows.reshape(len(rows), -1)
    width = rows.shape[1]
    use, t = terms(rows, weights)
    b = np.zeros(len(rows), dtype=np.int64) if bucket is None else np.asarray(bucket, dtype=np.int64).reshape(-1)
    total = [[Fraction(0)] * width for _ in range(n_buckets)]
    flag = 0
    for p, row in zip(use.tolist(), t.tolist()):
        for k, s in enumerate(row):
            q = gn.quantize_fraction(s)
            if q is None:
                flag |= 1
                continue
            total[b[p]][k] += q * gn.Q
    return np.asarray([[float(x) for x in r] for r in total], dtype=np.float64).reshape(n_buckets, width), flag


def drawn_cases(seed=2024):
    """name -> (rows [P][W], weights [P] or None, bucket [P] or None, n_buckets): the cases the model test and the C client share."""
    rng = np.random.default_rng(seed)
    cases = {}
    # weights of mixed sign and scale: columns cancel to the last bit (every row occurs with +s and -s, and once alone at 2^-40)
    base = rng.uniform(-1.0, 1.0, (6, 5))
    rows = np.concatenate([base, base, rng.uniform(-1.0, 1.0, (3, 5))])
    scale = np.asarray([1.0, 2.0 ** 40, 2.0 ** -40, 1.0, 2.0 ** 40, 2.0 ** -40])
    cases["cancel"] = (rows, np.concatenate([scale, -scale, [2.0 ** -40, 1.0, -(2.0 ** 40)]]), None, 1)
    rows = rng.uniform(-2.0, 2.0, (9, 4))
    rows[2] = np.nan
    rows[7] = np.nan
    w = rng.uniform(-3.0, 3.0, 9)
    w[4] = 0.0
    cases["nan_rows_zero_weight"] = (rows, w, None, 1)
    cases["unweighted"] = (rng.uniform(-1.0, 1.0, (11, 3)), None, None, 1)
    rows = rng.uniform(0.5, 1.0, (5, 3))
    rows[1] *= 2.0 ** -150  # terms below 2^-139 lose bits below 2^-192; below 2^-192 they vanish
    rows[3] *= 2.0 ** -200
    cases["truncated"] = (rows, np.asarray([1.0, 1.0, -1.0, 1.0, 2.0 ** -10]), None, 1)
    rows = rng.uniform(-1.0, 1.0, (4, 2))
    rows[1, 0] = 1.0
    cases["limit"] = (rows, np.asarray([1.0, 2.0 ** 63, 1.0, 1.0]), None, 1)  # a term at exactly 2^63
    cases["below_limit"] = (rows, np.asarray([1.0, np.nextafter(2.0 ** 63, 0.0), 1.0, 1.0]), None, 1)
    cases["infinite"] = (rows, np.asarray([1.0, 1.0, np.inf, 1.0]), None, 1)
    # a dictionary of a 2-parameter and a 4-parameter function: zeros behind the shorter one's parameters
    rows = rng.uniform(-1.0, 1.0, (10, 4))
    bucket = np.asarray([0, 1, 1, 0, 0, 1, 0, 1, 1, 0], dtype=np.int32)
    rows[bucket == 0, 2:] = 0.0
    rows[5] = np.nan
    cases["buckets"] = (rows, rng.uniform(-2.0, 2.0, 10), bucket, 2)
    return cases
