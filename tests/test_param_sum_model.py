"""The Python-integer model of the reduced parameter-gradient calls (tests/param_sum_util.py) against its definition in
fractions.Fraction, on drawn rows: weights of mixed sign and scale whose columns cancel, whole-NaN rows, a zero weight, terms that lose
bits below 2^-192, terms at and beyond the 2^63 limit, and the buckets of a two-function dictionary.  CPU only."""
import math

import numpy as np
import pytest

import gradient_native_util as gn
import param_sum_util as ps

CASES = ps.drawn_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_model_is_the_definition(name):
    rows, w, bucket, nb = CASES[name]
    got, flag = ps.param_sum(rows, w, bucket, nb)
    want, wflag = ps.param_sum_fraction(rows, w, bucket, nb)
    assert got.shape == (nb, rows.shape[1]) and flag == wflag
    assert gn.bits(got).tolist() == gn.bits(want).tolist()


def test_cancelling_columns_keep_the_last_bit():
    rows, w, _, _ = CASES["cancel"]
    got, flag = ps.param_sum(rows, w)
    assert flag == 0
    # the twelve paired rows cancel exactly; what is left is the exact sum of the three last rows' terms, at scales 2^-40, 1 and 2^40
    tail = [[float(w[12 + r]) * float(rows[12 + r, k]) for r in range(3)] for k in range(rows.shape[1])]
    assert got[0].tolist() == [math.fsum(t) for t in tail]
    naive = (rows * w[:, None]).sum(0)
    assert np.any(naive != got[0])  # (a float64 sum in row order does not get there)


def test_nan_rows_are_skipped_and_a_zero_weight_adds_nothing():
    rows, w, _, _ = CASES["nan_rows_zero_weight"]
    got, flag = ps.param_sum(rows, w)
    keep = [p for p in range(len(rows)) if p not in (2, 4, 7)]
    assert flag == 0 and gn.bits(got).tolist() == gn.bits(ps.param_sum(rows[keep], w[keep])[0]).tolist()
    assert np.isfinite(got).all()


def test_terms_below_the_quantum_are_truncated():
    rows, w, _, _ = CASES["truncated"]
    got, flag = ps.param_sum(rows, w)
    assert flag == 0
    exact = [math.fsum(float(w[p]) * float(rows[p, k]) for p in range(len(rows))) for k in range(rows.shape[1])]
    assert np.all(np.abs(got[0] - exact) <= 2.0 ** -190)
    assert ps.param_sum(rows[3:4], w[3:4])[0].tolist() == [[0.0, 0.0, 0.0]]  # (below 2^-192 altogether)


def test_the_limit_is_two_to_the_63():
    for name, want in (("limit", 1), ("infinite", 1), ("below_limit", 0)):
        rows, w, _, _ = CASES[name]
        assert ps.param_sum(rows, w)[1] == want, name
    rows, w, _, _ = CASES["limit"]
    assert float(w[1]) * float(rows[1, 0]) == 2.0 ** 63


def test_buckets_of_a_two_function_dictionary():
    rows, w, bucket, nb = CASES["buckets"]
    got, flag = ps.param_sum(rows, w, bucket, nb)
    assert flag == 0 and got.shape == (2, 4)
    assert got[0, 2:].tolist() == [0.0, 0.0] and not np.any(np.signbit(got[0, 2:]))
    for f in range(2):
        own = bucket == f
        assert gn.bits(got[f]).tolist() == gn.bits(ps.param_sum(rows[own], w[own])[0][0]).tolist()
