"""The Python-integer model of the exact accumulator (tests/gradient_native_util.py) against its definition: math.fsum wherever no value
has bits below the quantum, permutation invariance, and the edges listed in tests/exact_sum_cases.py.  CPU only."""
import math
import random
from fractions import Fraction

import numpy as np
import pytest

import gradient_native_util as gn
from exact_sum_cases import ULP63, cases

CASES = cases()


def _exact(values) -> bool:
    """No value has bits below q (and all are in range): the accumulator then holds the exact sum."""
    return all(gn.quantize(v) is not None and Fraction(gn.quantize(v)) * gn.Q == Fraction(v) for v in values)


@pytest.mark.parametrize("name", sorted(CASES))
def test_quantize_is_the_truncated_quotient(name):
    for v in CASES[name][:2000]:
        assert gn.quantize(v) == gn.quantize_fraction(v)


@pytest.mark.parametrize("name", sorted(CASES))
def test_equals_fsum_where_nothing_lies_below_the_quantum(name):
    values = CASES[name]
    acc = gn.ExactSum()
    for v in values:
        acc.add(v)
    if _exact(values):
        assert acc.flag == 0
        got, want = acc.finish(), math.fsum(values)
        assert gn.bits(got) == gn.bits(want + 0.0), (got, want)  # (fsum of nothing or of a cancelling sum is +0.0 too)
    else:
        assert name in ("below_q", "below_boundaries", "limit", "minus_limit", "inf", "nan"), name


@pytest.mark.parametrize("name", sorted(CASES))
def test_permutation_invariance(name):
    values = list(CASES[name])
    ref = gn.ExactSum()
    for v in values:
        ref.add(v)
    rnd = random.Random(7)
    for _ in range(3):
        rnd.shuffle(values)
        acc = gn.ExactSum()
        for v in values:
            acc.add(v)
        assert acc.limbs == ref.limbs and acc.flag == ref.flag and gn.bits(acc.finish()) == gn.bits(ref.finish())


def test_three_chunks_and_boundaries():
    acc = gn.ExactSum()
    acc.add(CASES["three_chunks"][0])
    assert [v != 0 for v in acc.limbs] == [True, True, True] + [False] * 5
    acc = gn.ExactSum()
    acc.add(CASES["three_chunks_high"][0])
    assert [v < 0 for v in acc.limbs] == [False, False, True, True, True, False, False, False]
    for k in range(8):
        acc = gn.ExactSum()
        acc.add(2.0 ** (32 * k - 192))
        assert acc.limbs == [1 if j == k else 0 for j in range(8)]
    for k in range(1, 8):  # one ulp below a boundary: the chunks below it, nothing in limb k
        acc = gn.ExactSum()
        acc.add(math.nextafter(2.0 ** (32 * k - 192), 0.0))
        assert acc.limbs[k] == 0 and acc.limbs[k - 1] == 0xFFFFFFFF


def test_truncation_toward_zero_below_the_quantum():
    assert [gn.quantize(v) for v in CASES["below_q"]] == [0, 0, 1, -1, 0, 0]
    assert gn.bits(gn.exact_sum(CASES["below_q"])) == gn.bits(0.0)


def test_range_limit():
    big = 2.0 ** 63 - ULP63
    assert math.nextafter(big, math.inf) == 2.0 ** 63
    acc = gn.ExactSum()
    acc.add(big)
    assert acc.flag == 0 and acc.finish() == big and acc.limbs[7] == 0x7FFFFFFF
    acc.add(-big)
    assert acc.flag == 0 and gn.bits(acc.finish()) == gn.bits(0.0)
    for name, kept in (("limit", 1.0), ("minus_limit", 1.0), ("inf", 2.0), ("nan", 3.0)):
        acc = gn.ExactSum()
        for v in CASES[name]:
            acc.add(v)
        assert acc.flag == 1 and acc.finish() == kept, name  # the offending value adds nothing


def test_headroom_of_a_limb():
    acc = gn.ExactSum()
    for v in CASES["alternating_largest_chunk"]:
        acc.add(v)
    assert acc.limbs == [0] * 8 and gn.bits(acc.finish()) == gn.bits(0.0)
    acc = gn.ExactSum()
    for v in CASES["same_sign_largest_chunk"]:
        acc.add(v)
    assert acc.limbs[2] == (1 << 16) * 0xFFFFFFFF and acc.limbs[3] == 0  # no carry propagation before finish
    assert acc.finish() == (1 << 16) * (2.0 ** 32 - 1) * 2.0 ** (64 - 192)


def test_zero_and_ties():
    assert gn.bits(gn.exact_sum(CASES["cancels_to_zero"])) == gn.bits(0.0)
    assert gn.exact_sum(CASES["tie_to_even_down"]) == 1.0
    assert gn.exact_sum(CASES["tie_to_even_up"]) == 1.0 + 2.0 ** -51
    assert gn.exact_sum(CASES["above_tie"]) == 1.0 + 2.0 ** -52
    assert gn.exact_sum(CASES["carry_into_new_bit"]) == 2.0
    assert gn.exact_sum(CASES["negative_total"]) == math.fsum(CASES["negative_total"]) < 0.0


def test_contribution_rule_skips_and_anchors():
    """Slot 0, the padding, d == 0 and a non-finite g give nothing; the dense anchor is the row, not idx[p][0]."""
    xyz = np.asarray([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [1.0, 2.0, 2.0], [4.0, 0.0, 3.0]])
    idx = np.asarray([[0, 1, 2, 3, -1], [0, 1, 3, 2, -1]], dtype=np.int32)  # row 1 of a dense call: slot 0 is the coincident atom 0
    dist = np.asarray([[0.0, 0.0, 3.0, 5.0, 0.0], [0.0, 0.0, 5.0, 3.0, 0.0]])
    g = np.asarray([[9.0, 0.5, 0.25, np.nan, 7.0], [0.0, 0.5, 0.125, 0.25, 0.0]])
    m, a, step = gn.side_steps(idx, dist, g, xyz, [2.0, 1.0])
    assert m.tolist() == [2, 3, 2] and a.tolist() == [0, 0, 0]
    assert np.array_equal(step[0], (2.0 * 0.25 / 3.0) * xyz[2])
    m, a, step = gn.side_steps(idx, dist, g, xyz, None, dense=True)
    assert m.tolist() == [2, 3, 2] and a.tolist() == [0, 1, 1]
    grad, flag = gn.side_gradient(idx, dist, g, xyz, [2.0, 1.0])
    assert flag == 0 and np.array_equal(grad[1], [0.0, 0.0, 0.0])
    _, flag = gn.side_gradient(idx, dist, g, xyz, [2.0 ** 70, 1.0])
    assert flag == 1
