"""A Python-integer model of the native gradient calls (test infrastructure, CPU only).

The accumulator of loco_hd_amd/csrc/lchd_exact_sum.h: a value s is cut to t = trunc(s / q) toward zero with q = 2^-192, the t are summed
as integers, and the sum is rounded once to the nearest double (ties to even).  Out of range (not finite, or |s| >= 2^63) adds nothing
and raises a flag.  `ExactSum.limbs` restates the eight little-endian int64 limbs, each the signed sum of the 32-bit chunks it carries.

The contribution rule of include/loco_hd_hip.h ("native coordinate gradients") in numpy float64 -- IEEE operations one at a time, as
the device computes them without contraction:

    use   = idx[p][k] >= 0  &&  dist[p][k] > 0  &&  isfinite(g[p][k])          (k >= 1)
    coef  = (v_p * g[p][k]) / dist[p][k]
    step_c = coef * (x[m][c] - x[a][c])               m = idx[p][k];  a = idx[p][0] (thresholded) or p (dense)
    acc[m][c] += step_c ;  acc[a][c] += -step_c
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

LIMBS, QUANTUM_LOG2, LIMIT_LOG2 = 8, -192, 63
Q = Fraction(1, 2 ** -QUANTUM_LOG2)


def quantize(s: float):
    """trunc(s / q) toward zero as a Python int; None if s is out of range."""
    s = float(s)
    if not math.isfinite(s) or abs(s) >= 2.0 ** LIMIT_LOG2:
        return None
    m, e = math.frexp(abs(s))  # |s| = m 2^e, 0.5 <= m < 1
    mant, sh = int(m * 2.0 ** 53), e - 53 - QUANTUM_LOG2  # |s| / q = mant 2^sh exactly
    t = mant << sh if sh >= 0 else mant >> -sh
    return -t if s < 0 else t


def quantize_fraction(s: float):
    """The same from the definition, with fractions.Fraction (slow; the tests pin `quantize` to it)."""
    s = float(s)
    if not math.isfinite(s) or abs(s) >= 2.0 ** LIMIT_LOG2:
        return None
    return int(Fraction(s) / Q)  # int() of a Fraction truncates toward zero


def round_total(total: int) -> float:
    """The correctly rounded double of q * total (int / int true division rounds to nearest, ties to even); +0.0 for 0."""
    return total / (1 << -QUANTUM_LOG2) if total else 0.0


class ExactSum:
    def __init__(self):
        self.total, self.flag, self.limbs = 0, 0, [0] * LIMBS

    def add(self, s: float):
        t = quantize(s)
        if t is None:
            self.flag |= 1
            return
        self.total += t
        sign, mag = (-1 if t < 0 else 1), abs(t)
        for k in range(LIMBS):
            self.limbs[k] += sign * ((mag >> (32 * k)) & 0xFFFFFFFF)
        assert mag >> (32 * LIMBS) == 0

    def finish(self) -> float:
        assert sum(v << (32 * k) for k, v in enumerate(self.limbs)) == self.total
        return round_total(self.total)


def exact_sum(values) -> float:
    acc = ExactSum()
    for v in values:
        acc.add(v)
    return acc.finish()


def side_steps(idx, dist, g, xyz, weights=None, dense=False):
    """The contributions of one side: (member atoms [M], anchor atoms [M], steps [M][3]) in float64, row-major over (pair, slot)."""
    idx, dist, g = np.asarray(idx), np.asarray(dist, dtype=np.float64), np.asarray(g, dtype=np.float64)
    xyz = np.asarray(xyz, dtype=np.float64)
    n_pairs = idx.shape[0]
    v = np.ones(n_pairs) if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
    anchor = np.arange(n_pairs) if dense else idx[:, 0].astype(np.int64)
    use = (idx >= 0) & (dist > 0.0) & np.isfinite(g) & ((anchor >= 0) & (anchor < len(xyz)))[:, None]
    use[:, 0] = False
    p, k = np.nonzero(use)
    m, a = idx[p, k].astype(np.int64), anchor[p]
    with np.errstate(over="ignore", invalid="ignore"):
        coef = (v[p] * g[p, k]) / dist[p, k]
        step = coef[:, None] * (xyz[m] - xyz[a])
    return m, a, step


def side_gradient(idx, dist, g, xyz, weights=None, dense=False):
    """One side of a native gradient call from the lists of the sensitivity call: (grad [N][3] float64, flag)."""
    xyz = np.asarray(xyz, dtype=np.float64)
    m, a, step = side_steps(idx, dist, g, xyz, weights, dense)
    total = [[0, 0, 0] for _ in range(len(xyz))]
    flag = 0
    for mi, ai, st in zip(m.tolist(), a.tolist(), step.tolist()):
        for c in range(3):
            t = quantize(st[c])
            if t is None:
                flag |= 1
                continue
            total[mi][c] += t
            total[ai][c] -= t  # (trunc is odd: trunc(-s / q) = -trunc(s / q))
    return np.asarray([[round_total(t) for t in row] for row in total], dtype=np.float64).reshape(len(xyz), 3), flag


def gradient(sens, xyz_a, xyz_b, weights=None, dense=False):
    """(grad_a, grad_b, flag) from a Sensitivity of NumPy arrays."""
    ga, fa = side_gradient(sens.idx_a, sens.dist_a, sens.g_a, xyz_a, weights, dense)
    gb, fb = side_gradient(sens.idx_b, sens.dist_b, sens.g_b, xyz_b, weights, dense)
    return ga, gb, fa | fb


def bits(a) -> np.ndarray:
    """float64 -> uint64 views: equality of bits (+0.0 and -0.0 differ, NaN payloads compare)."""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
