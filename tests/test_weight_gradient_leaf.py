"""The host leaf of the weight-function gradient, lchd_wf_cdf_grad (cdf_param_grad of lchd_math.h), without a GPU: against central
differences of lchd_wf_cdf in every parameter, its conventions at 0, at +inf and on and outside the support bounds, and the Euler
identity of hyper_exp."""
import numpy as np
import pytest

import loco_hd_amd as lh
from loco_hd_amd import _native as N

FAMILIES = {"uniform": [3.0, 10.0], "hyper_exp": [1.0, 0.5, 0.2, 0.05], "dagum": [4.0, 6.0, 1.5], "kumaraswamy": [2.0, 11.0, 2.0, 3.0]}
KINDS = {"hyper_exp": 0, "dagum": 1, "uniform": 2, "kumaraswamy": 3}
INF = float("inf")


def _grad(family, params, x):
    p, x = np.asarray(params, dtype=np.float64), np.asarray(x, dtype=np.float64)
    out = np.empty((len(x), len(p)))
    N.check(N.lib().lchd_wf_cdf_grad(KINDS[family], N.dp(p), len(p), N.dp(x), len(x), N.dp(out)))
    return out


def _cdf(family, params, x):
    p, out = np.asarray(params, dtype=np.float64), np.empty(len(x))
    N.check(N.lib().lchd_wf_cdf(KINDS[family], N.dp(p), len(p), N.dp(x), len(x), N.dp(out)))
    return out


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_wf_cdf_grad_against_central_differences_of_wf_cdf(family):
    """h = 1e-5 theta_k: truncation h^2 / 6 * |d^3F/dtheta^3| + rounding 2.2e-16 / (2 h); theta_k >= 0.05 gives 2.2e-10 for the latter
    (the pattern and the points of test_wf_pdf_against_central_differences_of_wf_cdf: away from the support bounds)."""
    params = FAMILIES[family]
    x = np.linspace(3.2, 9.8, 34)
    got = _grad(family, params, x)
    worst = 0.0
    for k, theta in enumerate(params):
        h = 1e-5 * theta
        up, dn = list(params), list(params)
        up[k], dn[k] = theta + h, theta - h
        fd = (_cdf(family, up, x) - _cdf(family, dn, x)) / (up[k] - dn[k])
        err = float(np.max(np.abs(got[:, k] - fd)))
        worst = max(worst, err)
        print(f"{family}, parameter {k}: max |grad - central difference| = {err:.3g}")
    assert worst <= 5e-10
    w = lh.WeightFunction(family, params)
    assert np.array_equal(w.cdf_param_grad_vec(x), got) and w.cdf_param_grad_vec(x).shape == (34, len(params))


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_zero_at_infinity_and_finite_everywhere(family):
    x = np.concatenate([[0.0, INF, 1e-300, 1e300], np.linspace(0.0, 20.0, 81), FAMILIES[family][:2]])
    got = _grad(family, FAMILIES[family], x)
    assert np.isfinite(got).all()
    assert np.all(got[1] == 0.0)


def test_conventions_of_uniform():
    got = _grad("uniform", [3.0, 10.0], [0.0, 2.999, 3.0, 6.5, 10.0, 10.001, INF])
    assert np.all(got[[0, 1, 5, 6]] == 0.0)  # outside the support
    assert np.array_equal(got[2], [-1.0 / 7.0, -0.0]) and np.array_equal(got[4], [0.0, -1.0 / 7.0])  # on the bounds: the inside branch
    assert np.array_equal(got[3], [(6.5 - 10.0) / 49.0, -(6.5 - 3.0) / 49.0])
    assert np.array_equal(_grad("uniform", [0.0, 10.0], [0.0])[0], [-0.1, -0.0])  # x = 0: the formula's value


def test_conventions_of_dagum_and_hyper_exp_at_zero():
    assert np.all(_grad("dagum", FAMILIES["dagum"], [0.0]) == 0.0)
    assert np.all(_grad("dagum", [0.0, 0.0, 0.0], [0.0, 1.0, INF])[[0, 2]] == 0.0)
    assert np.isfinite(_grad("dagum", [0.0, 0.0, 0.0], [0.0, 1.0, 5.0])).all()  # (parameters lchd_wf_validate accepts)
    assert np.all(_grad("hyper_exp", FAMILIES["hyper_exp"], [0.0]) == 0.0)  # (1 - F(0)) - 1 = 0 and a x e = 0


def test_conventions_of_kumaraswamy():
    steep = [2.0, 11.0, 0.5, 0.5]  # alpha < 1: dF/dz is infinite at z = 0; beta < 1: at z = 1
    got = _grad("kumaraswamy", steep, [1.9, 2.0, 6.0, 11.0, 11.1])
    assert np.isfinite(got).all()
    assert np.all(got[[0, 4]] == 0.0)  # outside the support
    assert np.all(got[1] == 0.0)       # z = 0: the bounds' limit is infinite (0 by convention), z^a ln z = 0, ln(1 - 0) = 0
    assert np.all(got[3] == 0.0)       # z = 1: likewise, and 0 * ln 0 = 0
    assert np.all(got[2] != 0.0)
    smooth = _grad("kumaraswamy", FAMILIES["kumaraswamy"], [2.0, 11.0])
    assert np.all(smooth == 0.0)       # alpha = 2, beta = 3: every derivative vanishes on both bounds


def test_euler_identity_of_hyper_exp():
    """F depends on the a_i through their ratios alone: sum_i a_i dF/da_i = 0 to rounding (terms of size <= 1 / N)."""
    for params in (FAMILIES["hyper_exp"], [3.0, 0.25, 1.5, 2.0, 0.01, 0.7]):
        n = len(params) // 2
        got = _grad("hyper_exp", params, np.linspace(0.0, 30.0, 61))
        worst = float(np.max(np.abs((got[:, :n] * np.asarray(params[:n])).sum(1))))
        print(f"max |sum_i a_i dF/da_i| = {worst:.3g}")
        assert worst <= 1e-15 and np.any(np.abs(got) > 1e-3)


def test_arguments():
    with pytest.raises(ValueError):
        _grad("uniform", [3.0, 10.0], [-1.0])
    with pytest.raises(ValueError):
        _grad("uniform", [10.0, 3.0], [1.0])
    assert lh.WeightFunction("uniform", [3.0, 10.0]).cdf_param_grad_vec([]).shape == (0, 2)
