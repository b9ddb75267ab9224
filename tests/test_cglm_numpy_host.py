"""tests/_cglm.py's NumPy model against mpmath (no GPU): the reference the device tests compare with stays inside the
bound they allow the device (_cglm.device_bounds), on the whole grid tests/test_gpu_cglm.py uses (both families, D in
{2, 8, 9, 33, 64} x n in {1, 63, 64, 65, 130}, with and without the intercept) and at its extreme points, and
its gradients are the derivatives of the mpmath value."""
import math

import numpy as np
import pytest

import _cglm as cg

import mpmath as mp

D_LIST = (2, 8, 9, 33, 64)
N_LIST = (1, 63, 64, 65, 130)


def model_for(family, D, n, intercept, seed, df=4.0):
    p = D - 1 - intercept
    X, y = cg.synthetic(family, n, p, seed, df=df)
    sd = np.linspace(0.8, 2.5, p + intercept)
    return X, y, sd, cg.ContGLMNumpy(X, y, family, sd, (0.2, 1.5), intercept, df=df)


@pytest.mark.parametrize("family", cg.FAMILIES)
@pytest.mark.parametrize("D", D_LIST)
@pytest.mark.parametrize("n", N_LIST)
def test_numpy_model_within_device_bounds_of_mpmath(family, D, n):
    """The whole grid of tests/test_gpu_cglm.py -- both families, every (D, n), with and without the intercept, the same
    data sets -- at four points each: an ordinary tau, a shape above kGammaAsym, a small scale, and tau = -3."""
    for intercept in (True, False):
        _, _, _, m = model_for(family, D, n, intercept, 1000 * D + n + len(family))
        assert m.dim == D
        rng = np.random.default_rng(D + n + intercept)
        x = rng.standard_normal((4, D)) * 0.5
        x[1, -1], x[2, -1], x[3, -1] = 3.0, -2.0, -3.0
        lpri, llik, gpri, glik = m.parts(x)
        _, el, _, eg = cg.exact_parts(m, x)
        _, b_llik, b_glik = cg.device_bounds(m, x)
        for k in range(x.shape[0]):
            ll, g = cg.mp_parts(m, x[k])
            assert abs(llik[k] - ll) <= b_llik[k], (k, llik[k] - ll, b_llik[k])
            assert abs(el[k] - ll) <= b_llik[k]
            assert np.all(np.abs(glik[k] - g) <= b_glik[k]), (k, np.abs(glik[k] - g) / b_glik[k])
            assert np.all(np.abs(eg[k] - g) <= b_glik[k])
        # the bound is a rounding bound, not a loose one
        assert np.all(b_llik <= 1e-9 * (1.0 + np.abs(llik)))


def _one_obs(family, y, eta, tau, df=4.0):
    """The NumPy terms of one observation and their bounds (an intercept-only model with b_0 = eta)."""
    m = cg.ContGLMNumpy(np.zeros((1, 0)), [y], family, 2.5, (0.0, 2.5), True, df=df)
    x = np.array([[eta, tau]])
    _, llik, _, glik = m.parts(x)
    _, b_llik, b_glik = cg.device_bounds(m, x)
    return llik[0], glik[0], b_llik[0], b_glik[0]


EXTREME = [("gamma_log", 2.5, 0.3, 30.0, 4.0), ("gamma_log", 2.5, 0.3, -30.0, 4.0), ("gamma_log", 1e-300, -700.0, 0.5, 4.0),
           ("gamma_log", 1e300, 700.0, 0.5, 4.0), ("gamma_log", 1e-300, 700.0, 0.5, 4.0), ("gamma_log", 1e300, -700.0, 0.5, 4.0),
           ("gamma_log", 0.7, 0.1, math.log(10.0), 4.0), ("gamma_log", 0.7, 0.1, math.log(9.999), 4.0)] + \
          [("student_t", yv, 0.4, tau, df) for df in (0.5, 1.0, 4.0, 1e6) for yv, tau in ((1e200, 0.3), (1.7, 30.0), (1.7, -30.0),
                                                                                       (1e200, -200.0), (-3e149, -1.0))]


@pytest.mark.parametrize("family,y,eta,tau,df", EXTREME)
def test_extreme_points_against_mpmath(family, y, eta, tau, df):
    llik, glik, b_llik, b_glik = _one_obs(family, y, eta, tau, df)
    t, d, gt = cg.mp_obs(family, y, eta, tau, df)
    if not math.isfinite(t):
        assert llik == -np.inf and t == -np.inf
        return
    assert math.isfinite(llik) and abs(llik - t) <= b_llik, (llik - t, b_llik)
    assert np.all(np.isfinite(glik))
    assert abs(glik[0] - d) <= b_glik[0] and abs(glik[1] - gt) <= b_glik[1], (glik, d, gt, b_glik)
    assert b_llik <= 1e-10 * (1.0 + abs(t))           # (a rounding bound, not a loose one)


@pytest.mark.parametrize("family", cg.FAMILIES)
def test_out_of_range_tau_is_minus_infinity_with_numbers_for_gradients(family):
    X, y, sd, m = model_for(family, 4, 20, True, 5)
    x = np.zeros((4, 4))
    x[:, -1] = (720.0, -720.0, 700.0, -700.0)            # e^+-720 is outside the normal range, e^+-700 inside
    lpri, llik, _, glik = m.parts(x)
    assert (llik == -np.inf).tolist() == [True, True, False, False]
    assert np.all(np.isfinite(llik[2:]))
    assert np.all(np.isfinite(glik[:2]))
    lp, g = m.logpdf(x), m.logpdfgrad(x)
    assert np.all(lp[:2] == -np.inf) and np.all(g[:2] == -np.inf)


@pytest.mark.parametrize("family", cg.FAMILIES)
def test_gradients_are_central_differences_of_the_mpmath_value(family):
    _, _, _, m = model_for(family, 5, 30, True, 77)
    x = np.random.default_rng(3).standard_normal(5) * 0.4
    _, _, _, glik = m.parts(x)
    h = 1e-6
    with mp.workdps(50):
        for c in range(5):
            e = np.zeros(5)
            e[c] = 1.0
            # (x +- h e in float64 is exact enough: the mp sum takes the perturbed doubles as they are)
            xp, xm = x + h * e, x - h * e
            fd = (mp.mpf(cg.mp_parts(m, xp, dps=50)[0]) - mp.mpf(cg.mp_parts(m, xm, dps=50)[0])) / mp.mpf(xp[c] - xm[c])
            # float(llik) rounds each side to 2^-53 |llik|: the quotient is good to ~1e-16 |llik| / 2e-6, and the
            # truncation is h^2 / 6 of a third derivative of the size of n
            ll = abs(cg.mp_parts(m, x)[0])
            assert abs(float(fd) - glik[0, c]) <= 1e-7 * (1.0 + ll + abs(glik[0, c])), (c, float(fd), glik[0, c])


def test_student_constant_both_branches_against_mpmath():
    for df in (1e-3, 0.5, 1.0, 4.0, 19.9, 20.0, 33.0, 1e6, 1e12):
        f = cg.df_const(df)
        with mp.workdps(40):
            d = mp.mpf(df)
            C = float(mp.loggamma((d + 1) / 2) - mp.loggamma(d / 2) - mp.log(d * mp.pi) / 2)
        assert abs(f["c"] - C) <= 64 * cg.U * f["mc"], (df, f["c"] - C)
