"""OrdinalRegression (SMCN_MODEL_ORDINAL) on the CPU: the data block it packs, input validation, and the numpy reference
density of tests/_ord.py against mpmath -- benign points, |eta| near 800, cutpoints at +-800, gaps of e^-700 between
cutpoints, the end classes -- the mpmath gradient against mpmath central differences, K = 2 against logistic regression,
and constrain()."""
import math

import numpy as np
import pytest

import _glm as gl
import _ord as od

U = od.U


def test_packing_and_names():
    from smcnuts_amd import OrdinalRegression, _capi
    X = np.arange(8.0).reshape(4, 2) / 10.0
    y = np.array([0, 3, 1, 3])
    t = OrdinalRegression(X, y, prior_sd=[1.0, 2.0], cutpoint_prior_sd=[3.0, 4.0, 5.0])
    assert t.model_id == _capi.MODEL_ORDINAL == 7
    assert t.n_classes == 4
    assert t.dim == t.constrained_dim == 2 + 3
    assert t.param_names() == ["beta.1", "beta.2", "cutpoint.1", "cutpoint.2", "cutpoint.3"]
    want = np.concatenate([[4, 4, 2], [1.0, 2.0], [3.0, 4.0, 5.0], [0, 3, 1, 3], X.reshape(-1)])
    np.testing.assert_array_equal(t.model_data, want)
    # no columns, an empty class beyond the largest label, float labels, the default priors
    t = OrdinalRegression(np.zeros((3, 0)), [0.0, 1.0, 1.0], n_classes=5)
    assert t.dim == 4 and t.param_names() == ["cutpoint.1", "cutpoint.2", "cutpoint.3", "cutpoint.4"]
    np.testing.assert_array_equal(t.model_data, [5, 3, 0, 5.0, 5.0, 5.0, 5.0, 0, 1, 1])
    t = OrdinalRegression(np.ones(3), [1, 0, 1], prior_sd=0.5)
    np.testing.assert_array_equal(t.model_data, [2, 3, 1, 0.5, 5.0, 1, 0, 1, 1, 1, 1])
    # the limits exactly: D = 64 with p = 0 (K = 65) and with K = 2 (p = 63)
    assert OrdinalRegression(np.zeros((3, 0)), [0, 64, 1]).dim == 64
    assert OrdinalRegression(np.zeros((3, 63)), [0, 1, 1]).dim == 64


def test_validation():
    from smcnuts_amd import OrdinalRegression
    X = np.zeros((4, 2))
    y = [0, 1, 2, 1]
    cases = [
        (dict(X=np.zeros((2, 2, 2))), "X must be an (n, p) matrix"),
        (dict(X=np.zeros((0, 2)), y=[]), "at least one observation"),
        (dict(y=[0, 1, 1]), "y must be a vector of the n = 4"),
        (dict(y=[0, 1.5, 1, 0]), "the labels y must be integers"),
        (dict(y=[0, np.nan, 1, 0]), "the labels y must be integers"),
        (dict(y=["a", "b", "a", "b"]), "the labels y must be integers"),
        (dict(y=[True, False, True, False]), "the labels y must be integers"),
        (dict(y=[0, -1, 1, 0]), "the labels y must be >= 0"),
        (dict(y=[0, 0, 0, 0]), "K = n_classes must be >= 2"),
        (dict(n_classes=1, y=[0, 0, 0, 0]), "K = n_classes must be >= 2"),
        (dict(n_classes=3.0), "n_classes must be an integer"),
        (dict(n_classes=2), "the labels y must be in 0..n_classes - 1 = 1"),
        (dict(X=np.zeros((4, 63))), "D = p + K - 1 = 63 + 2 = 65 coordinates; the device functor covers D <= 64"),
        (dict(X=np.zeros((4, 0)), y=[0, 65, 1, 0]), "D = p + K - 1 = 0 + 65 = 65"),
        (dict(X=np.array([[0, 1], [np.inf, 0], [0, 0], [1, 1]])), "X must be finite"),
        (dict(prior_sd=0.0), "prior_sd must be finite and > 0"),
        (dict(prior_sd=[1.0, np.nan]), "prior_sd must be finite and > 0"),
        (dict(prior_sd=[1.0, 2.0, 3.0]), "prior_sd must be a scalar or one value per column (2)"),
        (dict(cutpoint_prior_sd=-1.0), "cutpoint_prior_sd must be finite and > 0"),
        (dict(cutpoint_prior_sd=[1.0, np.inf]), "cutpoint_prior_sd must be finite and > 0"),
        (dict(cutpoint_prior_sd=[1.0, 2.0, 3.0]), "cutpoint_prior_sd must be a scalar or one value per cutpoint (K - 1 = 2)"),
    ]
    for kw, msg in cases:
        kw = dict(kw)
        args = (kw.pop("X", X), kw.pop("y", y))
        with pytest.raises(ValueError) as ei:
            OrdinalRegression(*args, **kw)
        assert msg in str(ei.value), (str(ei.value), msg)


@pytest.mark.parametrize("K,p", [(2, 3), (3, 0), (4, 2), (6, 5)])
def test_reference_against_mpmath(K, p):
    """The numpy reference (fsum) within the device's worst-case bound of the mpmath value, at benign points, |eta| near
    800, cutpoints at +-800, gaps of e^-700 (collapsed middle classes) and spread cutpoints; every class observed."""
    X, y = od.synthetic(K, 23, p, 10 * K + p)
    y[:K] = np.arange(K)                                  # (both end classes and every middle class)
    m = od.OrdinalNumpy(X, y, n_classes=K, prior_sd=np.linspace(0.7, 2.0, p), cutpoint_prior_sd=np.linspace(2, 6, K - 1))
    pts = od.points(m, np.random.default_rng(K + p))
    lpri, llik, gpri, glik = od.exact_parts(m, pts)
    b_lpri, b_llik, b_gpri, b_glik = od.device_bounds(m, pts)
    for i, x in enumerate(pts):
        mp_lpri, mp_llik, mp_gp, mp_gl = od.mp_parts(m, x)
        assert np.isfinite(lpri[i]) and np.isfinite(llik[i]), i     # (every finite x here: a finite density)
        assert abs(lpri[i] - mp_lpri) <= b_lpri[i], (i, lpri[i] - mp_lpri, b_lpri[i])
        assert abs(llik[i] - mp_llik) <= b_llik[i], (i, llik[i] - mp_llik, b_llik[i])
        assert np.all(np.abs(gpri[i] - mp_gp) <= b_gpri[i]), (i, gpri[i] - mp_gp, b_gpri[i])
        assert np.all(np.abs(glik[i] - mp_gl) <= b_glik[i]), (i, glik[i] - mp_gl, b_glik[i])


def test_log_domain_form_and_gradient_against_mpmath():
    """The log-domain form equals log(sigma(eta - c_k) - sigma(eta - c_{k+1})) at 80 digits, for every class; the analytic
    gradient (suffix-sum chain, Jacobian, count term) equals mpmath central differences of the density."""
    import mpmath as mp
    X, y = od.synthetic(4, 9, 2, 5)
    y[:4] = np.arange(4)
    m = od.OrdinalNumpy(X, y, prior_sd=[1.5, 0.8], cutpoint_prior_sd=[2.0, 3.0, 4.0])
    x = np.array([0.4, -0.7, -0.9, 0.1, -0.5])
    with mp.workdps(80):
        b, u, c, eta = od._mp_setup(m, x, mp)
        for i in range(len(y)):
            k, e = int(y[i]), eta[i]
            hi = mp.mpf(1) if k == 0 else 1 / (1 + mp.exp(-(e - c[k - 1])))
            lo = mp.mpf(0) if k == m.K - 1 else 1 / (1 + mp.exp(-(e - c[k])))
            assert abs(mp.log(hi - lo) - od._mp_logp(k, m.K, e, c, u, mp)) < mp.mpf(10) ** -70
    _, _, gp, gl_ = od.mp_parts(m, x)
    h = 1e-20
    for phi, want in ((0.0, gp), (1.0, gp + gl_)):
        with mp.workdps(60):
            for j in range(m.dim):
                xp = [mp.mpf(float(v)) for v in x]
                xm = list(xp)
                xp[j] += h
                xm[j] -= h
                fd = (od.mp_logpdf(m, xp, phi) - od.mp_logpdf(m, xm, phi)) / (2 * h)
                assert abs(float(fd) - want[j]) <= 1e-14 * (abs(want[j]) + 1.0), (phi, j, float(fd), want[j])


def test_two_classes_are_logistic_regression():
    """K = 2: the ordinal density at (b, u_1) is logistic regression's with intercept -c_1 = -u_1, value and gradient."""
    rng = np.random.default_rng(3)
    X, y = od.synthetic(2, 40, 4, 5)
    m = od.OrdinalNumpy(X, y, prior_sd=1.7, cutpoint_prior_sd=2.3)
    g = gl.GLMNumpy(X, y.astype(np.float64), "bernoulli_logit", prior_sd=np.array([2.3] + [1.7] * 4))
    assert m.dim == g.dim == 5
    pts = np.vstack([rng.standard_normal((4, 5)), rng.standard_normal((2, 5)) * 200.0])
    gpts = np.concatenate([-pts[:, 4:], pts[:, :4]], axis=1)
    a = od.exact_parts(m, pts)
    b = gl.exact_parts(g, gpts)
    ba, bb = od.device_bounds(m, pts), gl.device_bounds(g, gpts)
    assert np.all(np.abs(a[0] - b[0]) <= ba[0] + bb[0])
    assert np.all(np.abs(a[1] - b[1]) <= ba[1] + bb[1])
    np.testing.assert_array_equal(a[2][:, :4], b[2][:, 1:])
    np.testing.assert_array_equal(a[2][:, 4], -b[2][:, 0])
    assert np.all(np.abs(a[3][:, :4] - b[3][:, 1:]) <= ba[3][:, :4] + bb[2][:, 1:])
    assert np.all(np.abs(a[3][:, 4] + b[3][:, 0]) <= ba[3][:, 4] + bb[2][:, 0])


def test_non_finite_rules():
    """-inf (lpri and llik) once e^u overflows or a cutpoint is not finite; llik = -inf once X b overflows; collapsed
    middle cutpoints (e^u = 0) give a finite value."""
    X = np.array([[1e300], [0.5], [-1.0], [0.2]])
    m = od.OrdinalNumpy(X, [0, 1, 2, 1], n_classes=3)
    for u2 in (710.0, np.inf):
        lpri, llik, _, _ = m.parts(np.array([0.0, 0.0, u2]))
        assert lpri[0] == -np.inf and llik[0] == -np.inf
        assert m.logpdf(np.array([0.0, 0.0, u2])) == -np.inf
    m4 = od.OrdinalNumpy(np.zeros((4, 0)), [0, 1, 2, 3])
    lpri, llik, _, _ = m4.parts(np.array([1.0, 709.7, 709.7]))            # c_3 = 2 e^709.7 overflows
    assert lpri[0] == -np.inf and llik[0] == -np.inf
    lpri, llik, _, _ = m.parts(np.array([1e10, 0.0, 0.0]))                 # eta_0 = 1e310
    assert np.isfinite(lpri[0]) and llik[0] == -np.inf
    assert m.logpdf(np.array([1e10, 0.0, 0.0])) == -np.inf
    for u2 in (-700.0, -800.0, -1e300):
        lpri, llik, gpri, glik = m.parts(np.array([1e-3, 0.2, u2]))
        assert np.isfinite(lpri[0]) and np.isfinite(llik[0]), u2
        assert np.all(np.isfinite(gpri)) and np.all(np.isfinite(glik))
        L, R = od.log1mexp_e(u2)
        assert L == u2 and R == 1.0


def test_constrain_and_names():
    X, y = od.synthetic(6, 30, 3, 2)
    m = od.OrdinalNumpy(X, y, n_classes=6)
    x = np.random.default_rng(0).standard_normal((50, m.dim)) * 3.0
    c = m.constrain(x)
    np.testing.assert_array_equal(c[:, :3], x[:, :3])
    assert np.all(np.diff(c[:, 3:], axis=1) > 0.0)
    np.testing.assert_array_equal(c[:, 3], x[:, 3])
    assert np.all(np.abs((c[:, 4:] - c[:, 3:-1]) - np.exp(x[:, 4:])) <= 4 * U * (np.abs(c[:, 4:]) + np.abs(c[:, 3:-1])))
    np.testing.assert_array_equal(m.constrain(x[0]), c[0])
    assert m.param_names() == ["beta.1", "beta.2", "beta.3"] + [f"cutpoint.{k}" for k in range(1, 6)]
    assert math.isfinite(m.logpdf(x[0]))
