"""The GLM target's dispersion families on the host side (no GPU): the data block GLMTarget packs for "normal" and
"neg_binomial_2_log", its validation, and the numpy reference of tests/_glm_disp.py -- the device's algorithm -- against
mpmath at 40 digits, including the near-Poisson regime phi >> y + mu and the device digamma restated."""
import math

import numpy as np
import pytest

import _glm_disp as gd

from smcnuts_amd import GLMTarget, LinearRegression, NegativeBinomialRegression
from smcnuts_amd import _capi

U = gd.U
FAMILY_ID = {"normal": 2.0, "neg_binomial_2_log": 3.0}


@pytest.mark.parametrize("family", gd.DISP_FAMILIES)
@pytest.mark.parametrize("intercept", [True, False])
@pytest.mark.parametrize("per_coef", [False, True])
def test_packs_documented_layout(family, intercept, per_coef):
    n, p = 7, 3
    X, y = gd.synthetic(family, n, p, 0)
    Dc = p + intercept
    sd = np.linspace(0.5, 3.0, Dc) if per_coef else 1.7
    t = GLMTarget(X, y, family=family, prior_sd=sd, intercept=intercept, dispersion_prior=(0.3, 1.9))
    want = np.concatenate([[FAMILY_ID[family], n, p, 1.0 if intercept else 0.0],
                           np.broadcast_to(np.asarray(sd, dtype=np.float64), (Dc,)), [0.3, 1.9], y, X.reshape(-1)])
    assert t.model_id == _capi.MODEL_GLM == 4
    assert t.model_data.dtype == np.float64 and t.model_data.shape == (4 + Dc + 2 + n + n * p,)
    np.testing.assert_array_equal(t.model_data, want)
    assert t.dim == t.constrained_dim == Dc + 1
    names = (["Intercept"] if intercept else []) + [f"beta.{j + 1}" for j in range(p)]
    assert t.param_names() == names + ["sigma" if family == "normal" else "phi"]
    assert t.dispersion_prior == (0.3, 1.9)


def test_aliases_defaults_and_exports():
    import smcnuts_amd
    assert smcnuts_amd.LinearRegression is LinearRegression
    assert smcnuts_amd.NegativeBinomialRegression is NegativeBinomialRegression
    X, y = gd.synthetic("normal", 4, 2, 1)
    a = LinearRegression(X, y, prior_sd=1.0)
    assert a.family == "normal" and a.dim == 4 and a.param_names() == ["Intercept", "beta.1", "beta.2", "sigma"]
    assert a.dispersion_prior == (0.0, 2.5) and a.model_data[4 + 3] == 0.0 and a.model_data[4 + 3 + 1] == 2.5
    Xn, yn = gd.synthetic("neg_binomial_2_log", 4, 2, 1)
    b = NegativeBinomialRegression(Xn, yn, intercept=False, dispersion_prior=(1.0, 0.5))
    assert b.family == "neg_binomial_2_log" and b.dim == 3 and b.param_names() == ["beta.1", "beta.2", "phi"]
    np.testing.assert_array_equal(b.model_data[:8], [3.0, 4, 2, 0.0, 2.5, 2.5, 1.0, 0.5])
    # the families without a dispersion coordinate keep their block byte for byte
    c = GLMTarget(X, (y > 0).astype(float))
    assert c.model_data.shape == (4 + 3 + 4 + 8,) and c.dispersion_prior is None


@pytest.mark.parametrize("kw,match", [
    (dict(family="bernoulli_logit", y=[0, 1, 1], dispersion_prior=(0.0, 1.0)), "bernoulli_logit has no dispersion"),
    (dict(family="poisson_log", y=[0, 1, 1], dispersion_prior=(0.0, 1.0)), "poisson_log has no dispersion"),
    (dict(dispersion_prior=(np.nan, 1.0)), "m must be finite"),
    (dict(dispersion_prior=(0.0, 0.0)), "s must be finite and > 0"),
    (dict(dispersion_prior=(0.0, -1.0)), "s must be finite and > 0"),
    (dict(dispersion_prior=(0.0, np.inf)), "s must be finite and > 0"),
    (dict(dispersion_prior=1.0), r"pair \(m, s\)"),
    (dict(dispersion_prior=(1.0, 2.0, 3.0)), r"pair \(m, s\)"),
    (dict(y=[0.5, np.nan, 1.0]), "normal needs finite y"),
    (dict(y=[0.5, np.inf, 1.0]), "normal needs finite y"),
    (dict(family="neg_binomial_2_log", y=[0, -1, 3]), r"y in \{0, 1, 2, \.\.\., 2\^53\}"),
    (dict(family="neg_binomial_2_log", y=[0, 1.5, 3]), r"y in \{0, 1, 2, \.\.\., 2\^53\}"),
    (dict(family="neg_binomial_2_log", y=[0, 2.0 ** 54, 3]), r"y in \{0, 1, 2, \.\.\., 2\^53\}"),
    (dict(family="neg_binomial_2_log", y=[0, np.nan, 3]), r"y in \{0, 1, 2, \.\.\., 2\^53\}"),
    (dict(X_bad=np.nan), "X must be finite"),
    (dict(prior_sd=[1.0, 0.0, 2.0]), "prior_sd must be finite and > 0"),
    (dict(prior_sd=[1.0, 2.0, 3.0, 4.0]), r"prior_sd must be a scalar or one value per coefficient \(3\)"),
])
def test_rejects_bad_inputs(kw, match):
    X = np.array([[0.1, 0.2], [0.3, -0.4], [1.0, 2.0]])
    if "X_bad" in kw:
        X[1, 1] = kw.pop("X_bad")
    y = kw.pop("y", [0.5, -1.0, 2.0])
    kw.setdefault("family", "normal")
    with pytest.raises(ValueError, match=match):
        GLMTarget(X, y, **kw)


@pytest.mark.parametrize("family", gd.DISP_FAMILIES)
def test_rejects_too_many_coordinates(family):
    y = [0.0, 1.0, 2.0]
    assert GLMTarget(np.zeros((3, 63)), y, family=family, intercept=False).dim == 64
    assert GLMTarget(np.zeros((3, 62)), y, family=family).dim == 64
    with pytest.raises(ValueError, match=r"D = 65 coordinates \(64 coefficients and tau\).*D <= 64.*HostTarget"):
        GLMTarget(np.zeros((3, 63)), y, family=family)
    with pytest.raises(ValueError, match="no coefficients"):
        GLMTarget(np.zeros((3, 0)), y, family=family, intercept=False)
    assert GLMTarget(np.zeros((3, 2)), [2.0 ** 53, 0.0, 1.0], family=family).dim == 4   # the largest NB count


PHI_GRID = (1e-3, 0.5, 1.0, 7.3, 1e3, 1e6, 1e8)
Y_GRID = (0.0, 1.0, 2.0, 3.0, 10.0, 100.0, 1e4, 1e6)
ETA_GRID = (-30.0, -2.0, 0.0, 2.5, 30.0)


@pytest.mark.parametrize("phi", PHI_GRID)
def test_nb_reference_against_mpmath(phi):
    """term, d / d eta and d / d tau over the grid.  The term's error stays within 64 u of |y eta| + |y tau| + mu +
    lgamma(y + 1) + (y + phi) softplus(eta - tau) + y + 1 -- the Poisson term's own magnitudes, never lgamma(phi) or
    phi |tau| -- and the tau-gradient's within 64 u (y + mu + 1) (+ 64 u min(phi, 10) (1 + log1p y): the shifted
    series below phi = 10)."""
    tau = math.log(phi)
    yy, ee = np.meshgrid(np.array(Y_GRID), np.array(ETA_GRID), indexing="ij")
    term, d, gt, *_r = gd.nb_obs(yy, ee, tau)
    for i, y in enumerate(Y_GRID):
        for j, eta in enumerate(ETA_GRID):
            mt, md, mg = gd.mp_obs("neg_binomial_2_log", y, eta, tau)
            mu = math.exp(eta)
            sp = max(eta - tau, 0.0) + math.log1p(math.exp(-abs(eta - tau)))
            allowed = 64 * U * (abs(y * eta) + abs(y * tau) + mu + math.lgamma(y + 1) + (y + phi) * sp + y + 1)
            assert abs(term[i, j] - mt) <= allowed, (y, eta, phi, term[i, j], mt, allowed)
            sg = 1.0 / (1.0 + math.exp(-(eta - tau))) if eta - tau > -700 else 0.0
            assert abs(d[i, j] - md) <= 64 * U * (y + (y + phi) * sg + 1e-300), (y, eta, phi, d[i, j], md)
            allowed_g = 64 * U * (y + mu + 1 + min(phi, 10.0) * (1 + math.log1p(y)))
            assert abs(gt[i, j] - mg) <= allowed_g, (y, eta, phi, gt[i, j], mg, allowed_g)


def test_nb_near_poisson_plain_difference_is_not_enough():
    """At phi = 1e8, y = 3 the plain lgamma difference is off by ~1e-7; the reference (the device's algorithm) is not."""
    from scipy.special import gammaln
    phi, y, eta = 1e8, 3.0, 0.5
    mt, _, _ = gd.mp_obs("neg_binomial_2_log", y, eta, math.log(phi))
    term = gd.nb_obs(y, eta, math.log(phi))[0]
    L = math.log(math.exp(eta) + phi)
    plain = (gammaln(y + phi) - gammaln(phi) - math.lgamma(y + 1) + phi * (math.log(phi) - L) + y * (eta - L))
    assert abs(term - mt) <= 1e-14 * (1 + abs(mt))
    assert abs(plain - mt) > 1e-9


@pytest.mark.parametrize("tau", [-300.0, -100.0, -10.0, -1.0, 0.0, 0.7, 5.0, 20.0, 50.0])
def test_normal_reference_against_mpmath(tau):
    for y in (-1e3, -2.0, 0.0, 0.3, 1.0, 1e4):
        for eta in (-30.0, -2.0, 0.0, 2.5, 30.0):
            term, d, gt, m_term, m_d, m_gt, *_r = gd.normal_obs(y, eta, tau)
            mt, md, mg = gd.mp_obs("normal", y, eta, tau)
            assert abs(term - mt) <= 8 * U * m_term, (y, eta, tau, term, mt)
            assert abs(d - md) <= 8 * U * m_d + 1e-300, (y, eta, tau, d, md)
            assert abs(gt - mg) <= 8 * U * m_gt, (y, eta, tau, gt, mg)


def test_device_digamma_restated_against_mpmath():
    import mpmath as mp
    xs = np.concatenate([[1e-300, 1e-8, 1e-3, 0.1, 0.5, 1.0, 1.4616321449683622, 2.0, 3.7, 9.999, 10.0, 10.5, 55.0],
                         np.geomspace(1e-3, 1e12, 60)])
    got = gd.digamma(xs)
    lg, psi, xsh, P, S = gd.lgamma_digamma(xs)
    np.testing.assert_array_equal(psi, got)
    for x, g, l_, sh, p_, s_ in zip(xs, got, lg, xsh, P, S):
        with mp.workdps(40):
            ref = float(mp.digamma(mp.mpf(float(x))))
            lref = float(mp.loggamma(mp.mpf(float(x))))
        assert abs(g - ref) <= 8 * U * (abs(math.log(sh)) + s_ + 1.0), (x, g, ref)
        assert abs(l_ - lref) <= 8 * U * ((sh + 0.5) * abs(math.log(sh)) + sh + abs(math.log(p_)) + 1.0), (x, l_, lref)
    assert np.all(xsh >= 10.0) and np.all(xsh[xs >= 10.0] == xs[xs >= 10.0])


def test_non_finite_cases():
    X = np.array([[1.0], [2.0]])
    nb = gd.GLMDispNumpy(X, [0, 3], "neg_binomial_2_log", prior_sd=1.0, intercept=False)
    pts = np.array([[360.0, 0.0],          # eta = 720: e^eta overflows
                    [354.0, 0.0],          # eta = 708: finite
                    [0.0, 709.9],          # e^tau overflows
                    [0.0, 709.7],          # finite
                    [0.0, -708.5],         # e^tau below the normal range
                    [0.0, -708.3]])        # finite
    lpri, llik, _, _ = nb.parts(pts)
    assert np.all(np.isfinite(lpri))
    np.testing.assert_array_equal(np.isfinite(llik), [False, True, False, True, False, True])
    assert np.all(llik[[0, 2, 4]] == -np.inf)
    assert np.all(nb.logpdfgrad(pts[[0, 2, 4]], 1.0) == -np.inf)
    nm = gd.GLMDispNumpy(X, [0.5, -1.0], "normal", prior_sd=1.0, intercept=False)
    lpri, llik, _, glik = nm.parts(np.array([[0.1, -355.0], [0.1, -354.0], [0.1, -300.0], [0.1, 800.0]]))
    np.testing.assert_array_equal(np.isfinite(llik), [False, True, True, True])
    assert np.all(np.isfinite(glik[1:]))
    mt = math.fsum(gd.mp_obs("normal", yv, 0.1 * xv, -300.0)[0] for yv, xv in ((0.5, 1.0), (-1.0, 2.0)))
    assert abs(llik[2] - mt) <= 1e-15 * abs(mt)


@pytest.mark.parametrize("family", gd.DISP_FAMILIES)
def test_numpy_model_parts_and_constrain(family):
    X, y = gd.synthetic(family, 30, 3, 5)
    m = gd.GLMDispNumpy(X, y, family, prior_sd=np.array([0.7, 1.0, 1.5, 2.0]), dispersion_prior=(0.4, 1.3))
    rng = np.random.default_rng(3)
    for x in rng.standard_normal((3, 5)) * 0.5:
        lpri, llik, gpri, glik = gd.exact_parts(m, x)
        ref = math.fsum(gd.mp_obs(family, yi, float(np.dot(m.Z[i], x[:4])), x[4])[0] for i, yi in enumerate(y))
        assert abs(llik[0] - ref) <= 1e-12 * (1 + abs(ref))
        g = [math.fsum(gd.mp_obs(family, yi, float(np.dot(m.Z[i], x[:4])), x[4])[2] for i, yi in enumerate(y))]
        np.testing.assert_allclose(glik[0, -1], g[0], rtol=1e-11, atol=1e-11)
        lp = math.fsum([-0.5 * ((xc - mc) / s) ** 2 - math.log(s) - gd.HALF_LOG_2PI for xc, mc, s in zip(x, m.m, m.s)])
        assert abs(lpri[0] - lp) <= 1e-14 * (1 + abs(lp))
        np.testing.assert_allclose(gpri[0], -(x - m.m) / m.s ** 2, rtol=1e-15)
        np.testing.assert_allclose(m.logpdf(x, 0.3), lpri[0] + 0.3 * llik[0], rtol=1e-13)
        np.testing.assert_allclose(m.logpdfgrad(x, 0.3), gpri[0] + 0.3 * glik[0], rtol=1e-12, atol=1e-13)
        # the gradient against central differences of the density
        h = 1e-6
        fd = [(m.logpdf(x + h * e) - m.logpdf(x - h * e)) / (2 * h) for e in np.eye(5)]
        np.testing.assert_allclose(m.logpdfgrad(x), fd, rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(m.constrain(x), np.concatenate([x[:4], [math.exp(x[4])]]), rtol=1e-15)
