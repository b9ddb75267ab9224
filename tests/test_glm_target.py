"""The GLM target's host side (no GPU): the data block GLMTarget packs for SMCN_MODEL_GLM, its validation, and the
numpy reference density of tests/_glm.py against mpmath at 40 digits."""
import math

import numpy as np
import pytest

import _glm

from smcnuts_amd import GLMTarget, LogisticRegression, PoissonRegression
from smcnuts_amd import _capi


def _xy(n=5, p=3, family="bernoulli_logit", seed=0):
    return _glm.synthetic(family, n, p, seed)


@pytest.mark.parametrize("family", ["bernoulli_logit", "poisson_log"])
@pytest.mark.parametrize("intercept", [True, False])
@pytest.mark.parametrize("per_coef", [False, True])
def test_packs_documented_layout(family, intercept, per_coef):
    n, p = 7, 3
    X, y = _xy(n, p, family)
    D = p + intercept
    sd = np.linspace(0.5, 3.0, D) if per_coef else 1.7
    t = GLMTarget(X, y, family=family, prior_sd=sd, intercept=intercept)
    want = np.concatenate([[0.0 if family == "bernoulli_logit" else 1.0, n, p, 1.0 if intercept else 0.0],
                           np.broadcast_to(np.asarray(sd, dtype=np.float64), (D,)), y, X.reshape(-1)])
    assert t.model_id == _capi.MODEL_GLM == 4
    assert t.model_data.dtype == np.float64 and t.model_data.shape == (4 + D + n + n * p,)
    np.testing.assert_array_equal(t.model_data, want)
    assert t.dim == t.constrained_dim == D
    names = (["Intercept"] if intercept else []) + [f"beta.{j + 1}" for j in range(p)]
    assert t.param_names() == names


def test_aliases_and_param_names():
    X, y = _xy(4, 2)
    a = LogisticRegression(X, y, prior_sd=1.0)
    assert a.family == "bernoulli_logit" and a.dim == 3 and a.param_names() == ["Intercept", "beta.1", "beta.2"]
    Xp, yp = _xy(4, 2, "poisson_log")
    b = PoissonRegression(Xp, yp, intercept=False)
    assert b.family == "poisson_log" and b.dim == 2 and b.param_names() == ["beta.1", "beta.2"]
    c = GLMTarget(np.arange(3.0), [0, 1, 1])                  # a 1-D X is one covariate
    assert c.dim == 2 and c.model_data[2] == 1.0


@pytest.mark.parametrize("kw,match", [
    (dict(y=[0, 2, 1]), r"y in \{0, 1\}"),
    (dict(y=[0, 0.5, 1]), r"y in \{0, 1\}"),
    (dict(family="poisson_log", y=[0, -1, 3]), r"y in \{0, 1, 2"),
    (dict(family="poisson_log", y=[0, 1.5, 3]), r"y in \{0, 1, 2"),
    (dict(family="poisson_log", y=[0, np.nan, 3]), r"y in \{0, 1, 2"),
    (dict(X_bad=np.nan), "X must be finite"),
    (dict(X_bad=np.inf), "X must be finite"),
    (dict(prior_sd=0.0), "prior_sd must be finite and > 0"),
    (dict(prior_sd=-1.0), "prior_sd must be finite and > 0"),
    (dict(prior_sd=[1.0, 0.0, 2.0]), "prior_sd must be finite and > 0"),
    (dict(prior_sd=[1.0, 2.0]), "prior_sd must be a scalar or one value per coefficient"),
    (dict(y=[0, 1]), "y must be a vector"),
    (dict(family="probit"), "family must be one of"),
])
def test_rejects_bad_inputs(kw, match):
    X = np.array([[0.1, 0.2], [0.3, -0.4], [1.0, 2.0]])
    if "X_bad" in kw:
        X[1, 1] = kw.pop("X_bad")
    y = kw.pop("y", [0, 1, 1])
    with pytest.raises(ValueError, match=match):
        GLMTarget(X, y, **kw)


def test_rejects_too_many_coefficients():
    X = np.zeros((3, 64))
    assert GLMTarget(X, [0, 1, 0], intercept=False).dim == 64
    with pytest.raises(ValueError, match="D <= 64.*HostTarget"):
        GLMTarget(X, [0, 1, 0])                               # 64 columns + intercept = 65
    with pytest.raises(ValueError, match="no coefficients"):
        GLMTarget(np.zeros((3, 0)), [0, 1, 0], intercept=False)
    with pytest.raises(ValueError, match="at least one observation"):
        GLMTarget(np.zeros((0, 2)), [])
    with pytest.raises(ValueError, match=r"\(n, p\) matrix"):
        GLMTarget(np.zeros((2, 2, 2)), [0, 1])


def _cases():
    for family in ("bernoulli_logit", "poisson_log"):
        for n, p, seed in ((1, 1, 1), (9, 3, 2), (40, 6, 3)):
            yield family, n, p, seed


@pytest.mark.parametrize("family,n,p,seed", list(_cases()))
def test_numpy_reference_against_mpmath(family, n, p, seed):
    X, y = _glm.synthetic(family, n, p, seed)
    m = _glm.GLMNumpy(X, y, family=family, prior_sd=np.linspace(0.7, 2.0, p + 1))
    rng = np.random.default_rng(seed)
    for x in rng.standard_normal((3, p + 1)):
        lpri, llik, gpri, glik = _glm.exact_parts(m, x)
        ref = _glm.mp_llik(m, x)
        # the float64 terms and fsum: within a few ulp of each term's magnitude of the 40-digit value
        _, term, _ = m.terms(np.atleast_2d(x))
        assert abs(llik[0] - ref) <= 8 * _glm.U * (np.sum(np.abs(term)) + 1.0) * (p + 2), (llik[0], ref)
        g = _glm.mp_grad(m, x)
        np.testing.assert_allclose(glik[0], g, rtol=1e-13, atol=1e-13 * (1 + np.abs(g).max()))
        lp_mp = math.fsum([-0.5 * (xc / s) ** 2 - math.log(s) - 0.5 * math.log(2 * math.pi) for xc, s in zip(x, m.s)])
        assert abs(lpri[0] - lp_mp) <= 1e-14 * (1 + abs(lp_mp))
        # logpdf = lpri + phi llik; logpdfgrad = gpri + phi glik
        np.testing.assert_allclose(m.logpdf(x, 0.3), lpri[0] + 0.3 * llik[0], rtol=1e-13)
        np.testing.assert_allclose(m.logpdfgrad(x, 0.3), gpri[0] + 0.3 * glik[0], rtol=1e-12, atol=1e-13)


def test_numpy_reference_extreme_eta():
    """Logistic at eta = +-800 (softplus without overflow, residual exactly 0 or -1) and Poisson past exp's range."""
    X = np.array([[1.0], [-1.0], [1.0], [-1.0]])
    m = _glm.GLMNumpy(X, [1, 1, 0, 0], "bernoulli_logit", prior_sd=1.0, intercept=False)
    x = np.array([800.0])
    eta, term, d = m.terms(np.atleast_2d(x))
    np.testing.assert_array_equal(eta[0], [800.0, -800.0, 800.0, -800.0])
    np.testing.assert_array_equal(term[0], [0.0, -800.0, -800.0, 0.0])
    np.testing.assert_array_equal(d[0], [0.0, 1.0, -1.0, 0.0])
    assert _glm.mp_llik(m, x) == -1600.0
    assert m.parts(x)[1][0] == -1600.0
    p = _glm.GLMNumpy(np.array([[1.0], [2.0]]), [0, 3], "poisson_log", prior_sd=1.0, intercept=False)
    lpri, llik, _, _ = p.parts(np.array([355.0]))            # eta = 710: exp overflows
    assert llik[0] == -np.inf and np.isfinite(lpri[0])
    assert _glm.mp_llik(p, np.array([355.0])) == -np.inf
    assert p.logpdf(np.array([355.0]), 0.3) == -np.inf
    assert np.all(p.logpdfgrad(np.array([355.0]), 1.0) == -np.inf)
    ok = p.parts(np.array([354.0]))[1][0]                      # eta = 708: finite
    assert np.isfinite(ok)
    np.testing.assert_allclose(ok, _glm.mp_llik(p, np.array([354.0])), rtol=1e-15)
