"""HierarchicalGLM (SMCN_MODEL_HGLM) on the CPU: input validation, the data block it packs, and the numpy reference
density of tests/_hglm.py against mpmath at 40 digits -- every family, an empty group, Dc = 0, lt near both ends."""
import math

import numpy as np
import pytest

import _hglm as hg

U = hg.U


def _model(family, n, p, J, seed, intercept=True, empty=(), **kw):
    X, y, g = hg.synthetic(family, n, p, J, seed, empty=empty)
    sd = np.linspace(0.8, 2.5, p + intercept) if p + intercept else 1.0
    prior = (0.2, 1.5)
    m = hg.HGLMNumpy(X, y, g, family, sd, 1.3, prior, intercept, n_groups=J)
    return X, y, g, sd, prior, m


def test_packing_and_names():
    from smcnuts_amd import HierarchicalGLM, _capi
    X = np.arange(12.0).reshape(4, 3) / 10.0
    y = np.array([0.0, 2.0, 1.0, 5.0])
    g = [2, 0, 2, 1]
    t = HierarchicalGLM(X, y, g, family="poisson_log", prior_sd=[1.0, 2.0, 3.0, 4.0], group_sd_prior=0.5)
    assert t.model_id == _capi.MODEL_HGLM == 5
    assert t.dim == t.constrained_dim == 4 + 3 + 1
    assert t.param_names() == ["Intercept", "beta.1", "beta.2", "beta.3", "alpha.1", "alpha.2", "alpha.3", "tau"]
    want = np.concatenate([[1, 4, 3, 1, 3], [1.0, 2.0, 3.0, 4.0], [0.5], y, [2, 0, 2, 1], X.reshape(-1)])
    np.testing.assert_array_equal(t.model_data, want)
    # dispersion family, no intercept, n_groups beyond the largest index, numpy integer groups
    t = HierarchicalGLM(X, [0.1, -2.0, 3.0, 0.0], np.array([0, 0, 1, 1], dtype=np.int32), family="normal",
                        prior_sd=2.0, group_sd_prior=1.5, intercept=False, dispersion_prior=(0.3, 0.7), n_groups=4)
    assert t.dim == 3 + 4 + 2
    assert t.param_names() == ["beta.1", "beta.2", "beta.3", "alpha.1", "alpha.2", "alpha.3", "alpha.4", "tau", "sigma"]
    want = np.concatenate([[2, 4, 3, 0, 4], [2.0, 2.0, 2.0], [1.5], [0.3, 0.7], [0.1, -2.0, 3.0, 0.0], [0, 0, 1, 1],
                           X.reshape(-1)])
    np.testing.assert_array_equal(t.model_data, want)
    # the group intercepts alone (Dc = 0); NB names its dispersion phi; the default dispersion prior
    t = HierarchicalGLM(np.zeros((3, 0)), [1, 0, 4], [0, 1, 1], family="neg_binomial_2_log", intercept=False)
    assert t.dim == 0 + 2 + 2
    assert t.param_names() == ["alpha.1", "alpha.2", "tau", "phi"]
    np.testing.assert_array_equal(t.model_data[:9], [3, 3, 0, 0, 2, 1.0, 0.0, 2.5, 1.0])
    # D = 64 exactly
    t = HierarchicalGLM(np.zeros((3, 1)), [0, 1, 0], [0, 1, 60])
    assert t.dim == 64


def test_validation():
    from smcnuts_amd import HierarchicalGLM
    X = np.zeros((4, 2))
    y = np.array([0.0, 1.0, 1.0, 0.0])
    g = [0, 1, 1, 0]
    cases = [
        (dict(family="logit"), "family must be one of"),
        (dict(dispersion_prior=(0, 1)), "has no dispersion parameter"),
        (dict(family="normal", dispersion_prior=3.0), "dispersion_prior must be a pair"),
        (dict(family="normal", dispersion_prior=(np.inf, 1.0)), "dispersion_prior's m must be finite"),
        (dict(family="neg_binomial_2_log", dispersion_prior=(0.0, 0.0)), "dispersion_prior's s must be finite and > 0"),
        (dict(group_sd_prior=0.0), "group_sd_prior must be finite and > 0"),
        (dict(group_sd_prior=np.nan), "group_sd_prior must be finite and > 0"),
        (dict(group_sd_prior="wide"), "group_sd_prior must be a number"),
        (dict(X=np.zeros((2, 2, 2))), "X must be an (n, p) matrix"),
        (dict(X=np.zeros((0, 2)), y=[], g=[]), "at least one observation"),
        (dict(y=[0.0, 1.0, 1.0]), "y must be a vector of the n = 4"),
        (dict(g=[0, 1, 1]), "groups must be a vector of the n = 4"),
        (dict(g=[0, 1.5, 1, 0]), "groups must be integers"),
        (dict(g=[0, np.nan, 1, 0]), "groups must be integers"),
        (dict(g=["a", "b", "a", "b"]), "groups must be integers"),
        (dict(g=[True, False, True, False]), "groups must be integers"),
        (dict(g=[0, -1, 1, 0]), "groups must be >= 0"),
        (dict(n_groups=0), "n_groups must be an integer >= 1"),
        (dict(n_groups=2.0), "n_groups must be an integer >= 1"),
        (dict(g=[0, 1, 2, 0], n_groups=2), "groups must be in 0..n_groups - 1 = 1"),
        (dict(g=[0, 1, 62, 0]), "the device functor covers D <= 64"),
        (dict(g=[0, 1, 59, 0], family="normal"), "the device functor covers D <= 64"),
        (dict(X=np.array([[0, 1], [np.inf, 0], [0, 0], [1, 1]])), "X must be finite"),
        (dict(y=[0.0, 2.0, 1.0, 0.0]), "bernoulli_logit needs y in {0, 1}"),
        (dict(family="poisson_log", y=[0.0, 1.5, 1.0, 0.0]), "poisson_log needs y in {0, 1, 2, ...}"),
        (dict(family="normal", y=[0.0, np.nan, 1.0, 0.0]), "normal needs finite y"),
        (dict(family="neg_binomial_2_log", y=[0.0, -1.0, 1.0, 0.0]), "neg_binomial_2_log needs y in"),
        (dict(prior_sd=[1.0, 2.0]), "prior_sd must be a scalar or one value per coefficient (3)"),
        (dict(prior_sd=-1.0), "prior_sd must be finite and > 0"),
    ]
    for kw, msg in cases:
        a = dict(X=X, y=y, g=g)
        for k in ("X", "y", "g"):
            if k in kw:
                a[k] = kw.pop(k)
        with pytest.raises(ValueError) as ei:
            HierarchicalGLM(a["X"], a["y"], a["g"], **kw)
        assert msg in str(ei.value), (str(ei.value), msg)


POINTS = ("benign", "lt_high", "lt_low")


def _point(m, rng, kind):
    x = rng.standard_normal(m.dim) * 0.5
    if kind == "lt_high":                 # tau = e^300 (e^2lt just below overflow is 354.9): z tiny, alpha O(1)
        x[m.lt] = 300.0
        x[m.Dc:m.lt] *= math.exp(-300.0)
    elif kind == "lt_low":                # tau = e^-700: the group intercepts vanish
        x[m.lt] = -700.0
    return x


@pytest.mark.parametrize("family", hg.FAMILIES)
@pytest.mark.parametrize("shape", [(40, 3, 5, True, ()), (25, 0, 4, False, (2,)), (30, 2, 6, True, (0, 5))])
@pytest.mark.parametrize("kind", POINTS)
def test_reference_against_mpmath(family, shape, kind):
    """lpri, llik and both gradients of HGLMNumpy against 40-digit mpmath, within tests/_hglm.device_bounds (which
    the device is held to against the fsum reference): Dc = 0 and empty groups among the shapes."""
    n, p, J, ic, empty = shape
    *_, m = _model(family, n, p, J, 31 * n + J, intercept=ic, empty=empty)
    assert m.Dc == p + ic
    x = _point(m, np.random.default_rng(n + J + len(family)), kind)
    lp_mp, ll_mp, gp_mp, gl_mp = hg.mp_parts(m, x)
    lpri, llik, gpri, glik = hg.exact_parts(m, x[None, :])
    b_lpri, b_llik, b_glik = hg.device_bounds(m, x[None, :])
    assert np.isfinite(lp_mp) and np.isfinite(ll_mp)
    assert abs(lpri[0] - lp_mp) <= b_lpri[0], (lpri[0], lp_mp, b_lpri[0])
    assert abs(llik[0] - ll_mp) <= b_llik[0], (llik[0], ll_mp, b_llik[0])
    # (d / d lt = 1 - e^2lt / s_tau^2 cancels: its error is relative to e^2lt / s_tau^2)
    b_gpri = 8 * U * (np.abs(gp_mp) + 1.0 + math.exp(min(2.0 * x[m.lt], 700.0)) / m.s_tau ** 2)
    assert np.all(np.abs(gpri[0] - gp_mp) <= b_gpri), (gpri[0] - gp_mp, b_gpri)
    assert np.all(np.abs(glik[0] - gl_mp) <= b_glik[0] + 1e-300), (glik[0] - gl_mp, b_glik[0])
    for c in empty:                       # an empty group: its z has the prior only
        assert glik[0, m.Dc + c] == 0.0
    # logpdf / logpdfgrad are the parts put together
    for phi in (0.0, 0.4, 1.0):
        close = abs(m.logpdf(x, phi) - (lp_mp + phi * ll_mp)) <= b_lpri[0] + b_llik[0] + 4 * U * (abs(lp_mp) + abs(ll_mp))
        assert close
        gw = gp_mp + phi * gl_mp
        assert np.all(np.abs(m.logpdfgrad(x, phi) - gw) <= b_gpri + phi * b_glik[0] + 4 * U * np.abs(gw) + 1e-300)


def test_overflow_is_minus_inf():
    """e^(2 lt) overflows: lpri and llik -inf, so logpdf and every gradient entry; the dispersion families' own
    out-of-range rules still apply."""
    *_, m = _model("bernoulli_logit", 20, 2, 3, 5)
    x = np.zeros((2, m.dim))
    x[0, m.lt] = 355.0
    x[1, m.lt] = 800.0
    lpri, llik, _, _ = m.parts(x)
    assert np.all(lpri == -np.inf) and np.all(llik == -np.inf)
    assert np.all(m.logpdf(x) == -np.inf) and np.all(m.logpdfgrad(x) == -np.inf)
    x[:, m.lt] = 354.0
    assert np.all(np.isfinite(m.parts(x)[0]))
    *_, m = _model("neg_binomial_2_log", 20, 2, 3, 5)
    x = np.zeros((1, m.dim))
    x[0, -1] = 720.0
    assert m.logpdf(x)[0] == -np.inf and np.isfinite(m.parts(x)[0][0])


@pytest.mark.parametrize("family", hg.FAMILIES)
def test_permuting_observations(family):
    """Observations permuted together with their groups (and groups relabelled with z): the density changes only by
    rounding."""
    X, y, g, sd, prior, m = _model(family, 300, 3, 7, 11)
    rng = np.random.default_rng(3)
    x = rng.standard_normal((5, m.dim)) * 0.5
    perm = rng.permutation(len(y))
    m2 = hg.HGLMNumpy(X[perm], y[perm], g[perm], family, sd, 1.3, prior, True, n_groups=7)
    relabel = rng.permutation(7)                      # group j becomes relabel[j]
    m3 = hg.HGLMNumpy(X[perm], y[perm], relabel[g[perm]], family, sd, 1.3, prior, True, n_groups=7)
    x3 = x.copy()
    x3[:, m.Dc + relabel] = x[:, m.Dc:m.lt]
    lp = m.logpdf(x)
    _, b_llik, _ = hg.device_bounds(m, x)
    for mm, xx in ((m2, x), (m3, x3)):
        assert np.all(np.abs(mm.logpdf(xx) - lp) <= 2 * b_llik + 1e-12 * np.abs(lp))
    g1, g3 = m.logpdfgrad(x), m3.logpdfgrad(x3)
    g3b = g3.copy()
    g3b[:, m.Dc:m.lt] = g3[:, m.Dc + relabel]
    np.testing.assert_allclose(g3b, g1, rtol=1e-9, atol=1e-9 * np.abs(g1).max())
