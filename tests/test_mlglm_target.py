"""MultilevelGLM (SMCN_MODEL_MLGLM) on the CPU: input validation, the data block it packs against a restatement of the
layout, names, and the numpy reference density of tests/_mlglm.py against mpmath at 40 digits, against central
differences and -- with one term and z = 1 -- against tests/_hglm.py's HGLMNumpy."""
import math

import numpy as np
import pytest

import _hglm as hg
import _mlglm as ml

U = ml.U
DISP = ("normal", "neg_binomial_2_log")


def layout_block(family, X, y, terms, s, s_tau, intercept, disp_prior=None):
    """The data block of include/smcnuts_hip.h's SMCN_MODEL_MLGLM, restated: terms = [(g, z, J)]"""
    n, p = X.shape
    R = len(terms)
    out = [float(ml.FAMILIES.index(family)), float(n), float(p), float(int(intercept)), float(R)]
    out += [float(terms[r][2]) if r < R else 0.0 for r in range(4)]
    out += [float(v) for v in s] + [float(v) for v in s_tau]
    if disp_prior is not None:
        out += [float(disp_prior[0]), float(disp_prior[1])]
    out += [float(v) for v in y]
    for g, z, _ in terms:
        out += [float(v) for v in g] + [float(v) for v in z]
    for i in range(n):
        out += [float(v) for v in X[i]]
    return np.array(out, dtype=np.float64)


def test_packing_and_names():
    from smcnuts_amd import MultilevelGLM, _capi
    X = np.arange(12.0).reshape(4, 3) / 10.0
    y = np.array([0.0, 2.0, 1.0, 5.0])
    g = np.array([2, 0, 2, 1])
    days = np.array([0.5, -1.0, 2.0, 0.25])
    # (1 + days || subject): two terms on one factor
    t = MultilevelGLM(X, y, [(g,), (g, days)], family="poisson_log", prior_sd=[1.0, 2.0, 3.0, 4.0],
                      group_sd_prior=[0.5, 0.25])
    assert t.model_id == _capi.MODEL_MLGLM == 8
    assert t.dim == t.constrained_dim == 4 + 3 + 3 + 2
    assert t.n_groups == (3, 3)
    assert t.param_names() == ["Intercept", "beta.1", "beta.2", "beta.3", "alpha.1.1", "alpha.1.2", "alpha.1.3",
                               "alpha.2.1", "alpha.2.2", "alpha.2.3", "tau.1", "tau.2"]
    want = layout_block("poisson_log", X, y, [(g, np.ones(4), 3), (g, days, 3)], [1, 2, 3, 4], [0.5, 0.25], True)
    assert t.model_data.tobytes() == want.tobytes()
    np.testing.assert_array_equal(t.model_data[:9], [1, 4, 3, 1, 2, 3, 3, 0, 0])
    # crossed factors, dispersion, no intercept, n_groups beyond the largest index, z = None, a scalar group_sd_prior
    item = np.array([0, 0, 1, 1], dtype=np.int32)
    t = MultilevelGLM(X, [0.1, -2.0, 3.0, 0.0], [(g, None, 5), (item, None), (item, days, 4)], family="normal",
                      prior_sd=2.0, group_sd_prior=1.5, intercept=False, dispersion_prior=(0.3, 0.7))
    assert t.dim == 3 + (5 + 2 + 4) + 3 + 1
    assert t.param_names()[3:] == [f"alpha.1.{j}" for j in range(1, 6)] + ["alpha.2.1", "alpha.2.2"] \
        + [f"alpha.3.{j}" for j in range(1, 5)] + ["tau.1", "tau.2", "tau.3", "sigma"]
    want = layout_block("normal", X, [0.1, -2.0, 3.0, 0.0], [(g, np.ones(4), 5), (item, np.ones(4), 2), (item, days, 4)],
                        [2.0] * 3, [1.5] * 3, False, (0.3, 0.7))
    assert t.model_data.tobytes() == want.tobytes()
    # the varying terms alone (Dc = 0); NB names its dispersion phi; the default dispersion prior; four terms
    t = MultilevelGLM(np.zeros((3, 0)), [1, 0, 4], [([0, 1, 1],)] * 4, family="neg_binomial_2_log", intercept=False)
    assert t.dim == 0 + 8 + 4 + 1
    assert t.param_names()[-6:] == ["alpha.4.2", "tau.1", "tau.2", "tau.3", "tau.4", "phi"]
    np.testing.assert_array_equal(t.model_data[:15], [3, 3, 0, 0, 4, 2, 2, 2, 2, 1.0, 1.0, 1.0, 1.0, 0.0, 2.5])
    # D = 64 exactly
    t = MultilevelGLM(np.zeros((3, 1)), [0, 1, 0], [([0, 1, 29],), ([0, 1, 29],)])
    assert t.dim == 64


def test_validation():
    from smcnuts_amd import MultilevelGLM
    X = np.zeros((4, 2))
    y = np.array([0.0, 1.0, 1.0, 0.0])
    g = [0, 1, 1, 0]
    z = [0.5, 1.0, -1.0, 2.0]
    cases = [
        (dict(family="logit"), "family must be one of"),
        (dict(dispersion_prior=(0, 1)), "has no dispersion parameter"),
        (dict(family="normal", dispersion_prior=3.0), "dispersion_prior must be a pair"),
        (dict(family="normal", dispersion_prior=(np.inf, 1.0)), "dispersion_prior's m must be finite"),
        (dict(family="neg_binomial_2_log", dispersion_prior=(0.0, 0.0)), "dispersion_prior's s must be finite and > 0"),
        (dict(terms=3), "terms must be a sequence of"),
        (dict(terms=[]), "terms must hold 1 to 4 varying terms, not 0"),
        (dict(terms=[(g,)] * 5), "terms must hold 1 to 4 varying terms, not 5"),
        (dict(terms=[(g, z, 2, 1)]), "every term must be (groups,), (groups, z) or (groups, z, n_groups)"),
        (dict(terms=[()]), "every term must be (groups,), (groups, z) or (groups, z, n_groups)"),
        (dict(group_sd_prior="wide"), "group_sd_prior must be a number or one per term"),
        (dict(group_sd_prior=[1.0, 2.0]), "group_sd_prior must be a scalar or one value per term (1)"),
        (dict(group_sd_prior=0.0), "group_sd_prior must be finite and > 0"),
        (dict(terms=[(g,), (g, z)], group_sd_prior=[1.0, np.nan]), "group_sd_prior must be finite and > 0"),
        (dict(X=np.zeros((2, 2, 2))), "X must be an (n, p) matrix"),
        (dict(X=np.zeros((0, 2)), y=[], terms=[([],)]), "at least one observation"),
        (dict(y=[0.0, 1.0, 1.0]), "y must be a vector of the n = 4"),
        (dict(terms=[([0, 1, 1],)]), "term 1: groups must be a vector of the n = 4"),
        (dict(terms=[(g,), ([0, 1.5, 1, 0],)]), "term 2: groups must be integers"),
        (dict(terms=[([0, np.nan, 1, 0],)]), "term 1: groups must be integers"),
        (dict(terms=[(["a", "b", "a", "b"],)]), "term 1: groups must be integers"),
        (dict(terms=[([True, False, True, False],)]), "term 1: groups must be integers"),
        (dict(terms=[([0, -1, 1, 0],)]), "term 1: groups must be >= 0"),
        (dict(terms=[(g, ["a", "b", "c", "d"])]), "term 1: z must be numbers"),
        (dict(terms=[(g, [1.0, 2.0])]), "term 1: z must be a vector of the n = 4"),
        (dict(terms=[(g,), (g, [1.0, np.inf, 0.0, 0.0])]), "term 2: z must be finite"),
        (dict(terms=[(g, None, 0)]), "term 1: n_groups must be an integer >= 1"),
        (dict(terms=[(g, None, 2.0)]), "term 1: n_groups must be an integer >= 1"),
        (dict(terms=[([0, 1, 2, 0], None, 2)]), "term 1: groups must be in 0..n_groups - 1 = 1"),
        (dict(terms=[([0, 1, 29, 0],), ([0, 1, 29, 0],)]), "the device functor covers D <= 64"),
        (dict(terms=[(g, None, 60)], family="normal"), "the device functor covers D <= 64"),
        (dict(X=np.array([[0, 1], [np.inf, 0], [0, 0], [1, 1]])), "X must be finite"),
        (dict(y=[0.0, 2.0, 1.0, 0.0]), "bernoulli_logit needs y in {0, 1}"),
        (dict(family="poisson_log", y=[0.0, 1.5, 1.0, 0.0]), "poisson_log needs y in {0, 1, 2, ...}"),
        (dict(family="normal", y=[0.0, np.nan, 1.0, 0.0]), "normal needs finite y"),
        (dict(family="neg_binomial_2_log", y=[0.0, -1.0, 1.0, 0.0]), "neg_binomial_2_log needs y in"),
        (dict(prior_sd=[1.0, 2.0]), "prior_sd must be a scalar or one value per coefficient (3)"),
        (dict(prior_sd=-1.0), "prior_sd must be finite and > 0"),
    ]
    for kw, msg in cases:
        a = dict(X=X, y=y, terms=[(g, z)])
        for k in ("X", "y", "terms"):
            if k in kw:
                a[k] = kw.pop(k)
        with pytest.raises(ValueError) as ei:
            MultilevelGLM(a["X"], a["y"], a["terms"], **kw)
        assert str(ei.value).startswith("MultilevelGLM: "), str(ei.value)
        assert msg in str(ei.value), (str(ei.value), msg)


def test_unsupported_criteria_and_prediction_refuse():
    """No PredictMixin and no pointwise partials: the target and the sampler refuse as for every unsupported target."""
    from smcnuts_amd import MultilevelGLM, SMCSampler
    X = np.zeros((6, 1))
    t = MultilevelGLM(X, [0, 1, 1, 0, 1, 0], [(np.arange(6) % 3,)])
    x = np.zeros((2, t.dim))
    for call in (lambda: t.pointwise_loglik(x), lambda: t.pointwise(x), lambda: t.pointwise(x, np.zeros(2)),
                 lambda: t.loo(x), lambda: t.loo(x, np.zeros(2))):
        with pytest.raises(NotImplementedError, match="GLMTarget"):
            call()
    assert not hasattr(t, "predict") and not hasattr(t, "predict_draws") and not hasattr(t, "predict_partials")
    assert getattr(t, "_ctx", None) is None
    smc = SMCSampler.__new__(SMCSampler)
    smc.lkernel, smc.target = "forwardsLKernel", t
    for call in (smc.pointwise, smc.loo, lambda: smc.predict(X), lambda: smc.predict_draws(X), smc.predict_draws):
        with pytest.raises(NotImplementedError, match="MultilevelGLM.*GLMTarget"):
            call()


# (Dc, [(J, factor)], intercept, empty, zero): a slope beside an intercept on one factor; crossed factors with Dc = 0
SHAPES = [(40, 3, [(5, 0), (5, 0)], True, (0, 4), None), (25, 0, [(4, 0), (3, 1)], False, (1, 2), None),
          (30, 2, [(1, 0), (6, 1), (2, 2), (6, 1)], True, (1, 0), 3)]


def _model(family, shape, seed):
    n, p, terms, ic, empty, zero = shape
    X, y, tm = ml.synthetic(family, n, p, terms, seed, intercept=ic, empty=empty, zero=zero)
    sd = np.linspace(0.8, 2.5, p + ic) if p + ic else 1.0
    st = np.linspace(1.3, 0.6, len(terms))
    return ml.MLGLMNumpy(X, y, tm, family, sd, st, (0.2, 1.5), ic)


def _point(m, rng, kind, r=0):
    x = rng.standard_normal(m.dim) * 0.5
    if kind == "lt_high":                 # tau_r = e^300 (e^2lt just below overflow is 354.9): u tiny, the effects O(1)
        x[m.lt0 + r] = 300.0
        x[m.u_slice(r)] *= math.exp(-300.0)
    elif kind == "lt_low":                # tau_r = e^-700: the term vanishes
        x[m.lt0 + r] = -700.0
    return x


@pytest.mark.parametrize("family", ml.FAMILIES)
@pytest.mark.parametrize("shape", range(len(SHAPES)))
@pytest.mark.parametrize("kind", ("benign", "lt_high", "lt_low"))
def test_reference_against_mpmath(family, shape, kind):
    """lpri, llik and both gradients of MLGLMNumpy against 40-digit mpmath, within _mlglm.device_bounds (which the
    device is held to against the fsum reference); the extreme lt on the last term."""
    m = _model(family, SHAPES[shape], 31 * shape + 7)
    r = m.R - 1
    x = _point(m, np.random.default_rng(shape + len(family)), kind, r)
    lp_mp, ll_mp, gp_mp, gl_mp = ml.mp_parts(m, x)
    lpri, llik, gpri, glik = ml.exact_parts(m, x[None, :])
    b_lpri, b_llik, b_glik = ml.device_bounds(m, x[None, :])
    assert np.isfinite(lp_mp) and np.isfinite(ll_mp)
    assert abs(lpri[0] - lp_mp) <= b_lpri[0], (lpri[0], lp_mp, b_lpri[0])
    assert abs(llik[0] - ll_mp) <= b_llik[0], (llik[0], ll_mp, b_llik[0])
    # (d / d lt_r = 1 - e^2lt / s_tau^2 cancels: its error is relative to e^2lt / s_tau^2)
    b_gpri = 8 * U * (np.abs(gp_mp) + 1.0)
    for q in range(m.R):
        b_gpri[m.lt0 + q] += 8 * U * math.exp(min(2.0 * x[m.lt0 + q], 700.0)) / m.s_tau[q] ** 2
    assert np.all(np.abs(gpri[0] - gp_mp) <= b_gpri), (gpri[0] - gp_mp, b_gpri)
    assert np.all(np.abs(glik[0] - gl_mp) <= b_glik[0] + 1e-300), (glik[0] - gl_mp, b_glik[0])
    n, p, terms, ic, empty, zero = SHAPES[shape]
    for q, (J, f) in enumerate(terms):    # a level without observations, a term with z = 0: the prior only
        if f == terms[empty[0]][1]:
            assert glik[0, m.off[q] + empty[1]] == 0.0
    if zero is not None:
        assert np.all(glik[0, m.u_slice(zero)] == 0.0) and glik[0, m.lt0 + zero] == 0.0
    for phi in (0.0, 0.4, 1.0):           # logpdf / logpdfgrad are the parts put together
        assert abs(m.logpdf(x, phi) - (lp_mp + phi * ll_mp)) <= b_lpri[0] + b_llik[0] + 4 * U * (abs(lp_mp) + abs(ll_mp))
        gw = gp_mp + phi * gl_mp
        assert np.all(np.abs(m.logpdfgrad(x, phi) - gw) <= b_gpri + phi * b_glik[0] + 4 * U * np.abs(gw) + 1e-300)


@pytest.mark.parametrize("family", ml.FAMILIES)
@pytest.mark.parametrize("kind", ("benign", "lt_low"))
def test_gradient_against_central_differences(family, kind):
    """logpdfgrad against central differences of logpdf with h = 1e-5: truncation h^2 |f'''| / 6 and rounding
    u |f| / h, both far below 1e-5 (1 + |g|) at these points (|f| < 1e4)."""
    m = _model(family, SHAPES[2], 5)
    x = _point(m, np.random.default_rng(len(family)), kind, 1)
    g = m.logpdfgrad(x, 0.7)
    h = 1e-5
    for c in range(m.dim):
        e = np.zeros(m.dim)
        e[c] = h
        fd = (m.logpdf(x + e, 0.7) - m.logpdf(x - e, 0.7)) / (2 * h)
        assert abs(fd - g[c]) <= 1e-5 * (1.0 + abs(g[c])), (c, fd, g[c])


@pytest.mark.parametrize("family", ml.FAMILIES)
def test_one_intercept_term_is_the_hierarchical_model(family):
    """R = 1, z = 1: the same operations in the same order as HGLMNumpy -- equal, not close."""
    X, y, g = hg.synthetic(family, 120, 3, 6, 17, empty=(4,))
    sd = np.linspace(0.8, 2.5, 4)
    h = hg.HGLMNumpy(X, y, g, family, sd, 1.3, (0.2, 1.5), True, n_groups=6)
    m = ml.MLGLMNumpy(X, y, [(g, None, 6)], family, sd, 1.3, (0.2, 1.5), True)
    assert m.dim == h.dim and m.lt0 == h.lt
    rng = np.random.default_rng(2)
    x = rng.standard_normal((6, h.dim)) * 0.5
    x[4, h.lt] = 300.0
    x[4, h.Dc:h.lt] *= math.exp(-300.0)
    x[5, h.lt] = 355.0
    for a, b in zip(h.parts(x), m.parts(x)):
        np.testing.assert_array_equal(a, b)
    for phi in (0.0, 0.3, 1.0):
        np.testing.assert_array_equal(h.logpdf(x, phi), m.logpdf(x, phi))
        np.testing.assert_array_equal(h.logpdfgrad(x, phi), m.logpdfgrad(x, phi))
    np.testing.assert_array_equal(h.constrain(x[:4]), m.constrain(x[:4]))
    for a, b in zip(hg.exact_parts(h, x), ml.exact_parts(m, x)):
        np.testing.assert_array_equal(a, b)


def test_overflow_is_minus_inf():
    """Any e^(2 lt_r) overflows: lpri and llik -inf, so logpdf and every gradient entry."""
    m = _model("bernoulli_logit", SHAPES[2], 5)
    for r in range(m.R):
        x = np.zeros((2, m.dim))
        x[0, m.lt0 + r] = 355.0
        x[1, m.lt0 + r] = 800.0
        lpri, llik, _, _ = m.parts(x)
        assert np.all(lpri == -np.inf) and np.all(llik == -np.inf)
        assert np.all(m.logpdf(x) == -np.inf) and np.all(m.logpdfgrad(x) == -np.inf)
        x[:, m.lt0 + r] = 354.0
        assert np.all(np.isfinite(m.parts(x)[0]))
