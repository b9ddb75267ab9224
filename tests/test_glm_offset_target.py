"""GLMTarget with offsets and weights, host side (no GPU): the SMCN_MODEL_OGLM block it packs, its argument checks,
the new-row blocks, the scope refusals, and the numpy reference of tests/_glm_ow.py against identities and mpmath."""
import math

import numpy as np
import pytest

import _glm_ow

from smcnuts_amd import GLMTarget, LinearRegression, LogisticRegression, NegativeBinomialRegression, PoissonRegression
from smcnuts_amd import _capi

FAMILIES = _glm_ow.FAMILIES


def _data(family, n=9, p=3, seed=0, flags=3):
    return _glm_ow.synthetic(family, n, p, seed, scale=0.5, flags=flags)


def _kw(family):
    return dict(dispersion_prior=(0.3, 1.5)) if family in ("normal", "neg_binomial_2_log") else {}


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("flags", [1, 2, 3])
@pytest.mark.parametrize("intercept", [True, False])
def test_packs_documented_layout(family, flags, intercept):
    n, p = 7, 3
    X, y, o, w = _data(family, n, p, flags=flags)
    Dc = p + intercept
    disp = family in ("normal", "neg_binomial_2_log")
    sd = np.linspace(0.5, 3.0, Dc)
    t = GLMTarget(X, y, family=family, prior_sd=sd, intercept=intercept, offset=o, weights=w, **_kw(family))
    assert t.model_id == _capi.MODEL_OGLM == 10
    assert (t.offset is None) == (o is None) and (t.weights is None) == (w is None)
    want = np.concatenate([[FAMILIES.index(family), n, p, 1.0 if intercept else 0.0, flags], sd,
                           [0.3, 1.5] if disp else [], y, o if flags & 1 else [], w if flags & 2 else [], X.reshape(-1)])
    assert t.model_data.dtype == np.float64
    assert t.model_data.shape == (5 + Dc + 2 * disp + n * (1 + (flags & 1) + (flags >> 1)) + n * p,)
    np.testing.assert_array_equal(t.model_data, want)
    np.testing.assert_array_equal(t.model_data, _glm_ow.block(X, y, family, sd, intercept, (0.3, 1.5), o, w))
    assert t.dim == t.constrained_dim == Dc + disp
    assert GLMTarget.model_id == _capi.MODEL_GLM            # (the class keeps SMCN_MODEL_GLM's id)


@pytest.mark.parametrize("family", FAMILIES)
def test_without_either_the_object_is_unchanged(family):
    X, y, _, _ = _data(family)
    a = GLMTarget(X, y, family=family, prior_sd=1.3, **_kw(family))
    b = GLMTarget(X, y, family=family, prior_sd=1.3, offset=None, weights=None, **_kw(family))
    assert a.model_id == b.model_id == _capi.MODEL_GLM
    assert a.model_data.tobytes() == b.model_data.tobytes()
    assert b.offset is None and b.weights is None


def test_aliases_and_exposure():
    X, y, o, w = _data("poisson_log")
    e = np.exp(o)
    a = PoissonRegression(X, y, exposure=e, weights=w)
    assert a.model_id == _capi.MODEL_OGLM and a.family == "poisson_log"
    np.testing.assert_array_equal(a.offset, np.log(e))
    np.testing.assert_array_equal(a.weights, w)
    b = NegativeBinomialRegression(X, y, exposure=e)
    np.testing.assert_array_equal(b.offset, np.log(e))
    assert b.weights is None and b.model_data[4] == 1.0 and b.family == "neg_binomial_2_log"
    assert PoissonRegression(X, y, offset=o).model_data[4] == 1.0
    yb = (y > 0).astype(float)
    c = LogisticRegression(X, yb, weights=w)
    assert c.model_data[4] == 2.0 and c.offset is None
    d = LinearRegression(X, y - 1.5, offset=o, weights=w)
    assert d.model_data[4] == 3.0 and d.family == "normal"
    assert PoissonRegression(X, y).model_id == _capi.MODEL_GLM
    for bad in (np.where(np.arange(len(y)) == 2, 0.0, e), np.where(np.arange(len(y)) == 2, np.inf, e), -e,
                np.where(np.arange(len(y)) == 2, np.nan, e)):
        with pytest.raises(ValueError, match="exposure must be finite and > 0"):
            PoissonRegression(X, y, exposure=bad)
    with pytest.raises(ValueError, match="give offset or exposure, not both"):
        PoissonRegression(X, y, offset=o, exposure=e)
    with pytest.raises(ValueError, match="give offset or exposure, not both"):
        NegativeBinomialRegression(X, y, offset=o, exposure=e)
    with pytest.raises(ValueError, match="offset must be a vector of the n = 9 observations' offsets"):
        PoissonRegression(X, y, exposure=e[:-1])
    with pytest.raises(ValueError, match="exposure must be a vector"):
        PoissonRegression(X, y, exposure=e.reshape(-1, 1))
    with pytest.raises(TypeError):
        LogisticRegression(X, yb, exposure=e)              # (no exposure for a Bernoulli outcome)


def test_argument_checks():
    X, y, o, w = _data("bernoulli_logit")
    n = len(y)
    with pytest.raises(ValueError, match="GLMTarget: weights must be finite and >= 0"):
        GLMTarget(X, y, weights=np.where(np.arange(n) == 1, -0.5, 1.0))
    for v in (np.nan, np.inf):
        with pytest.raises(ValueError, match="GLMTarget: weights must be finite and >= 0"):
            GLMTarget(X, y, weights=np.where(np.arange(n) == 1, v, 1.0))
        with pytest.raises(ValueError, match="GLMTarget: offset must be finite"):
            GLMTarget(X, y, offset=np.where(np.arange(n) == 1, v, 0.0))
    with pytest.raises(ValueError, match="GLMTarget: at least one weight must be > 0"):
        GLMTarget(X, y, weights=np.zeros(n))
    with pytest.raises(ValueError, match="weights must be a vector of the n = 9 observations' weights"):
        GLMTarget(X, y, weights=w[:-1])
    with pytest.raises(ValueError, match="offset must be a vector of the n = 9 observations' offsets"):
        GLMTarget(X, y, offset=np.concatenate([o, [0.0]]))
    with pytest.raises(ValueError, match="offset must be a vector"):
        GLMTarget(X, y, offset=np.zeros((n, 1)))
    with pytest.raises(ValueError, match="offset must be numeric"):
        GLMTarget(X, y, offset=["a"] * n)
    # the other targets keep their signatures
    from smcnuts_amd import WideGLMTarget
    with pytest.raises(TypeError):
        WideGLMTarget(np.zeros((3, 70)), np.zeros(3), offset=np.zeros(3))


def test_new_row_blocks():
    X, y, o, w = _data("poisson_log", n=6, p=2)
    Xn, on = X[:4] + 0.5, np.array([0.1, -0.2, 0.3, 0.0])
    yn = np.array([0.0, 2.0, 1.0, 5.0])
    for flags in (1, 2, 3):
        t = GLMTarget(X, y, family="poisson_log", offset=o if flags & 1 else None, weights=w if flags & 2 else None)
        kw = dict(offset_new=on) if flags & 1 else {}
        blk, has_y = t._predict_block(Xn, yn, **kw)
        want = np.concatenate([[1.0, 4.0, 2.0, 1.0, flags], yn, on if flags & 1 else [],
                               np.ones(4) if flags & 2 else [], Xn.reshape(-1)])
        np.testing.assert_array_equal(blk, want)
        assert has_y
        blk, has_y = t._predict_block(Xn, None, **kw)
        np.testing.assert_array_equal(blk[5:9], np.zeros(4))
        assert not has_y
        if flags & 1:
            for call in (lambda: t._predict_block(Xn, yn), lambda: t.predict(np.zeros(3), Xn),
                         lambda: t.predict_loglik(np.zeros(3), Xn, yn), lambda: t.predict_partials(np.zeros(3), Xn),
                         lambda: t.predict_draws(np.zeros((1, 3)), Xn, 4)):
                with pytest.raises(ValueError, match="offset_new is required"):
                    call()
            with pytest.raises(ValueError, match="offset_new must be a vector of the m = 4 rows"):
                t._predict_block(Xn, yn, offset_new=on[:3])
            with pytest.raises(ValueError, match="offset_new must be finite"):
                t._predict_block(Xn, yn, offset_new=np.array([0.0, np.nan, 0.0, 0.0]))
        else:
            with pytest.raises(ValueError, match="offset_new is for a GLMTarget fitted with offsets only"):
                t._predict_block(Xn, yn, offset_new=on)
    plain = GLMTarget(X, y, family="poisson_log")
    with pytest.raises(ValueError, match="offset_new is for a GLMTarget fitted with offsets only"):
        plain.predict(np.zeros(3), Xn, offset_new=on)
    blk, _ = plain._predict_block(Xn, yn)
    np.testing.assert_array_equal(blk, np.concatenate([[1.0, 4.0, 2.0, 1.0], yn, Xn.reshape(-1)]))


def test_weighted_fit_refuses_pointwise_and_loo():
    X, y, o, w = _data("bernoulli_logit")
    t = GLMTarget(X, y, weights=w)
    x = np.zeros((2, t.dim))
    for call in (lambda: t.pointwise(x), lambda: t.loo(x), lambda: t.pointwise_loglik(x),
                 lambda: t.pointwise_partials(x)):
        with pytest.raises(NotImplementedError, match="not implemented for a fit with weights"):
            call()
    # (SMCSampler.pointwise() / loo() ask the target the same question: tests/test_gpu_glm_offset.py)
    GLMTarget(X, y, offset=o)._refuse_weighted()           # offsets alone keep the criteria


# ---- the reference itself -------------------------------------------------------------------------------------------
def _model(family, X, y, o, w, intercept=True):
    return _glm_ow.GLMOWNumpy(X, y, family, 1.7, intercept, (0.3, 1.5), o, w)


def _x(model, M=3, seed=5):
    return np.random.default_rng(seed).standard_normal((M, model.dim)) * 0.4


@pytest.mark.parametrize("family", FAMILIES)
def test_reference_integer_weights_are_replicated_rows(family):
    X, y, o, _ = _data(family, n=11, flags=1)
    w = np.array([0, 1, 2, 3, 1, 0, 2, 1, 3, 1, 2], dtype=np.float64)
    rep = np.repeat(np.arange(11), w.astype(int))
    a = _model(family, X, y, o, w)
    b = _model(family, X[rep], y[rep], o[rep], None)
    x = _x(a)
    pa, pb = _glm_ow.exact_parts(a, x), _glm_ow.exact_parts(b, x)
    np.testing.assert_array_equal(pa[0], pb[0])
    np.testing.assert_allclose(pa[1], pb[1], rtol=1e-14)
    np.testing.assert_allclose(pa[3], pb[3], rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(a.logpdf(x), b.logpdf(x), rtol=1e-13)
    np.testing.assert_allclose(a.logpdfgrad(x), b.logpdfgrad(x), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("family", FAMILIES)
def test_reference_constant_offset_is_a_shifted_intercept(family):
    X, y, _, w = _data(family, n=10, flags=2)
    c = 0.625
    a = _model(family, X, y, np.full(10, c), w)
    b = _model(family, X, y, None, w)
    x = _x(a)
    xs = x.copy()
    xs[:, 0] += c
    np.testing.assert_allclose(_glm_ow.exact_parts(a, x)[1], _glm_ow.exact_parts(b, xs)[1], rtol=1e-13)
    np.testing.assert_allclose(_glm_ow.exact_parts(a, x)[3], _glm_ow.exact_parts(b, xs)[3], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("flags", [1, 2, 3])
def test_reference_against_mpmath(family, flags):
    X, y, o, w = _data(family, n=12, p=3, seed=3, flags=flags)
    m = _model(family, X, y, o, w)
    x = _x(m, M=2)
    llik = _glm_ow.exact_parts(m, x)[1]
    b = _glm_ow.device_bounds(m, x)[1]
    for k in range(2):
        want = _glm_ow.mp_llik(m, x[k])
        assert abs(llik[k] - want) <= b[k], (llik[k], want, b[k])      # (the bound covers the reference's own rounding)
        assert b[k] <= 1e-11 * max(1.0, abs(want))                       # and is no loose one
    np.testing.assert_allclose(m.parts(x)[1], llik, rtol=1e-13)


def test_reference_zero_weight_row_with_overflowing_term_is_dropped():
    X, y, o, _ = _data("poisson_log", n=8, flags=1)
    o[3] = 800.0                                                         # exp(eta_3) overflows
    w = np.ones(8)
    full = _model("poisson_log", X, y, o, w)
    x = _x(full)
    assert np.all(_glm_ow.exact_parts(full, x)[1] == -np.inf)
    assert np.all(full.logpdf(x) == -np.inf)
    assert _glm_ow.mp_llik(full, x[0]) == -np.inf
    w[3] = 0.0
    drop = _model("poisson_log", X, y, o, w)
    keep = np.arange(8) != 3
    rest = _model("poisson_log", X[keep], y[keep], o[keep], None)
    pa, pb = _glm_ow.exact_parts(drop, x), _glm_ow.exact_parts(rest, x)
    assert np.all(np.isfinite(pa[1])) and np.all(np.isfinite(pa[3]))
    np.testing.assert_array_equal(pa[1], pb[1])
    np.testing.assert_array_equal(pa[3], pb[3])
    assert np.all(np.isfinite(drop.logpdfgrad(x)))
    assert math.isfinite(_glm_ow.mp_llik(drop, x[0]))
