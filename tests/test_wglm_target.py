"""The wide GLM target's host side (no GPU): WideGLMTarget packs SMCN_MODEL_GLM's data block for SMCN_MODEL_WGLM, takes
GLMTarget's arguments with GLMTarget's checks, and covers 64 < D <= 256 only.  Nothing here creates a context."""
import numpy as np
import pytest

import _glm
import _glm_disp as gd

import smcnuts_amd
from smcnuts_amd import GLMTarget, WideGLMTarget
from smcnuts_amd import _capi

FAMILIES = ("bernoulli_logit", "poisson_log", "normal", "neg_binomial_2_log")
DISP = {"normal": "sigma", "neg_binomial_2_log": "phi"}


@pytest.fixture(autouse=True)
def no_context(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a context was created")
    monkeypatch.setattr(_capi, "Context", refuse)


def _xy(family, n, p, seed=0):
    return (gd.synthetic if family in DISP else _glm.synthetic)(family, n, p, seed)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("D", [65, 256])
@pytest.mark.parametrize("intercept", [True, False])
def test_packs_glm_layout(family, D, intercept):
    """The block is SMCN_MODEL_GLM's, word for word: [family, n, p, intercept, s_1..s_Dc, (m_tau, s_tau), y, X]."""
    disp = family in DISP
    Dc = D - disp
    n, p = 5, Dc - intercept
    X, y = _xy(family, n, p)
    sd = np.linspace(0.5, 3.0, Dc)
    kw = dict(dispersion_prior=(0.25, 1.5)) if disp else {}
    t = WideGLMTarget(X, y, family=family, prior_sd=sd, intercept=intercept, **kw)
    want = np.concatenate([[float(FAMILIES.index(family)), n, p, 1.0 if intercept else 0.0], sd,
                           [0.25, 1.5] if disp else [], y, X.reshape(-1)])
    assert t.model_id == _capi.MODEL_WGLM == 9
    assert t.model_data.dtype == np.float64
    np.testing.assert_array_equal(t.model_data, want)
    assert t.dim == t.constrained_dim == D
    names = (["Intercept"] if intercept else []) + [f"beta.{j + 1}" for j in range(p)] + ([DISP[family]] if disp else [])
    assert t.param_names() == names and len(names) == D
    assert t.family == family and t.intercept == intercept
    assert t.dispersion_prior == ((0.25, 1.5) if disp else None)
    np.testing.assert_array_equal(t.X, X)
    np.testing.assert_array_equal(t.y, y)
    np.testing.assert_array_equal(t.prior_sd, sd)


def test_same_block_as_glmtarget_would_pack():
    """One column fewer and GLMTarget takes the data: the two blocks differ by that column alone."""
    X, y = _xy("normal", 4, 64)
    w = WideGLMTarget(X, y, family="normal", prior_sd=1.5, dispersion_prior=(0.0, 1.0))       # D = 66
    g = GLMTarget(X[:, :62], y, family="normal", prior_sd=1.5, dispersion_prior=(0.0, 1.0))   # D = 64
    assert w.dim == 66 and g.dim == 64
    np.testing.assert_array_equal(w.model_data[[0, 1, 3]], g.model_data[[0, 1, 3]])
    assert w.model_data[2] == 64.0 and g.model_data[2] == 62.0
    np.testing.assert_array_equal(w.model_data[4 + 65:4 + 65 + 2 + 4], g.model_data[4 + 63:4 + 63 + 2 + 4])
    assert smcnuts_amd.WideGLMTarget is WideGLMTarget


@pytest.mark.parametrize("family", FAMILIES)
def test_size_limits(family):
    disp = family in DISP
    y = [0.0, 1.0, 1.0]
    kw = dict(family=family)
    # D = 64: GLMTarget's
    with pytest.raises(ValueError, match=r"^WideGLMTarget: D = 64 .*64 < D <= 256.*GLMTarget"):
        WideGLMTarget(np.zeros((3, 64 - disp)), y, intercept=False, **kw)
    with pytest.raises(ValueError, match=r"^WideGLMTarget: D = 3 .*GLMTarget"):
        WideGLMTarget(np.zeros((3, 2 - disp)), y, **kw)
    # D = 65 and D = 256 accepted
    assert WideGLMTarget(np.zeros((3, 65 - disp)), y, intercept=False, **kw).dim == 65
    assert WideGLMTarget(np.zeros((3, 64 - disp)), y, **kw).dim == 65
    assert WideGLMTarget(np.zeros((3, 255 - disp)), y, **kw).dim == 256
    # D = 257: host-evaluated
    with pytest.raises(ValueError, match=r"^WideGLMTarget: D = 257 .*D <= 256.*HostTarget"):
        WideGLMTarget(np.zeros((3, 256 - disp)), y, **kw)
    with pytest.raises(ValueError, match="WideGLMTarget: no coefficients"):
        WideGLMTarget(np.zeros((3, 0)), y, intercept=False, **kw)


@pytest.mark.parametrize("family", sorted(DISP))
def test_64_coefficients_and_tau_are_65_coordinates(family):
    t = WideGLMTarget(np.zeros((3, 63)), [0.0, 1.0, 2.0], family=family)
    assert t.dim == 65 and t.param_names()[-1] == DISP[family] and len(t.prior_sd) == 64
    with pytest.raises(ValueError, match=r"D = 64 coordinates \(63 coefficients and tau\).*GLMTarget"):
        WideGLMTarget(np.zeros((3, 62)), [0.0, 1.0, 2.0], family=family)
    with pytest.raises(ValueError, match=r"D = 257 coordinates \(256 coefficients and tau\).*HostTarget"):
        WideGLMTarget(np.zeros((3, 255)), [0.0, 1.0, 2.0], family=family)


def test_glmtarget_points_to_the_wide_class():
    with pytest.raises(ValueError, match=r"^GLMTarget: D = 65 coefficients; the device functor covers D <= 64\. "
                                         r"WideGLMTarget .*64 < D <= 256.*HostTarget"):
        GLMTarget(np.zeros((3, 64)), [0, 1, 0])
    with pytest.raises(ValueError, match=r"D = 65 coordinates \(64 coefficients and tau\).*D <= 64.*WideGLMTarget.*HostTarget"):
        GLMTarget(np.zeros((3, 63)), [0.0, 1.0, 2.0], family="normal")


@pytest.mark.parametrize("kw,match", [
    (dict(y=[0, 2, 1]), r"bernoulli_logit needs y in \{0, 1\}$"),
    (dict(family="poisson_log", y=[0, -1, 3]), r"poisson_log needs y in \{0, 1, 2, \.\.\.\}$"),
    (dict(family="poisson_log", y=[0, np.nan, 3]), r"poisson_log needs y in \{0, 1, 2, \.\.\.\}$"),
    (dict(family="normal", y=[0.5, np.inf, 1.0]), "normal needs finite y"),
    (dict(family="neg_binomial_2_log", y=[0, 2.0 ** 54, 3]), r"neg_binomial_2_log needs y in \{0, 1, 2, \.\.\., 2\^53\}$"),
    (dict(X_bad=np.nan), "X must be finite"),
    (dict(X_bad=-np.inf), "X must be finite"),
    (dict(prior_sd=0.0), "prior_sd must be finite and > 0"),
    (dict(prior_sd=np.full(66, np.inf)), "prior_sd must be finite and > 0"),
    (dict(prior_sd=[1.0, 2.0]), r"prior_sd must be a scalar or one value per coefficient \(D = 66\)"),
    (dict(family="normal", y=[0.0, 1.0, 2.0], prior_sd=[1.0, 2.0]),
     r"prior_sd must be a scalar or one value per coefficient \(66\)"),
    (dict(y=[0, 1]), r"y must be a vector of the n = 3 observations"),
    (dict(family="probit"), "family must be one of"),
    (dict(dispersion_prior=(0.0, 1.0)), "bernoulli_logit has no dispersion parameter"),
    (dict(family="normal", y=[0.0, 1.0, 2.0], dispersion_prior=(np.nan, 1.0)), "dispersion_prior's m must be finite"),
    (dict(family="normal", y=[0.0, 1.0, 2.0], dispersion_prior=(0.0, 0.0)), "dispersion_prior's s must be finite and > 0"),
    (dict(family="neg_binomial_2_log", dispersion_prior=1.0), r"dispersion_prior must be a pair \(m, s\)"),
])
def test_rejects_what_glmtarget_rejects(kw, match):
    """The same refusal from both classes, each under its own name."""
    X = np.full((3, 65), 0.25)
    if "X_bad" in kw:
        X[1, 2] = kw.pop("X_bad")
    y = kw.pop("y", [0, 1, 1])
    with pytest.raises(ValueError, match=match) as wide:
        WideGLMTarget(X, y, **kw)
    assert str(wide.value).startswith("WideGLMTarget: ")
    if "prior_sd" in kw and np.ndim(kw["prior_sd"]) == 1:
        return                                              # (the count in the message is the wider model's)
    with pytest.raises(ValueError) as narrow:
        GLMTarget(X[:, :5], y, **kw)
    assert str(narrow.value) == "GLMTarget: " + str(wide.value)[len("WideGLMTarget: "):]


def test_shape_refusals():
    with pytest.raises(ValueError, match="WideGLMTarget: at least one observation"):
        WideGLMTarget(np.zeros((0, 70)), [])
    with pytest.raises(ValueError, match=r"WideGLMTarget: X must be an \(n, p\) matrix"):
        WideGLMTarget(np.zeros((2, 70, 2)), [0, 1])


def test_no_pointwise_and_no_predict():
    t = WideGLMTarget(np.zeros((3, 70)), [0, 1, 0])
    x = np.zeros((2, 71))
    g = GLMTarget(np.zeros((3, 2)), [0, 1, 0])
    for call in (lambda: t.pointwise_loglik(x), lambda: t.pointwise(x), lambda: t.loo(x)):
        with pytest.raises(NotImplementedError, match=r"^WideGLMTarget: pointwise log-likelihood .* implemented for GLMTarget"):
            call()
    assert not [a for a in dir(t) if a.startswith("predict") or a.startswith("_predict") or a.startswith("_draws")]
    assert not hasattr(t, "pointwise_partials")
    assert [a for a in dir(g) if a.startswith("predict")]
    assert not isinstance(t, GLMTarget) and not isinstance(g, WideGLMTarget)
