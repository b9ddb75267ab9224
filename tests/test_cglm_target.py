"""ContinuousGLM (gamma and Student-t regression), host side (no GPU): defaults, aliases and exports, the SMCN_MODEL_CGLM
block it packs word for word, parameter names, every argument refusal with its message, and the scope refusals, all
before any context exists."""
import inspect

import numpy as np
import pytest

import _cglm as cg

import smcnuts_amd
from smcnuts_amd import ContinuousGLM, GammaRegression, RobustRegression, _capi, _checks
from smcnuts_amd.model.targets import DeviceTarget
from smcnuts_amd.predict import PredictMixin


def _data(family, n=9, p=3, seed=0):
    return cg.synthetic(family, n, p, seed, scale=0.5)


def test_defaults_aliases_and_exports():
    sig = inspect.signature(ContinuousGLM.__init__)
    got = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert got == dict(family="gamma_log", prior_sd=2.5, intercept=True, dispersion_prior=(0.0, 2.5), df=4.0)
    assert list(sig.parameters)[:3] == ["self", "X", "y"]
    for name in ("ContinuousGLM", "GammaRegression", "RobustRegression"):
        assert getattr(smcnuts_amd, name) is getattr(smcnuts_amd.model.targets, name)
    assert issubclass(ContinuousGLM, DeviceTarget) and not issubclass(ContinuousGLM, PredictMixin)
    assert ContinuousGLM.model_id == _capi.MODEL_CGLM == 12
    X, y = _data("gamma_log")
    a, b = GammaRegression(X, y, prior_sd=1.5, dispersion_prior=(0.1, 2.0)), \
        ContinuousGLM(X, y, family="gamma_log", prior_sd=1.5, dispersion_prior=(0.1, 2.0))
    assert type(a) is ContinuousGLM and a.family == "gamma_log" and a.df is None
    assert a.model_data.tobytes() == b.model_data.tobytes()
    X, y = _data("student_t")
    c, d = RobustRegression(X, y, df=7.0, intercept=False), ContinuousGLM(X, y, family="student_t", df=7.0, intercept=False)
    assert type(c) is ContinuousGLM and c.family == "student_t" and c.df == 7.0
    assert c.model_data.tobytes() == d.model_data.tobytes()
    assert RobustRegression(X, y).df == 4.0 and inspect.signature(RobustRegression).parameters["df"].default == 4.0
    # the existing families and their ids are what they were
    assert _checks.GLM_FAMILIES == ("bernoulli_logit", "poisson_log", "normal", "neg_binomial_2_log")
    assert _checks.CONTINUOUS_FAMILIES == cg.FAMILIES
    assert 11 not in {v for k, v in vars(_capi).items() if k.startswith("MODEL_")}      # (id 11 stays unassigned)


@pytest.mark.parametrize("family", cg.FAMILIES)
@pytest.mark.parametrize("intercept", [True, False])
def test_packs_documented_layout_and_names(family, intercept):
    n, p = 7, 3
    X, y = _data(family, n, p)
    Dc = p + intercept
    sd = np.linspace(0.5, 3.0, Dc)
    t = ContinuousGLM(X, y, family=family, prior_sd=sd, intercept=intercept, dispersion_prior=(0.3, 1.5),
                      **(dict(df=2.5) if family == "student_t" else {}))
    want = np.concatenate([[cg.FAMILIES.index(family), n, p, 1.0 if intercept else 0.0, 2.5 if family == "student_t" else 0.0],
                           sd, [0.3, 1.5], y, X.reshape(-1)])
    assert t.model_data.dtype == np.float64 and t.model_data.shape == (5 + Dc + 2 + n + n * p,)
    np.testing.assert_array_equal(t.model_data, want)
    assert t.dim == t.constrained_dim == Dc + 1
    names = (["Intercept"] if intercept else []) + ["beta.1", "beta.2", "beta.3"] + \
        ["shape" if family == "gamma_log" else "sigma"]
    assert t.param_names() == names
    m = cg.ContGLMNumpy(X, y, family, sd, (0.3, 1.5), intercept, df=2.5)
    assert m.param_names() == names and m.dim == t.dim
    assert t.dispersion_prior == (0.3, 1.5) and t.intercept == bool(intercept)
    np.testing.assert_array_equal(t.prior_sd, sd)
    # a vector X is one column; a scalar prior_sd is one value for all
    t1 = ContinuousGLM(X[:, 0], y, family=family)
    assert t1.dim == 3 and t1.model_data[2] == 1.0 and np.all(t1.model_data[5:7] == 2.5)
    np.testing.assert_array_equal(t1.model_data[7:9], [0.0, 2.5])


def test_argument_refusals():
    X, y = _data("gamma_log")
    Xs, ys = _data("student_t")
    who = "ContinuousGLM: "

    def refuses(msg, *a, **k):
        with pytest.raises(ValueError) as ei:
            ContinuousGLM(*a, **k)
        assert str(ei.value).startswith(who) and msg in str(ei.value), (str(ei.value), msg)

    refuses("family must be one of ('gamma_log', 'student_t'), not 'normal'", X, y, family="normal")
    refuses("family must be one of", X, y, family=None)
    for bad, msg in ((0.0, "gamma_log needs y > 0 and y holds zeros"), (-1.0, "gamma_log needs finite y > 0"),
                     (np.inf, "gamma_log needs finite y > 0"), (np.nan, "gamma_log needs finite y > 0")):
        yb = y.copy()
        yb[3] = bad
        refuses(msg, X, yb)
    for bad in (np.inf, -np.inf, np.nan):
        yb = ys.copy()
        yb[0] = bad
        refuses("student_t needs finite y", Xs, yb, family="student_t")
    ContinuousGLM(Xs, -np.abs(ys), family="student_t")              # (negative responses are student_t's to take)
    for bad in (0.0, -1.0, np.inf, np.nan):
        refuses("df must be finite and > 0", Xs, ys, family="student_t", df=bad)
    refuses("df must be a number", Xs, ys, family="student_t", df="four")
    refuses("gamma_log has no degrees of freedom; df is for student_t", X, y, df=3.0)
    ContinuousGLM(X, y, df=4.0)                                     # (the default, spelled out)
    refuses("D = 65 coordinates (64 coefficients and tau); the device functor covers D <= 64", np.ones((3, 63)), y[:3])
    assert ContinuousGLM(np.ones((3, 63)), y[:3], intercept=False).dim == 64
    assert ContinuousGLM(np.ones((3, 62)), y[:3]).dim == 64
    refuses("no coefficients (p = 0 without an intercept)", np.zeros((9, 0)), y, intercept=False)
    assert ContinuousGLM(np.zeros((9, 0)), y).dim == 2
    refuses("X must be an (n, p) matrix", np.zeros((3, 3, 3)), y)
    refuses("y must be a vector of the n = 9 observations X has rows for", X, y[:-1])
    refuses("at least one observation", np.zeros((0, 2)), np.zeros(0))
    Xb = X.copy()
    Xb[2, 1] = np.nan
    refuses("X must be finite", Xb, y)
    refuses("prior_sd must be a scalar or one value per coefficient (4)", X, y, prior_sd=[1.0, 2.0])
    refuses("prior_sd must be finite and > 0", X, y, prior_sd=0.0)
    refuses("prior_sd must be finite and > 0", X, y, prior_sd=[1.0, np.inf, 1.0, 1.0])
    refuses("dispersion_prior must be a pair (m, s)", X, y, dispersion_prior=1.0)
    refuses("dispersion_prior's m must be finite", X, y, dispersion_prior=(np.nan, 1.0))
    refuses("dispersion_prior's s must be finite and > 0", X, y, dispersion_prior=(0.0, 0.0))
    # the aliases word their refusals as the class does
    with pytest.raises(ValueError, match="ContinuousGLM: gamma_log needs y > 0 and y holds zeros"):
        GammaRegression(X, np.zeros(9))
    with pytest.raises(ValueError, match="ContinuousGLM: df must be finite and > 0"):
        RobustRegression(Xs, ys, df=-2.0)


@pytest.mark.parametrize("family", cg.FAMILIES)
def test_scope_refusals_before_any_context(family):
    X, y = _data(family)
    t = ContinuousGLM(X, y, family=family)
    x = np.zeros((2, t.dim))
    for call in (lambda: t.pointwise(x), lambda: t.pointwise_loglik(x), lambda: t.loo(x)):
        with pytest.raises(NotImplementedError, match="ContinuousGLM: pointwise log-likelihood and the criteria built on it "
                                                      r".* are implemented for GLMTarget \(bernoulli_logit, poisson_log, "
                                                      r"normal, neg_binomial_2_log\) only"):
            call()
    for call in (lambda: t.calibration(x), lambda: t.calibration_points(x), lambda: t.calibration_partials(x)):
        with pytest.raises(NotImplementedError, match=r"ContinuousGLM: calibration checks .* are implemented for "
                                                      r"GLMTarget \(bernoulli_logit, poisson_log, normal, "
                                                      r"neg_binomial_2_log\) only"):
            call()
    assert t._ctx is None                                 # nothing above opened a device context
    assert not [a for a in dir(t) if a.startswith("predict")]
