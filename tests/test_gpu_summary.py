"""Posterior summaries (weighted quantiles and tail masses selected on the device) against the exact reference of
tests/_summary.py: the rank window always, exact equality wherever the reference is unambiguous (its docstring)."""
import numpy as np
import pytest

import _cat
import _glm
import _glm_disp as gd
import _hglm
import _ord
import _pointwise as pw
import _summary as S
from _tol import close

pytestmark = pytest.mark.gpu

DS = (1, 2, 17, 64, 65, 512)
MS = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 4097)
P1 = (0.5,)
P16 = tuple(np.random.default_rng(16).permutation(np.concatenate([S.DEFAULT, np.linspace(0.031, 0.969, 11)])))
_targets = {}


def gauss(D):
    from smcnuts_amd import GaussianTarget
    if D not in _targets:
        _targets[D] = GaussianTarget(D)
    return _targets[D]


def population(D, M, weighted):
    rng = np.random.default_rng(1000 * D + M)
    x = S.dup_values(rng, M, D)
    lw = 3.0 * rng.standard_normal(M)
    return x, (lw if weighted else None)


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("M", MS)
def test_grid(D, M):
    t = gauss(D)
    for weighted in (True, False):
        x, lw = population(D, M, weighted)
        cols = S.columns(x, lw)
        at = np.tile([0.0, -0.5, 1.3], (D, 1)) if D == 17 else None
        for probs in (P1, S.DEFAULT, P16):
            s = t.summary(x, lw, probs=probs, at=at)
            what = f"D={D} M={M} weighted={weighted} nq={len(probs)}"
            np.testing.assert_array_equal(s.probs, probs)
            assert s.n_particles == M and s.names == t.param_names()
            S.check(s.quantiles, x, lw, probs, True, what, got_cdf=s.cdf, at=at, cols=cols)
        w = S.weights(lw, M)
        close(s.ess, np.sum(w) ** 2 / np.sum(w * w), rtol=(M + 16) * 4 * S.U, what="summary: ESS of the weights")
        close(s.mean, (w / w.sum()) @ x, rtol=0.0, atol=1e-12, what="summary: mean of supplied points")


@pytest.mark.parametrize("M", (1, 65, 4097))
def test_edge_probabilities(M):
    t = gauss(17)
    for weighted in (True, False):
        x, lw = population(17, M, weighted)
        probs = (1.0, 1e-300, 0.5)
        s = t.summary(x, lw, probs=probs)
        S.check(s.quantiles, x, lw, probs, False, f"edge probabilities M={M} weighted={weighted}")
        if not weighted:
            np.testing.assert_array_equal(s.quantiles[:, 0], x.max(axis=0))
            np.testing.assert_array_equal(s.quantiles[:, 1], x.min(axis=0))


def _special(M, seed=0):
    rng = np.random.default_rng(seed + M)
    return rng.standard_normal((M, 3)), 3.0 * rng.standard_normal(M)


@pytest.mark.parametrize("M", (65, 257))
def test_identical_column(M):
    x, lw = _special(M)
    x[:, 1] = 0.7
    s = gauss(3).summary(x, lw, at=0.7)
    S.check(s.quantiles, x, lw, S.DEFAULT, True, "identical column", got_cdf=s.cdf, at=s.at)
    assert np.all(s.quantiles[1] == 0.7) and s.cdf[1, 0] == 1.0


@pytest.mark.parametrize("M", (65, 257))
def test_infinities_and_signed_zeros(M):
    x, lw = _special(M, 1)
    rng = np.random.default_rng(M)
    pick = rng.integers(0, 6, M)
    x[:, 1] = np.choose(pick, [np.full(M, -np.inf), np.full(M, np.inf), np.zeros(M), -np.zeros(M), x[:, 1], x[:, 1]])
    probs = (0.01, 0.1, 0.3, 0.5, 0.7, 0.9, 0.99)
    at = np.array([[0.0, -np.inf, np.inf, -0.0]] * 3)
    s = gauss(3).summary(x, lw, probs=probs, at=at)
    S.check(s.quantiles, x, lw, probs, True, "infinities and zeros", got_cdf=s.cdf, at=at)
    assert np.isinf(s.quantiles[1, 0]) and s.quantiles[1, 0] < 0 and np.isinf(s.quantiles[1, -1]) and s.quantiles[1, -1] > 0
    assert s.cdf[1, 0] == s.cdf[1, 3] and s.cdf[1, 2] == 1.0


@pytest.mark.parametrize("M", (65, 257))
def test_nan_with_positive_weight(M):
    x, lw = _special(M, 2)
    x[5, 1] = np.nan
    s = gauss(3).summary(x, lw, at=0.0)
    assert np.all(np.isnan(s.quantiles[1])) and np.all(np.isnan(s.cdf[1]))
    assert np.all(np.isfinite(s.quantiles[[0, 2]])) and np.all(np.isfinite(s.cdf[[0, 2]]))
    S.check(s.quantiles, x, lw, S.DEFAULT, True, "NaN, positive weight", got_cdf=s.cdf, at=s.at)


@pytest.mark.parametrize("M", (65, 257))
def test_nan_with_zero_weight(M):
    x, lw = _special(M, 3)
    x[5, 1] = np.nan
    lw[5] = -np.inf
    s = gauss(3).summary(x, lw, at=0.0)
    assert np.all(np.isfinite(s.quantiles)) and np.all(np.isfinite(s.cdf))
    S.check(s.quantiles, x, lw, S.DEFAULT, True, "NaN, zero weight", got_cdf=s.cdf, at=s.at)


@pytest.mark.parametrize("M", (65, 257))
def test_one_particle_holds_all_the_weight(M):
    x, _ = _special(M, 4)
    lw = np.full(M, -np.inf)
    lw[M // 3] = -2.5
    s = gauss(3).summary(x, lw, probs=(1e-300, 0.025, 0.5, 1.0), at=x[M // 3][:, None])
    np.testing.assert_array_equal(s.quantiles, np.repeat(x[M // 3][:, None], 4, axis=1))
    np.testing.assert_array_equal(s.cdf, np.ones((3, 1)))
    assert abs(s.ess - 1.0) < 1e-12


@pytest.mark.parametrize("M", (65, 257))
def test_weights_from_exp_minus_700_to_one(M):
    x, _ = _special(M, 5)
    lw = np.random.default_rng(M).permutation(np.linspace(-700.0, 0.0, M))
    probs = (1e-300, 0.025, 0.5, 0.975, 1.0)
    s = gauss(3).summary(x, lw, probs=probs, at=0.0)
    S.check(s.quantiles, x, lw, probs, False, "weights e^-700 .. 1", got_cdf=s.cdf, at=s.at)


@pytest.mark.parametrize("M", (65, 257))
def test_all_weights_zero(M):
    x, _ = _special(M, 6)
    s = gauss(3).summary(x, np.full(M, -np.inf), at=0.0)
    assert np.all(np.isnan(s.quantiles)) and np.all(np.isnan(s.cdf)) and s.ess == 0.0
    assert s.quantiles.shape == (3, 5) and s.cdf.shape == (3, 1)


@pytest.mark.parametrize("D", (3, 64))
def test_order_independence(D):
    M = 4097
    x, lw = population(D, M, True)
    t = gauss(D)
    a = t.summary(x, lw, probs=P16, at=[0.0, 0.5])
    b = t.summary(x, lw, probs=P16, at=[0.0, 0.5])
    perm = np.random.default_rng(D).permutation(M)
    c = t.summary(x[perm], lw[perm], probs=P16, at=[0.0, 0.5])
    for other in (b, c):
        assert a.quantiles.tobytes() == other.quantiles.tobytes()
        assert a.cdf.tobytes() == other.cdf.tobytes()


def _constrain_targets():
    from smcnuts_amd import (ArmaModel, CategoricalRegression, HierarchicalGLM, NegativeBinomialRegression,
                             OrdinalRegression)
    X, y, g = _hglm.synthetic("bernoulli_logit", 65, 1, 3, 5)
    Xo, yo = _ord.synthetic(4, 65, 2, 6)
    Xn, yn = gd.synthetic("neg_binomial_2_log", 65, 1, 7)
    Xc, yc = _cat.synthetic(3, 65, 2, 8)
    return dict(arma=lambda: ArmaModel(), hglm=lambda: HierarchicalGLM(X, y, g, family="bernoulli_logit"),
                ordinal=lambda: OrdinalRegression(Xo, yo, n_classes=4),
                negbin=lambda: NegativeBinomialRegression(Xn, yn), categorical=lambda: CategoricalRegression(Xc, yc, n_classes=3))


@pytest.mark.parametrize("name", ["arma", "hglm", "ordinal", "negbin", "categorical"])
def test_constrain_paths(name):
    t = _constrain_targets()[name]()
    if name == "hglm":
        assert t.constrained_dim == t.dim and t.dim == 2 + 3 + 1
    if name == "negbin":
        assert t.dim == 3
    rng = np.random.default_rng(11)
    M = 257
    x = 0.3 * rng.standard_normal((M, t.dim))
    lw = 3.0 * rng.standard_normal(M)
    v = t.constrain(x)
    if name != "categorical":                             # (its coordinates are reported as they are)
        assert not np.array_equal(v, x)
    s = t.summary(x, lw, at=0.0)
    assert s.names == t.param_names()
    S.check(s.quantiles, v, lw, S.DEFAULT, True, f"{name}: quantiles of constrain(x)", got_cdf=s.cdf, at=s.at)


def _logistic(n=65, D=3, seed=4):
    from smcnuts_amd import LogisticRegression
    X, y = _glm.synthetic("bernoulli_logit", n, D - 1, seed, scale=0.5)
    return LogisticRegression(X, y), _glm.GLMNumpy(X, y, "bernoulli_logit", 2.5)


def _check_resident(smc, t, what):
    K = smc.K
    s = smc.summary(at=0.0)
    v = t.constrain(smc.x_saved[-1])
    S.check(s.quantiles, v, smc.logw_saved[-1], S.DEFAULT, False, what, got_cdf=s.cdf, at=s.at)
    np.testing.assert_array_equal(s.mean, smc.mean_estimate[K])
    np.testing.assert_array_equal(s.sd, np.sqrt(smc.variance_estimate[K]))
    close(s.ess, smc.ess[K], rtol=(smc.N + 16) * 4 * S.U, what="summary: ess against smc.ess[K]")
    w = S.weights(smc.logw_saved[-1], smc.N)
    close(s.ess, np.sum(w) ** 2 / np.sum(w * w), rtol=1e-11, what="summary: ess against the saved weights")
    lo_hi = s.interval(0.95)
    assert np.all(lo_hi[:, 0] <= s.quantile(0.5)) and np.all(s.quantile(0.5) <= lo_hi[:, 1])
    assert s.n_particles == smc.N and s.names == t.param_names()
    return s


def test_resident_forward():
    from smcnuts_amd import SMCSampler
    t, _ = _logistic()
    smc = SMCSampler(K=3, N=1024, target=t, step_size=0.05, seed=5)
    with pytest.raises(RuntimeError, match="sample"):
        smc.summary()
    smc.sample(show_progress=False)
    assert smc.device_resident
    s = _check_resident(smc, t, "resident, forward L-kernel")
    again = smc.summary(at=0.0)
    assert s.quantiles.tobytes() == again.quantiles.tobytes() and s.cdf.tobytes() == again.cdf.tobytes()
    # the same population uploaded gives the same bits as the resident one
    up = t.summary(smc.x_saved[-1], smc.logw_saved[-1], at=0.0)
    assert up.quantiles.tobytes() == s.quantiles.tobytes() and up.cdf.tobytes() == s.cdf.tobytes()


def test_resident_gaussian_lkernel_tempered():
    from smcnuts_amd import SMCSampler
    t, _ = _logistic()
    smc = SMCSampler(K=60, N=1024, target=t, step_size=0.05, seed=5, lkernel="GaussianApproxLKernel", tempering=True)
    smc.sample(show_progress=False)
    assert not smc.device_resident and smc.phi[-1] == 1.0
    _check_resident(smc, t, "resident, Gaussian L-kernel with tempering")


@pytest.mark.parametrize("world", [2, 4])
def test_shards(world):
    from smcnuts_amd import SMCSampler
    from tests.test_sharding import _run_shards
    kw = dict(K=4, N=2048, step_size=0.05, seed=3)
    out = {}

    def drive(s):
        s.sample(show_progress=False)
        out[s.comm.rank] = s.summary(probs=P16, at=[0.0, 0.3])

    ranks = _run_shards(lambda c: SMCSampler(target=pw.make("poisson_log", 150, 7, 9)[0], comm=c, **kw), world, drive,
                        device=True)
    assert sorted(out) == list(range(world))
    for r in range(1, world):
        assert out[r].quantiles.tobytes() == out[0].quantiles.tobytes() and out[r].cdf.tobytes() == out[0].cdf.tobytes()
        np.testing.assert_array_equal(out[r].mean, out[0].mean)
        assert out[r].ess == out[0].ess
    x = np.concatenate([s.x_saved[-1] for s in ranks])
    lw = np.concatenate([s.logw_saved[-1] for s in ranks])
    assert x.shape == (2048, 7)
    S.check(out[0].quantiles, x, lw, P16, False, f"{world} shards", got_cdf=out[0].cdf, at=out[0].at)


class _ScaledLogistic:
    """The NumPy logistic density with a constrain() of its own (the last coordinate reported as its exponential)."""

    def __init__(self, m):
        self.m, self.dim, self.constrained_dim = m, m.dim, m.dim

    def logpdf(self, x, phi=1.0):
        return self.m.logpdf(x, phi=phi)

    def logpdfgrad(self, x, phi=1.0):
        return self.m.logpdfgrad(x, phi=phi)

    def constrain(self, x):
        v = np.array(x, dtype=np.float64, copy=True)
        v[..., -1] = np.exp(v[..., -1])
        return v

    def param_names(self):
        return [f"b{i}" for i in range(self.dim - 1)] + ["scale"]


def test_host_evaluated_target():
    from smcnuts_amd import HostTarget, SMCSampler
    _, m = _logistic()
    model = _ScaledLogistic(m)
    smc = SMCSampler(K=2, N=256, target=model, step_size=0.05, seed=2)
    smc.sample(show_progress=False)
    assert smc.target.host_evaluated and smc.phi[-1] == 1.0
    s = smc.summary(at=1.0)
    v = model.constrain(smc.x_saved[-1])
    S.check(s.quantiles, v, smc.logw_saved[-1], S.DEFAULT, False, "host-evaluated target, resident", got_cdf=s.cdf, at=s.at)
    np.testing.assert_array_equal(s.mean, smc.mean_estimate[-1])
    assert s.names == model.param_names()
    rng = np.random.default_rng(3)
    x, lw = 0.3 * rng.standard_normal((257, 3)), 3.0 * rng.standard_normal(257)
    h = HostTarget(model).summary(x, lw, at=1.0)
    S.check(h.quantiles, model.constrain(x), lw, S.DEFAULT, True, "host-evaluated target, points", got_cdf=h.cdf, at=h.at)


def test_guards():
    from smcnuts_amd import SMCSampler
    t, _ = _logistic()
    asym = SMCSampler(K=3, N=1024, target=t, step_size=0.05, seed=1, lkernel="asymptoticLKernel", tempering=True)
    asym.sample(show_progress=False)
    with pytest.raises(NotImplementedError, match="asymptotic"):
        asym.summary()
    early = SMCSampler(K=1, N=1024, target=_logistic()[0], step_size=0.05, seed=1, lkernel="GaussianApproxLKernel",
                       tempering=True)
    with pytest.raises(RuntimeError, match="sample"):
        early.summary()
    early.sample(show_progress=False)
    assert early.phi[-1] < 1.0
    with pytest.raises(RuntimeError, match="temperature"):
        early.summary()
    ok = SMCSampler(K=2, N=1024, target=_logistic()[0], step_size=0.05, seed=1)
    ok.sample(show_progress=False)
    for kw, word in ((dict(probs=(0.0,)), "probs"), (dict(probs=(0.5, 1.01)), "probs"), (dict(probs=(np.nan,)), "probs"),
                     (dict(probs=np.linspace(0.1, 0.9, 17)), "probs"), (dict(at=np.zeros((2, 1))), "at"),
                     (dict(at=np.zeros(17)), "at")):
        with pytest.raises(ValueError, match=word):
            ok.summary(**kw)
    from smcnuts_amd._capi import SmcnError, dptr
    ctx = ok.samples.ctx
    with pytest.raises(SmcnError, match="resident"):
        ctx.call("smcn_summary_begin", None, None, None, 5, 0, dptr(np.empty(4)))
    print(ok.summary(at=0.0))
