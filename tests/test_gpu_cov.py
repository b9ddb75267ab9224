"""Posterior covariance on the device (smcn_cov_partials: fp64 MFMA) against the references and the per-entry bound of
tests/_cov.py; the lane map bit for bit on integer data."""
import numpy as np
import pytest

import _cov as CV
import _glm
import _glm_disp as gd
import _hglm
import _ord
import _pointwise as pw
from _tol import close

pytestmark = pytest.mark.gpu

_targets = {}


def gauss(D):
    from smcnuts_amd import GaussianTarget
    if D not in _targets:
        _targets[D] = GaussianTarget(D)
    return _targets[D]


def partial(D, x, lw, centre=None, slices=0):
    """(augmented sums, centre used, header) of the points x through the C entry points."""
    ctx = gauss(D)._context(x.shape[0])
    head, Dc = ctx.summary_begin(x, lw)
    assert Dc == D
    aug, cen = ctx.cov_partials(head[0], Dc, centre, slices)
    return aug, cen, head, ctx


@pytest.mark.parametrize("Dc", (15, 16, 17, 47))
@pytest.mark.parametrize("M", (1, 3, 64, 65, 130))
def test_lane_map_exact(Dc, M):
    v, lw = CV.int_population(Dc, M)
    want = CV.int_gram(v, lw)
    for slices in (0, 1, 3):
        aug, cen, _, _ = partial(Dc, v, lw, centre=np.zeros(Dc), slices=slices)
        np.testing.assert_array_equal(aug, want, err_msg=f"Dc={Dc} M={M} slices={slices}")
        np.testing.assert_array_equal(cen, np.zeros(Dc))
    assert aug[Dc, Dc] == np.isfinite(lw).sum()
    np.testing.assert_array_equal(aug[Dc, :Dc], v[np.isfinite(lw)].sum(axis=0))


@pytest.mark.parametrize("Dc", (1, 2, 15, 16, 17, 33, 64, 65, 256))
@pytest.mark.parametrize("M", (1, 2, 63, 64, 65, 257, 4097))
def test_grid(Dc, M):
    t = gauss(Dc)
    for weighted in (True, False):
        x, lw = CV.population(Dc, M, weighted)
        what = f"Dc={Dc} M={M} weighted={weighted}"
        c = t.covariance(x, lw)
        CV.check(c.mean, c.cov, x, lw, c.centre, what)
        assert c.cov.tobytes() == c.cov.T.copy().tobytes(), f"{what}: cov not symmetric"
        CV.check_corr(c.corr, c.cov, what)
        if M > 2:
            assert np.all(np.diagonal(c.corr) == 1.0)
        assert c.n_particles == M and c.names == t.param_names()
        w = CV.weights(lw, M)
        close(c.ess, np.sum(w) ** 2 / np.sum(w * w), rtol=CV.TOL(M), what="covariance: ESS of the weights")


def test_slices():
    Dc, M = 17, 4097
    x, lw = CV.population(Dc, M, True)
    t = gauss(Dc)
    from smcnuts_amd.covariance import combine_cov_partials
    centre = np.average(x, axis=0, weights=CV.weights(lw, M)) + 0.003
    ref, got = None, {}
    for slices in (1, 2, 17, 40, 0):
        aug, cen, head, ctx = partial(Dc, x, lw, centre=centre, slices=slices)
        np.testing.assert_array_equal(cen, centre)
        again, _ = ctx.cov_partials(head[0], Dc, centre, slices)
        assert aug.tobytes() == again.tobytes(), f"slices={slices}: two calls differ"
        assert aug.tobytes() == aug.T.copy().tobytes()
        mean, cov, _, _ = combine_cov_partials([aug], cen)
        ref = CV.check(mean, cov, x, lw, cen, f"slices={slices}", ref=ref)
        got[slices] = aug
    Ms, Dcs, rule, cap = ctx.cov_dims()
    assert (Ms, Dcs) == (M, Dc) and 1 <= rule <= cap
    aug, _, _, _ = partial(Dc, x, lw, centre=centre, slices=rule)
    assert aug.tobytes() == got[0].tobytes(), "slices = 0 is the rule's own count"
    assert any(got[a].tobytes() != got[b].tobytes() for a, b in ((1, 2), (2, 17), (17, 40)))   # the geometry did change
    from smcnuts_amd._capi import SmcnError
    with pytest.raises(SmcnError, match="slices"):
        ctx.cov_partials(head[0], Dc, centre, cap + 1)


def test_ill_conditioned():
    rng = np.random.default_rng(5)
    M = 4097
    v = 1e8 + 1e-4 * rng.standard_normal((M, 2)) @ np.array([[1.0, 0.6], [0.0, 0.8]])
    lw = 3.0 * rng.standard_normal(M)
    w = CV.weights(lw, M)
    em, ec = CV.exact_floats(v, w)
    absmean = np.abs(v).T @ w / w.sum()
    t = gauss(2)
    c = t.covariance(v, lw)
    CV.check(c.mean, c.cov, v, lw, c.centre, "ill-conditioned, against the exact rational value", ref=(em, ec, absmean))
    wn = w / w.sum()
    naive = (v * wn[:, None]).T @ v - np.outer(wn @ v, wn @ v)
    assert np.all(np.abs(naive - ec) > 0.5 * np.abs(ec)), "the naive formula has no correct digit here"
    assert np.all(np.abs(c.cov - ec) < 1e-6 * np.abs(ec))


def _rules_population():
    rng = np.random.default_rng(8)
    M, Dc = 130, 5
    return rng.standard_normal((M, Dc)) + np.arange(Dc), 3.0 * rng.standard_normal(M), M, Dc


def test_rules_zero_weight_values_are_never_multiplied():
    x, lw, M, Dc = _rules_population()
    lw[7] = -np.inf
    lw[70] = lw.max() - 900.0                              # exp underflows to 0
    t = gauss(Dc)
    base = t.covariance(x, lw)
    x2 = x.copy()
    x2[7, 1] = np.nan
    x2[70, 3] = np.nan
    x2[70, 0] = np.inf
    other = t.covariance(x2, lw)
    for a, b in ((base.mean, other.mean), (base.cov, other.cov), (base.corr, other.corr)):
        assert np.all(np.isfinite(a)) and a.tobytes() == b.tobytes()
    CV.check(base.mean, base.cov, np.delete(x, (7, 70), axis=0), np.delete(lw, (7, 70)), base.centre,
             "two rows without weight")


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_rules_non_finite_value_with_weight(value):
    x, lw, M, Dc = _rules_population()
    t = gauss(Dc)
    base = t.covariance(x, lw)
    x2 = x.copy()
    x2[9, 2] = value
    c = t.covariance(x2, lw)
    bad = np.zeros((Dc, Dc), dtype=bool)
    bad[2, :] = bad[:, 2] = True
    for m in (c.cov, c.corr):
        assert np.all(np.isnan(m[bad])) and np.all(np.isfinite(m[~bad]))
    assert np.isnan(c.mean[2]) and np.all(np.isfinite(np.delete(c.mean, 2)))
    keep = [0, 1, 3, 4]
    assert c.cov[np.ix_(keep, keep)].tobytes() == base.cov[np.ix_(keep, keep)].tobytes()


def test_rules_no_weight_and_constant_column():
    x, lw, M, Dc = _rules_population()
    t = gauss(Dc)
    c = t.covariance(x, np.full(M, -np.inf))
    assert np.all(np.isnan(c.mean)) and np.all(np.isnan(c.cov)) and np.all(np.isnan(c.corr)) and c.ess == 0.0
    assert c.cov.shape == (Dc, Dc)
    x[:, 3] = 0.7
    c = t.covariance(x, lw)
    CV.check(c.mean, c.cov, x, lw, c.centre, "constant column")
    assert c.cov[3, 3] >= 0.0
    row = c.corr[3]
    assert np.all(np.isnan(row)) or np.all((row >= -1.0) & (row <= 1.0))
    CV.check_corr(c.corr, c.cov, "constant column")


def _constrain_targets():
    from smcnuts_amd import (GaussianTarget, HierarchicalGLM, LogisticRegression, MultilevelGLM,
                             NegativeBinomialRegression, OrdinalRegression, WideGLMTarget)
    import _mlglm
    X, y, g = _hglm.synthetic("bernoulli_logit", 65, 1, 3, 5)
    Xo, yo = _ord.synthetic(4, 65, 2, 6)
    Xn, yn = gd.synthetic("neg_binomial_2_log", 65, 1, 7)
    Xl, yl = _glm.synthetic("bernoulli_logit", 65, 2, 4, scale=0.5)
    return dict(glm=lambda: LogisticRegression(Xl, yl), negbin=lambda: NegativeBinomialRegression(Xn, yn),
                hglm=lambda: HierarchicalGLM(X, y, g, family="bernoulli_logit"),
                ordinal=lambda: OrdinalRegression(Xo, yo, n_classes=4), gaussian=lambda: GaussianTarget(6),
                wide=lambda: _wide(WideGLMTarget), multilevel=lambda: _multilevel(MultilevelGLM, _mlglm))


def _wide(WideGLMTarget):
    rng = np.random.default_rng(12)
    X = 0.3 * rng.standard_normal((40, 64))
    y = (rng.random(40) < 0.5).astype(float)
    return WideGLMTarget(X, y, family="bernoulli_logit")


def _multilevel(MultilevelGLM, _mlglm):
    X, y, terms = _mlglm.synthetic("bernoulli_logit", 60, 2, [(3, 0), (3, 0)], 13)      # varying intercept and slope
    return MultilevelGLM(X, y, terms, family="bernoulli_logit")


@pytest.mark.parametrize("name", ["glm", "negbin", "hglm", "ordinal", "gaussian", "wide", "multilevel"])
def test_constrain_paths(name):
    t = _constrain_targets()[name]()
    if name == "wide":
        assert t.dim == 65
    rng = np.random.default_rng(11)
    M = 257
    x = 0.3 * rng.standard_normal((M, t.dim))
    lw = 3.0 * rng.standard_normal(M)
    v = np.atleast_2d(t.constrain(x))
    if name in ("negbin", "hglm", "ordinal", "multilevel"):
        assert not np.array_equal(v, x)
    c = t.covariance(x, lw)
    assert c.names == list(t.param_names()) and c.cov.shape == (v.shape[1], v.shape[1])
    CV.check(c.mean, c.cov, v, lw, c.centre, f"{name}: covariance of constrain(x)")
    CV.check_corr(c.corr, c.cov, name)


def _logistic(n=65, D=3, seed=4):
    from smcnuts_amd import LogisticRegression
    X, y = _glm.synthetic("bernoulli_logit", n, D - 1, seed, scale=0.5)
    return LogisticRegression(X, y), _glm.GLMNumpy(X, y, "bernoulli_logit", 2.5)


def _check_resident(smc, t, what):
    K = smc.K
    c = smc.covariance()
    v = np.atleast_2d(t.constrain(smc.x_saved[-1]))
    lw = smc.logw_saved[-1]
    ref = CV.check(c.mean, c.cov, v, lw, smc.mean_estimate[K], what)
    rm, rc, ram = ref
    bm, bc = CV.bounds(rm, rc, ram, smc.mean_estimate[K], smc.N)
    close(CV.share(c.mean, smc.mean_estimate[K], bm), 0.0, rtol=0.0, atol=1.0,
          what="covariance: mean against mean_estimate[K]")
    close(CV.share(np.diagonal(c.cov), smc.variance_estimate[K], np.diagonal(bc)), 0.0, rtol=0.0, atol=1.0,
          what="covariance: diag(cov) against variance_estimate[K]")
    up = t.covariance(smc.x_saved[-1], lw)
    close(CV.share(c.cov, up.cov, bc), 0.0, rtol=0.0, atol=1.0, what="covariance: resident against uploaded")
    close(CV.share(c.mean, up.mean, bm), 0.0, rtol=0.0, atol=1.0, what="covariance: resident mean against uploaded")
    for i in range(c.mean.size):
        assert c.contrast(np.eye(c.mean.size)[i]) == (c.mean[i], c.sd[i])
    assert c.n_particles == smc.N and c.names == t.param_names() and c.ess == smc.ess[K]
    again = smc.covariance()
    assert again.cov.tobytes() == c.cov.tobytes() and again.mean.tobytes() == c.mean.tobytes()
    return c


def test_resident_forward():
    from smcnuts_amd import SMCSampler
    t, _ = _logistic()
    smc = SMCSampler(K=3, N=1024, target=t, step_size=0.05, seed=5)
    with pytest.raises(RuntimeError, match="sample"):
        smc.covariance()
    smc.sample(show_progress=False)
    print(_check_resident(smc, t, "resident, forward L-kernel"))


def test_resident_gaussian_lkernel():
    from smcnuts_amd import SMCSampler
    t, _ = _logistic()
    smc = SMCSampler(K=3, N=1024, target=t, step_size=0.05, seed=5, lkernel="GaussianApproxLKernel")
    smc.sample(show_progress=False)
    _check_resident(smc, t, "resident, Gaussian L-kernel")


@pytest.mark.parametrize("world", [2, 4])
def test_shards(world):
    from smcnuts_amd import SMCSampler
    from smcnuts_amd.covariance import device_covariance
    from tests.test_sharding import _run_shards
    kw = dict(K=4, N=2048, step_size=0.05, seed=3)
    out, own = {}, {}

    def drive(s):
        s.sample(show_progress=False)
        out[s.comm.rank] = s.covariance()
        own[s.comm.rank] = device_covariance(s.samples.ctx, s.comm)       # no centre given: the shards agree on one

    ranks = _run_shards(lambda c: SMCSampler(target=pw.make("poisson_log", 150, 7, 9)[0], comm=c, **kw), world, drive,
                        device=True)
    assert sorted(out) == list(range(world))
    for r in range(1, world):
        for a, b in ((out[r].cov, out[0].cov), (out[r].corr, out[0].corr), (out[r].mean, out[0].mean)):
            assert a.tobytes() == b.tobytes()
        for a, b in zip(own[r], own[0]):
            assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
    x = np.concatenate([s.x_saved[-1] for s in ranks])
    lw = np.concatenate([s.logw_saved[-1] for s in ranks])
    assert x.shape == (2048, 7)
    K = ranks[0].K
    ref = CV.check(out[0].mean, out[0].cov, x, lw, ranks[0].mean_estimate[K], f"{world} shards")
    mean, cov, corr, ess, used = own[0]
    CV.check(mean, cov, x, lw, used, f"{world} shards, their own centre", ref=ref)
    # one shard of the same population
    one = ranks[0].target.covariance(x, lw)
    bm, bc = CV.bounds(*ref, ranks[0].mean_estimate[K], 2048)
    close(CV.share(out[0].cov, one.cov, bc), 0.0, rtol=0.0, atol=1.0, what="covariance: shards against one shard")


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
    c = smc.covariance()
    v = model.constrain(smc.x_saved[-1])
    CV.check(c.mean, c.cov, v, smc.logw_saved[-1], smc.mean_estimate[-1], "host-evaluated target, resident")
    assert c.names == model.param_names()
    rng = np.random.default_rng(3)
    x, lw = 0.3 * rng.standard_normal((257, 3)), 3.0 * rng.standard_normal(257)
    h = HostTarget(model).covariance(x, lw)
    CV.check(h.mean, h.cov, model.constrain(x), lw, h.centre, "host-evaluated target, points")


def test_refusals():
    from smcnuts_amd import SMCSampler
    from smcnuts_amd._capi import SmcnError
    t, _ = _logistic()
    asym = SMCSampler(K=3, N=1024, target=t, step_size=0.05, seed=1, lkernel="asymptoticLKernel", tempering=True)
    asym.sample(show_progress=False)
    with pytest.raises(NotImplementedError, match="asymptotic"):
        asym.covariance()
    early = SMCSampler(K=1, N=1024, target=_logistic()[0], step_size=0.05, seed=1, lkernel="GaussianApproxLKernel",
                       tempering=True)
    with pytest.raises(RuntimeError, match="sample"):
        early.covariance()
    early.sample(show_progress=False)
    assert early.phi[-1] < 1.0
    with pytest.raises(RuntimeError, match="temperature"):
        early.covariance()
    ctx = gauss(3)._context(4)
    head, Dv = ctx.summary_begin(None, None, np.zeros((4, 1024)))
    assert Dv == 1024
    with pytest.raises(SmcnError, match="1023"):
        ctx.cov_partials(head[0], 1024)
    head, Dv = ctx.summary_begin(None, None, np.arange(4.0 * 1023).reshape(4, 1023))
    aug, _ = ctx.cov_partials(head[0], 1023)              # the largest size accepted
    assert aug[1023, 1023] == 4.0 and aug.tobytes() == aug.T.copy().tobytes()
