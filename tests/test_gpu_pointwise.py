"""Pointwise log-likelihood, WAIC and IS-LOO of the device GLM targets against the NumPy references of tests/_pointwise.py.
Every bound is derived there (module docstring); per-element bounds are asserted element by element and recorded
through _tol.close with the largest bound as atol."""
import math
import time

import numpy as np
import pytest

import _glm
import _glm_disp as gd
import _pointwise as pw
from _tol import close

pytestmark = pytest.mark.gpu

DS = (1, 2, 8, 9, 16, 17, 32, 33, 63, 64)
NS = (1, 7, 64, 65, 1000)
MS = (1, 63, 64, 65, 1000)
GRID = [(f, D, n) for f in pw.FAMILIES for D in DS for n in NS if not (f in gd.DISP_FAMILIES and D < 2)]


def _llik_bound(m, x):
    return (gd.device_bounds(m, x) if m.family in gd.DISP_FAMILIES else _glm.device_bounds(m, x))[1]


def _check_loglik(t, m, x, what):
    got = t.pointwise_loglik(x)
    ll, e_term, _, _ = pw.terms(m, x)
    assert got.shape == ll.shape
    fin = np.isfinite(ll)
    np.testing.assert_array_equal(got[~fin], ll[~fin], err_msg=f"{what}: non-finite pattern")
    assert np.all(np.isfinite(got[fin])), what
    err = np.abs(got[fin] - ll[fin])
    assert np.all(err <= e_term[fin]), f"{what}: max excess {np.max(err - e_term[fin]):.3e}"
    close(got[fin], ll[fin], rtol=0.0, atol=float(np.max(e_term[fin], initial=1e-300)), what="pointwise_loglik")
    # row sums against the density's own llik
    llik = t.logpdf_parts(x)[1]
    rows = np.all(fin, axis=1)
    assert np.all(np.isneginf(llik[~rows])), what
    rows &= np.isfinite(llik)                               # (a sum of finite terms may itself overflow)
    # (the sum of the two bounds: the terms' own, and device_bounds' bound of llik, which holds the summation's share)
    with np.errstate(all="ignore"):
        b = np.sum(e_term, axis=1) + _llik_bound(m, x)
    s = np.array([math.fsum(r.tolist()) for r in got[rows]])
    assert np.all(np.abs(s - llik[rows]) <= b[rows]), what
    if np.any(rows):
        close(s, llik[rows], rtol=0.0, atol=float(np.max(b[rows])), what="row sums of pointwise_loglik against llik")


@pytest.mark.parametrize("family,D,n", GRID)
def test_pointwise_loglik_grid(family, D, n):
    t, m = pw.make(family, n, D, 100 * D + n)
    for M in MS:
        x = pw.points(m, M, M + D)
        _check_loglik(t, m, x, f"{family} D={D} n={n} M={M}")
    one = t.pointwise_loglik(x[0])
    assert one.shape == (n,)
    np.testing.assert_array_equal(one, t.pointwise_loglik(x[:1])[0])


def _extreme_points(family):
    """Rows for a model with an intercept and two columns (D = 3, or 4 with tau)."""
    if family == "bernoulli_logit":
        return np.array([[800.0, 0, 0], [-800.0, 0, 0], [0, 800.0, -800.0]])
    if family == "poisson_log":
        return np.array([[709.0, 0, 0], [710.5, 0, 0], [-800.0, 0, 0], [0.3, 0.1, 0.2]])
    if family == "normal":
        return np.array([[0.1, 0.2, 0.3, -350.0], [0.1, 0.2, 0.3, -356.0], [0.1, 0.2, 0.3, 300.0], [1e6, 0, 0, 0.0]])
    return np.array([[709.0, 0, 0, 0.5], [710.5, 0, 0, 0.5], [-800.0, 0, 0, 0.5], [0.1, 0.2, 0.3, 710.0],
                     [0.1, 0.2, 0.3, -709.0], [0.1, 0.2, 0.3, -708.0], [0.1, 0.2, 0.3, 100.0], [0.1, 0.2, 0.3, 5.0]])


@pytest.mark.parametrize("family", pw.FAMILIES)
def test_pointwise_loglik_extreme_points(family):
    from smcnuts_amd import GLMTarget
    X, y = pw.synthetic(family, 65, 2, 7)
    if family in gd.DISP_FAMILIES:
        t = GLMTarget(X, y, family=family, prior_sd=2.0, dispersion_prior=(0.0, 1.0))
        m = gd.GLMDispNumpy(X, y, family, 2.0, (0.0, 1.0))
    else:
        t = GLMTarget(X, y, family=family, prior_sd=2.0)
        m = _glm.GLMNumpy(X, y, family, 2.0)
    x = _extreme_points(family)
    ll = pw.terms(m, x)[0]
    if family != "bernoulli_logit":
        assert np.any(np.isneginf(ll)) and np.any(np.isfinite(ll))
    _check_loglik(t, m, x, f"{family} extreme")


def _check_stats(t, m, x, logw, what, report=None):
    ll, e_term, mean, e_mean = pw.terms(m, x)
    ref, b = pw.criteria_bounds(ll, logw, e_term, mean, e_mean)
    got = t.pointwise(x, logw)
    pw.assert_pointwise(got, ref, b, what=what, close=close, report=report)
    assert got.n_particles == ref["n_particles"]
    close(got.ess, ref["ess"], rtol=(x.shape[0] + 16) * 4 * _glm.U, what="weights' ESS")
    return got, ref, b


@pytest.mark.parametrize("family,D,n", GRID)
def test_pointwise_stats_grid(family, D, n):
    t, m = pw.make(family, n, D, 100 * D + n)
    rng = np.random.default_rng(D + n)
    for M in MS:
        x = pw.points(m, M, M + D)
        what = f"{family} D={D} n={n} M={M}"
        lw = 3.0 * rng.standard_normal(M)
        got, ref, b = _check_stats(t, m, x, lw, what + " random logw")
        _check_stats(t, m, x, None, what + " equal weights")
        ll, _, mean, _ = pw.terms(m, x)
        for sh in (1.0e5, -1.0e5):
            # against the reference on the shifted weights within the derived bounds, and unchanged against the unshifted
            # call within both calls' bounds plus what the rounding of lw + sh moves (weight_shift_bounds)
            g2, _, b2 = _check_stats(t, m, x, lw + sh, what + f" logw {sh:+g}")
            bs = pw.weight_shift_bounds(ll, lw, mean, _glm.U * float(np.max(np.abs(lw + sh))))
            pw.assert_pointwise(g2, pw.as_ref(got), {k: b[k] + b2[k] + bs[k] for k in pw.FIELDS},
                                what=what + f" logw {sh:+g} against unshifted", close=close)
        if M == 1:
            continue            # (a third of one weight is that weight: no contributing particle would be left)
        lw3 = lw.copy()
        lw3[::3] = -np.inf
        g3, _, b3 = _check_stats(t, m, x, lw3, what + " a third of the weights -inf")
        # -inf-weight particles at points whose terms overflow / are out of range: as if they were not there
        xo = x.copy()
        if family in gd.DISP_FAMILIES:
            xo[::3, -1] = 800.0 if family == "neg_binomial_2_log" else -400.0
        else:
            xo[::3, :] = 1.0e4
        g4 = t.pointwise(xo, lw3)
        g5 = t.pointwise(x[lw3 > -np.inf], lw3[lw3 > -np.inf])
        for k in pw.FIELDS:
            np.testing.assert_array_equal(getattr(g4, k), getattr(g3, k),
                                          err_msg=f"{what} {k}: zero-weight particles changed the result")
        # the call without those particles sums the same terms in other slices: both within b3 of the same reference
        pw.assert_pointwise(g5, pw.as_ref(g3), {k: 2.0 * b3[k] for k in pw.FIELDS},
                            what=what + " without the zero-weight particles", close=close)


@pytest.mark.parametrize("family", ["poisson_log", "neg_binomial_2_log"])
def test_inf_rule(family):
    """One positive-weight particle whose term overflows in some observations."""
    from smcnuts_amd import GLMTarget
    X, y = pw.synthetic(family, 200, 2, 5)                  # two columns, no intercept
    X[:, 0] = np.random.default_rng(6).random(200) < 0.3    # (an indicator: eta of the particle below is 1500 or 0)
    if family == "neg_binomial_2_log":
        t = GLMTarget(X, y, family=family, prior_sd=2.0, intercept=False, dispersion_prior=(0.0, 1.0))
        m = gd.GLMDispNumpy(X, y, family, 2.0, (0.0, 1.0), intercept=False)
    else:
        t = GLMTarget(X, y, family=family, prior_sd=2.0, intercept=False)
        m = _glm.GLMNumpy(X, y, family, 2.0, intercept=False)
    x = pw.points(m, 50, 1)
    x[17, 0], x[17, 1] = 1500.0, 0.0
    lw = np.random.default_rng(3).standard_normal(50)
    got, ref, _ = _check_stats(t, m, x, lw, f"{family} -inf rule")
    bad = np.isneginf(pw.terms(m, x)[0][17])
    assert 10 < np.sum(bad) < 190
    assert np.all(np.isfinite(got.lppd_i))
    assert np.all(np.isneginf(got.mean_loglik_i[bad])) and np.all(np.isneginf(got.elpd_loo_i[bad]))
    assert np.all(got.loo_ess_i[bad] == 0.0)
    for k in ("p_waic_i", "elpd_waic_i", "fitted_i"):
        assert np.all(np.isnan(getattr(got, k)[bad])) and np.all(np.isfinite(getattr(got, k)[~bad]))


def test_ill_conditioned_variance():
    """normal, sigma = e^-6, 2000 particles 1e-6 apart around a point whose intercept is 4.7 off the data: terms of size 1.8e6
    with a spread of order 1.  p_waic_i within its derived bound of the exact rational variance of the float64 terms; the
    naive formula sum W ll^2 - mean^2 misses that bound 100-fold on the observation with the largest |ll|."""
    from smcnuts_amd import GLMTarget
    rng = np.random.default_rng(11)
    n, p = 70, 2
    X = rng.standard_normal((n, p)) / math.sqrt(p)
    beta = np.array([0.3, -0.5, 0.8])
    y = beta[0] + X @ beta[1:] + math.exp(-6.0) * rng.standard_normal(n)
    t = GLMTarget(X, y, family="normal", prior_sd=2.0, dispersion_prior=(0.0, 3.0))
    m = gd.GLMDispNumpy(X, y, "normal", 2.0, (0.0, 3.0))
    x = np.empty((2000, 4))
    x[:, :3] = beta + np.array([4.7, 0.0, 0.0]) + 1.0e-6 * rng.standard_normal((2000, 3))
    x[:, 3] = -6.0
    ll, e_term, mean, e_mean = pw.terms(m, x)
    assert 1.0e6 < np.max(np.abs(ll)) < 3.0e6
    ref, b = pw.criteria_bounds(ll, None, e_term, mean, e_mean)
    got = t.pointwise(x)
    exact = np.array([pw.exact_variance(ll[:, i]) for i in range(n)])
    err = np.abs(got.p_waic_i - exact)
    print(f"p_waic_i: max |device - exact| {np.max(err):.3e}, max bound {np.max(b['p_waic_i']):.3e}, "
          f"variances {np.min(exact):.3g} .. {np.max(exact):.3g}")
    assert np.all(err <= b["p_waic_i"]), f"excess {np.max(err - b['p_waic_i']):.3e}"
    close(got.p_waic_i, exact, rtol=0.0, atol=float(np.max(b["p_waic_i"])), what="p_waic_i, ill-conditioned")
    assert np.max(b["p_waic_i"]) < 1.0e-6                     # (the bound follows the spread, not ll^2)
    i = int(np.argmax(np.max(np.abs(ll), axis=0)))
    naive = abs(pw.naive_variance(ll[:, i]) - exact[i])
    print(f"observation {i}: naive error {naive:.3e}, bound {b['p_waic_i'][i]:.3e}")
    assert naive > 100.0 * b["p_waic_i"][i]
    pw.assert_pointwise(got, ref, b, what="ill-conditioned", close=close)


@pytest.mark.parametrize("family", pw.FAMILIES)
def test_mergeability_and_repeatability(family):
    from smcnuts_amd import combine_pointwise_partials
    t, m = pw.make(family, 130, 9, 21)
    x = pw.points(m, 1000, 4)
    lw = 3.0 * np.random.default_rng(8).standard_normal(1000)
    lw[5:900:11] = -np.inf
    whole = t.pointwise_partials(x, lw)
    again = t.pointwise_partials(x, lw)
    np.testing.assert_array_equal(whole, again)               # bit-identical: no dependence on block scheduling
    one = combine_pointwise_partials([whole])
    ll, e_term, mean, e_mean = pw.terms(m, x)
    ref, b = pw.criteria_bounds(ll, lw, e_term, mean, e_mean)
    pw.assert_pointwise(one, ref, b, what=f"{family} one call", close=close)
    for split in [(1, 999), (64, 936), (333, 333, 334)]:
        parts, m0 = [], 0
        for k in split:
            parts.append(t.pointwise_partials(x[m0:m0 + k], lw[m0:m0 + k]))
            m0 += k
        got = combine_pointwise_partials(parts)
        pw.assert_pointwise(got, ref, b, factor=2.0, what=f"{family} split {split}")
        for k in pw.FIELDS:
            g, o = getattr(got, k), getattr(one, k)
            assert np.all(np.abs(g - o) <= 2.0 * b[k]), f"{family} split {split} {k}"
        assert got.n_particles == one.n_particles


def _resident_check(smc, t, m, factor=1.0, what=""):
    got = smc.pointwise()
    x, lw = smc.x_saved[-1], smc.logw_saved[-1]
    ll, e_term, mean, e_mean = pw.terms(m, x)
    ref, b = pw.criteria_bounds(ll, lw, e_term, mean, e_mean)
    pw.assert_pointwise(got, ref, b, factor=factor, what=what + " resident vs reference", close=close)
    host = t.pointwise(x, lw)
    for k in pw.FIELDS:
        g, h = getattr(got, k), getattr(host, k)
        fin = np.isfinite(h)
        assert np.all(np.abs(g[fin] - h[fin]) <= 2.0 * factor * b[k][fin]), f"{what} {k}: resident vs uploaded"
    return got


@pytest.mark.parametrize("family,D,lkernel,tempering,K", [("bernoulli_logit", 6, "forwardsLKernel", False, 8),
                                                          ("poisson_log", 20, "forwardsLKernel", False, 8),
                                                          ("normal", 5, "forwardsLKernel", False, 8),
                                                          ("neg_binomial_2_log", 24, "forwardsLKernel", False, 8),
                                                          ("bernoulli_logit", 5, "GaussianApproxLKernel", True, 40)])
def test_resident_path(family, D, lkernel, tempering, K):
    from smcnuts_amd import SMCSampler
    t, m = pw.make(family, 150, D, 3 * D)
    smc = SMCSampler(K=K, N=4096, target=t, step_size=0.05, seed=5, lkernel=lkernel, tempering=tempering)
    with pytest.raises(RuntimeError, match="sample"):
        smc.pointwise()
    smc.sample(show_progress=False)
    assert smc.device_resident == (not tempering)
    _resident_check(smc, t, m, what=f"{family} D={D} {lkernel}")


def test_resident_two_shards():
    from smcnuts_amd import SMCSampler
    from tests.test_sharding import _run_shards
    def mk():
        return pw.make("poisson_log", 150, 7, 9)

    t, m = mk()
    kw = dict(K=4, N=2048, step_size=0.05, seed=3)
    one = SMCSampler(target=t, **kw)
    one.sample(show_progress=False)
    ref = _resident_check(one, t, m, what="one shard")
    out = {}

    def drive(s):
        s.sample(show_progress=False)
        out[s.comm.rank] = s.pointwise()

    _run_shards(lambda c: SMCSampler(target=mk()[0], comm=c, **kw), 2, drive, device=True)
    x, lw = one.x_saved[-1], one.logw_saved[-1]
    ll, e_term, mean, e_mean = pw.terms(m, x)
    _, b = pw.criteria_bounds(ll, lw, e_term, mean, e_mean)
    assert sorted(out) == [0, 1]
    for r in (0, 1):
        assert out[r].n_particles == ref.n_particles
        for k in pw.FIELDS:
            g, o = getattr(out[r], k), getattr(ref, k)
            assert np.all(np.abs(g - o) <= 2.0 * b[k]), f"rank {r} {k}: {np.max(np.abs(g - o)):.3e}"


def test_resident_errors():
    from smcnuts_amd import GaussianTarget, SMCSampler
    t, _ = pw.make("bernoulli_logit", 100, 5, 2)
    asym = SMCSampler(K=3, N=1024, target=t, step_size=0.05, seed=1, lkernel="asymptoticLKernel", tempering=True)
    asym.sample(show_progress=False)
    with pytest.raises(NotImplementedError, match="asymptotic"):
        asym.pointwise()
    early = SMCSampler(K=1, N=1024, target=pw.make("bernoulli_logit", 100, 5, 2)[0], step_size=0.05, seed=1,
                       lkernel="GaussianApproxLKernel", tempering=True)
    early.sample(show_progress=False)
    assert early.phi[-1] < 1.0
    with pytest.raises(RuntimeError, match="temperature"):
        early.pointwise()
    g = SMCSampler(K=2, N=1024, target=GaussianTarget(3), step_size=0.3, seed=1)
    g.sample(show_progress=False)
    with pytest.raises(NotImplementedError, match="GLMTarget"):
        g.pointwise()
    # the C entry points of a context of another model fail with a message
    from smcnuts_amd._capi import SmcnError
    with pytest.raises(SmcnError, match="SMCN_MODEL_GLM"):
        g.samples.ctx.pointwise_dims()
    with pytest.raises(SmcnError, match="SMCN_MODEL_GLM"):
        g.samples.ctx.call("smcn_pointwise_partials", None, None, 1024, None)


def test_full_size():
    """N = 65 536, n = 10 000, D = 25, logistic: against the NumPy reference in chunks of 64 observations (the chunk's
    matrices stay below 512 MB together)."""
    from smcnuts_amd import GLMTarget
    N, n, D = 65536, 10000, 25
    X, y = _glm.synthetic("bernoulli_logit", n, D - 1, 77, scale=0.5)
    sd = np.linspace(0.8, 2.5, D)
    t = GLMTarget(X, y, family="bernoulli_logit", prior_sd=sd)
    rng = np.random.default_rng(5)
    x = 0.3 * rng.standard_normal((N, D))
    lw = 3.0 * rng.standard_normal(N)
    t.pointwise(x[:256], lw[:256])                             # (context, staging buffers)
    t0 = time.perf_counter()
    got = t.pointwise(x, lw)
    t_dev = time.perf_counter() - t0
    t0 = time.perf_counter()
    used = {k: 0.0 for k in pw.FIELDS}
    for i0 in range(0, n, 64):
        sl = slice(i0, min(n, i0 + 64))
        m = _glm.GLMNumpy(X[sl], y[sl], "bernoulli_logit", sd)
        ll, e_term, mean, e_mean = pw.terms(m, x)
        ref, b = pw.criteria_bounds(ll, lw, e_term, mean, e_mean)

        class Part:
            pass

        part = Part()
        for k in pw.FIELDS:
            setattr(part, k, getattr(got, k)[sl])
        pw.assert_pointwise(part, ref, b, what=f"full size, observations {i0}..", report=used)
    t_ref = time.perf_counter() - t0
    print(f"full size: device {t_dev * 1e3:.1f} ms (upload and download included), NumPy reference {t_ref:.1f} s; "
          f"largest share of the bound used: { {k: round(v, 4) for k, v in used.items()} }")
    close(got.ess, 1.0 / np.sum(np.exp(2.0 * (lw - np.max(lw) - np.log(np.sum(np.exp(lw - np.max(lw))))))),
          rtol=(N + 16) * 4 * _glm.U, what="weights' ESS, full size")       # (as _check_stats: two sums of N weights)


def _laplace(m, iters=60):
    """Posterior mode and sds of a NumPy model by damped Newton with a central-difference Hessian of its gradient."""
    D = m.dim
    x = np.zeros(D)
    if m.family == "poisson_log" or m.family == "neg_binomial_2_log":
        x[0] = math.log(max(np.mean(m.y), 0.1))
    H = None
    for _ in range(iters):
        g = m.logpdfgrad(x)
        H = np.empty((D, D))
        for j in range(D):
            e = np.zeros(D)
            e[j] = 1e-5
            H[:, j] = (m.logpdfgrad(x + e) - m.logpdfgrad(x - e)) / 2e-5
        H = 0.5 * (H + H.T)
        step = np.linalg.solve(-H, g)
        f0, s = m.logpdf(x), 1.0
        while m.logpdf(x + s * step) < f0 and s > 1e-6:
            s *= 0.5
        x = x + s * step
        if np.max(np.abs(s * step)) < 1e-10:
            break
    return x, np.sqrt(np.diag(np.linalg.inv(-H)))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_poisson_or_negative_binomial(seed):
    """Overdispersed counts (NB2, phi = 0.5): the NB fit beats the Poisson fit by more than 4 standard errors of the paired
    elpd_waic difference; p_waic of the NB fit near its D = 5; IS-LOO of the NB fit reliable and equal to WAIC."""
    from smcnuts_amd import NegativeBinomialRegression, PoissonRegression, SMCSampler, compare
    rng = np.random.default_rng(seed)
    n, p, phi = 500, 3, 0.5
    X = rng.standard_normal((n, p)) / math.sqrt(3.0)
    b = 0.7 * rng.standard_normal(p)
    mu = np.exp(1.5 + X @ b)
    y = rng.poisson(rng.gamma(phi, mu / phi)).astype(np.float64)
    fits = {}
    for name, target, model in (("pois", PoissonRegression(X, y), _glm.GLMNumpy(X, y, "poisson_log", 2.5)),
                                ("nb", NegativeBinomialRegression(X, y), gd.GLMDispNumpy(X, y, "neg_binomial_2_log", 2.5, (0.0, 2.5)))):
        mode, sd = _laplace(model)
        smc = SMCSampler(K=20, N=16384, target=target, step_size=float(np.min(sd)) / 3.0, seed=100 + seed)
        smc.sample(show_progress=False)
        print(f"seed {seed} {name}: Laplace sds {np.round(sd, 4)}, final ESS {smc.ess[-1]:.0f}")
        assert smc.ess[-1] > 1000
        fits[name] = smc.pointwise()
    nb, pois = fits["nb"], fits["pois"]
    c = compare(nb, pois)
    print(f"seed {seed}: elpd_waic diff {c['elpd_waic_diff']:.1f} +- {c['se_elpd_waic_diff']:.1f}, nb p_waic {nb.p_waic:.2f}, "
          f"nb min loo_ess / ess {np.min(nb.loo_ess_i) / nb.ess:.3f}, nb |waic - loo| {abs(nb.elpd_waic - nb.elpd_loo):.3f}, "
          f"pois min loo_ess {np.min(pois.loo_ess_i):.1f}")
    assert c["elpd_waic_diff"] > 4.0 * c["se_elpd_waic_diff"]
    assert 2.5 <= nb.p_waic <= 10.0
    assert np.min(nb.loo_ess_i) >= 0.1 * nb.ess
    assert abs(nb.elpd_waic - nb.elpd_loo) < 1.0
