"""ContinuousGLM on the device (SMCN_MODEL_CGLM: gamma_log and student_t; GlmContModel) against exact references and
against the same model evaluated on the host (tests/_cglm.py's numpy density through HostTarget / oracle/pynuts.PyNUTS).

Shapes: 8 lanes per particle for D <= 8, a whole wavefront for 9 <= D <= 64; observations in passes of 8 / chunks of
64.  Every value tolerance is the worst-case bound of the evaluation it checks (_cglm.device_bounds)."""
import functools
import math

import numpy as np
import pytest

import _cglm as cg
import _cov as CV
import _stepsize as SZ
import _summary as S
from _tol import close

from oracle.pynuts import PyNUTS

pytestmark = pytest.mark.gpu

FAMILIES = cg.FAMILIES
U = cg.U
TAU0 = {"gamma_log": math.log(3.0), "student_t": math.log(0.7)}


def _pair(family, X, y, sd=2.0, prior=(0.0, 1.0), intercept=True, df=4.0):
    from smcnuts_amd import ContinuousGLM
    kw = dict(df=df) if family == "student_t" else {}
    return (ContinuousGLM(X, y, family=family, prior_sd=sd, intercept=intercept, dispersion_prior=prior, **kw),
            cg.ContGLMNumpy(X, y, family, sd, prior, intercept, df=df))


def _check_values(t, m, x, exact=None):
    """logpdf_parts, logpdf and logpdfgrad of the device target at x against (lpri, llik, gpri, glik) -- exact_parts unless
    given -- within device_bounds."""
    lpri, llik, gpri, glik = cg.exact_parts(m, x) if exact is None else exact
    b_lpri, b_llik, b_glik = cg.device_bounds(m, x)
    a, b = t.logpdf_parts(x)
    close(a, lpri, rtol=0.0, atol=b_lpri.max() + 1e-300)
    fin = np.isfinite(llik)
    assert np.array_equal(np.isfinite(b), fin), (b, llik)
    assert np.all(b[~fin] == -np.inf)
    print("llik: largest share of the bound", float(np.max(np.abs(b[fin] - llik[fin]) / b_llik[fin], initial=0.0)))
    assert np.all(np.abs(b[fin] - llik[fin]) <= b_llik[fin]), (b[fin] - llik[fin], b_llik[fin])
    for phi in (0.0, 0.3, 1.0):
        lp = t.logpdf(x, phi)
        g = t.logpdfgrad(x, phi)
        assert np.all(lp[~fin] == -np.inf) and np.all(g[~fin] == -np.inf)
        want = lpri[fin] + phi * llik[fin]
        bound = b_lpri[fin] + phi * b_llik[fin] + 2 * U * (np.abs(lpri[fin]) + phi * np.abs(llik[fin]))
        assert np.all(np.abs(lp[fin] - want) <= bound), (lp[fin] - want, bound)
        gw = gpri[fin] + phi * glik[fin]
        # (the prior's gradient -(x - m) / s^2: the device rounds x - m, s s, its reciprocal and the product, then the sum
        #  with phi glik -- 5 roundings of |gpri|; the reference's own -v / s^2 has 3)
        gb = phi * b_glik[fin] + U * (8 * np.abs(gpri[fin]) + 2 * phi * np.abs(glik[fin])) + 1e-300
        print(f"grad, phi = {phi}: largest share of the bound", float(np.max(np.abs(g[fin] - gw) / gb, initial=0.0)))
        assert np.all(np.abs(g[fin] - gw) <= gb), np.max(np.abs(g[fin] - gw) - gb)


D_LIST = (2, 8, 9, 33, 64)          # 8 | 9: either side of the 8-lane shape's capacity; 64: the ceiling
N_LIST = (1, 63, 64, 65, 130)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("D", D_LIST)
@pytest.mark.parametrize("n", N_LIST)
def test_values_against_exact_reference(family, D, n):
    """logpdf, logpdfgrad and logpdf_parts at phi in {0, 0.3, 1}, against math.fsum over the float64 terms, with and
    without the intercept, 200 points each; tau spans shapes either side of kGammaAsym."""
    for intercept in (True, False):
        p = D - 1 - intercept
        if p < 0 or p + intercept < 1:
            continue
        X, y = cg.synthetic(family, n, p, 1000 * D + n + len(family))
        sd = np.linspace(0.8, 2.5, p + intercept)
        t, m = _pair(family, X, y, sd, (0.2, 1.5), bool(intercept))
        assert t.dim == D
        rng = np.random.default_rng(D + n + intercept)
        x = rng.standard_normal((200, D)) * 0.5
        x[:, -1] = rng.uniform(-3.0, 4.0, 200)
        _check_values(t, m, x)


def _mp_exact(m, x):
    lpri, _, gpri, _ = cg.exact_parts(m, x)
    ll, gl = zip(*(cg.mp_parts(m, xk) for xk in x))
    return lpri, np.array(ll), gpri, np.array(gl)


@pytest.mark.parametrize("y", [2.5, 1e-300, 1e300])
def test_gamma_extreme_points_against_mpmath(y):
    """One observation, eta = b_0: tau = +-30 (shape 1e13 -- Stirling -- and 1e-13), eta = +-700 with the smallest and the
    largest y; where the term is beyond the doubles (mpmath: -inf) the device says -inf."""
    t, m = _pair("gamma_log", np.zeros((1, 0)), [y], 2.5, (0.0, 2.5))
    c = math.log(y)
    x = np.array([[0.3, 30.0], [0.3, -30.0], [c + 0.2, 30.0], [c - 0.1, -30.0], [700.0, 0.5], [-700.0, 0.5], [c, 2.0],
                  [700.0, math.log(10.0)], [-700.0, math.log(9.99)]])
    exact = _mp_exact(m, x)
    assert np.isfinite(exact[1]).sum() >= 4
    _check_values(t, m, x, exact)


@pytest.mark.parametrize("df", [0.5, 1.0, 4.0, 1e6])
def test_student_far_outlier_against_mpmath(df):
    """One y = 1e200 among ordinary rows: the term and the gradient are finite and within bound, at tau = +-30 (sigma tiny
    or huge: z^2 would overflow at the tiny one) and at ordinary tau."""
    X, y = cg.synthetic("student_t", 9, 2, 31, df=4.0)
    y[4] = 1e200
    t, m = _pair("student_t", X, y, 2.0, (0.0, 1.0), df=df)
    rng = np.random.default_rng(2)
    x = rng.standard_normal((6, 4)) * 0.5
    x[:, -1] = (0.3, 30.0, -30.0, -200.0, 200.0, -1.0)
    exact = _mp_exact(m, x)
    assert np.all(np.isfinite(exact[1])) and np.all(np.isfinite(exact[3]))
    _check_values(t, m, x, exact)
    assert np.all(np.isfinite(t.logpdfgrad(x)))


@pytest.mark.parametrize("family", FAMILIES)
def test_tau_outside_the_normal_range(family):
    """-inf parts, and what every target returns for the density and the gradient where the density is -inf."""
    X, y = cg.synthetic(family, 20, 2, 5)
    t, m = _pair(family, X, y)
    x = np.zeros((4, 4))
    x[:, -1] = (720.0, -720.0, 700.0, -700.0)
    a, b = t.logpdf_parts(x)
    assert (b == -np.inf).tolist() == [True, True, False, False] and np.all(np.isfinite(a))
    _check_values(t, m, x)
    np.testing.assert_array_equal(t.logpdf(x)[:2], m.logpdf(x)[:2])
    np.testing.assert_array_equal(t.logpdfgrad(x)[:2], m.logpdfgrad(x)[:2])


class _PyNUTSDepth(PyNUTS):
    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self._lvl, self.top = 0, -1

    def build_tree(self, x, r, grad, logu, direction, depth, phi):
        if self._lvl == 0:
            self.top = depth
        self._lvl += 1
        try:
            return super().build_tree(x, r, grad, logu, direction, depth, phi)
        finally:
            self._lvl -= 1


@pytest.mark.parametrize("family,D,eps", [(f, D, 0.01) for f in FAMILIES for D in (6, 25)])
def test_nuts_on_tapes_against_pynuts(family, D, eps):
    """NUTSProposal(ContinuousGLM).rvs on drawn tapes: draws, leapfrogs and depth exact, x' and r' to 1e-12 (the
    tolerance tests/test_gpu_glm_disp.py uses for this comparison), against the reference-shaped NUTS over the numpy
    density."""
    from smcnuts_amd.proposal.nuts import NUTSProposal
    X, y = cg.synthetic(family, 200, D - 2, D, scale=0.5)
    t, m = _pair(family, X, y)
    rng = np.random.default_rng(7 * D + len(family))
    N = 24
    x = rng.standard_normal((N, D)) * 0.1
    x[:, -1] = TAU0[family] + 0.1 * rng.standard_normal(N)
    r = rng.standard_normal((N, D))
    tapes = [np.concatenate([[rng.exponential()], rng.random(2100)]) for _ in range(N)]
    tape = np.concatenate(tapes)
    tape_off = np.concatenate([[0], np.cumsum([len(v) for v in tapes])]).astype(np.int64)
    prop = NUTSProposal(t, None, eps)
    xn, rn = prop.rvs(x, r, 1.0, tape=tape, tape_off=tape_off)
    st = prop.last_stats
    assert not st["flags"].any()
    want_x, want_r = np.zeros_like(x), np.zeros_like(r)
    nleap, depth, ndraws = np.zeros(N, np.int64), np.zeros(N, np.int64), np.zeros(N, np.int64)
    for i in range(N):
        ref = _PyNUTSDepth(m, eps)
        want_x[i:i + 1], want_r[i:i + 1] = ref.rvs(x[i:i + 1], r[i:i + 1], 1.0, tapes=[tapes[i]])
        nleap[i], depth[i], ndraws[i] = ref.nleap, ref.top + 1, ref.ndraws[0]
    assert nleap.max() >= 15
    np.testing.assert_array_equal(st["ndraws"], ndraws)
    np.testing.assert_array_equal(st["nleap"], nleap)
    np.testing.assert_array_equal(st["depth"], depth)
    close(xn, want_x, rtol=1e-12, atol=1e-12)
    close(rn, want_r, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("family,D,eps", [("gamma_log", 6, 0.02), ("student_t", 8, 0.02), ("gamma_log", 25, 0.02),
                                          ("student_t", 40, 0.02)])
def test_philox_mode_against_host_target(family, D, eps):
    """Production RNG: device-native target and HostTarget(numpy model), same seed and state: same momenta, trees and
    draws, x' and r' to round-off."""
    from smcnuts_amd import HostTarget, _capi
    N, seed, it = 1024, 4242, 5
    X, y = cg.synthetic(family, 100, D - 2, 11 * D, scale=0.5)
    t, m = _pair(family, X, y)
    h = HostTarget(m)
    x = np.random.default_rng(D).standard_normal((N, D)) * 0.1
    x[:, -1] += TAU0[family]
    out = []
    for tgt in (t, h):
        ctx = _capi.Context(N, tgt.model_id, tgt.model_data)
        if tgt is h:
            h.attach(ctx)
        ctx.set_seed(seed)
        ctx.set_state(x=x, logw=np.zeros(N))
        ctx.propose_nuts(eps, 1.0, it)
        r, xn, rn, _ = ctx.get_proposal()
        out.append((r, xn, rn, ctx.tree_stats(), ctx.last_leapfrogs()))
        ctx.close()
    (r0, x0, q0, s0, l0), (r1, x1, q1, s1, l1) = out
    np.testing.assert_array_equal(r0, r1)
    mism = np.flatnonzero((s0["ndraws"] != s1["ndraws"]) | (s0["nleap"] != s1["nleap"]))
    assert mism.size == 0, f"particles {mism.tolist()} took a different tree"
    assert l0 == l1 == int(s0["nleap"].sum())
    assert s0["nleap"].mean() >= 4
    close(x0, x1, rtol=1e-12, atol=1e-12)
    close(q0, q1, rtol=1e-12, atol=1e-12)


LOOPS = [(lk, temp) for lk in ("forwardsLKernel", "GaussianApproxLKernel", "asymptoticLKernel") for temp in (False, True)]


@pytest.mark.parametrize("lkernel,tempering", LOOPS)
@pytest.mark.parametrize("family,D", [("gamma_log", 5), ("student_t", 20)])
def test_full_loop_against_host_target(lkernel, tempering, family, D):
    """Every L-kernel, with and without tempering, one family in each shape: the same phi ladder, leapfrogs,
    resampling and particles as the numpy model through HostTarget; mean estimates in constrained space (shape / sigma)
    alike."""
    from smcnuts_amd import SMCSampler
    X, y = cg.synthetic(family, 40, D - 2, 3 * D, scale=0.5)
    t, m = _pair(family, X, y)
    kw = dict(K=5, N=1024, step_size=0.05, seed=9, lkernel=lkernel, tempering=tempering)
    dev = SMCSampler(target=t, **kw)
    dev.sample(show_progress=False)
    host = SMCSampler(target=m, **kw)
    assert not host.device_resident
    host.sample(show_progress=False)
    np.testing.assert_array_equal(dev.leapfrogs, host.leapfrogs)
    assert list(dev.resampled) == list(host.resampled)
    close(dev.phi, host.phi, rtol=1e-12, atol=1e-15)
    close(dev.x_saved, host.x_saved, rtol=1e-10, atol=1e-11)
    close(dev.ess, host.ess, rtol=1e-10)
    close(dev.mean_estimate, host.mean_estimate, rtol=1e-10, atol=1e-12)
    close(dev.variance_estimate, host.variance_estimate, rtol=1e-8, atol=1e-12)
    assert np.all(dev.mean_estimate[:, -1] > 0.0)           # (e^tau, not tau)


@pytest.mark.parametrize("family", FAMILIES)
def test_constrain_and_x0(family):
    """constrain() reports e^tau for the last coordinate and the coefficients as they are, under the parameter's name; a
    run from x0 / logq0 repeats on the host target."""
    from smcnuts_amd import SMCSampler
    X, y = cg.synthetic(family, 40, 2, 5, scale=0.5)
    t, m = _pair(family, X, y)
    x = np.random.default_rng(1).standard_normal((300, 4))
    c = t.constrain(x)
    np.testing.assert_array_equal(c[:, :3], x[:, :3])
    close(c[:, 3], np.exp(x[:, 3]), rtol=1e-15, atol=0.0)
    assert t.param_names()[-1] == ("shape" if family == "gamma_log" else "sigma")
    rng = np.random.default_rng(3)
    x0 = 0.3 * rng.standard_normal((512, 4))
    logq0 = -0.5 * np.sum((x0 / 0.3) ** 2, axis=1) - 4 * math.log(0.3) - 2 * math.log(2 * math.pi)
    kw = dict(K=3, N=512, step_size=0.05, seed=2, x0=x0, logq0=logq0)
    dev = SMCSampler(target=t, **kw)
    dev.sample(show_progress=False)
    host = SMCSampler(target=m, **kw)
    host.sample(show_progress=False)
    close(dev.x_saved, host.x_saved, rtol=1e-10, atol=1e-11)
    close(dev.mean_estimate, host.mean_estimate, rtol=1e-10, atol=1e-12)


@functools.lru_cache(maxsize=None)
def _quadrature(family):
    """Posterior of (intercept, tau) with no covariate, by the midpoint rule on a fine grid (the posterior sds span 25
    cells and more: the rule's error is far below the Monte-Carlo standard errors): mean and variance of
    (b_0, shape / sigma).  Computed once per family."""
    rng = np.random.default_rng(2026)
    n = 60
    if family == "gamma_log":
        y = rng.gamma(2.0, math.exp(0.5) / 2.0, n)
        g0, g1 = np.linspace(-0.4, 1.6, 401), np.linspace(-1.0, 2.4, 301)
    else:
        y = 0.8 + 1.3 * rng.standard_normal(n) * np.sqrt(4.0 / rng.chisquare(4.0, n))
        g0, g1 = np.linspace(-1.0, 2.6, 401), np.linspace(-1.0, 1.6, 301)
    m = cg.ContGLMNumpy(np.zeros((n, 0)), y, family, 2.5, (0.0, 2.5))
    B0, B1 = np.meshgrid(g0, g1, indexing="ij")
    pts = np.stack([B0.ravel(), B1.ravel()], axis=1)
    lp = np.concatenate([m.logpdf(pts[i:i + 100000]) for i in range(0, len(pts), 100000)])
    w = np.exp(lp - lp.max())
    w /= w.sum()
    W = w.reshape(B0.shape)
    assert max(W[[0, -1], :].max(), W[:, [0, -1]].max()) < 1e-12
    c = np.stack([pts[:, 0], np.exp(pts[:, 1])], axis=1)
    mean = w @ c
    var = w @ (c - mean) ** 2
    return y, mean, var


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("lkernel,tempering", [("forwardsLKernel", False), ("GaussianApproxLKernel", True)])
def test_posterior_moments_against_quadrature(family, lkernel, tempering):
    """Intercept-only gamma / Student-t regression, n = 60: SMCSampler's final estimates of (b_0, shape / sigma) within 5
    Monte-Carlo standard errors (from the run's ESS) of the quadrature mean and variance -- the criterion of
    tests/test_gpu_glm_disp.py."""
    from smcnuts_amd import ContinuousGLM, SMCSampler
    y, mean, var = _quadrature(family)
    t = ContinuousGLM(np.zeros((len(y), 0)), y, family=family, prior_sd=2.5, dispersion_prior=(0.0, 2.5))
    # (step 0.03: the posterior sds are 0.1-0.3 in both coordinates)
    smc = SMCSampler(K=20, N=65536, target=t, step_size=0.03, lkernel=lkernel, tempering=tempering, seed=17)
    smc.sample(show_progress=False)
    ess = float(smc.ess[-1])
    assert ess > 1000
    mse = np.sqrt(var / ess)
    print(smc.mean_estimate[-1], mean, mse, smc.variance_estimate[-1], var)
    assert np.all(np.abs(smc.mean_estimate[-1] - mean) <= 5 * mse), (smc.mean_estimate[-1], mean, mse)
    # (shape / sigma are skewed: 4 sqrt(2) var / sqrt(ESS) covers the standard error of the variance estimate)
    vse = 4 * math.sqrt(2.0) * var / math.sqrt(ess)
    assert np.all(np.abs(smc.variance_estimate[-1] - var) <= 5 * vse), (smc.variance_estimate[-1], var, vse)


@pytest.mark.parametrize("family,lkernel,tempering,D", [("gamma_log", "forwardsLKernel", False, 6),
                                                        ("student_t", "GaussianApproxLKernel", True, 6),
                                                        ("student_t", "forwardsLKernel", False, 30),
                                                        ("gamma_log", "asymptoticLKernel", True, 30)])
def test_two_shards_equal_one_and_runs_repeat(family, lkernel, tempering, D):
    from smcnuts_amd import SMCSampler
    from tests.test_sharding import _run_shards
    X, y = cg.synthetic(family, 150, D - 2, D, scale=0.5)
    make_t = lambda: _pair(family, X, y)[0]
    kw = dict(K=4, N=2048, step_size=0.05, seed=3, lkernel=lkernel, tempering=tempering)
    one = SMCSampler(target=make_t(), **kw)
    one.sample(show_progress=False)
    again = SMCSampler(target=make_t(), **kw)
    again.sample(show_progress=False)
    np.testing.assert_array_equal(again.x_saved, one.x_saved)
    np.testing.assert_array_equal(again.logw_saved, one.logw_saved)
    np.testing.assert_array_equal(again.phi, one.phi)
    sh = _run_shards(lambda c: SMCSampler(target=make_t(), comm=c, **kw), 2, lambda s: s.sample(show_progress=False),
                     device=True)
    for s in sh:
        assert list(s.resampled) == list(one.resampled)
        close(s.phi, one.phi, rtol=1e-12, atol=1e-15)
        close(s.ess, one.ess, rtol=1e-11)
        close(s.mean_estimate, one.mean_estimate, rtol=1e-10, atol=1e-13)
    close(np.concatenate([s.x_saved for s in sh], axis=1), one.x_saved, rtol=1e-10, atol=1e-13)
    assert sum(int(s.leapfrogs.sum()) for s in sh) == int(one.leapfrogs.sum())


def test_robust_regression_recovers_the_slope_linear_does_not():
    """RobustRegression(df = 4) has the true slope 2 within 3 of its own posterior sd; LinearRegression on the same data
    misses it by more than 3 of ITS own (larger) posterior sd -- and so by far more than 3 of the robust fit's.  The data
    set (_cglm.outlier_data, seed 8: the first one tried) separates the two by a wide margin: by quadrature over the NumPy
    models (tests/test_cglm_robust_host.py) the robust slope is 1.88 +- 0.09, 1.3 sd off, the linear one 6.31 +- 0.65,
    6.6 sd off."""
    from smcnuts_amd import LinearRegression, RobustRegression, SMCSampler
    x, y = cg.outlier_data()
    out = {}
    for name, t in (("robust", RobustRegression(x, y, df=4.0)), ("linear", LinearRegression(x, y))):
        smc = SMCSampler(K=20, N=8192, target=t, step_size="auto", lkernel="GaussianApproxLKernel", tempering=True, seed=5)
        smc.sample(show_progress=False)
        out[name] = (float(smc.mean_estimate[-1][1]), math.sqrt(float(smc.variance_estimate[-1][1])))
    print(out)
    (rm, rs), (lm, ls) = out["robust"], out["linear"]
    assert abs(rm - 2.0) <= 3.0 * rs and rs < 0.2
    assert abs(lm - 2.0) > 3.0 * ls > 3.0 * rs


@pytest.mark.parametrize("family", FAMILIES)
def test_auto_step_size_summary_and_covariance(family):
    """step_size="auto" runs; the probe, summary() and covariance() agree with their NumPy references (tests/_stepsize.py,
    _summary.py, _cov.py) to the tolerances of their own test files."""
    from smcnuts_amd import SMCSampler
    X, y = cg.synthetic(family, 65, 3, 21, scale=0.5)
    t, m = _pair(family, X, y)
    # the probe per particle against NumPy over the numpy model (tests/test_gpu_stepsize.py: TOL)
    rng = np.random.default_rng(4)
    x = 0.1 * rng.standard_normal((37, 5))
    x[:, -1] += TAU0[family]
    r = rng.standard_normal((37, 5))
    ladder = SZ.OCTAVES / 16.0                            # (the reference leaves the band in 6 % of the entries here)
    want = SZ.probe_reference(lambda v: m.logpdf(v), lambda v: m.logpdfgrad(v), x, r, ladder)
    part, acc, fb = t._context(37).stepsize_probe(ladder, x=x, r=r, n_leapfrog=SZ.N_LEAP, want_particles=True)
    SZ.compare_entries(want, acc, fb, close, rtol=4.9e-13, atol=4.9e-13)
    pr = t.probe_step_size(x)
    assert 0.0 < pr.step_size < 4.0
    # a sampler on "auto": constructs, samples, reports
    smc = SMCSampler(K=4, N=1024, target=t, step_size="auto", seed=4)
    smc.sample(show_progress=False)
    assert np.all(np.isfinite(smc.mean_estimate[-1])) and smc.mean_estimate[-1][-1] > 0.0
    v = t.constrain(smc.x_saved[-1])
    lw = smc.logw_saved[-1]
    s = smc.summary(at=0.5)
    assert s.names == t.param_names()
    S.check(s.quantiles, v, lw, S.DEFAULT, False, f"{family}: resident summary", got_cdf=s.cdf, at=s.at)
    up = t.summary(smc.x_saved[-1], lw, at=0.5)
    assert up.quantiles.tobytes() == s.quantiles.tobytes() and up.cdf.tobytes() == s.cdf.tobytes()
    c = t.covariance(smc.x_saved[-1], lw)
    assert c.names == t.param_names()
    CV.check(c.mean, c.cov, np.atleast_2d(v), lw, c.centre, f"{family}: covariance of constrain(x)")
    CV.check_corr(c.corr, c.cov, family)


def test_creation_errors():
    """What ContinuousGLM refuses in Python, the library refuses at context creation with a message of its own that names
    the continuous GLM target; id 11 is still no model."""
    from smcnuts_amd import _capi
    n = 3

    def data(family, p, ic, y, X=None, s=1.0, mt=0.0, st=1.0, df=None):
        Dc = p + ic
        X = np.zeros((n, p)) if X is None else X
        df = (4.0 if family == 1 else 0.0) if df is None else df
        return np.concatenate([[family, n, p, ic, df], np.full(Dc, s), [mt, st], np.asarray(y, dtype=np.float64),
                               X.reshape(-1)])

    Y = [0.5, 1.0, 2.0]
    cases = [
        (data(2, 2, 1, Y), "family must be 0 (gamma_log) or 1 (student_t)"),
        (data(0.5, 2, 1, Y), "family must be 0 (gamma_log) or 1 (student_t)"),
        (np.concatenate([[0, 2.5, 2, 1, 0], np.ones(12)]), "n must be an integer >= 1"),
        (np.concatenate([[0, 3, 1.5, 1, 0], np.ones(12)]), "p must be an integer >= 0"),
        (np.concatenate([[0, 3, 2, 0.5, 0], np.ones(12)]), "intercept must be 0 or 1"),
        (data(0, 64, 0, Y), "D = Dc + 1 <= 64 coordinates"),
        (data(1, 63, 1, Y), "D = Dc + 1 <= 64 coordinates"),
        (data(0, 2, 1, Y, X=np.array([[0, 1], [np.nan, 0], [0, 0]])), "X must be finite"),
        (data(0, 2, 1, [0.5, 0.0, 1.0]), "gamma_log needs finite y > 0 (a zero has no gamma density"),
        (data(0, 2, 1, [0.5, -1.0, 1.0]), "gamma_log needs finite y > 0"),
        (data(0, 2, 1, [0.5, np.inf, 1.0]), "gamma_log needs finite y > 0"),
        (data(1, 2, 1, [0.5, np.nan, 1.0]), "student_t needs finite y"),
        (data(1, 2, 1, [0.5, -np.inf, 1.0]), "student_t needs finite y"),
        (data(1, 2, 1, Y, df=0.0), "student_t needs df finite and > 0"),
        (data(1, 2, 1, Y, df=-1.0), "student_t needs df finite and > 0"),
        (data(1, 2, 1, Y, df=np.inf), "student_t needs df finite and > 0"),
        (data(1, 2, 1, Y, df=np.nan), "student_t needs df finite and > 0"),
        (data(0, 2, 1, Y, df=4.0), "gamma_log has no df: the slot must be 0"),
        (data(0, 2, 1, Y, s=-1.0), "prior sds must be finite and > 0"),
        (data(1, 2, 1, Y, s=np.inf), "prior sds must be finite and > 0"),
        (data(0, 2, 1, Y, mt=np.inf), "m_tau must be finite"),
        (data(0, 2, 1, Y, st=0.0), "s_tau must be finite and > 0"),
        (data(1, 2, 1, Y, st=np.nan), "s_tau must be finite and > 0"),
        (data(0, 2, 1, Y)[:-1], "data = [family, n, p, intercept, df, s_1..s_Dc, m_tau, s_tau, y_1..y_n, X (n x p, row-major)]"),
        (np.append(data(1, 2, 1, Y), 0.0), "data = [family, n, p, intercept, df, s_1..s_Dc, m_tau, s_tau, y_1..y_n, X"),
        (data(0, 0, 0, Y), "no coefficients"),
    ]
    for md, msg in cases:
        with pytest.raises(_capi.SmcnError) as ei:
            _capi.Context(64, _capi.MODEL_CGLM, md)
        assert "continuous GLM target: " in str(ei.value) and msg in str(ei.value), (str(ei.value), msg)
    for fam, p, ic in ((0, 63, 0), (1, 62, 1)):
        ok = _capi.Context(64, _capi.MODEL_CGLM, data(fam, p, ic, Y))
        assert ok.D == ok.Dc == 64
        ok.close()
    with pytest.raises(_capi.SmcnError, match="unknown model id"):
        _capi.Context(64, 11, data(0, 2, 1, Y))


def test_scope_refusals_through_the_c_entry_points():
    """Pointwise, PSIS, calibration and predict calls on an id-12 context fail with their scope messages."""
    from smcnuts_amd import _capi
    X, y = cg.synthetic("gamma_log", 20, 2, 1)
    t, _ = _pair("gamma_log", X, y)
    ctx = _capi.Context(64, t.model_id, t.model_data)
    x = np.zeros((64, 4))
    ctx.set_state(x=x, logw=np.zeros(64))
    pw = "pointwise criteria cover the SMCN_MODEL_GLM families"
    for call in (ctx.pointwise_dims, lambda: ctx.pointwise_loglik(x), lambda: ctx.pointwise_partials(),
                 ctx.calibration_dims, lambda: ctx.calibration_points(x), lambda: ctx.calibration_partials(),
                 lambda: ctx.psis_loo()):
        with pytest.raises(_capi.SmcnError, match=pw):
            call()
    with pytest.raises(_capi.SmcnError, match="held-out prediction covers the regression targets"):
        ctx.predict_set_data(np.zeros(5), False)
    ctx.close()
