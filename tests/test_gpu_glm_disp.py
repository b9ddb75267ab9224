"""The GLM target's dispersion families on the device (GLMTarget family "normal" / "neg_binomial_2_log";
GlmModel with DISP) against exact references and against the same model evaluated on the host (tests/_glm_disp.py's numpy
density through HostTarget / oracle/pynuts.PyNUTS).

Shapes: 8 lanes per particle for D <= 8, a whole wavefront for 9 <= D <= 64; observations in passes of 8 / chunks of
64.  Every value tolerance is the worst-case bound of the evaluation it checks (_glm_disp.device_bounds)."""
import math

import numpy as np
import pytest

import _glm_disp as gd
from _tol import close

from oracle.pynuts import PyNUTS

pytestmark = pytest.mark.gpu

FAMILIES = gd.DISP_FAMILIES
U = gd.U


def _target(family, n, p, seed, intercept=True, scale=None, tau=None, prior=(0.2, 1.5)):
    from smcnuts_amd import GLMTarget
    X, y = gd.synthetic(family, n, p, seed, scale=scale, tau=tau)
    sd = np.linspace(0.8, 2.5, p + intercept)
    t = GLMTarget(X, y, family=family, prior_sd=sd, intercept=intercept, dispersion_prior=prior)
    return t, gd.GLMDispNumpy(X, y, family, sd, prior, intercept)


def _points(model, rng, extreme):
    """Benign points; (extreme) the overflow points and the near-Poisson / far-tail values of tau."""
    D = model.dim
    x = rng.standard_normal((4, D)) * 0.5
    if extreme:
        i, j = np.unravel_index(int(np.argmax(np.abs(model.Z))), model.Z.shape)
        z = model.Z[i, j]
        e = np.zeros((5, D))
        if model.family == "normal":
            e[:, -1] = (-360.0, -300.0, 50.0, -5.0, 20.0)     # e^-2tau overflows; huge; tiny
            e[3, j] = 30.0 / z
        else:
            e[0, j] = 720.0 / z                                # e^eta overflows
            e[1, -1] = math.log(1e8)                           # near-Poisson
            e[2, -1] = 720.0                                   # e^tau overflows
            e[3, -1] = -709.0                                  # e^tau below the normal range
            e[4, j], e[4, -1] = 25.0 / z, math.log(1e6)
        x = np.vstack([x, e])
    return x


D_LIST = (2, 3, 8, 9, 16, 17, 33, 64)
N_LIST = (1, 7, 64, 65, 1000, 100003)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("D", D_LIST)
@pytest.mark.parametrize("n", N_LIST)
def test_values_against_exact_reference(family, D, n):
    """logpdf, logpdfgrad and logpdf_parts at phi in {0, 0.3, 1}, against math.fsum over the float64 terms."""
    intercept = D % 2 == 0                                # both layouts of the design row (Dc = D - 1)
    p = D - 1 - intercept
    t, m = _target(family, n, p, 1000 * D + n + len(family), intercept=intercept)
    assert t.dim == D
    rng = np.random.default_rng(D + n)
    x = _points(m, rng, extreme=n <= 1000)
    lpri, llik, gpri, glik = gd.exact_parts(m, x)
    b_lpri, b_llik, b_glik = gd.device_bounds(m, x)
    a, b = t.logpdf_parts(x)
    close(a, lpri, rtol=0.0, atol=b_lpri.max() + 1e-300)
    fin = np.isfinite(llik)
    assert np.array_equal(np.isfinite(b), fin), (b, llik)
    assert np.all(b[~fin] == -np.inf)
    assert np.all(np.abs(b[fin] - llik[fin]) <= b_llik[fin]), (b[fin] - llik[fin], b_llik[fin])
    for phi in (0.0, 0.3, 1.0):
        lp = t.logpdf(x, phi)
        g = t.logpdfgrad(x, phi)
        assert np.all(lp[~fin] == -np.inf) and np.all(g[~fin] == -np.inf)
        want = lpri[fin] + phi * llik[fin]
        bound = b_lpri[fin] + phi * b_llik[fin] + 2 * U * (np.abs(lpri[fin]) + phi * np.abs(llik[fin]))
        assert np.all(np.abs(lp[fin] - want) <= bound), (lp[fin] - want, bound)
        gw = gpri[fin] + phi * glik[fin]
        gb = phi * b_glik[fin] + 2 * U * (np.abs(gpri[fin]) + phi * np.abs(glik[fin])) + 1e-300
        assert np.all(np.abs(g[fin] - gw) <= gb), np.max(np.abs(g[fin] - gw) - gb)


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


TAPE_CASES = [(f, D, eps) for f in FAMILIES for D, eps in ((2, 0.01), (8, 0.01), (9, 0.01), (33, 0.01))]


@pytest.mark.parametrize("family,D,eps", TAPE_CASES)
def test_nuts_on_tapes_against_pynuts(family, D, eps):
    """NUTSProposal(GLMTarget).rvs on drawn tapes: draws, leapfrogs and depth exact, x' and r' to 1e-12, against the
    reference-shaped NUTS over the numpy density."""
    from smcnuts_amd import GLMTarget
    from smcnuts_amd.proposal.nuts import NUTSProposal
    X, y = gd.synthetic(family, 200, D - 2, D, scale=0.5)
    t = GLMTarget(X, y, family=family, prior_sd=2.0, dispersion_prior=(0.0, 1.0))
    m = gd.GLMDispNumpy(X, y, family, 2.0, (0.0, 1.0))
    rng = np.random.default_rng(7 * D + len(family))
    N = 24
    x = rng.standard_normal((N, D)) * 0.1
    x[:, -1] = np.log(0.7 if family == "normal" else 3.0) + 0.1 * rng.standard_normal(N)
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


@pytest.mark.parametrize("family,D,eps", [("normal", 6, 0.02), ("neg_binomial_2_log", 8, 0.03),
                                          ("normal", 25, 0.03), ("neg_binomial_2_log", 40, 0.02)])
def test_philox_mode_against_host_target(family, D, eps):
    """Production RNG: device-native target and HostTarget(numpy model), same seed and state: same momenta, trees and
    draws, x' and r' to round-off."""
    from smcnuts_amd import GLMTarget, HostTarget, _capi
    N, seed, it = 4096, 4242, 5                           # (the numpy NB density is the slow side: N n per call)
    X, y = gd.synthetic(family, 200, D - 2, 11 * D, scale=0.5)
    t = GLMTarget(X, y, family=family, prior_sd=2.0, dispersion_prior=(0.0, 1.0))
    h = HostTarget(gd.GLMDispNumpy(X, y, family, 2.0, (0.0, 1.0)))
    x = np.random.default_rng(D).standard_normal((N, D)) * 0.1
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
@pytest.mark.parametrize("family,D", [("normal", 5), ("neg_binomial_2_log", 20)])
def test_full_loop_against_host_target(lkernel, tempering, family, D):
    """Every L-kernel, with and without tempering: the same phi ladder, leapfrogs, resampling and particles as the
    numpy model through HostTarget; mean estimates in constrained space (sigma / phi) alike."""
    from smcnuts_amd import GLMTarget, SMCSampler
    X, y = gd.synthetic(family, 120, D - 2, 3 * D, scale=0.5)
    kw = dict(K=5, N=1024, step_size=0.05, seed=9, lkernel=lkernel, tempering=tempering)
    dev = SMCSampler(target=GLMTarget(X, y, family=family, prior_sd=2.0, dispersion_prior=(0.0, 1.0)), **kw)
    dev.sample(show_progress=False)
    host = SMCSampler(target=gd.GLMDispNumpy(X, y, family, 2.0, (0.0, 1.0)), **kw)
    assert not host.device_resident
    host.sample(show_progress=False)
    np.testing.assert_array_equal(dev.leapfrogs, host.leapfrogs)
    assert list(dev.resampled) == list(host.resampled)
    close(dev.phi, host.phi, rtol=1e-12, atol=1e-15)
    close(dev.x_saved, host.x_saved, rtol=1e-10, atol=1e-11)
    close(dev.ess, host.ess, rtol=1e-10)
    close(dev.mean_estimate, host.mean_estimate, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("family", FAMILIES)
def test_constrained_space(family):
    """constrain() and mean_estimate report sigma / phi = e^tau for the last coordinate, the coefficients as they are."""
    from smcnuts_amd import GLMTarget, SMCSampler
    X, y = gd.synthetic(family, 80, 2, 5, scale=0.5)
    t = GLMTarget(X, y, family=family, prior_sd=2.0, dispersion_prior=(0.0, 1.0))
    x = np.random.default_rng(1).standard_normal((300, 4))
    c = t.constrain(x)
    np.testing.assert_array_equal(c[:, :3], x[:, :3])
    close(c[:, 3], np.exp(x[:, 3]), rtol=1e-15, atol=0.0)
    kw = dict(K=4, N=1024, step_size=0.05, seed=2)
    dev = SMCSampler(target=t, **kw)
    dev.sample(show_progress=False)
    m = gd.GLMDispNumpy(X, y, family, 2.0, (0.0, 1.0))
    host = SMCSampler(target=m, **kw)                      # (the numpy model's constrain() exps the last coordinate)
    host.sample(show_progress=False)
    close(dev.x_saved, host.x_saved, rtol=1e-10, atol=1e-11)
    close(dev.mean_estimate, host.mean_estimate, rtol=1e-10, atol=1e-12)
    close(dev.variance_estimate, host.variance_estimate, rtol=1e-8, atol=1e-12)
    assert np.all(dev.mean_estimate[:, -1] > 0.0)


def _quadrature(family):
    """Posterior of (intercept, tau) with no covariate, by the midpoint rule on a fine grid: mean and variance of
    (b_0, sigma / phi)."""
    rng = np.random.default_rng(2025)
    n = 60
    if family == "normal":
        y = 0.8 + 1.3 * rng.standard_normal(n)
        g0, g1 = np.linspace(-1.0, 2.6, 901), np.linspace(-0.6, 1.4, 801)
    else:
        y = rng.poisson(rng.gamma(2.0, 4.0 / 2.0, n)).astype(np.float64)
        g0, g1 = np.linspace(0.4, 2.4, 901), np.linspace(-2.5, 4.5, 801)
    m = gd.GLMDispNumpy(np.zeros((n, 0)), y, family, 2.5, (0.0, 2.5))
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
    """Intercept-only normal / NB regression, n = 60: SMCSampler's final estimates of (b_0, sigma / phi) within 5
    Monte-Carlo standard errors (from the run's ESS) of the quadrature mean and variance."""
    from smcnuts_amd import GLMTarget, SMCSampler
    y, mean, var = _quadrature(family)
    t = GLMTarget(np.zeros((len(y), 0)), y, family=family, prior_sd=2.5, dispersion_prior=(0.0, 2.5))
    # (step 0.03: the posterior sds are 0.1-0.3 in both coordinates)
    smc = SMCSampler(K=20, N=65536, target=t, step_size=0.03, lkernel=lkernel, tempering=tempering, seed=17)
    smc.sample(show_progress=False)
    ess = float(smc.ess[-1])
    assert ess > 1000
    mse = np.sqrt(var / ess)
    assert np.all(np.abs(smc.mean_estimate[-1] - mean) <= 5 * mse), (smc.mean_estimate[-1], mean, mse)
    # (sigma / phi are skewed: 4 sqrt(2) var / sqrt(ESS) covers the standard error of the variance estimate)
    vse = 4 * math.sqrt(2.0) * var / math.sqrt(ess)
    assert np.all(np.abs(smc.variance_estimate[-1] - var) <= 5 * vse), (smc.variance_estimate[-1], var, vse)


@pytest.mark.parametrize("family,lkernel,tempering,D", [("normal", "forwardsLKernel", False, 6),
                                                        ("neg_binomial_2_log", "GaussianApproxLKernel", True, 6),
                                                        ("neg_binomial_2_log", "forwardsLKernel", False, 30)])
def test_two_shards_equal_one_and_runs_repeat(family, lkernel, tempering, D):
    from smcnuts_amd import GLMTarget, SMCSampler
    from tests.test_sharding import _run_shards
    X, y = gd.synthetic(family, 150, D - 2, D, scale=0.5)
    make_t = lambda: GLMTarget(X, y, family=family, prior_sd=2.0, dispersion_prior=(0.0, 1.0))
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


def test_creation_errors():
    """What GLMTarget refuses in Python, the library refuses at context creation with a message of its own."""
    from smcnuts_amd import _capi
    n = 3

    def data(family, p, ic, y, X=None, s=1.0, mt=0.0, st=1.0):
        Dc = p + ic
        X = np.zeros((n, p)) if X is None else X
        return np.concatenate([[family, n, p, ic], np.full(Dc, s), [mt, st], np.asarray(y, dtype=np.float64),
                               X.reshape(-1)])

    cases = [
        (data(2, 64, 0, [0, 1, 0]), "D <= 64 coefficients; larger models run host-evaluated"),
        (data(3, 63, 1, [0, 1, 0]), "D <= 64 coefficients; larger models run host-evaluated"),
        (data(2, 2, 1, [0, np.nan, 1]), "normal needs finite y"),
        (data(2, 2, 1, [0, -np.inf, 1]), "normal needs finite y"),
        (data(3, 2, 1, [0, -1, 1]), "neg_binomial_2_log needs y in {0, 1, 2, .., 2^53}"),
        (data(3, 2, 1, [0, 0.5, 1]), "neg_binomial_2_log needs y in {0, 1, 2, .., 2^53}"),
        (data(3, 2, 1, [0, 2.0 ** 54, 1]), "neg_binomial_2_log needs y in {0, 1, 2, .., 2^53}"),
        (data(2, 2, 1, [0, 1, 0], mt=np.inf), "m_tau must be finite"),
        (data(3, 2, 1, [0, 1, 0], st=0.0), "s_tau must be finite and > 0"),
        (data(3, 2, 1, [0, 1, 0], st=np.nan), "s_tau must be finite and > 0"),
        (data(2, 2, 1, [0, 1, 0], s=-1.0), "prior sds must be finite and > 0"),
        (data(3, 2, 1, [0, 1, 0], X=np.array([[0, 1], [np.nan, 0], [0, 0]])), "X must be finite"),
        (data(3, 2, 1, [0, 1, 0])[:-1], "for families 2 (normal) and 3 (neg_binomial_2_log)"),
        (data(4, 2, 1, [0, 1, 0]), "family must be 0 (bernoulli_logit) or 1 (poisson_log), or 2 (normal) or 3"),
        (np.delete(data(2, 2, 1, [0, 1, 0]), [7, 8]), "for a block without m_tau, s_tau"),
        (data(3, 0, 0, [0, 1, 0]), "no coefficients"),
    ]
    for md, msg in cases:
        with pytest.raises(_capi.SmcnError) as ei:
            _capi.Context(64, _capi.MODEL_GLM, md)
        assert msg in str(ei.value), (str(ei.value), msg)
    for fam, p, ic in ((2, 63, 0), (3, 62, 1)):
        ok = _capi.Context(64, _capi.MODEL_GLM, data(fam, p, ic, [0, 3, 1]))
        assert ok.D == ok.Dc == 64
        ok.close()
