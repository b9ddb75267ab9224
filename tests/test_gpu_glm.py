"""The canonical-link GLM target on the device (GLMTarget; SMCN_MODEL_GLM) against exact references and against the
same model evaluated on the host (tests/_glm.py's numpy density through HostTarget / oracle/pynuts.PyNUTS).

Shapes: the device functor groups 8 lanes per particle for D <= 16 and a whole wavefront for 17 <= D <= 64, and takes
its observations in passes of 8 / chunks of 64 -- the D and n below sit on both sides of each of those boundaries.
Every value tolerance is the worst-case bound of the evaluation it checks (_glm.device_bounds)."""
import math

import numpy as np
import pytest

import _glm
from _tol import close

from oracle.pynuts import PyNUTS

pytestmark = pytest.mark.gpu

FAMILIES = ("bernoulli_logit", "poisson_log")
U = _glm.U


def _target(family, n, p, seed, intercept=True, prior_sd=None, scale=None):
    from smcnuts_amd import GLMTarget
    X, y = _glm.synthetic(family, n, p, seed, scale=scale)
    sd = np.linspace(0.8, 2.5, p + intercept) if prior_sd is None else prior_sd
    return GLMTarget(X, y, family=family, prior_sd=sd, intercept=intercept), _glm.GLMNumpy(X, y, family, sd, intercept)


def _points(model, rng, extreme):
    """Benign points, and (extreme) points whose linear predictor reaches |eta| ~ 800 (logistic) or exp's overflow
    and the values just below it (Poisson)."""
    D = model.dim
    x = rng.standard_normal((4, D)) * 0.5
    if extreme:
        i, j = np.unravel_index(int(np.argmax(np.abs(model.Z))), model.Z.shape)
        z = model.Z[i, j]                                  # eta_i = v at x = v / z e_j, and |eta_k| <= |v| elsewhere
        e = np.zeros((3, D))
        if model.family == "bernoulli_logit":
            e[0, j], e[1, j], e[2, j] = 800.0 / z, -800.0 / z, 40.0 / z
        else:
            e[0, j] = 720.0 / z                            # exp(eta_i) overflows: llik = -inf
            e[1, j] = 700.0 / z                            # large, finite
            e[2, j] = -700.0 / z
        x = np.vstack([x, e])
    return x


D_LIST = (1, 2, 8, 9, 16, 17, 32, 33, 63, 64)
N_LIST = (1, 7, 64, 65, 1000, 100003)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("D", D_LIST)
@pytest.mark.parametrize("n", N_LIST)
def test_values_against_exact_reference(family, D, n):
    """logpdf, logpdfgrad and logpdf_parts at phi in {0, 0.3, 1}, against math.fsum over the float64 terms."""
    intercept = D % 2 == 1                                # both layouts of the design row
    p = D - intercept
    t, m = _target(family, n, p, 1000 * D + n, intercept=intercept)
    assert t.dim == D
    rng = np.random.default_rng(D + n)
    x = _points(m, rng, extreme=n <= 1000)
    lpri, llik, gpri, glik = _glm.exact_parts(m, x)
    b_lpri, b_llik, b_glik = _glm.device_bounds(m, x)
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
        gb = phi * b_glik[fin] + 2 * U * (np.abs(gpri[fin]) + phi * np.abs(glik[fin]))
        assert np.all(np.abs(g[fin] - gw) <= gb), np.max(np.abs(g[fin] - gw) - gb)


class _PyNUTSDepth(PyNUTS):
    """PyNUTS recording the number of doublings of its tree (the depth the device reports)."""

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


TAPE_CASES = [(f, D, eps) for f in FAMILIES for D, eps in ((2, 0.01), (16, 0.01), (17, 0.01), (64, 0.02))]
TAPE_CASES[4] = ("poisson_log", 2, 0.001)      # (this posterior is 10x narrower: trees of 2^4-2^8 at this step)


@pytest.mark.parametrize("family,D,eps", TAPE_CASES)
def test_nuts_on_tapes_against_pynuts(family, D, eps):
    """NUTSProposal(GLMTarget).rvs on drawn tapes: draws consumed, leapfrogs and depth exact, x' and r' to 1e-12,
    against the reference-shaped NUTS over the numpy density (trees of up to 2^8-2^9 leapfrogs)."""
    from smcnuts_amd.proposal.nuts import NUTSProposal
    X, y = _glm.synthetic(family, 200, D - 1, D, scale=0.5)
    from smcnuts_amd import GLMTarget
    t = GLMTarget(X, y, family=family, prior_sd=2.0)
    m = _glm.GLMNumpy(X, y, family, 2.0)
    rng = np.random.default_rng(7 * D + len(family))
    N = 24
    x = rng.standard_normal((N, D)) * 0.1
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
    assert nleap.max() >= 63
    np.testing.assert_array_equal(st["ndraws"], ndraws)
    np.testing.assert_array_equal(st["nleap"], nleap)
    np.testing.assert_array_equal(st["depth"], depth)
    close(xn, want_x, rtol=1e-12, atol=1e-12)
    close(rn, want_r, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("family,D,eps", [("bernoulli_logit", 8, 0.05), ("poisson_log", 12, 0.02),
                                          ("bernoulli_logit", 25, 0.03), ("poisson_log", 40, 0.02)])
def test_philox_mode_against_host_target(family, D, eps):
    """Production RNG: the device-native target and HostTarget(numpy model) on the same seed and state -- the same
    momenta, trees and draws, x' and r' to round-off.  Any mismatch names its particles."""
    from smcnuts_amd import GLMTarget, HostTarget, _capi
    N, seed, it = 20000, 4242, 5
    X, y = _glm.synthetic(family, 300, D - 1, 11 * D, scale=0.5)
    t = GLMTarget(X, y, family=family, prior_sd=2.0)
    h = HostTarget(_glm.GLMNumpy(X, y, family, 2.0))
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
    assert mism.size == 0, f"particles {mism.tolist()} took a different tree (ndraws {s0['ndraws'][mism].tolist()} vs {s1['ndraws'][mism].tolist()})"
    assert l0 == l1 == int(s0["nleap"].sum())
    assert s0["nleap"].mean() >= 4
    close(x0, x1, rtol=1e-12, atol=1e-12)
    close(q0, q1, rtol=1e-12, atol=1e-12)


def _posterior_2d():
    rng = np.random.default_rng(2024)
    n = 50
    X = rng.standard_normal((n, 1))
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-(0.3 + 1.2 * X[:, 0])))).astype(np.float64)
    m = _glm.GLMNumpy(X, y, "bernoulli_logit", 2.5)
    # 2-D quadrature: the midpoint rule on a fine grid around the mode (mean ~1.7, sd ~0.5 in both coordinates; the
    # grid's edges carry weights below 1e-17)
    g0, g1 = np.linspace(-5.0, 8.5, 1201), np.linspace(-5.0, 8.5, 1201)
    B0, B1 = np.meshgrid(g0, g1, indexing="ij")
    pts = np.stack([B0.ravel(), B1.ravel()], axis=1)
    lp = np.concatenate([m.logpdf(pts[i:i + 100000]) for i in range(0, len(pts), 100000)])
    w = np.exp(lp - lp.max())
    w /= w.sum()
    mean = w @ pts
    var = w @ (pts - mean) ** 2
    W = w.reshape(1201, 1201)
    assert max(W[[0, -1], :].max(), W[:, [0, -1]].max()) < 1e-17     # (the mass left off the grid: far below the MC error)
    return X, y, mean, var


@pytest.mark.parametrize("lkernel,tempering", [("forwardsLKernel", False), ("GaussianApproxLKernel", True)])
def test_posterior_moments_against_quadrature(lkernel, tempering):
    """Logistic regression, intercept and one covariate, n = 50: SMCSampler's final estimates within 5 Monte-Carlo
    standard errors (from the run's ESS) of the quadrature mean and variance."""
    from smcnuts_amd import LogisticRegression, SMCSampler
    X, y, mean, var = _posterior_2d()
    smc = SMCSampler(K=20, N=65536, target=LogisticRegression(X, y, prior_sd=2.5), step_size=0.2, lkernel=lkernel,
                     tempering=tempering, seed=17)
    assert smc.device_resident == (not tempering)
    smc.sample(show_progress=False)
    ess = float(smc.ess[-1])
    assert ess > 1000
    mse = np.sqrt(var / ess)
    assert np.all(np.abs(smc.mean_estimate[-1] - mean) <= 5 * mse), (smc.mean_estimate[-1], mean, mse)
    # the variance estimate's standard error: sqrt(Var[(x - mu)^2] / ESS) <= sqrt(2) var / sqrt(ESS) for a near-Gaussian
    # posterior; 3 sqrt(2) var / sqrt(ESS) covers the skew of this one
    vse = 3 * math.sqrt(2.0) * var / math.sqrt(ess)
    assert np.all(np.abs(smc.variance_estimate[-1] - var) <= 5 * vse), (smc.variance_estimate[-1], var, vse)


LOOPS = [(lk, temp) for lk in ("forwardsLKernel", "GaussianApproxLKernel", "asymptoticLKernel") for temp in (False, True)]


@pytest.mark.parametrize("lkernel,tempering", LOOPS)
@pytest.mark.parametrize("D", [5, 20])
def test_full_loop_against_host_target(lkernel, tempering, D):
    """Every L-kernel, with and without tempering: the device-native target and the same model on the host give the
    same phi ladder and the same particles.  No divergent particle is tolerated."""
    from smcnuts_amd import GLMTarget, SMCSampler
    family = "bernoulli_logit" if D == 5 else "poisson_log"
    X, y = _glm.synthetic(family, 120, D - 1, 3 * D, scale=0.5)
    kw = dict(K=5, N=1024, step_size=0.05, seed=9, lkernel=lkernel, tempering=tempering)
    dev = SMCSampler(target=GLMTarget(X, y, family=family, prior_sd=2.0), **kw)
    dev.sample(show_progress=False)
    host = SMCSampler(target=_glm.GLMNumpy(X, y, family, 2.0), **kw)
    assert not host.device_resident
    host.sample(show_progress=False)
    np.testing.assert_array_equal(dev.leapfrogs, host.leapfrogs)
    assert list(dev.resampled) == list(host.resampled)
    close(dev.phi, host.phi, rtol=1e-12, atol=1e-15)
    close(dev.x_saved, host.x_saved, rtol=1e-10, atol=1e-11)
    close(dev.ess, host.ess, rtol=1e-10)
    close(dev.mean_estimate, host.mean_estimate, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("lkernel,tempering,D", [("forwardsLKernel", False, 6), ("GaussianApproxLKernel", True, 6),
                                                 ("forwardsLKernel", False, 30)])
def test_two_shards_equal_one_and_runs_repeat(lkernel, tempering, D):
    """Two InProcessComm shards make the run one shard makes, particle for particle; two runs with one seed are
    bit-identical."""
    from smcnuts_amd import GLMTarget, SMCSampler
    from tests.test_sharding import _run_shards
    X, y = _glm.synthetic("bernoulli_logit", 150, D - 1, D, scale=0.5)
    make_t = lambda: GLMTarget(X, y, prior_sd=2.0)
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

    def data(family, p, ic, y, X=None, s=1.0):
        D = p + ic
        X = np.zeros((n, p)) if X is None else X
        return np.concatenate([[family, n, p, ic], np.full(D, s), np.asarray(y, dtype=np.float64), X.reshape(-1)])

    cases = [
        (data(0, 65, 0, [0, 1, 0]), "D <= 64 coefficients; larger models run host-evaluated"),
        (data(0, 64, 1, [0, 1, 0]), "D <= 64 coefficients; larger models run host-evaluated"),
        (data(0, 2, 1, [0, 2, 1]), "bernoulli_logit needs y in {0, 1}"),
        (data(1, 2, 1, [0, -1, 1]), "poisson_log needs y in {0, 1, 2, ..}"),
        (data(1, 2, 1, [0, 0.5, 1]), "poisson_log needs y in {0, 1, 2, ..}"),
        (data(0, 2, 1, [0, 1, 0], s=0.0), "prior sds must be finite and > 0"),
        (data(0, 2, 1, [0, 1, 0], X=np.array([[0, 1], [np.inf, 0], [0, 0]])), "X must be finite"),
        (data(2, 2, 1, [0, 1, 0]), "family must be 0 (bernoulli_logit) or 1 (poisson_log)"),
        (data(0, 2, 1, [0, 1, 0])[:-1], "GLM target: data = [family, n, p, intercept"),
        (data(0, 0, 0, [0, 1, 0]), "no coefficients"),
    ]
    for md, msg in cases:
        with pytest.raises(_capi.SmcnError, match=None) as ei:
            _capi.Context(64, _capi.MODEL_GLM, md)
        assert msg in str(ei.value), (str(ei.value), msg)
    ok = _capi.Context(64, _capi.MODEL_GLM, data(1, 64, 0, [0, 3, 1]))
    assert ok.D == ok.Dc == 64
    ok.close()
