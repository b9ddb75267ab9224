"""The categorical regression target on the device (CategoricalRegression; GlmCatModel, 8 lanes per particle up to
D = 8, one wavefront per particle above) against exact references and against the same model evaluated on the host
(tests/_cat.py's numpy density through HostTarget / oracle/pynuts.PyNUTS).  Every value tolerance is the worst-case
bound of the evaluation it checks (_cat.device_bounds)."""
import math

import numpy as np
import pytest

import _cat as ct
import _glm as gl
from _tol import close

from oracle.pynuts import PyNUTS

pytestmark = pytest.mark.gpu

U = ct.U
# D -> (K, p): both sides of the 8 / 9 boundary between the two shapes, K = 2 with Dc = 17, D = 64, K = 16
SHAPES = {2: (3, 0), 8: (3, 3), 9: (4, 2), 17: (2, 16), 64: (5, 15), 60: (16, 3)}


def _target(K, n, p, seed, scale=0.7):
    from smcnuts_amd import CategoricalRegression
    X, y = ct.synthetic(K, n, p, seed, scale=scale)
    sd = np.linspace(0.8, 2.5, p + 1)
    return CategoricalRegression(X, y, n_classes=K, prior_sd=sd), ct.CategoricalNumpy(X, y, n_classes=K, prior_sd=sd)


def _check_values(t, m, x):
    lpri, llik, gpri, glik = ct.exact_parts(m, x)
    b_lpri, b_llik, b_glik = ct.device_bounds(m, x)
    a, b = t.logpdf_parts(x)
    assert np.all(np.abs(a - lpri) <= b_lpri), (a - lpri, b_lpri)
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
        gb = 8 * U * np.abs(gpri[fin]) + phi * b_glik[fin] + 2 * U * (np.abs(gpri[fin]) + phi * np.abs(glik[fin])) \
            + 1e-300
        assert np.all(np.abs(g[fin] - gw) <= gb), np.max(np.abs(g[fin] - gw) - gb)
    return fin


@pytest.mark.parametrize("D", sorted(SHAPES))
@pytest.mark.parametrize("n", (7, 1000, 20011))
def test_values_against_exact_reference(D, n):
    """logpdf, logpdfgrad and logpdf_parts at phi in {0, 0.3, 1}, against math.fsum over the float64 terms: benign
    points, logits at +-800, ties and a dominating class."""
    K, p = SHAPES[D]
    t, m = _target(K, n, p, 1000 * D + n)
    assert t.dim == D
    x = ct.points(m, np.random.default_rng(D + n))
    fin = _check_values(t, m, x)
    assert fin.all()                                    # (every finite x: a finite density)


@pytest.mark.parametrize("D", (8, 24))
def test_overflowing_logits_give_minus_inf(D):
    """X b overflowing in one row: llik, logpdf and the gradient are -inf, in both shapes; the point beside it is finite."""
    K, p = (3, 3) if D == 8 else (5, 5)
    t0, m0 = _target(K, 40, p, 3)
    X = m0.Z[:, 1:].copy()
    X[:, 0] = np.clip(X[:, 0], -0.5, 0.5)
    X[5, 0] = 1e300
    from smcnuts_amd import CategoricalRegression
    t = CategoricalRegression(X, m0.y, n_classes=K, prior_sd=2.0)
    m = ct.CategoricalNumpy(X, m0.y, n_classes=K, prior_sd=2.0)
    x = np.zeros((3, D))
    x[0, 1] = 1e10                                       # class 1's beta_1: eta_5,1 = 1e310
    x[1, D - p] = -1e10                                  # the last class's: -1e310 (the largest logit stays finite)
    x[2, 1] = 1e-300                                     # finite
    lp = t.logpdf(x)
    want = m.logpdf(x)
    assert lp[0] == -np.inf and want[0] == -np.inf
    assert np.all(t.logpdfgrad(x)[0] == -np.inf)
    assert np.isfinite(lp[2])
    assert np.isfinite(lp[1]) == np.isfinite(want[1])
    if np.isfinite(want[1]):
        close(lp[1], want[1], rtol=1e-12)
    _check_values(t, m, x[2:])


@pytest.mark.parametrize("D", (8, 24))
@pytest.mark.parametrize("M", (1, 7, 64, 65, 1000, 100003))
def test_particle_counts(D, M):
    """Batches of every size against the numpy density, within twice the device's bound (numpy's own sums are
    within the same)."""
    K, p = (3, 3) if D == 8 else (5, 5)
    t, m = _target(K, 50, p, 7 * D)
    x = np.random.default_rng(M).standard_normal((M, D)) * 0.6
    a, b = t.logpdf_parts(x)
    lpri, llik, gpri, glik = m.parts(x)
    b_lpri, b_llik, b_glik = ct.device_bounds(m, x)
    assert np.all(np.abs(a - lpri) <= 2 * b_lpri)
    assert np.all(np.abs(b - llik) <= 2 * b_llik)
    g = t.logpdfgrad(x)
    gb = 2 * (8 * U * np.abs(gpri) + b_glik + 2 * U * (np.abs(gpri) + np.abs(glik)))
    assert np.all(np.abs(g - (gpri + glik)) <= gb)


@pytest.mark.parametrize("p", (3, 16))
def test_two_classes_on_the_device_are_logistic_regression(p):
    """K = 2 against LogisticRegression on the device (the 8-lane and the wavefront shape), within both bounds."""
    from smcnuts_amd import CategoricalRegression, LogisticRegression
    X, y = ct.synthetic(2, 300, p, 11 + p)
    tc = CategoricalRegression(X, y, prior_sd=1.5)
    tl = LogisticRegression(X, y.astype(np.float64), prior_sd=1.5)
    mc = ct.CategoricalNumpy(X, y, prior_sd=1.5)
    ml = gl.GLMNumpy(X, y.astype(np.float64), "bernoulli_logit", prior_sd=1.5)
    x = np.random.default_rng(p).standard_normal((9, p + 1))
    x[-1] *= 300.0
    a1, b1 = tc.logpdf_parts(x)
    a2, b2 = tl.logpdf_parts(x)
    bc, bl = ct.device_bounds(mc, x), gl.device_bounds(ml, x)
    assert np.all(np.abs(a1 - a2) <= bc[0] + bl[0])
    assert np.all(np.abs(b1 - b2) <= bc[1] + bl[1])
    g1, g2 = tc.logpdfgrad(x), tl.logpdfgrad(x)
    gpri = -x / mc.s ** 2
    assert np.all(np.abs(g1 - g2) <= bc[2] + bl[2] + 32 * U * np.abs(gpri) + 4 * U * np.abs(g2) + 1e-300)


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


@pytest.mark.parametrize("K,p,eps", ((3, 3, 0.03), (5, 5, 0.03)))
def test_nuts_on_tapes_against_pynuts(K, p, eps):
    """NUTSProposal(CategoricalRegression).rvs on drawn tapes (D = 8: 8 lanes; D = 24: a wavefront): draws, leapfrogs
    and depth exact, x' and r' to 1e-12, against the reference-shaped NUTS over the numpy density."""
    from smcnuts_amd.proposal.nuts import NUTSProposal
    t, m = _target(K, 200, p, 5 * K + p)
    D = t.dim
    rng = np.random.default_rng(7 * D)
    N = 16
    x = rng.standard_normal((N, D)) * 0.3
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
    assert nleap.max() >= 7
    np.testing.assert_array_equal(st["ndraws"], ndraws)
    np.testing.assert_array_equal(st["nleap"], nleap)
    np.testing.assert_array_equal(st["depth"], depth)
    close(xn, want_x, rtol=1e-12, atol=1e-12)
    close(rn, want_r, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("K,p,eps", ((3, 3, 0.05), (5, 5, 0.04)))
def test_philox_mode_against_host_target(K, p, eps):
    """Production RNG: device-native target and HostTarget(numpy model), same seed and state: same momenta, trees and
    draws, x' and r' to round-off."""
    from smcnuts_amd import HostTarget, _capi
    N, seed, it = 2048, 4242, 5
    t, m = _target(K, 200, p, 11 * K)
    h = HostTarget(m)
    x = np.random.default_rng(K).standard_normal((N, t.dim)) * 0.3
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


LOOPS = [("forwardsLKernel", False), ("forwardsLKernel", True), ("GaussianApproxLKernel", False),
         ("GaussianApproxLKernel", True), ("asymptoticLKernel", False), ("asymptoticLKernel", True)]


@pytest.mark.parametrize("lkernel,tempering,K,p", [lt + (3, 2) for lt in LOOPS] + [("forwardsLKernel", False, 4, 4)])
def test_full_loop_against_host_target(lkernel, tempering, K, p):
    """The device-resident loop (forwards, no tempering) and the host-driven loop: the same phi ladder, leapfrogs,
    resampling and particles as the numpy model through HostTarget; mean and variance estimates alike."""
    from smcnuts_amd import SMCSampler
    t, m = _target(K, 120, p, 3 * K + p)
    kw = dict(K=5, N=1024, step_size=0.05, seed=9, lkernel=lkernel, tempering=tempering)
    dev = SMCSampler(target=t, **kw)
    assert dev.device_resident == (lkernel == "forwardsLKernel" and not tempering)
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


@pytest.mark.parametrize("lkernel", ("forwardsLKernel", "GaussianApproxLKernel"))
@pytest.mark.parametrize("K,p", [(3, 2), (5, 5)])
def test_constrained_space_is_the_identity(lkernel, K, p):
    """constrain() returns x; mean_estimate / variance_estimate are the weighted moments of x itself, on the
    device-resident loop (forwards) and the host-driven one (Gaussian L-kernel)."""
    from smcnuts_amd import SMCSampler
    t, m = _target(K, 80, p, 5)
    x = np.random.default_rng(1).standard_normal((300, m.dim))
    np.testing.assert_array_equal(t.constrain(x), x)
    np.testing.assert_array_equal(t.constrain(x[0]), x[0])
    smc = SMCSampler(target=t, K=4, N=2048, step_size=0.05, seed=2, lkernel=lkernel)
    smc.sample(show_progress=False)
    assert smc.device_resident == (lkernel == "forwardsLKernel")
    for k in range(smc.K + 1):
        lw = smc.logw_saved[k]
        w = np.exp(lw - lw.max())
        w /= w.sum()
        c = smc.x_saved[k]
        mean = w @ c
        var = w @ (c - mean) ** 2
        close(smc.mean_estimate[k], mean, rtol=1e-10, atol=1e-12)
        close(smc.variance_estimate[k], var, rtol=1e-8, atol=1e-12)


def _quadrature():
    """K = 3, intercept only, n = 50: posterior mean and variance of (b_1, b_2) by the midpoint rule on a 2-D grid."""
    rng = np.random.default_rng(7)
    n, s = 50, 2.0
    y = rng.choice(3, size=n, p=[0.5, 0.3, 0.2])
    c = np.array([(y == k).sum() for k in range(3)], dtype=np.float64)
    g = np.linspace(-9.0, 7.0, 1601)
    B1, B2 = np.meshgrid(g, g, indexing="ij")
    lse = np.logaddexp(0.0, np.logaddexp(B1, B2))
    lp = -0.5 * (B1 / s) ** 2 - 0.5 * (B2 / s) ** 2 + c[1] * B1 + c[2] * B2 - n * lse
    w = np.exp(lp - lp.max())
    for ax in range(2):
        edge = np.take(w, [0, -1], axis=ax).max()
        assert edge < 1e-12 * w.max(), (ax, edge)
    w /= w.sum()
    mean = np.array([np.sum(w * B1), np.sum(w * B2)])
    var = np.array([np.sum(w * (B1 - mean[0]) ** 2), np.sum(w * (B2 - mean[1]) ** 2)])
    return y, s, mean, var


@pytest.mark.parametrize("lkernel,tempering", [("forwardsLKernel", False), ("GaussianApproxLKernel", True)])
def test_posterior_moments_against_quadrature(lkernel, tempering):
    """Categorical regression, K = 3, no covariate, n = 50 (D = 2): SMCSampler's final estimates of (b_1, b_2) within
    5 Monte-Carlo standard errors (from the run's ESS) of the quadrature mean and variance."""
    from smcnuts_amd import CategoricalRegression, SMCSampler
    y, s, mean, var = _quadrature()
    t = CategoricalRegression(np.zeros((len(y), 0)), y, n_classes=3, prior_sd=s)
    smc = SMCSampler(K=20, N=65536, target=t, step_size=0.1, lkernel=lkernel, tempering=tempering, seed=17)
    smc.sample(show_progress=False)
    ess = float(smc.ess[-1])
    assert ess > 1000
    mse = np.sqrt(var / ess)
    assert np.all(np.abs(smc.mean_estimate[-1] - mean) <= 5 * mse), (smc.mean_estimate[-1], mean, mse)
    vse = 4 * math.sqrt(2.0) * var / math.sqrt(ess)
    assert np.all(np.abs(smc.variance_estimate[-1] - var) <= 5 * vse), (smc.variance_estimate[-1], var, vse)


@pytest.mark.parametrize("K,p,lkernel,tempering", [(3, 3, "forwardsLKernel", False),
                                                   (6, 3, "GaussianApproxLKernel", True)])
def test_two_shards_equal_one_and_runs_repeat(K, p, lkernel, tempering):
    from smcnuts_amd import SMCSampler
    from tests.test_sharding import _run_shards
    make_t = lambda: _target(K, 150, p, K)[0]
    kw = dict(K=4, N=2048, step_size=0.05, seed=3, lkernel=lkernel, tempering=tempering, wide_eval=False)
    one = SMCSampler(target=make_t(), **kw)
    one.sample(show_progress=False)
    again = SMCSampler(target=make_t(), **kw)
    again.sample(show_progress=False)
    np.testing.assert_array_equal(again.x_saved, one.x_saved)
    np.testing.assert_array_equal(again.logw_saved, one.logw_saved)
    np.testing.assert_array_equal(again.phi, one.phi)
    np.testing.assert_array_equal(again.mean_estimate, one.mean_estimate)
    sh = _run_shards(lambda c: SMCSampler(target=make_t(), comm=c, **kw), 2, lambda s: s.sample(show_progress=False),
                     device=True)
    for s in sh:
        assert list(s.resampled) == list(one.resampled)
        close(s.phi, one.phi, rtol=1e-12, atol=1e-15)
        close(s.ess, one.ess, rtol=1e-11)
        close(s.mean_estimate, one.mean_estimate, rtol=1e-10, atol=1e-13)
        close(s.variance_estimate, one.variance_estimate, rtol=1e-9, atol=1e-13)
    close(np.concatenate([s.x_saved for s in sh], axis=1), one.x_saved, rtol=1e-10, atol=1e-13)
    assert sum(int(s.leapfrogs.sum()) for s in sh) == int(one.leapfrogs.sum())


def test_creation_errors():
    """What CategoricalRegression refuses in Python, the library refuses at context creation with a message of its
    own."""
    from smcnuts_amd import _capi
    n = 3

    def data(K, p, ic, y, X=None, s=1.0):
        D = (int(K) - 1) * (p + ic) if np.isfinite(K) and K == int(K) and K >= 2 else p + ic
        X = np.zeros((n, p)) if X is None else X
        return np.concatenate([[K, n, p, ic], np.full(D, s), np.asarray(y, dtype=np.float64), X.reshape(-1)])

    cases = [
        (data(1, 2, 1, [0, 0, 0]), "K must be an integer in [2, 16]"),
        (data(17, 2, 1, [0, 1, 0]), "K must be an integer in [2, 16]"),
        (data(2.5, 2, 1, [0, 1, 0]), "K must be an integer in [2, 16]"),
        (data(np.nan, 2, 1, [0, 1, 0]), "K must be an integer in [2, 16]"),
        (data(3, 2, 1, [0, 3, 0]), "every label y must be an integer in [0, K)"),
        (data(3, 2, 1, [0, -1, 0]), "every label y must be an integer in [0, K)"),
        (data(3, 2, 1, [0, 0.5, 0]), "every label y must be an integer in [0, K)"),
        (data(3, 2, 1, [0, np.nan, 0]), "every label y must be an integer in [0, K)"),
        (data(3, 2, 1, [0, 1, 0], s=0.0), "prior sds must be finite and > 0"),
        (data(3, 2, 1, [0, 1, 0], s=np.inf), "prior sds must be finite and > 0"),
        (data(3, 2, 1, [0, 1, 0], X=np.array([[0, 1], [np.nan, 0], [0, 0]])), "X must be finite"),
        (data(3, 32, 1, [0, 1, 0]), "D = (K - 1) (p + intercept) <= 64 coefficients; larger models run host-evaluated"),
        (data(16, 4, 1, [0, 1, 0]), "D = (K - 1) (p + intercept) <= 64 coefficients; larger models run host-evaluated"),
        (data(3, 0, 0, [0, 1, 0]), "no coefficients"),
        (data(3, 2, 2, [0, 1, 0]), "intercept must be 0 or 1"),
        (data(3, 2, 1, [0, 1, 0])[:-1], "categorical target: data = [K, n, p, intercept, s_1..s_D"),
        (data(3, 2, 1, [0, 1, 0])[:3], "categorical target: data = "),
    ]
    for md, msg in cases:
        with pytest.raises(_capi.SmcnError) as ei:
            _capi.Context(64, _capi.MODEL_CATEGORICAL, md)
        assert msg in str(ei.value), (str(ei.value), msg)
    for K, p, ic in ((2, 0, 1), (16, 3, 1), (3, 31, 1), (9, 8, 0)):
        ok = _capi.Context(64, _capi.MODEL_CATEGORICAL, data(K, p, ic, [0, K - 1, 1]))
        assert ok.D == ok.Dc == (K - 1) * (p + ic)
        ok.close()
