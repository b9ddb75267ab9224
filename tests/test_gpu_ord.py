"""The ordinal regression target on the device (OrdinalRegression; GlmOrdModel, 8 lanes per particle up to D = 8, one
wavefront per particle above) against exact references and against the same model evaluated on the host
(tests/_ord.py's numpy density through HostTarget / oracle/pynuts.PyNUTS).  Every value tolerance is the worst-case
bound of the evaluation it checks (_ord.device_bounds)."""
import math

import numpy as np
import pytest

import _glm as gl
import _ord as od
from _tol import close

from oracle.pynuts import PyNUTS

pytestmark = pytest.mark.gpu

U = od.U
# name -> (K, p): both sides of the 8 / 9 boundary between the two shapes, D = 64, and K = 65 without columns
SHAPES = {"D3": (3, 1), "D8": (5, 4), "D9": (4, 6), "D30": (6, 25), "D64": (5, 60), "K65": (65, 0)}


def _target(K, n, p, seed, scale=0.7):
    from smcnuts_amd import OrdinalRegression
    X, y = od.synthetic(K, n, p, seed, scale=scale)
    y[:min(K, n)] = np.arange(min(K, n))                 # (the end classes and the middle ones occur)
    sd = np.linspace(0.8, 2.5, p)
    t = np.linspace(2.0, 6.0, K - 1)
    return (OrdinalRegression(X, y, n_classes=K, prior_sd=sd, cutpoint_prior_sd=t),
            od.OrdinalNumpy(X, y, n_classes=K, prior_sd=sd, cutpoint_prior_sd=t))


def _check_values(t, m, x):
    lpri, llik, gpri, glik = od.exact_parts(m, x)
    b_lpri, b_llik, b_gpri, b_glik = od.device_bounds(m, x)
    a, b = t.logpdf_parts(x)
    fin_p = np.isfinite(lpri)
    assert np.array_equal(np.isfinite(a), fin_p), (a, lpri)
    assert np.all(a[~fin_p] == -np.inf)
    assert np.all(np.abs(a[fin_p] - lpri[fin_p]) <= b_lpri[fin_p]), (a - lpri, b_lpri)
    fin = np.isfinite(llik) & fin_p
    assert np.array_equal(np.isfinite(b), np.isfinite(llik)), (b, llik)
    assert np.all(b[~np.isfinite(llik)] == -np.inf)
    assert np.all(np.abs(b[fin] - llik[fin]) <= b_llik[fin]), (b[fin] - llik[fin], b_llik[fin])
    for phi in (0.0, 0.3, 1.0):
        lp = t.logpdf(x, phi)
        g = t.logpdfgrad(x, phi)
        assert np.all(lp[~fin] == -np.inf) and np.all(g[~fin] == -np.inf)
        want = lpri[fin] + phi * llik[fin]
        bound = b_lpri[fin] + phi * b_llik[fin] + 2 * U * (np.abs(lpri[fin]) + phi * np.abs(llik[fin]))
        assert np.all(np.abs(lp[fin] - want) <= bound), (lp[fin] - want, bound)
        gw = gpri[fin] + phi * glik[fin]
        gb = b_gpri[fin] + phi * b_glik[fin] + 2 * U * (np.abs(gpri[fin]) + phi * np.abs(glik[fin])) + 1e-300
        assert np.all(np.abs(g[fin] - gw) <= gb), np.max(np.abs(g[fin] - gw) - gb)
    return fin


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("n", (7, 1000, 20011))
def test_values_against_exact_reference(shape, n):
    """logpdf, logpdfgrad and logpdf_parts at phi in {0, 0.3, 1}, against math.fsum over the float64 terms: benign
    points, |eta| near 800, cutpoints at +-800, gaps of e^-700 between cutpoints, spread cutpoints."""
    K, p = SHAPES[shape]
    t, m = _target(K, n, p, 1000 * K + 10 * p + n)
    assert t.dim == p + K - 1
    x = od.points(m, np.random.default_rng(K + p + n))
    fin = _check_values(t, m, x)
    assert fin.all()                                    # (every finite x here: a finite density)


@pytest.mark.parametrize("K,p", ((3, 3), (5, 20)))
def test_non_finite_rules(K, p):
    """-inf (lpri, llik, logpdf, gradient) once e^u overflows or a cutpoint overflows; llik = -inf once X b overflows;
    collapsed middle cutpoints (e^u = 0) give a finite value; in both shapes."""
    from smcnuts_amd import OrdinalRegression
    _, m0 = _target(K, 40, p, 3)
    X = np.clip(m0.X, -0.5, 0.5)
    X[5, 0] = 1e300
    t = OrdinalRegression(X, m0.y, n_classes=K)
    m = od.OrdinalNumpy(X, m0.y, n_classes=K)
    D = t.dim
    x = np.zeros((6, D))
    x[0, p + 1] = 710.0                                  # e^u_2 overflows
    x[1, p + 1:] = 709.7                                 # c_{K-1} = (K - 2) e^709.7 overflows
    x[2, 0] = 1e10                                       # eta_5 = 1e310
    x[3, p + 1:] = -800.0                                # e^u = 0: collapsed middle classes (observed)
    x[4, p + 1:] = -700.0
    x[5, 1] = 1e-300
    if K == 3:
        x[1, p + 1] = 710.0
    a, b = t.logpdf_parts(x)
    lp, g = t.logpdf(x), t.logpdfgrad(x)
    for i in (0, 1):
        assert a[i] == -np.inf and b[i] == -np.inf and lp[i] == -np.inf and np.all(g[i] == -np.inf), i
    assert np.isfinite(a[2]) and b[2] == -np.inf and lp[2] == -np.inf and np.all(g[2] == -np.inf)
    assert np.all(np.isfinite(lp[3:])) and np.all(np.isfinite(g[3:]))
    assert np.all(m.counts[1:K - 1] > 0)
    close(b[3], m.parts(x[3])[1][0], rtol=1e-12)
    _check_values(t, m, x[3:])


@pytest.mark.parametrize("K,p", ((3, 3), (5, 5)))
@pytest.mark.parametrize("M", (1, 7, 64, 65, 1000, 100003))
def test_particle_counts(K, p, M):
    """Batches of every size against the numpy density, within twice the device's bound (numpy's own sums are within
    the same)."""
    t, m = _target(K, 50, p, 7 * K + p)
    x = np.random.default_rng(M).standard_normal((M, t.dim)) * 0.6
    a, b = t.logpdf_parts(x)
    lpri, llik, gpri, glik = m.parts(x)
    b_lpri, b_llik, b_gpri, b_glik = od.device_bounds(m, x)
    assert np.all(np.abs(a - lpri) <= 2 * b_lpri)
    assert np.all(np.abs(b - llik) <= 2 * b_llik)
    g = t.logpdfgrad(x)
    gb = 2 * (b_gpri + b_glik + 2 * U * (np.abs(gpri) + np.abs(glik)))
    assert np.all(np.abs(g - (gpri + glik)) <= gb)


@pytest.mark.parametrize("p", (3, 16))
def test_two_classes_on_the_device_are_logistic_regression(p):
    """K = 2 at (b, u_1) against LogisticRegression on the device at (-u_1, b) (the 8-lane and the wavefront shape),
    within both bounds."""
    from smcnuts_amd import LogisticRegression, OrdinalRegression
    X, y = od.synthetic(2, 300, p, 11 + p)
    to = OrdinalRegression(X, y, prior_sd=1.5, cutpoint_prior_sd=2.0)
    tl = LogisticRegression(X, y.astype(np.float64), prior_sd=np.array([2.0] + [1.5] * p))
    mo = od.OrdinalNumpy(X, y, prior_sd=1.5, cutpoint_prior_sd=2.0)
    ml = gl.GLMNumpy(X, y.astype(np.float64), "bernoulli_logit", prior_sd=np.array([2.0] + [1.5] * p))
    x = np.random.default_rng(p).standard_normal((9, p + 1))
    x[-1] *= 300.0
    xl = np.concatenate([-x[:, p:], x[:, :p]], axis=1)
    a1, b1 = to.logpdf_parts(x)
    a2, b2 = tl.logpdf_parts(xl)
    bo, bl = od.device_bounds(mo, x), gl.device_bounds(ml, xl)
    assert np.all(np.abs(a1 - a2) <= bo[0] + bl[0])
    assert np.all(np.abs(b1 - b2) <= bo[1] + bl[1])
    g1, g2 = to.logpdfgrad(x), tl.logpdfgrad(xl)
    g2 = np.concatenate([g2[:, 1:], -g2[:, :1]], axis=1)
    gpri = np.concatenate([-x[:, :p] / 1.5 ** 2, -x[:, p:] / 2.0 ** 2], axis=1)
    assert np.all(np.abs(g1 - g2) <= bo[2] + bo[3] + np.concatenate([bl[2][:, 1:], bl[2][:, :1]], axis=1)
                  + 32 * U * np.abs(gpri) + 4 * U * np.abs(g2) + 1e-300)


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
    """NUTSProposal(OrdinalRegression).rvs on drawn tapes (D = 5: 8 lanes; D = 9: a wavefront): draws, leapfrogs and
    depth exact, x' and r' to 1e-12, against the reference-shaped NUTS over the numpy density."""
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


@pytest.mark.parametrize("lkernel,tempering,K,p", [lt + (3, 2) for lt in LOOPS] + [("forwardsLKernel", False, 5, 6)])
def test_full_loop_against_host_target(lkernel, tempering, K, p):
    """The device-resident loop (forwards, no tempering) and the host-driven loop: the same phi ladder, leapfrogs,
    resampling and particles as the numpy model through HostTarget; mean and variance estimates (of the cutpoints) alike."""
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
@pytest.mark.parametrize("K,p", [(3, 2), (6, 5)])
def test_constrained_space(lkernel, K, p):
    """constrain() reports (b, c_1..c_{K-1}), strictly increasing; mean_estimate / variance_estimate are the weighted
    moments of constrain(x_saved), on the device-resident loop (forwards) and the host-driven one (Gaussian L-kernel)."""
    from smcnuts_amd import SMCSampler
    t, m = _target(K, 80, p, 5)
    x = np.random.default_rng(1).standard_normal((300, m.dim)) * 2.0
    c = t.constrain(x)
    # (the same running sum; the increments' exp within an ulp on either side)
    e_c = (np.arange(1, K) + 2) * 2 * U * np.cumsum(np.abs(m.increments(x)), axis=1)
    np.testing.assert_array_equal(c[:, :p], m.constrain(x)[:, :p])
    assert np.all(np.abs(c[:, p:] - m.constrain(x)[:, p:]) <= e_c)
    np.testing.assert_array_equal(t.constrain(x[0]), c[0])
    np.testing.assert_array_equal(c[:, :p], x[:, :p])
    assert np.all(np.diff(c[:, p:], axis=1) > 0.0)
    smc = SMCSampler(target=t, K=4, N=2048, step_size=0.05, seed=2, lkernel=lkernel)
    smc.sample(show_progress=False)
    assert smc.device_resident == (lkernel == "forwardsLKernel")
    for k in range(smc.K + 1):
        lw = smc.logw_saved[k]
        w = np.exp(lw - lw.max())
        w /= w.sum()
        cs = m.constrain(smc.x_saved[k])
        mean = w @ cs
        var = w @ (cs - mean) ** 2
        close(smc.mean_estimate[k], mean, rtol=1e-10, atol=1e-12)
        close(smc.variance_estimate[k], var, rtol=1e-8, atol=1e-12)


def _quadrature():
    """K = 3, no covariate, n = 50: posterior mean and variance of (c_1, c_2) by the midpoint rule on a 2-D grid over
    c_1 < c_2 (the ordered restriction; the density vanishes on the diagonal where class 1 is observed)."""
    rng = np.random.default_rng(7)
    n, s = 50, 3.0
    y = rng.choice(3, size=n, p=[0.4, 0.35, 0.25])
    cnt = np.array([(y == k).sum() for k in range(3)], dtype=np.float64)
    g = np.linspace(-5.0, 5.0, 2001)
    C1, C2 = np.meshgrid(g, g, indexing="ij")
    with np.errstate(divide="ignore", invalid="ignore"):
        lp = -0.5 * (C1 / s) ** 2 - 0.5 * (C2 / s) ** 2 \
            + cnt[0] * -np.logaddexp(0.0, -C1) \
            + cnt[1] * (np.log(np.abs(1.0 / (1.0 + np.exp(C1)) - 1.0 / (1.0 + np.exp(C2))))) \
            + cnt[2] * -np.logaddexp(0.0, C2)
    lp = np.where(C1 < C2, lp, -np.inf)
    w = np.exp(lp - lp.max())
    for ax in range(2):
        edge = np.take(w, [0, -1], axis=ax).max()
        assert edge < 1e-12 * w.max(), (ax, edge)
    w /= w.sum()
    mean = np.array([np.sum(w * C1), np.sum(w * C2)])
    var = np.array([np.sum(w * (C1 - mean[0]) ** 2), np.sum(w * (C2 - mean[1]) ** 2)])
    return y, s, mean, var


@pytest.mark.parametrize("lkernel,tempering", [("forwardsLKernel", False), ("GaussianApproxLKernel", True)])
def test_posterior_moments_against_quadrature(lkernel, tempering):
    """Ordinal regression, K = 3, no covariate, n = 50 (D = 2): SMCSampler's final estimates of (c_1, c_2) within 5
    Monte-Carlo standard errors (from the run's ESS) of the quadrature mean and variance."""
    from smcnuts_amd import OrdinalRegression, SMCSampler
    y, s, mean, var = _quadrature()
    t = OrdinalRegression(np.zeros((len(y), 0)), y, n_classes=3, cutpoint_prior_sd=s)
    smc = SMCSampler(K=20, N=65536, target=t, step_size=0.1, lkernel=lkernel, tempering=tempering, seed=17)
    smc.sample(show_progress=False)
    ess = float(smc.ess[-1])
    assert ess > 1000
    mse = np.sqrt(var / ess)
    assert np.all(np.abs(smc.mean_estimate[-1] - mean) <= 5 * mse), (smc.mean_estimate[-1], mean, mse)
    vse = 4 * math.sqrt(2.0) * var / math.sqrt(ess)
    assert np.all(np.abs(smc.variance_estimate[-1] - var) <= 5 * vse), (smc.variance_estimate[-1], var, vse)


@pytest.mark.parametrize("K,p,lkernel,tempering", [(3, 3, "forwardsLKernel", False),
                                                   (6, 5, "GaussianApproxLKernel", True)])
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
    """What OrdinalRegression refuses in Python, the library refuses at context creation with a message of its own."""
    from smcnuts_amd import _capi
    n = 3

    def data(K, p, y, X=None, s=1.0, t=2.0):
        Km1 = int(K) - 1 if np.isfinite(K) and K == int(K) and K >= 2 else 1
        X = np.zeros((n, p)) if X is None else X
        return np.concatenate([[K, n, p], np.full(p, s), np.full(Km1, t), np.asarray(y, dtype=np.float64),
                               X.reshape(-1)])

    cases = [
        (data(1, 2, [0, 0, 0]), "K must be an integer >= 2"),
        (data(2.5, 2, [0, 1, 0]), "K must be an integer >= 2"),
        (data(np.nan, 2, [0, 1, 0]), "K must be an integer >= 2"),
        (data(3, 2, [0, 3, 0]), "every label y must be an integer in [0, K)"),
        (data(3, 2, [0, -1, 0]), "every label y must be an integer in [0, K)"),
        (data(3, 2, [0, 0.5, 0]), "every label y must be an integer in [0, K)"),
        (data(3, 2, [0, np.nan, 0]), "every label y must be an integer in [0, K)"),
        (data(3, 2, [0, 1, 0], s=0.0), "prior sds (s for the coefficients, t for the cutpoints) must be finite and > 0"),
        (data(3, 2, [0, 1, 0], t=np.inf), "prior sds (s for the coefficients, t for the cutpoints) must be finite"),
        (data(3, 2, [0, 1, 0], X=np.array([[0, 1], [np.nan, 0], [0, 0]])), "X must be finite"),
        (data(3, 63, [0, 1, 0]), "D = p + K - 1 <= 64 coordinates; larger models run host-evaluated"),
        (data(66, 0, [0, 1, 0]), "D = p + K - 1 <= 64 coordinates; larger models run host-evaluated"),
        (data(3, 2, [0, 1, 0])[:-1], "ordinal target: data = [K, n, p, s_1..s_p, t_1..t_{K-1}"),
        (data(3, 2, [0, 1, 0])[:2], "ordinal target: data = "),
    ]
    bad_n = data(3, 2, [0, 1, 0])
    bad_n[1] = 0.0
    cases.append((bad_n, "n must be an integer >= 1"))
    bad_p = data(3, 2, [0, 1, 0])
    bad_p[2] = -1.0
    cases.append((bad_p, "p must be an integer >= 0"))
    for md, msg in cases:
        with pytest.raises(_capi.SmcnError) as ei:
            _capi.Context(64, _capi.MODEL_ORDINAL, md)
        assert msg in str(ei.value), (str(ei.value), msg)
    for K, p in ((2, 0), (2, 63), (65, 0), (5, 4), (6, 10)):
        ok = _capi.Context(64, _capi.MODEL_ORDINAL, data(K, p, [0, K - 1, 1]))
        assert ok.D == ok.Dc == p + K - 1
        ok.close()
