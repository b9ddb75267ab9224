"""The varying-intercept (hierarchical) GLM target on the device (HierarchicalGLM; GlmHierModel, one wavefront per
particle) against exact references and against the same model evaluated on the host (tests/_hglm.py's numpy density
through HostTarget / oracle/pynuts.PyNUTS).  Every value tolerance is the worst-case bound of the evaluation it checks
(_hglm.device_bounds)."""
import math

import numpy as np
import pytest

import _hglm as hg
from _tol import close

from oracle.pynuts import PyNUTS

pytestmark = pytest.mark.gpu

FAMILIES = hg.FAMILIES
U = hg.U
DISP = ("normal", "neg_binomial_2_log")


def _shape(family, D):
    """(p, intercept, J) with Dc + J + 1 (+ 1) = D: Dc = 0 at D = 4 for the dispersion families"""
    extra = 2 if family in DISP else 1
    if D == 4:
        return (0, 0, 4 - extra) if family in DISP else (0, 1, 4 - extra - 1)
    Dc = 5 if D == 17 else 10
    return Dc - 1, 1, D - Dc - extra


def _target(family, n, p, ic, J, seed, empty=(), group_sd=1.3, prior=(0.2, 1.5)):
    from smcnuts_amd import HierarchicalGLM
    X, y, g = hg.synthetic(family, n, p, J, seed, empty=empty)
    sd = np.linspace(0.8, 2.5, p + ic) if p + ic else 1.0
    kw = dict(dispersion_prior=prior) if family in DISP else {}
    t = HierarchicalGLM(X, y, g, family=family, prior_sd=sd, group_sd_prior=group_sd, intercept=bool(ic), n_groups=J,
                        **kw)
    return t, hg.HGLMNumpy(X, y, g, family, sd, group_sd, prior, bool(ic), n_groups=J)


def _points(m, rng):
    """Benign points, lt at both ends, e^2lt overflowing, and the dispersion coordinate's far values."""
    D = m.dim
    x = rng.standard_normal((4, D)) * 0.5
    e = rng.standard_normal((4, D)) * 0.5
    e[0, m.lt] = 300.0
    e[0, m.Dc:m.lt] *= math.exp(-300.0)
    e[1, m.lt] = -700.0
    e[2, m.lt] = 355.0                                   # e^2lt overflows: -inf
    e[3, m.lt] = -3.0
    if m.family == "normal":
        e[3, -1] = -360.0                                # e^-2 ld overflows
    elif m.family == "neg_binomial_2_log":
        e[3, -1] = math.log(1e8)                         # near-Poisson
    return np.vstack([x, e])


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("D", (4, 17, 64))
@pytest.mark.parametrize("n", (7, 1000, 20011))
def test_values_against_exact_reference(family, D, n):
    """logpdf, logpdfgrad and logpdf_parts at phi in {0, 0.3, 1}, against math.fsum over the float64 terms; one group
    left empty."""
    p, ic, J = _shape(family, D)
    t, m = _target(family, n, p, ic, J, 1000 * D + n + len(family), empty=(J - 1,) if J > 2 else ())
    assert t.dim == D
    x = _points(m, np.random.default_rng(D + n))
    lpri, llik, gpri, glik = hg.exact_parts(m, x)
    b_lpri, b_llik, b_glik = hg.device_bounds(m, x)
    a, b = t.logpdf_parts(x)
    finp = np.isfinite(lpri)
    assert np.all(a[~finp] == -np.inf)
    assert np.all(np.abs(a[finp] - lpri[finp]) <= b_lpri[finp]), (a[finp] - lpri[finp], b_lpri[finp])
    fin = np.isfinite(llik)
    assert np.array_equal(np.isfinite(b), fin), (b, llik)
    assert np.all(b[~fin] == -np.inf)
    assert np.all(np.abs(b[fin] - llik[fin]) <= b_llik[fin]), (b[fin] - llik[fin], b_llik[fin])
    fin = fin & finp
    assert fin.sum() >= 6
    for phi in (0.0, 0.3, 1.0):
        lp = t.logpdf(x, phi)
        g = t.logpdfgrad(x, phi)
        assert np.all(lp[~fin] == -np.inf) and np.all(g[~fin] == -np.inf)
        want = lpri[fin] + phi * llik[fin]
        bound = b_lpri[fin] + phi * b_llik[fin] + 2 * U * (np.abs(lpri[fin]) + phi * np.abs(llik[fin]))
        assert np.all(np.abs(lp[fin] - want) <= bound), (lp[fin] - want, bound)
        # (d / d lt of the prior cancels: its error is relative to e^2lt / s_tau^2)
        e2 = np.exp(np.minimum(2.0 * x[fin, m.lt], 700.0))[:, None] / m.s_tau ** 2
        gb_pri = 8 * U * (np.abs(gpri[fin]) + np.where(np.arange(D) == m.lt, 1.0 + e2, 0.0))
        gw = gpri[fin] + phi * glik[fin]
        gb = gb_pri + phi * b_glik[fin] + 2 * U * (np.abs(gpri[fin]) + phi * np.abs(glik[fin])) + 1e-300
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


def _start(m, rng, N):
    x = rng.standard_normal((N, m.dim)) * 0.3
    x[:, m.lt] = math.log(0.8) + 0.1 * rng.standard_normal(N)
    if m.disp:
        x[:, -1] = math.log(0.7 if m.family == "normal" else 3.0) + 0.1 * rng.standard_normal(N)
    return x


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("D,eps", ((4, 0.02), (17, 0.02)))
def test_nuts_on_tapes_against_pynuts(family, D, eps):
    """NUTSProposal(HierarchicalGLM).rvs on drawn tapes: draws, leapfrogs and depth exact, x' and r' to 1e-12, against
    the reference-shaped NUTS over the numpy density."""
    from smcnuts_amd.proposal.nuts import NUTSProposal
    p, ic, J = _shape(family, D)
    t, m = _target(family, 200, p, ic, J, 5 * D + len(family))
    rng = np.random.default_rng(7 * D + len(family))
    N = 16
    x = _start(m, rng, N)
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


@pytest.mark.parametrize("family,D,eps", [("bernoulli_logit", 25, 0.03), ("normal", 40, 0.02)])
def test_philox_mode_against_host_target(family, D, eps):
    """Production RNG: device-native target and HostTarget(numpy model), same seed and state: same momenta, trees and
    draws, x' and r' to round-off."""
    from smcnuts_amd import HostTarget, _capi
    N, seed, it = 2048, 4242, 5                           # (the numpy density is the slow side: N n per call)
    p, J = 5, D - 6 - (2 if family in DISP else 1)
    t, m = _target(family, 200, p, 1, J, 11 * D)
    h = HostTarget(m)
    x = _start(m, np.random.default_rng(D), N)
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


LOOPS = [("forwardsLKernel", False), ("GaussianApproxLKernel", True), ("asymptoticLKernel", False)]


@pytest.mark.parametrize("lkernel,tempering", LOOPS)
@pytest.mark.parametrize("family,p,J", [("poisson_log", 2, 5), ("normal", 3, 9)])
def test_full_loop_against_host_target(lkernel, tempering, family, p, J):
    """The device-resident loop (forwards, no tempering) and the host-driven loop: the same phi ladder, leapfrogs,
    resampling and particles as the numpy model through HostTarget; mean and variance estimates in constrained space
    (alpha = tau z, tau, sigma) alike."""
    from smcnuts_amd import SMCSampler
    t, m = _target(family, 120, p, 1, J, 3 * J, group_sd=1.0, prior=(0.0, 1.0))
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


@pytest.mark.parametrize("family", ("bernoulli_logit", "neg_binomial_2_log"))
@pytest.mark.parametrize("lkernel", ("forwardsLKernel", "GaussianApproxLKernel"))
def test_constrained_space(family, lkernel):
    """constrain() reports (b, tau z, tau [, phi]); mean_estimate / variance_estimate are the weighted moments of
    constrain(x) on the host, on the device-resident loop (forwards) and the host-driven one (Gaussian L-kernel)."""
    from smcnuts_amd import SMCSampler
    t, m = _target(family, 80, 2, 1, 4, 5, group_sd=1.0, prior=(0.0, 1.0))
    x = np.random.default_rng(1).standard_normal((300, m.dim))
    close(t.constrain(x), m.constrain(x), rtol=1e-15, atol=0.0)
    close(t.constrain(x[0]), m.constrain(x[0]), rtol=1e-15, atol=0.0)
    smc = SMCSampler(target=t, K=4, N=2048, step_size=0.05, seed=2, lkernel=lkernel)
    smc.sample(show_progress=False)
    assert smc.device_resident == (lkernel == "forwardsLKernel")
    # every generation: weighted moments of the numpy constrain() of the saved particles
    for k in range(smc.K + 1):
        lw = smc.logw_saved[k]
        w = np.exp(lw - lw.max())
        w /= w.sum()
        c = m.constrain(smc.x_saved[k])
        mean = w @ c
        var = w @ (c - mean) ** 2
        close(smc.mean_estimate[k], mean, rtol=1e-10, atol=1e-12)
        close(smc.variance_estimate[k], var, rtol=1e-8, atol=1e-12)
    assert np.all(smc.mean_estimate[:, m.lt] > 0.0)


def _quadrature():
    """Logistic regression, intercept only, J = 2 groups, n = 60: posterior mean and variance of (b_0, alpha_1,
    alpha_2, tau) by the midpoint rule on a 4-D grid over (b_0, z_1, z_2, lt), and a bound on the posterior mass the
    lt range [L, H] leaves out."""
    rng = np.random.default_rng(7)
    n, J = 60, 2
    g = np.arange(n) % J
    y = (rng.random(n) < np.where(g == 0, 0.35, 0.7)).astype(np.float64)
    s0, st = 1.5, 1.0
    k = np.array([y[g == j].sum() for j in range(J)])
    nj = np.array([(g == j).sum() for j in range(J)], dtype=np.float64)
    b0 = np.linspace(-9.0, 9.0, 73)
    zz = np.linspace(-8.0, 8.0, 57)
    L, H = -11.5, math.log(6.5)
    lt = np.linspace(L, H, 56)
    hb, hz, hl = b0[1] - b0[0], zz[1] - zz[0], lt[1] - lt[0]

    def sp(v):
        return np.maximum(v, 0.0) + np.log1p(np.exp(-np.abs(v)))

    def lgroup(eta, j):                                  # the group's log likelihood: constant eta within a group
        return k[j] * eta - nj[j] * sp(eta)
    B, Z1, Z2, LT = np.meshgrid(b0, zz, zz, lt, indexing="ij", sparse=True)
    tau = np.exp(LT)
    lp = (-0.5 * (B / s0) ** 2 - 0.5 * Z1 ** 2 - 0.5 * Z2 ** 2 + LT - 0.5 * tau ** 2 / st ** 2
          + lgroup(B + tau * Z1, 0) + lgroup(B + tau * Z2, 1))
    mx = lp.max()
    w = np.exp(lp - mx)
    Zint = w.sum() * hb * hz * hz * hl                   # the normaliser, relative to e^mx, of the same density
    for ax in range(3):                                  # b_0, z_1, z_2: the grid holds their tails
        edge = np.take(w, [0, -1], axis=ax).max()
        assert edge < 1e-10 * w.max(), (ax, edge / w.max())
    wn = w / w.sum()
    c = [np.broadcast_to(B, w.shape), tau * Z1, tau * Z2, np.broadcast_to(tau, w.shape)]
    mean = np.array([np.sum(wn * v) for v in c])
    var = np.array([np.sum(wn * (v - mean[i]) ** 2) for i, v in enumerate(c)])
    # mass outside lt in [L, H], relative to Zint.  Below L: lt's prior density is <= (2 / (st sqrt(2 pi))) e^lt and
    # the likelihood is at most that at alpha = 0 times e^(n_j tau |z_j|) (|d loglik / d eta| <= 1 per observation), so
    # with E e^(c |z|) <= 2 e^(c^2 / 2) the mass is <= (2 / (st sqrt(2 pi))) e^L * G0 * prod_j 2 e^((n_j e^L)^2 / 2),
    # G0 = int N(b_0; 0, s0^2) lik(b_0, alpha = 0) db_0.  Above H: the prior mass of tau > e^H times the largest
    # likelihood any (b_0, alpha) reaches (each group at its own best constant eta).
    bb = np.linspace(-12.0, 12.0, 24001)
    g0 = np.sum(np.exp(-0.5 * (bb / s0) ** 2 + lgroup(bb, 0) + lgroup(bb, 1) - mx)) * (bb[1] - bb[0]) \
        / (s0 * math.sqrt(2 * math.pi))
    low = 2.0 / (st * math.sqrt(2 * math.pi)) * math.exp(L) * g0 * np.prod(2.0 * np.exp(0.5 * (nj * math.exp(L)) ** 2))
    ph = k / nj
    lmax = np.sum(k * np.log(ph) + (nj - k) * np.log1p(-ph))
    high = math.erfc(math.exp(H) / (st * math.sqrt(2.0))) * st * math.sqrt(math.pi / 2.0) * math.exp(lmax - mx) \
        * (2 * math.pi) ** 1.5 * s0
    # (the prior's normalising constants on both sides: the grid density above leaves out 1 / (s0 (2 pi)^(3/2)) and
    #  the half-normal's 2 / (st sqrt(2 pi)); low and high carry them relative to it)
    trunc = (low * (2 * math.pi) ** 1.5 * s0 / (2.0 / (st * math.sqrt(2 * math.pi))) + high) / Zint
    # (and the rule's own error at the lower end, where the density has not decayed: half a cell of its last row)
    trunc += 0.5 * w[..., 0].sum() / w.sum()
    return y, g, mean, var, trunc


@pytest.mark.parametrize("lkernel,tempering", [("forwardsLKernel", False), ("GaussianApproxLKernel", True)])
def test_posterior_moments_against_quadrature(lkernel, tempering):
    """Varying-intercept logistic regression, J = 2, no covariate, n = 60: SMCSampler's final estimates of (b_0,
    alpha_1, alpha_2, tau) within 5 Monte-Carlo standard errors (from the run's ESS) of the quadrature mean and
    variance, whose lt truncation is bounded."""
    from smcnuts_amd import HierarchicalGLM, SMCSampler
    y, g, mean, var, trunc = _quadrature()
    assert trunc < 1e-4, trunc
    t = HierarchicalGLM(np.zeros((len(y), 0)), y, g, family="bernoulli_logit", prior_sd=1.5, group_sd_prior=1.0)
    smc = SMCSampler(K=20, N=65536, target=t, step_size=0.05, lkernel=lkernel, tempering=tempering, seed=17)
    smc.sample(show_progress=False)
    ess = float(smc.ess[-1])
    assert ess > 1000
    slack = trunc * (np.abs(mean) + var + 1.0) * 10
    mse = np.sqrt(var / ess)
    assert np.all(np.abs(smc.mean_estimate[-1] - mean) <= 5 * mse + slack), (smc.mean_estimate[-1], mean, mse)
    # (tau and the alphas are skewed: 4 sqrt(2) var / sqrt(ESS) covers the standard error of the variance estimate)
    vse = 4 * math.sqrt(2.0) * var / math.sqrt(ess)
    assert np.all(np.abs(smc.variance_estimate[-1] - var) <= 5 * vse + slack), (smc.variance_estimate[-1], var, vse)


@pytest.mark.parametrize("family,lkernel,tempering,p,J", [("bernoulli_logit", "forwardsLKernel", False, 3, 8),
                                                          ("neg_binomial_2_log", "GaussianApproxLKernel", True, 4, 20)])
def test_two_shards_equal_one_and_runs_repeat(family, lkernel, tempering, p, J):
    from smcnuts_amd import SMCSampler
    from tests.test_sharding import _run_shards
    make_t = lambda: _target(family, 150, p, 1, J, J, group_sd=1.0, prior=(0.0, 1.0))[0]
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
    """What HierarchicalGLM refuses in Python, the library refuses at context creation with a message of its own."""
    from smcnuts_amd import _capi
    n = 3

    def data(family, p, ic, J, y, g=(0, 0, 0), X=None, s=1.0, st=1.0, md=0.0, sd=1.0):
        Dc = p + ic
        X = np.zeros((n, p)) if X is None else X
        return np.concatenate([[family, n, p, ic, J], np.full(Dc, s), [st], [md, sd] if family >= 2 else [],
                               np.asarray(y, dtype=np.float64), np.asarray(g, dtype=np.float64), X.reshape(-1)])

    cases = [
        (data(0, 2, 1, 0, [0, 1, 0]), "J must be an integer >= 1"),
        (data(0, 2, 1, 2.5, [0, 1, 0]), "J must be an integer >= 1"),
        (data(0, 2, 1, 2, [0, 1, 0], g=(0, 2, 1)), "every group index g must be an integer in [0, J)"),
        (data(0, 2, 1, 2, [0, 1, 0], g=(0, -1, 1)), "every group index g must be an integer in [0, J)"),
        (data(0, 2, 1, 2, [0, 1, 0], g=(0, 0.5, 1)), "every group index g must be an integer in [0, J)"),
        (data(1, 2, 1, 2, [0, 1, 0], g=(0, np.nan, 1)), "every group index g must be an integer in [0, J)"),
        (data(0, 2, 1, 61, [0, 1, 0]), "D = Dc + J + 1 (+ 1) <= 64 coordinates; larger models run host-evaluated"),
        (data(3, 2, 1, 60, [0, 1, 0]), "D = Dc + J + 1 (+ 1) <= 64 coordinates; larger models run host-evaluated"),
        (data(0, 2, 1, 2, [0, 1, 0], st=0.0), "s_tau must be finite and > 0"),
        (data(0, 2, 1, 2, [0, 1, 0], st=np.inf), "s_tau must be finite and > 0"),
        (data(2, 2, 1, 2, [0, 1, 0], md=np.nan), "m_d must be finite"),
        (data(3, 2, 1, 2, [0, 1, 0], sd=-1.0), "s_d must be finite and > 0"),
        (data(0, 2, 1, 2, [0, 2, 0]), "bernoulli_logit needs y in {0, 1}"),
        (data(1, 2, 1, 2, [0, 1.5, 0]), "poisson_log needs y in {0, 1, 2, ..}"),
        (data(2, 2, 1, 2, [0, np.inf, 0]), "normal needs finite y"),
        (data(3, 2, 1, 2, [0, -1, 0]), "neg_binomial_2_log needs y in {0, 1, 2, .., 2^53}"),
        (data(0, 2, 1, 2, [0, 1, 0], s=0.0), "prior sds must be finite and > 0"),
        (data(0, 2, 1, 2, [0, 1, 0], X=np.array([[0, 1], [np.nan, 0], [0, 0]])), "X must be finite"),
        (data(0, 2, 1, 2, [0, 1, 0])[:-1], "hierarchical GLM target: data = [family, n, p, intercept, J"),
        (data(4, 2, 1, 2, [0, 1, 0]), "family must be 0 (bernoulli_logit), 1 (poisson_log), 2 (normal) or 3"),
        (data(0, 2, 2, 2, [0, 1, 0]), "intercept must be 0 or 1"),
        (data(0, 2, 1, 2, [0, 1, 0])[:4], "hierarchical GLM target: data = "),
    ]
    for md, msg in cases:
        with pytest.raises(_capi.SmcnError) as ei:
            _capi.Context(64, _capi.MODEL_HGLM, md)
        assert msg in str(ei.value), (str(ei.value), msg)
    for fam, p, ic, J in ((0, 2, 1, 60), (3, 0, 0, 62), (1, 0, 0, 1)):
        ok = _capi.Context(64, _capi.MODEL_HGLM, data(fam, p, ic, J, [0, 3, 1] if fam else [0, 1, 1], g=(0, 0, J - 1)))
        assert ok.D == ok.Dc == p + ic + J + 1 + (fam >= 2)
        ok.close()
