"""The multilevel GLM target on the device (MultilevelGLM; GlmMultiModel, one wavefront per particle) against exact
references, against HierarchicalGLM where the two models coincide, and against the same model evaluated on the host
(tests/_mlglm.py's numpy density through HostTarget / oracle/pynuts.PyNUTS).  Every value tolerance is the worst-case
bound of the evaluation it checks (_mlglm.device_bounds).  The shapes are the smallest at which the functor can go
wrong: D = 2 and D = 64, an odd Dc (the pad column live), two terms on one factor, four terms, a level without
observations and a term with z = 0, n = 1 and either side of the 64-row chunk."""
import math

import numpy as np
import pytest

import _hglm as hg
import _mlglm as ml
import _summary as S
from _tol import close
from test_gpu_hglm import LOOPS, _PyNUTSDepth

pytestmark = pytest.mark.gpu

FAMILIES = ml.FAMILIES
U = ml.U
DISP = ("normal", "neg_binomial_2_log")
# layout: (Dc, [(J, factor)], dispersion, empty (term, level), zero term)
LAYOUTS = {1: (0, [(1, 0)], False, None, None),
           2: (1, [(3, 0), (3, 0)], False, (0, 2), 1),
           3: (3, [(1, 0), (5, 1), (2, 2), (3, 3)], True, (1, 4), 3),
           4: (5, [(18, 0), (18, 0), (20, 1)], False, (2, 19), 1),
           5: (4, [(18, 0), (18, 0), (20, 1)], True, (2, 19), 1)}
DIMS = {1: 2, 2: 9, 3: 19, 4: 64, 5: 64}


def _target(family, n, layout, seed, group_sd=None, prior=(0.2, 1.5)):
    """MultilevelGLM and its numpy model on layout's (Dc, J) -- the dispersion coordinate follows `family`"""
    from smcnuts_amd import MultilevelGLM
    Dc, terms, _, empty, zero = LAYOUTS[layout]
    ic = 1 if Dc else 0
    p = Dc - ic
    X, y, tm = ml.synthetic(family, n, p, terms, seed, intercept=bool(ic), empty=empty, zero=zero)
    sd = np.linspace(0.8, 2.5, Dc) if Dc else 1.0
    st = np.linspace(1.3, 0.7, len(terms)) if group_sd is None else group_sd
    kw = dict(dispersion_prior=prior) if family in DISP else {}
    t = MultilevelGLM(X, y, tm, family=family, prior_sd=sd, group_sd_prior=st, intercept=bool(ic), **kw)
    return t, ml.MLGLMNumpy(X, y, tm, family, sd, st, prior, bool(ic))


def _points(m, rng):
    """Benign points; each lt_r in turn at 300 (u scaled by e^-300), -700 and 355 (e^2lt overflows); the dispersion
    coordinate's far values."""
    D = m.dim
    x = rng.standard_normal((4, D)) * 0.5
    e = rng.standard_normal((3 * m.R + 1, D)) * 0.5
    inf = np.zeros(len(e), dtype=bool)
    for r in range(m.R):
        e[3 * r, m.lt0 + r] = 300.0
        e[3 * r, m.u_slice(r)] *= math.exp(-300.0)
        e[3 * r + 1, m.lt0 + r] = -700.0
        e[3 * r + 2, m.lt0 + r] = 355.0
        inf[3 * r + 2] = True
    e[-1, m.lt0] = -3.0
    if m.family == "normal":
        e[-1, -1] = -360.0                               # e^-2 ld overflows
    elif m.family == "neg_binomial_2_log":
        e[-1, -1] = math.log(1e8)                        # near-Poisson
    return np.vstack([x, e]), np.concatenate([np.zeros(4, dtype=bool), inf])


def _check_values(t, m, x, lt_inf):
    D = m.dim
    lpri, llik, gpri, glik = ml.exact_parts(m, x)
    b_lpri, b_llik, b_glik = ml.device_bounds(m, x)
    a, b = t.logpdf_parts(x)
    finp = np.isfinite(lpri)
    assert np.array_equal(~finp, lt_inf)
    assert np.all(a[~finp] == -np.inf) and np.all(b[~finp] == -np.inf)
    assert np.all(np.abs(a[finp] - lpri[finp]) <= b_lpri[finp]), (a[finp] - lpri[finp], b_lpri[finp])
    fin = np.isfinite(llik)
    assert np.array_equal(np.isfinite(b), fin), (b, llik)
    assert np.all(b[~fin] == -np.inf)
    assert np.all(np.abs(b[fin] - llik[fin]) <= b_llik[fin]), (b[fin] - llik[fin], b_llik[fin])
    fin = fin & finp
    assert fin.sum() >= 6
    lts = np.arange(m.lt0, m.lt0 + m.R)
    for phi in (0.0, 0.3, 1.0):
        lp = t.logpdf(x, phi)
        g = t.logpdfgrad(x, phi)
        assert np.all(lp[~fin] == -np.inf) and np.all(g[~fin] == -np.inf)
        want = lpri[fin] + phi * llik[fin]
        bound = b_lpri[fin] + phi * b_llik[fin] + 2 * U * (np.abs(lpri[fin]) + phi * np.abs(llik[fin]))
        assert np.all(np.abs(lp[fin] - want) <= bound), (lp[fin] - want, bound)
        # (d / d lt_r of the prior cancels: its error is relative to e^2lt_r / s_tau_r^2)
        pad = np.zeros((int(fin.sum()), D))
        pad[:, lts] = 1.0 + np.exp(np.minimum(2.0 * x[fin][:, lts], 700.0)) / m.s_tau ** 2
        gb_pri = 8 * U * (np.abs(gpri[fin]) + pad)
        gw = gpri[fin] + phi * glik[fin]
        gb = gb_pri + phi * b_glik[fin] + 2 * U * (np.abs(gpri[fin]) + phi * np.abs(glik[fin])) + 1e-300
        assert np.all(np.abs(g[fin] - gw) <= gb), np.max(np.abs(g[fin] - gw) - gb)
    return fin, t.logpdfgrad(x, 0.0), t.logpdfgrad(x, 1.0)


@pytest.mark.parametrize("n", (1, 7, 64, 65, 130))
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_values_against_exact_reference(layout, n):
    """logpdf, logpdfgrad and logpdf_parts at phi in {0, 0.3, 1}, against math.fsum over the float64 terms, for both
    families of the layout (with or without the dispersion coordinate); a level without observations and a term with
    z = 0 keep the prior's gradient alone."""
    Dc, terms, disp, empty, zero = LAYOUTS[layout]
    for family in (DISP if disp else ("bernoulli_logit", "poisson_log")):
        t, m = _target(family, n, layout, 1000 * layout + n + len(family))
        assert t.dim == m.dim == DIMS[layout] and m.Dc == Dc
        x, lt_inf = _points(m, np.random.default_rng(layout + n))
        fin, g0, g1 = _check_values(t, m, x, lt_inf)      # (the device's gradient at phi = 0: its prior's)
        if zero is not None:
            cols = list(range(*m.u_slice(zero).indices(m.dim))) + [m.lt0 + zero]
            assert np.all(m.z[zero] == 0.0)
            np.testing.assert_array_equal(g1[fin][:, cols], g0[fin][:, cols])
        if empty is not None:
            r, j = empty
            assert not np.any(m.g[r] == j)
            np.testing.assert_array_equal(g1[fin][:, m.off[r] + j], g0[fin][:, m.off[r] + j])


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("n,p,J", [(1, 0, 1), (65, 2, 5), (130, 4, 58)])
def test_one_intercept_term_against_hierarchical_glm(family, n, p, J):
    """R = 1, z = 1 is HierarchicalGLM's density: the two device functors on the same data and points, within the sum of
    their bounds."""
    from smcnuts_amd import HierarchicalGLM, MultilevelGLM
    if family in DISP and J == 58:
        J = 57                                            # (D = 64 with the dispersion coordinate)
    X, y, g = hg.synthetic(family, n, p, J, 7 * n + J, empty=(J - 1,) if J > 2 else ())
    sd = np.linspace(0.8, 2.5, p + 1)
    kw = dict(dispersion_prior=(0.2, 1.5)) if family in DISP else {}
    th = HierarchicalGLM(X, y, g, family=family, prior_sd=sd, group_sd_prior=1.3, n_groups=J, **kw)
    tm = MultilevelGLM(X, y, [(g, None, J)], family=family, prior_sd=sd, group_sd_prior=1.3, **kw)
    mh = hg.HGLMNumpy(X, y, g, family, sd, 1.3, (0.2, 1.5), True, n_groups=J)
    mm = ml.MLGLMNumpy(X, y, [(g, None, J)], family, sd, 1.3, (0.2, 1.5), True)
    assert th.dim == tm.dim == mm.dim
    x, _ = _points(mm, np.random.default_rng(n + J))
    bh, bm = hg.device_bounds(mh, x), ml.device_bounds(mm, x)
    ph, pm = th.logpdf_parts(x), tm.logpdf_parts(x)
    for k in range(2):
        fin = np.isfinite(ph[k])
        assert np.array_equal(np.isfinite(pm[k]), fin) and np.all(pm[k][~fin] == ph[k][~fin])
        assert np.all(np.abs(pm[k][fin] - ph[k][fin]) <= bh[k][fin] + bm[k][fin])
    fin = np.isfinite(ph[0]) & np.isfinite(ph[1])
    assert fin.sum() >= 6
    # (each prior gradient within 8 u of its magnitude, d / d lt relative to 1 + e^2lt / s_tau^2, as in the value test)
    gpri = np.abs(mh.prior_terms(x)[1][fin])
    gpri[:, mh.lt] += 1.0 + np.exp(np.minimum(2.0 * x[fin, mh.lt], 700.0)) / mh.s_tau ** 2
    for phi in (0.0, 1.0):
        gh, gm = th.logpdfgrad(x, phi), tm.logpdfgrad(x, phi)
        assert np.all(gm[~fin] == -np.inf) and np.all(gh[~fin] == -np.inf)
        slack = 16 * U * gpri + 4 * U * np.abs(gh[fin])
        assert np.all(np.abs(gm[fin] - gh[fin]) <= phi * (bh[2][fin] + bm[2][fin]) + slack + 1e-300)


def _start(m, rng, N):
    x = rng.standard_normal((N, m.dim)) * 0.3
    x[:, m.lt0:m.lt0 + m.R] = math.log(0.8) + 0.1 * rng.standard_normal((N, m.R))
    if m.disp:
        x[:, -1] = math.log(0.7 if m.family == "normal" else 3.0) + 0.1 * rng.standard_normal(N)
    return x


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("layout,eps", ((2, 0.02), (3, 0.02)))
def test_nuts_on_tapes_against_pynuts(family, layout, eps):
    """NUTSProposal(MultilevelGLM).rvs on drawn tapes: draws, leapfrogs and depth exact, x' and r' to 1e-12, against
    the reference-shaped NUTS over the numpy density."""
    from smcnuts_amd.proposal.nuts import NUTSProposal
    t, m = _target(family, 200, layout, 5 * layout + len(family))
    D = m.dim
    rng = np.random.default_rng(7 * layout + len(family))
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


@pytest.mark.parametrize("family,layout,eps", [("bernoulli_logit", 4, 0.03), ("normal", 3, 0.02)])
def test_philox_mode_against_host_target(family, layout, eps):
    """Production RNG: device-native target and HostTarget(numpy model), same seed and state: same momenta bit for bit,
    same trees for every particle, x' and r' to round-off."""
    from smcnuts_amd import HostTarget, _capi
    N, seed, it = 512, 4242, 5
    t, m = _target(family, 200, layout, 11 * layout)
    h = HostTarget(m)
    x = _start(m, np.random.default_rng(layout), N)
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


@pytest.mark.parametrize("lkernel,tempering", LOOPS)
@pytest.mark.parametrize("family", ("poisson_log", "normal"))
def test_full_loop_against_host_target(lkernel, tempering, family):
    """The device-resident loop (forwards, no tempering) and the host-driven loop: the same phi ladder, leapfrogs,
    resampling and particles as the numpy model through HostTarget; mean and variance estimates in constrained space
    (tau_r u_rj, tau_r, sigma) alike."""
    from smcnuts_amd import SMCSampler
    t, m = _target(family, 90, 3, 17, group_sd=1.0, prior=(0.0, 1.0))
    kw = dict(K=4, N=512, step_size=0.05, seed=9, lkernel=lkernel, tempering=tempering)
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


@pytest.mark.parametrize("family,layout", (("bernoulli_logit", 2), ("neg_binomial_2_log", 3)))
@pytest.mark.parametrize("lkernel", ("forwardsLKernel", "GaussianApproxLKernel"))
def test_constrained_space(family, layout, lkernel):
    """constrain() (smcn_target_constrain) reports (b, tau_r u_rj .., tau_1..tau_R [, phi]); mean_estimate /
    variance_estimate are the weighted moments and summary() the weighted quantiles of the numpy constrain() of the
    particles, on the device-resident loop (forwards) and the host-driven one (Gaussian L-kernel)."""
    from smcnuts_amd import SMCSampler
    t, m = _target(family, 80, layout, 5, group_sd=1.0, prior=(0.0, 1.0))
    x = np.random.default_rng(1).standard_normal((300, m.dim))
    close(t.constrain(x), m.constrain(x), rtol=1e-15, atol=0.0)
    close(t.constrain(x[0]), m.constrain(x[0]), rtol=1e-15, atol=0.0)
    assert t.param_names() == m.param_names()
    # uploaded points: the quantiles of the device's own constrain(x), exactly
    lw = 3.0 * np.random.default_rng(2).standard_normal(300)
    s = t.summary(x, lw, at=0.0)
    S.check(s.quantiles, t.constrain(x), lw, S.DEFAULT, True, "quantiles of constrain(x)", got_cdf=s.cdf, at=s.at)
    smc = SMCSampler(target=t, K=3, N=1024, step_size=0.05, seed=2, lkernel=lkernel)
    smc.sample(show_progress=False)
    assert smc.device_resident == (lkernel == "forwardsLKernel")
    for k in range(smc.K + 1):            # every generation: weighted moments of the numpy constrain() of the particles
        lwk = smc.logw_saved[k]
        w = np.exp(lwk - lwk.max())
        w /= w.sum()
        c = m.constrain(smc.x_saved[k])
        mean = w @ c
        var = w @ (c - mean) ** 2
        close(smc.mean_estimate[k], mean, rtol=1e-10, atol=1e-12)
        close(smc.variance_estimate[k], var, rtol=1e-8, atol=1e-12)
    assert np.all(smc.mean_estimate[:, m.lt0:m.lt0 + m.R] > 0.0)
    s = smc.summary(at=0.0)
    S.check(s.quantiles, t.constrain(smc.x_saved[-1]), smc.logw_saved[-1], S.DEFAULT, False, "resident summary",
            got_cdf=s.cdf, at=s.at)
    np.testing.assert_array_equal(s.mean, smc.mean_estimate[smc.K])
    np.testing.assert_array_equal(s.sd, np.sqrt(smc.variance_estimate[smc.K]))
    assert s.names == t.param_names()


@pytest.mark.parametrize("family,lkernel,tempering,layout", [("bernoulli_logit", "forwardsLKernel", False, 2),
                                                             ("neg_binomial_2_log", "GaussianApproxLKernel", True, 3)])
def test_two_shards_equal_one_and_runs_repeat(family, lkernel, tempering, layout):
    from smcnuts_amd import SMCSampler
    from tests.test_sharding import _run_shards
    make_t = lambda: _target(family, 150, layout, layout, group_sd=1.0, prior=(0.0, 1.0))[0]
    kw = dict(K=3, N=1024, step_size=0.05, seed=3, lkernel=lkernel, tempering=tempering, wide_eval=False)
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
    """What MultilevelGLM refuses in Python, the library refuses at context creation with a message of its own; the
    pointwise criteria and held-out prediction keep their scope."""
    from smcnuts_amd import _capi
    n = 3

    def data(family, p, ic, Js, y, g=(0, 0, 0), z=(1.0, 0.5, -2.0), X=None, s=1.0, st=1.0, md=0.0, sd=1.0, R=None):
        Dc = p + ic
        X = np.zeros((n, p)) if X is None else X
        R = len(Js) if R is None else R
        gz = [np.asarray(v, dtype=np.float64) for _ in range(len(Js)) for v in (g, z)]
        return np.concatenate([[family, n, p, ic, R], list(Js) + [0] * (4 - len(Js)), np.full(Dc, s),
                               np.full(len(Js), st), [md, sd] if family >= 2 else [], np.asarray(y, dtype=np.float64)]
                              + gz + [X.reshape(-1)])

    too_big = "D = Dc + J_1 + .. + J_R + R (+ 1) <= 64 coordinates; larger models run host-evaluated"
    cases = [
        (data(0, 2, 1, (2,), [0, 1, 0], R=0), "R must be an integer in [1, 4]"),
        (data(0, 2, 1, (2,), [0, 1, 0], R=5), "R must be an integer in [1, 4]"),
        (data(0, 2, 1, (2,), [0, 1, 0], R=1.5), "R must be an integer in [1, 4]"),
        (data(0, 2, 1, (0,), [0, 1, 0]), "J_r must be an integer >= 1"),
        (data(0, 2, 1, (2, 2.5), [0, 1, 0]), "J_r must be an integer >= 1"),
        (data(0, 2, 1, (2, 2), [0, 1, 0], R=1), "J_r must be an integer >= 1 (the levels of term r) for r <= R and 0 beyond R"),
        (data(0, 2, 1, (2,), [0, 1, 0], g=(0, 2, 1)), "every group index g_r must be an integer in [0, J_r)"),
        (data(0, 2, 1, (2, 2), [0, 1, 0], g=(0, -1, 1)), "every group index g_r must be an integer in [0, J_r)"),
        (data(1, 2, 1, (2,), [0, 1, 0], g=(0, np.nan, 1)), "every group index g_r must be an integer in [0, J_r)"),
        (data(0, 2, 1, (2,), [0, 1, 0], z=(0.0, np.inf, 1.0)), "z must be finite"),
        (data(0, 2, 1, (30, 30), [0, 1, 0]), too_big),
        (data(3, 2, 1, (19, 19, 20), [0, 1, 0]), too_big),
        (data(0, 2, 1, (2,), [0, 1, 0], st=0.0), "s_tau must be finite and > 0"),
        (data(0, 2, 1, (2, 3), [0, 1, 0], st=np.inf), "s_tau must be finite and > 0"),
        (data(2, 2, 1, (2,), [0, 1, 0], md=np.nan), "m_d must be finite"),
        (data(3, 2, 1, (2,), [0, 1, 0], sd=-1.0), "s_d must be finite and > 0"),
        (data(0, 2, 1, (2,), [0, 2, 0]), "bernoulli_logit needs y in {0, 1}"),
        (data(1, 2, 1, (2,), [0, 1.5, 0]), "poisson_log needs y in {0, 1, 2, ..}"),
        (data(2, 2, 1, (2,), [0, np.inf, 0]), "normal needs finite y"),
        (data(3, 2, 1, (2,), [0, -1, 0]), "neg_binomial_2_log needs y in {0, 1, 2, .., 2^53}"),
        (data(0, 2, 1, (2,), [0, 1, 0], s=0.0), "prior sds must be finite and > 0"),
        (data(0, 2, 1, (2,), [0, 1, 0], X=np.array([[0, 1], [np.nan, 0], [0, 0]])), "X must be finite"),
        (data(0, 2, 1, (2,), [0, 1, 0])[:-1], "multilevel GLM target: data = [family, n, p, intercept, R, J_1"),
        (data(4, 2, 1, (2,), [0, 1, 0]), "family must be 0 (bernoulli_logit), 1 (poisson_log), 2 (normal) or 3"),
        (data(0, 2, 2, (2,), [0, 1, 0]), "intercept must be 0 or 1"),
        (data(0, 2, 1, (2,), [0, 1, 0])[:8], "multilevel GLM target: data = "),
    ]
    for md, msg in cases:
        with pytest.raises(_capi.SmcnError) as ei:
            _capi.Context(64, _capi.MODEL_MLGLM, md)
        assert "smcn_ctx_create: multilevel GLM target: " in str(ei.value), str(ei.value)
        assert msg in str(ei.value), (str(ei.value), msg)
    for fam, p, ic, Js in ((0, 2, 1, (29, 30)), (3, 0, 0, (20, 20, 10, 9)), (1, 0, 0, (1,))):
        ok = _capi.Context(64, _capi.MODEL_MLGLM, data(fam, p, ic, Js, [0, 3, 1] if fam else [0, 1, 1],
                                                       g=(0, 0, min(Js) - 1)))
        assert ok.D == ok.Dc == p + ic + sum(Js) + len(Js) + (fam >= 2)
        with pytest.raises(_capi.SmcnError, match="smcn_pointwise_dims: pointwise criteria cover the SMCN_MODEL_GLM "
                                                  "families"):
            ok.pointwise_dims()
        with pytest.raises(_capi.SmcnError, match="held-out prediction covers the regression targets"):
            ok.predict_set_data(np.array([fam, 1.0, p, ic, len(Js)] + [0.0] * 8), False)
        ok.close()
