"""GLMTarget with offsets and weights on the device (SMCN_MODEL_OGLM) against the exact references of tests/_glm_ow.py,
against today's GLMTarget kernels through the model's identities, and against the same model evaluated on the host
(HostTarget / oracle/pynuts.PyNUTS over the numpy density).

Shapes: the functors group 8 lanes per particle for D <= 16 (families 0, 1) / D <= 8 (families 2, 3, D counting tau) and
a whole wavefront above, and take their observations in passes of 8 / chunks of 64 -- the D and n below sit on both sides
of each of those boundaries.  Every value tolerance is the worst-case bound of the evaluation it checks
(_glm_ow.device_bounds)."""
import math

import numpy as np
import pytest

import _glm
import _glm_disp as gd
import _glm_ow as ow
import _pointwise as pw
import _predict as pr
import _predict_draws as dr
import _psis as ps
from _tol import close

from oracle.pynuts import PyNUTS

gpu = pytest.mark.gpu
U = _glm.U
DISP_PRIOR = (0.2, 1.5)
N_LIST = (1, 7, 8, 9, 63, 64, 65, 129)
# D: the ends of the range and each dispatch boundary with its successor (D counts tau for the dispersion families)
D_OF = {f: (1, 2, 16, 17, 63, 64) for f in ow.CANONICAL}
D_OF.update({f: (2, 8, 9, 63, 64) for f in gd.DISP_FAMILIES})
VALUE_CASES = [(f, fl, D) for f in ow.FAMILIES for fl in (1, 2, 3) for D in D_OF[f]]


def _shape(family, D, intercept=None):
    """(p, intercept) of a model with D coordinates; both layouts of the design row by D's parity unless told"""
    Dc = D - (1 if family in gd.DISP_FAMILIES else 0)
    ic = (Dc % 2 == 1) if intercept is None else intercept
    return Dc - ic, bool(ic)


def _target(family, n, D, seed, flags, prior_sd=None, scale=0.5, intercept=None, data=None):
    """(GLMTarget, numpy model) with offsets / weights by `flags`"""
    from smcnuts_amd import GLMTarget
    p, ic = _shape(family, D, intercept)
    X, y, o, w = ow.synthetic(family, n, p, seed, scale=scale, flags=flags) if data is None else data
    sd = np.linspace(0.8, 2.5, p + ic) if prior_sd is None else prior_sd
    kw = dict(dispersion_prior=DISP_PRIOR) if family in gd.DISP_FAMILIES else {}
    t = GLMTarget(X, y, family=family, prior_sd=sd, intercept=ic, offset=o, weights=w, **kw)
    assert t.dim == D
    return t, ow.GLMOWNumpy(X, y, family, sd, ic, DISP_PRIOR, o, w)


def _points(m, rng, extreme):
    from test_gpu_glm import _points as canon
    from test_gpu_glm_disp import _points as disp
    return (disp if m.disp else canon)(m, rng, extreme)


def _assert_values(t, m, x, what):
    """logpdf_parts, logpdf and logpdfgrad at phi in {0, 0.3, 1} within device_bounds; -inf exactly where the reference
    has it"""
    lpri, llik, gpri, glik = ow.exact_parts(m, x)
    b_lpri, b_llik, b_glik = ow.device_bounds(m, x)
    a, b = t.logpdf_parts(x)
    assert np.all(np.abs(a - lpri) <= b_lpri), (what, a - lpri, b_lpri)      # (each particle to its own bound)
    close(a, lpri, rtol=0.0, atol=b_lpri.max() + 1e-300)
    fin = np.isfinite(llik)
    assert np.array_equal(np.isfinite(b), fin), (what, b, llik)
    assert np.all(b[~fin] == -np.inf), what
    err = np.abs(b[fin] - llik[fin])
    print(f"{what}: llik error / bound {np.max(err / np.maximum(b_llik[fin], 1e-300), initial=0.0):.3f}")
    assert np.all(err <= b_llik[fin]), (what, err, b_llik[fin])
    for phi in (0.0, 0.3, 1.0):
        lp = t.logpdf(x, phi)
        g = t.logpdfgrad(x, phi)
        assert np.all(lp[~fin] == -np.inf) and np.all(g[~fin] == -np.inf), what
        want = lpri[fin] + phi * llik[fin]
        bound = b_lpri[fin] + phi * b_llik[fin] + 2 * U * (np.abs(lpri[fin]) + phi * np.abs(llik[fin]))
        assert np.all(np.abs(lp[fin] - want) <= bound), (what, lp[fin] - want, bound)
        gw = gpri[fin] + phi * glik[fin]
        gb = phi * b_glik[fin] + 2 * U * (np.abs(gpri[fin]) + phi * np.abs(glik[fin]))
        assert np.all(np.abs(g[fin] - gw) <= gb), (what, np.max(np.abs(g[fin] - gw) - gb))
    return llik


@gpu
@pytest.mark.parametrize("family,flags,D", VALUE_CASES)
def test_values_against_exact_reference(family, flags, D):
    seen_inf = False
    for n in N_LIST:
        t, m = _target(family, n, D, 1000 * D + 10 * n + flags, flags)
        x = _points(m, np.random.default_rng(D + n), extreme=True)
        llik = _assert_values(t, m, x, f"{family} flags={flags} D={D} n={n}")
        seen_inf |= bool(np.any(np.isneginf(llik)))
    if family != "bernoulli_logit":
        assert seen_inf                                       # (the extreme points reach the families' -inf rules)


@gpu
@pytest.mark.parametrize("family", ow.FAMILIES)
@pytest.mark.parametrize("D", [3, 20])
def test_zero_weight_row_with_overflowing_term_is_dropped(family, D):
    """A row whose exp(eta) overflows (its offset is 800) but whose weight is 0: llik and the gradient are finite and
    equal the reference on the remaining rows.  With weight 1 the same row makes the count families -inf."""
    n = 70
    p, ic = _shape(family, D)
    X, y, o, w = ow.synthetic(family, n, p, 5 * D, scale=0.5, flags=3)
    o[[3, 66]] = 800.0
    w[[3, 66]] = 0.0
    w[4] = 1.0
    t, m = _target(family, n, D, 0, 3, data=(X, y, o, w))
    keep = np.ones(n, dtype=bool)
    keep[[3, 66]] = False
    _, rest = _target(family, n - 2, D, 0, 3, data=(X[keep], y[keep], o[keep], w[keep]))
    x = np.random.default_rng(D).standard_normal((5, D)) * 0.3
    llik = _assert_values(t, m, x, f"{family} D={D} dropped rows")
    assert np.all(np.isfinite(llik))
    ref = ow.exact_parts(rest, x)
    np.testing.assert_array_equal(ow.exact_parts(m, x)[1], ref[1])
    b = ow.device_bounds(rest, x)
    got_l, got_g = t.logpdf_parts(x)[1], t.logpdfgrad(x, 1.0) - t.logpdfgrad(x, 0.0)
    assert np.all(np.isfinite(got_l)) and np.all(np.isfinite(got_g))
    assert np.all(np.abs(got_l - ref[1]) <= b[1])
    assert np.all(np.abs(got_g - ref[3]) <= b[2] + 4 * U * (np.abs(ref[2]) + np.abs(ref[3])))
    if family in ("poisson_log", "neg_binomial_2_log"):
        w[3] = 1.0
        t2, m2 = _target(family, n, D, 0, 3, data=(X, y, o, w))
        assert np.all(t2.logpdf_parts(x)[1] == -np.inf) and np.all(ow.exact_parts(m2, x)[1] == -np.inf)


# ---- identities on the device ------------------------------------------------------------------------------------------
def _plain(family, X, y, sd, ic):
    from smcnuts_amd import GLMTarget
    if family in gd.DISP_FAMILIES:
        return (GLMTarget(X, y, family=family, prior_sd=sd, intercept=ic, dispersion_prior=DISP_PRIOR),
                gd.GLMDispNumpy(X, y, family, sd, DISP_PRIOR, ic))
    return GLMTarget(X, y, family=family, prior_sd=sd, intercept=ic), _glm.GLMNumpy(X, y, family, sd, ic)


def _plain_bounds(mp, x):
    return gd.device_bounds(mp, x) if isinstance(mp, gd.GLMDispNumpy) else _glm.device_bounds(mp, x)


@gpu
@pytest.mark.parametrize("family", ow.FAMILIES)
@pytest.mark.parametrize("D", [5, 24])
def test_integer_weights_equal_replicated_rows(family, D):
    """Weights in 0..3 against the replicated rows through today's GLMTarget kernels: llik and the gradient agree
    within the sum of both sides' bounds."""
    n = 67
    p, ic = _shape(family, D)
    X, y, _, _ = ow.synthetic(family, n, p, 11 * D, scale=0.5, flags=0)
    w = np.random.default_rng(D).integers(0, 4, n).astype(np.float64)
    sd = np.linspace(0.8, 2.5, p + ic)
    t, m = _target(family, n, D, 0, 2, prior_sd=sd, data=(X, y, None, w))
    rep = np.repeat(np.arange(n), w.astype(int))
    tp, mp = _plain(family, X[rep], y[rep], sd, ic)
    assert tp.model_id != t.model_id
    x = np.random.default_rng(D + 1).standard_normal((6, D)) * 0.4
    ba, bb = ow.device_bounds(m, x), _plain_bounds(mp, x)
    la, lb = t.logpdf_parts(x)[1], tp.logpdf_parts(x)[1]
    # (in exact arithmetic the two sides are the same sum: w_i term_i is w_i copies of term_i)
    assert np.all(np.abs(la - lb) <= ba[1] + bb[1]), (la - lb, ba[1], bb[1])
    ga = t.logpdfgrad(x, 1.0) - t.logpdfgrad(x, 0.0)
    gb = tp.logpdfgrad(x, 1.0) - tp.logpdfgrad(x, 0.0)
    slack = 8 * U * (np.abs(t.logpdfgrad(x, 1.0)) + np.abs(t.logpdfgrad(x, 0.0)))
    # (slack: what taking the likelihood's gradient as logpdfgrad(phi = 1) - logpdfgrad(phi = 0) rounds)
    assert np.all(np.abs(ga - gb) <= ba[2] + bb[2] + slack), np.max(np.abs(ga - gb) - ba[2] - bb[2])


@gpu
@pytest.mark.parametrize("family", ow.FAMILIES)
@pytest.mark.parametrize("D", [4, 19])
def test_constant_offset_equals_shifted_intercept(family, D):
    n, c = 65, 0.625
    p, ic = _shape(family, D, intercept=True)
    X, y, _, _ = ow.synthetic(family, n, p, 13 * D, scale=0.5, flags=0)
    sd = np.linspace(0.8, 2.5, p + ic)
    t, m = _target(family, n, D, 0, 1, prior_sd=sd, intercept=True, data=(X, y, np.full(n, c), None))
    tp, mp = _plain(family, X, y, sd, True)
    x = np.random.default_rng(D).standard_normal((6, D)) * 0.4
    xs = x.copy()
    xs[:, 0] += c
    ba, bb = ow.device_bounds(m, x), _plain_bounds(mp, xs)
    la, lb = t.logpdf_parts(x)[1], tp.logpdf_parts(xs)[1]
    # (x_0 + c is rounded on the shifted side: every eta moves by at most u |x_0 + c|, llik by that times sum_i |d_i|;
    #  the factor 2 covers the change of d over so small a step)
    d_sum = np.sum(np.abs(m.obs(x)[2]), axis=1)
    assert np.all(np.abs(la - lb) <= ba[1] + bb[1] + 2 * U * np.abs(xs[:, 0]) * d_sum), (la - lb, ba[1], bb[1])


# ---- NUTS --------------------------------------------------------------------------------------------------------------
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


# one per functor shape and family group: 8 lanes and one wavefront per particle, canonical and dispersion families
TAPE_CASES = [("bernoulli_logit", 3, 16, 0.01), ("poisson_log", 1, 17, 0.005), ("normal", 3, 8, 0.01),
              ("neg_binomial_2_log", 2, 9, 0.01)]


@gpu
@pytest.mark.parametrize("family,flags,D,eps", TAPE_CASES)
def test_nuts_on_tapes_against_pynuts(family, flags, D, eps):
    """NUTSProposal(GLMTarget).rvs on drawn tapes: draws consumed, leapfrogs and depth exact, x' and r' to 1e-12, against
    the reference-shaped NUTS over the numpy density."""
    from smcnuts_amd.proposal.nuts import NUTSProposal
    t, m = _target(family, 200, D, 7 * D, flags, prior_sd=2.0, intercept=True)
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
    print(f"{family} D={D}: leapfrogs {nleap.min()}..{nleap.max()}")
    assert nleap.max() >= 15
    np.testing.assert_array_equal(st["ndraws"], ndraws)
    np.testing.assert_array_equal(st["nleap"], nleap)
    np.testing.assert_array_equal(st["depth"], depth)
    close(xn, want_x, rtol=1e-12, atol=1e-12)
    close(rn, want_r, rtol=1e-12, atol=1e-12)


@gpu
@pytest.mark.parametrize("family,flags,D,n,eps", [("poisson_log", 1, 12, 300, 0.02), ("bernoulli_logit", 2, 25, 100, 0.05),
                                                  ("normal", 3, 6, 300, 0.02), ("neg_binomial_2_log", 3, 12, 40, 0.05)])
def test_philox_mode_against_host_target(family, flags, D, n, eps):
    """Production RNG: the device-native target and HostTarget(numpy model) on the same seed and state -- the same
    momenta, trees and draws, x' and r' to round-off.  Any mismatch names its particles."""
    from smcnuts_amd import HostTarget, _capi
    N, seed, it = 2048, 4242, 5
    t, m = _target(family, n, D, 11 * D, flags, prior_sd=2.0, intercept=True)    # (n: the host side's cost per leapfrog)
    h = HostTarget(m)
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


# ---- full loop ---------------------------------------------------------------------------------------------------------
LOOPS = [(lk, temp) for lk in ("forwardsLKernel", "GaussianApproxLKernel", "asymptoticLKernel") for temp in (False, True)]


def _loop_case(which):
    """(make device target, numpy model): a Poisson regression on rates with exposures, a weighted logistic regression"""
    from smcnuts_amd import LogisticRegression, PoissonRegression
    if which == "poisson_exposure":
        X, y, o, _ = ow.synthetic("poisson_log", 120, 19, 60, scale=0.5, flags=1)
        return (lambda: PoissonRegression(X, y, prior_sd=2.0, exposure=np.exp(o)),
                ow.GLMOWNumpy(X, y, "poisson_log", 2.0, True, DISP_PRIOR, np.log(np.exp(o)), None))
    X, y, _, w = ow.synthetic("bernoulli_logit", 120, 4, 15, scale=0.5, flags=2)
    return (lambda: LogisticRegression(X, y, prior_sd=2.0, weights=w),
            ow.GLMOWNumpy(X, y, "bernoulli_logit", 2.0, True, DISP_PRIOR, None, w))


@gpu
@pytest.mark.parametrize("lkernel,tempering", LOOPS)
@pytest.mark.parametrize("which", ["poisson_exposure", "logistic_weights"])
def test_full_loop_against_host_target(lkernel, tempering, which):
    """Every L-kernel, with and without tempering: the device-native target and the same model on the host give the
    same phi ladder and the same particles.  No divergent particle is tolerated."""
    from smcnuts_amd import SMCSampler, _capi
    make, m = _loop_case(which)
    kw = dict(K=5, N=1024, step_size=0.05, seed=9, lkernel=lkernel, tempering=tempering)
    dev = SMCSampler(target=make(), **kw)
    assert dev.target.model_id == _capi.MODEL_OGLM
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


@gpu
@pytest.mark.parametrize("lkernel,tempering,family,D", [("forwardsLKernel", False, "bernoulli_logit", 6),
                                                        ("GaussianApproxLKernel", True, "neg_binomial_2_log", 6),
                                                        ("forwardsLKernel", False, "poisson_log", 30)])
def test_two_shards_equal_one_and_runs_repeat(lkernel, tempering, family, D):
    """Two InProcessComm shards make the run one shard makes, particle for particle; two runs with one seed are
    bit-identical.  The dispersion family's constrained report (phi = e^tau) goes through the moments."""
    from smcnuts_amd import SMCSampler
    from tests.test_sharding import _run_shards
    make_t = lambda: _target(family, 150, D, D, 3, prior_sd=2.0, intercept=True)[0]
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
    if family == "neg_binomial_2_log":
        # the cmodel rule: the last constrained coordinate is phi = e^tau -- constrain(), the summary and the covariance
        t = one.target
        x, lw = one.samples.ctx.get_state()[:2]
        c = x.copy()
        c[:, -1] = np.exp(x[:, -1])
        close(t.constrain(x), c, rtol=1e-14, atol=0.0)
        assert t.param_names()[-1] == "phi"
        W = np.exp(lw - lw.max())
        W /= W.sum()
        mean = W @ c
        close(t.summary(x, lw).mean, mean, rtol=1e-10, atol=1e-12)
        cv = t.covariance(x, lw)
        close(cv.mean, mean, rtol=1e-10, atol=1e-12)
        close(cv.cov, (W[:, None] * (c - mean)).T @ (c - mean), rtol=1e-8, atol=1e-12)
        assert np.all(one.mean_estimate[:, -1] > 0.0)          # (phi, not log phi, in the sampler's moments)


# ---- pointwise, LOO and prediction with offsets --------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("family", ow.FAMILIES)
@pytest.mark.parametrize("D", [3, 17, 33])
def test_pointwise_and_loo_with_offsets(family, D):
    from test_gpu_psis import _assert_loo
    t, m = _target(family, 70, D, 100 + D, 1)
    M = 200
    x = pw.points(m, M, 7 + D)
    lw = np.random.default_rng(M + D).standard_normal(M)
    ma, xa = m.pair(x)
    ll, e_term, mean, e_mean = pw.terms(ma, xa)
    what = f"{family} D={D}"
    got = t.pointwise_loglik(x)
    assert got.shape == ll.shape and np.all(np.isfinite(ll))
    err = np.abs(got - ll)
    assert np.all(err <= e_term), f"{what}: max excess {np.max(err - e_term):.3e}"
    close(got, ll, rtol=0.0, atol=float(np.max(e_term)), what="pointwise_loglik with offsets")
    # the terms are not those of the model without its offsets
    assert np.max(np.abs(ll - pw.terms(m.base, x)[0])) > 1e-3
    # row sums against the density's own llik
    s = np.array([math.fsum(r.tolist()) for r in got])
    b = np.sum(e_term, axis=1) + ow.device_bounds(m, x)[1]
    assert np.all(np.abs(s - t.logpdf_parts(x)[1]) <= b), what
    ref, bnd = pw.criteria_bounds(ll, lw, e_term, mean, e_mean)
    pwise = t.pointwise(x, lw)
    pw.assert_pointwise(pwise, ref, bnd, what=what, close=close)
    assert pwise.n_particles == ref["n_particles"]
    # LOO: the reference on the device's own matrix, as tests/test_gpu_psis.py
    loo = t.loo(x, lw)
    _assert_loo(loo, ps.reference(got, lw), what)
    for k in pw.FIELDS:
        np.testing.assert_array_equal(getattr(loo.plain, k), getattr(pwise, k))


def _new_rows(m, rows, seed):
    """(X_new, y_new, offset_new, numpy model at the new rows)"""
    p = m.Z.shape[1] - m.intercept
    X, y, o, _ = ow.synthetic(m.family, rows, p, seed, scale=0.5, flags=1 if m.has_offset else 0)
    return X, y, o, m.at(X, y, o)


@gpu
@pytest.mark.parametrize("family", ow.FAMILIES)
@pytest.mark.parametrize("flags,D", [(1, 3), (3, 17), (1, 33), (2, 5)])
def test_predict_at_new_rows(family, flags, D):
    """predict(..., offset_new=) with and without y_new against tests/_predict.py over terms that include the offset;
    after a fit with weights the new rows carry weight 1 (flags 2, 3: the scope's second half)."""
    t, m = _target(family, 40, D, 50 + D, flags)
    Xn, yn, on, mn = _new_rows(m, 65, 3 * D)
    M = 150
    x = pw.points(m, M, D)
    lw = 2.0 * np.random.default_rng(D).standard_normal(M)
    kw = dict(offset_new=on) if flags & 1 else {}
    ma, xa = mn.pair(x)
    T = pr.terms(ma, xa)
    ref = pr.reference(T, lw)
    b = pr.bounds(T, lw, ref)
    what = f"{family} flags={flags} D={D}"
    got = t.predict(x, Xn, yn, None, lw, **kw)
    pr.assert_prediction(got, ref, b, what=what, close=close)
    assert got.n_particles == ref["n_particles"] and got.n_new == 65
    pr.assert_loglik(t.predict_loglik(x, Xn, yn, **kw), T, close=close, what=what + " predict_loglik")
    g0 = t.predict(x, Xn, None, None, lw, **kw)
    assert g0.lpd_i is None and g0.n_inf_i is None
    for k in ("mean_i", "var_i"):
        np.testing.assert_array_equal(getattr(g0, k), getattr(got, k))
    if flags & 1:
        # the offsets matter: without them the means differ
        T0 = pr.terms(mn.base, x)
        assert np.max(np.abs(T0["mean"] - T["mean"])) > 1e-3


@gpu
def test_sampler_predict_pointwise_and_draws_with_exposure():
    """SMCSampler over a Poisson regression with exposures: predict(offset_new=), pointwise(), loo() and predict_draws()
    (X_new = None: the training rows with their own offsets) from the resident particles equal the target's calls on the
    downloaded state, and the argument checks come first."""
    from smcnuts_amd import PoissonRegression, SMCSampler
    X, y, o, _ = ow.synthetic("poisson_log", 60, 3, 8, scale=0.5, flags=1)
    t = PoissonRegression(X, y, prior_sd=2.0, exposure=np.exp(o))
    smc = SMCSampler(K=4, N=512, target=t, step_size=0.1, seed=5)
    Xn, on = X[:9] * 0.5, o[:9] + 0.25
    with pytest.raises(ValueError, match="offset_new is required"):
        smc.predict(Xn)
    smc.sample(show_progress=False)
    x, lw = smc.samples.ctx.get_state()[:2]
    got = smc.predict(Xn, y[:9], offset_new=on)
    want = t.predict(x, Xn, y[:9], None, lw, offset_new=on)
    for k in ("lpd_i", "mean_i", "var_i"):
        np.testing.assert_array_equal(getattr(got, k), getattr(want, k))
    a, b = smc.pointwise(), t.pointwise(x, lw)
    for k in pw.FIELDS:
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k))
    np.testing.assert_array_equal(smc.loo().elpd_loo_i, t.loo(x, lw).elpd_loo_i)
    d1 = smc.predict_draws(n_draws=64, seed=12)
    d2 = t.predict_draws(x, X, 64, seed=12, logw=lw, offset_new=t.offset)
    np.testing.assert_array_equal(d1.ancestors, d2.ancestors)
    np.testing.assert_array_equal(d1.y, d2.y)
    d3 = t.predict_draws(x, X, 64, seed=12, logw=lw, offset_new=t.offset + 3.0)
    assert d3.y.mean() > 4.0 * d2.y.mean()                       # (e^3 times the exposure)


# ---- predictive draws --------------------------------------------------------------------------------------------------
DRAW_ROWS, DRAW_S, DRAW_M = 65, 256, 130
DRAW_CASES = [(f, D) for f in ow.FAMILIES for D in (3, 17)]


def _draw_case(family, D):
    """(target, numpy model at the new rows, X_new, offset_new, x, lw, seed)"""
    t, m = _target(family, 40, D, 80 + D, 3)
    Xn, _, on, mn = _new_rows(m, DRAW_ROWS, 5 * D)
    seed = 300 + D
    x = pw.points(m, DRAW_M, seed)
    if family in ("poisson_log", "neg_binomial_2_log"):
        x[1::2, :m.Dc] *= 6.0                                 # (mu on both sides of the Poisson sampler's branch at 10)
    lw = 3.0 * np.random.default_rng(seed).standard_normal(DRAW_M)
    return t, mn, Xn, on, x, lw, seed


@pytest.mark.parametrize("family,D", DRAW_CASES)
def test_draw_inputs_meet_the_ambiguity_cap(family, D):
    """No GPU: on the restatement's own ancestors, at most 0.1 % of the draws of each case below are ambiguous."""
    _, mn, _, _, x, lw, seed = _draw_case(family, D)
    anc, amb_a = dr.ancestors(lw, DRAW_M, DRAW_S, seed)
    ma, xa = mn.pair(x)
    y, amb, _ = dr.model_draws(ma, xa, anc, seed)
    assert y.shape == (DRAW_S, DRAW_ROWS)
    assert amb.sum() <= 1e-3 * y.size and amb_a.sum() <= 1e-3 * DRAW_S, (int(amb.sum()), int(amb_a.sum()))


@gpu
@pytest.mark.parametrize("family,D", DRAW_CASES)
def test_predictive_draws_with_offsets(family, D):
    t, mn, Xn, on, x, lw, seed = _draw_case(family, D)
    got = t.predict_draws(x, Xn, DRAW_S, seed=seed, logw=lw, offset_new=on)
    a, amb_a = dr.ancestors(lw, DRAW_M, DRAW_S, seed)
    assert amb_a.sum() <= 1e-3 * DRAW_S
    np.testing.assert_array_equal(got.ancestors[~amb_a], a[~amb_a])
    ma, xa = mn.pair(x)
    y, amb, e_y = dr.model_draws(ma, xa, got.ancestors, seed)
    gy = got.y
    assert gy.shape == y.shape == (DRAW_S, DRAW_ROWS)
    print(f"{family} D={D}: {int(amb.sum())} ambiguous draws of {y.size}")
    assert amb.sum() <= 1e-3 * y.size
    ok = ~amb
    np.testing.assert_array_equal(np.isnan(gy)[ok], np.isnan(y)[ok])
    fin = ok & ~np.isnan(y)
    if family == "normal":
        assert np.all(np.abs(gy - y)[fin] <= e_y[fin])
        close(gy[fin], y[fin], rtol=0.0, atol=float(np.max(e_y[fin], initial=1e-300)), what="normal draws with offsets")
    else:
        np.testing.assert_array_equal(gy[fin], y[fin])
    assert got.n_bad == int(np.isnan(gy).sum())
    # the offsets reach the draws: the model without them gives other outcomes
    y0 = dr.model_draws(mn.base, x, got.ancestors, seed)[0]
    assert np.mean(y0[fin] != gy[fin]) > 0.05


# ---- scope -------------------------------------------------------------------------------------------------------------
@gpu
def test_weighted_fit_refuses_pointwise_and_loo():
    from smcnuts_amd import SMCSampler, _capi
    t, m = _target("bernoulli_logit", 50, 4, 3, 2)
    smc = SMCSampler(K=3, N=256, target=t, step_size=0.1, seed=2)
    smc.sample(show_progress=False)
    for call in (smc.pointwise, smc.loo):
        with pytest.raises(NotImplementedError, match="not implemented for a fit with weights"):
            call()
    x, lw = smc.samples.ctx.get_state()[:2]
    for call in (lambda: t.pointwise(x, lw), lambda: t.loo(x, lw), lambda: t.pointwise_loglik(x)):
        with pytest.raises(NotImplementedError, match="not implemented for a fit with weights"):
            call()
    # the library says so itself
    ctx = smc.samples.ctx
    for call in (ctx.pointwise_partials, lambda: ctx.pointwise_loglik(x), ctx.pointwise_dims,
                 lambda: ctx.psis_candidates(0.0, 256, x, lw)):
        with pytest.raises(_capi.SmcnError, match="of a fit with weights .SMCN_MODEL_OGLM, flags & 2. are not implemented"):
            call()
    # prediction after the weighted fit, from the resident particles, equals the reference
    Xn, yn, _, mn = _new_rows(m, 20, 4)
    got = smc.predict(Xn, yn)
    ma, xa = mn.pair(x)
    T = pr.terms(ma, xa)
    ref = pr.reference(T, lw)
    pr.assert_prediction(got, ref, pr.bounds(T, lw, ref), what="after a weighted fit", close=close)
    assert smc.predict_draws(Xn, n_draws=16, seed=1).y.shape == (16, 20)


# ---- creation errors through the C ABI -----------------------------------------------------------------------------------
@gpu
def test_creation_errors():
    from smcnuts_amd import _capi
    n = 3

    def data(flags, fam=0, p=2, ic=1, y=(0, 1, 0), o=(0.0, 0.5, -0.5), w=(1.0, 0.0, 2.0), pri=()):
        fl = int(flags)                                       # (a fractional flags slot: laid out as its integer part)
        return np.concatenate([[fam, n, p, ic, flags], np.ones(p + ic), pri, np.asarray(y, dtype=np.float64),
                               o if fl & 1 else [], w if fl & 2 else [], np.zeros(n * p)])

    who = "smcn_ctx_create: offset GLM target: "
    cases = [
        (data(0), who + "flags = 0 (neither offsets nor weights) is SMCN_MODEL_GLM's model"),
        (data(4), who + "flags must be 1 (offsets), 2 (weights) or 3 (both)"),
        (data(1.5), who + "flags must be 1 (offsets), 2 (weights) or 3 (both)"),
        (data(1, o=(0.0, np.inf, 0.0)), who + "the offsets o must be finite"),
        (data(3, o=(np.nan, 0.0, 0.0)), who + "the offsets o must be finite"),
        (data(2, w=(1.0, -1.0, 1.0)), who + "the weights w must be finite and >= 0"),
        (data(3, w=(1.0, np.inf, 1.0)), who + "the weights w must be finite and >= 0"),
        (data(2, w=(0.0, 0.0, 0.0)), who + "at least one weight w must be > 0"),
        (data(3)[:-1], who + "data = [family, n, p, intercept, flags, s_1..s_D, y_1..y_n, o_1..o_n (flags & 1)"),
        (data(3, fam=2), who + "family must be 0 (bernoulli_logit) or 1 (poisson_log) for a block without m_tau, s_tau"),
        (data(3, fam=2, pri=(0.0, 1.0))[:-1], who + "data = [family, n, p, intercept, flags, s_1..s_Dc, m_tau, s_tau, y_1..y_n, "
                                              "o_1..o_n (flags & 1), w_1..w_n (flags & 2), X (n x p, row-major)] for families 2"),
        (data(3, fam=4), who + "family must be 0 (bernoulli_logit) or 1 (poisson_log), or 2 (normal) or 3 "
                               "(neg_binomial_2_log) with a dispersion prior"),
        (np.where(np.arange(len(data(3))) == 6, 0.0, data(3)), who + "prior sds must be finite and > 0"),
        (data(3, fam=3, pri=(np.inf, 1.0)), who + "m_tau must be finite"),
        (data(3, fam=3, pri=(0.0, 0.0)), who + "s_tau must be finite and > 0"),
        (data(1, y=(0, 2, 1)), who + "bernoulli_logit needs y in {0, 1}"),
        (data(1, p=64), who + "the device functor covers D <= 64 coefficients"),
    ]
    for md, msg in cases:
        with pytest.raises(_capi.SmcnError, match=None) as ei:
            _capi.Context(64, _capi.MODEL_OGLM, md)
        assert msg in str(ei.value), (str(ei.value), msg)
    ok = _capi.Context(64, _capi.MODEL_OGLM, data(3, fam=3, p=62, pri=(0.0, 1.0)))
    assert ok.D == ok.Dc == 64
    ok.close()
    with pytest.raises(_capi.SmcnError, match="unknown model id"):
        _capi.Context(64, 11, data(3))
