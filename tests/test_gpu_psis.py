"""Pareto-smoothed LOO on the device against the NumPy reference of tests/_psis.py, applied to the DEVICE'S OWN term matrix
(pointwise_loglik) and to lw - mw: candidates, tail lengths and cutoffs are compared exactly, the other columns through
_tol.close with the bounds of tests/_psis.py (16 x the distance of the float64 reference from the mpmath evaluation,
tightened to 10 x what the device was observed to use; every figure is printed before it is asserted)."""
import numpy as np
import pytest

import _glm
import _pointwise as pw
import _psis as ps
from _tol import close

pytestmark = pytest.mark.gpu

FLOAT_COLS = (("pareto_k", "pareto_k_i"), ("elpd_psis", "elpd_loo_i"), ("psis_ess", "psis_ess_i"), ("sigma", "sigma_i"))


# (one call site per column: _tol keeps its record of the tolerance used per call site)
_CLOSE = {
    "pareto_k": lambda g, r, b, w: close(g, r, rtol=b, atol=b, err_msg=w, what="psis pareto_k"),
    "elpd_psis": lambda g, r, b, w: close(g, r, rtol=b, atol=b, err_msg=w, what="psis elpd_psis"),
    "psis_ess": lambda g, r, b, w: close(g, r, rtol=b, atol=b, err_msg=w, what="psis psis_ess"),
    "sigma": lambda g, r, b, w: close(g, r, rtol=b, atol=b, err_msg=w, what="psis sigma"),
}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _assert_loo(got, ref, what, bound=ps.BOUND, exact_cutoff=True):
    np.testing.assert_array_equal(got.tail_len_i, ref["tail_len"], err_msg=f"{what}: tail_len")
    if exact_cutoff:
        np.testing.assert_array_equal(_bits(got.cutoff_i), _bits(ref["cutoff"]), err_msg=f"{what}: cutoff bits")
    for col, attr in FLOAT_COLS:
        g, r = getattr(got, attr), ref[col]
        fin = np.isfinite(r) & np.isfinite(g)
        print(f"{what} {col}: max |got - ref| / (1 + |ref|) = "
              f"{np.max(np.abs(g[fin] - r[fin]) / (1 + np.abs(r[fin])), initial=0.0):.3e} (bound {bound[col]:.3e})")
        _CLOSE[col](g, r, bound[col], f"{what}: {col}")


def _check(t, x, lw, what):
    """loo() of the points against the reference on the device's own matrix; the selection itself bit for bit."""
    ll = t.pointwise_loglik(x)
    ref = ps.reference(ll, lw)
    got = t.loo(x, lw)
    _assert_loo(got, ref, what)
    lwp, llk = ps.contributing(ll, lw)
    S = lwp.shape[0]
    assert got.n_particles == S
    # stage 1 alone: this rank's candidates are the S's T_cap largest, ties in particle order, with their ll
    mw = float(np.max(np.asarray(lw)[np.isfinite(lw)])) if lw is not None else 0.0
    ctx = t._context(x.shape[0])
    lr_c, ll_c = ctx.psis_candidates(mw, S, x, lw)
    want_lr, want_ll = ps.candidates(lwp, llk, ps.tail_len(S) + 1)
    np.testing.assert_array_equal(_bits(lr_c + 0.0), _bits(want_lr + 0.0), err_msg=f"{what}: candidate lr")
    np.testing.assert_array_equal(_bits(ll_c + 0.0), _bits(want_ll + 0.0), err_msg=f"{what}: candidate ll")
    # tail membership: the candidates above the cutoff are the reference's tail, particle by particle
    for i in (0, ll.shape[1] - 1):
        mine = np.sort(lr_c[i][lr_c[i] > got.cutoff_i[i]])
        np.testing.assert_array_equal(mine, np.sort((lwp - llk[:, i])[ref["tail"][i]]), err_msg=f"{what}: tail of {i}")
    # the Pointwise of the same call and p_loo
    plain = t.pointwise(x, lw)
    for k in pw.FIELDS:
        np.testing.assert_array_equal(getattr(got.plain, k), getattr(plain, k))
    np.testing.assert_array_equal(got.p_loo_i, plain.lppd_i - got.elpd_loo_i)
    return got, ref


@pytest.mark.parametrize("D", [3, 17, 33])
@pytest.mark.parametrize("family", pw.FAMILIES)
def test_grid(family, D):
    t, m = pw.make(family, 70, D, 100 + pw.FAMILIES.index(family))
    for M in (24, 25, 64, 65, 1000):
        x = pw.points(m, M, 7 + M)
        lw = np.random.default_rng(M).standard_normal(M)
        got, ref = _check(t, x, lw, f"{family} D={D} M={M}")
        assert np.all(np.isinf(got.pareto_k_i)) == (M == 24)      # 24 particles: M = 4 < 5, nothing is smoothed
        if M == 24:
            np.testing.assert_array_equal(got.tail_len_i <= 4, True)
            close(got.elpd_loo_i, got.plain.elpd_loo_i, rtol=ps.BOUND["elpd_psis"], atol=ps.BOUND["elpd_psis"],
                  what="unsmoothed elpd_psis against plain elpd_loo")


def test_equal_weights():
    t, m = pw.make("bernoulli_logit", 70, 3, 100)
    _check(t, pw.points(m, 200, 1), None, "equal weights")


def test_many_slices():
    t, m = pw.make("bernoulli_logit", 5, 3, 5)
    x = pw.points(m, 4096, 11)
    lw = np.random.default_rng(3).standard_normal(4096)
    got, _ = _check(t, x, lw, "4096 particles, n = 5")
    assert np.all(got.tail_len_i == ps.tail_len(4096))


@pytest.mark.parametrize("shift", [0.0, 1e5, -1e5])
def test_nonfinite_weights_and_offsets(shift):
    t, m = pw.make("poisson_log", 70, 3, 101)
    x = pw.points(m, 1000, 4)
    lw = 3.0 * np.random.default_rng(8).standard_normal(1000) + shift
    lw[5:900:11] = -np.inf
    lw[7], lw[8] = np.nan, np.inf
    got, _ = _check(t, x, lw, f"non-finite log-weights, offset {shift}")
    assert got.n_particles == int(np.sum(np.isfinite(lw)))


def test_duplicated_particles_tie_at_the_cutoff():
    t, m = pw.make("normal", 70, 3, 102)
    rng = np.random.default_rng(12)
    x = pw.points(m, 400, 6)
    lw = rng.standard_normal(400)
    src = rng.integers(0, 400, size=400)
    dup = rng.random(400) < 0.7
    x[dup], lw[dup] = x[src[dup]], lw[src[dup]]
    got, ref = _check(t, x, lw, "duplicated particles")
    ll = t.pointwise_loglik(x)
    lr = (lw - lw.max())[:, None] - ll
    ties = [int(np.sum(lr[:, i] == got.cutoff_i[i])) for i in range(70)]
    assert max(ties) > 1, "no observation with a tie at the cutoff"
    assert np.any(got.tail_len_i < ps.tail_len(400))


def test_inf_rule():
    from smcnuts_amd import GLMTarget
    X, y = pw.synthetic("poisson_log", 70, 2, 5)
    X[:, 0] = 0.0
    X[33, 0] = 1.0                                           # eta of the particle below: 1500 at observation 33 alone
    t = GLMTarget(X, y, family="poisson_log", prior_sd=2.0, intercept=False)
    m = _glm.GLMNumpy(X, y, "poisson_log", 2.0, intercept=False)
    x = pw.points(m, 100, 1)
    lw = np.random.default_rng(3).standard_normal(100)
    clean = t.loo(x, lw)
    x[17, 0] = 1500.0
    got, _ = _check(t, x, lw, "-inf rule")
    assert got.pareto_k_i[33] == np.inf and got.elpd_loo_i[33] == -np.inf
    assert got.psis_ess_i[33] == 0.0 and got.tail_len_i[33] == 0
    others = np.arange(70) != 33
    for attr in ("pareto_k_i", "elpd_loo_i", "psis_ess_i", "tail_len_i", "cutoff_i"):
        np.testing.assert_array_equal(getattr(got, attr)[others], getattr(clean, attr)[others])
    assert got.n_high_k >= 1


def _numpy_body(lwp, ll, cutoff):
    lr = lwp - ll
    b = lr <= cutoff
    mb = np.max(lr[b])
    e = np.exp(lr[b] - mb)
    return [mb, np.sum(e), np.sum(e * e), np.sum(np.exp(lwp[b]))]


@pytest.mark.parametrize("T", [5, 768, 4096])
def test_fit_on_synthetic_pareto_tails(T):
    """smcn_psis_fit alone, fed tails that are exact generalised-Pareto quantiles (no particles, no model)."""
    ks = (-0.3, 0.0, 0.2, 0.7, 1.2)
    t, _ = pw.make("bernoulli_logit", 5, 3, 5)
    ctx = t._context(64)
    lr_c, ll_c, body, refs = [], [], [], []
    for k in ks:
        lwp, ll = ps.gpd_tail_case(T, k)
        S = lwp.shape[0]
        r = ps.psis_obs(lwp, ll)
        a, b = ps.candidates(lwp, ll[:, None], T + 1)
        lr_c.append(a[0]), ll_c.append(b[0]), body.append(_numpy_body(lwp, ll, r["cutoff"])), refs.append(r)
    out = ctx.psis_fit(np.array(lr_c), np.array(ll_c), np.array(body), 0.0, S)
    np.testing.assert_array_equal(out[:, 3], [T] * len(ks))
    np.testing.assert_array_equal(_bits(out[:, 4]), _bits([r["cutoff"] for r in refs]))
    for j, col in ((0, "pareto_k"), (1, "elpd_psis"), (2, "psis_ess"), (5, "sigma")):
        want = np.array([r[col] for r in refs])
        print(f"fit alone T={T} {col}: max |got - ref| / (1 + |ref|) = {np.max(np.abs(out[:, j] - want) / (1 + np.abs(want))):.3e}"
              f" (bound {ps.BOUND[col]:.3e})")
        _CLOSE[col](out[:, j], want, ps.BOUND[col], f"fit alone T={T}: {col}")
    if T == 768:
        for k, v in zip(ks, out[:, 0]):
            assert abs(v - (T * k + 5.0) / (T + 10.0)) < 0.005
    # the candidates in any order give the same bits: the fit sorts its tail itself
    perm = np.random.default_rng(T).permutation(T + 1)
    again = ctx.psis_fit(np.array(lr_c)[:, perm], np.array(ll_c)[:, perm], np.array(body), 0.0, S)
    np.testing.assert_array_equal(_bits(again), _bits(out))


def test_repeatable_and_staged_calls_equal_the_wrapper():
    from smcnuts_amd import merge_candidates
    t, m = pw.make("neg_binomial_2_log", 130, 9, 21)
    x = pw.points(m, 1000, 4)
    lw = 3.0 * np.random.default_rng(8).standard_normal(1000)
    lw[5:900:11] = -np.inf
    ctx = t._context(1000)
    out, head = ctx.psis_loo(x, lw)
    again, _ = ctx.psis_loo(x, lw)
    np.testing.assert_array_equal(_bits(out), _bits(again))
    mw, S = head[0], int(head[3])
    assert mw == np.max(lw[np.isfinite(lw)]) and S == int(np.sum(np.isfinite(lw)))
    lr_c, ll_c = ctx.psis_candidates(mw, S, x, lw)
    glr, gll, cut = merge_candidates([(lr_c, ll_c)])
    np.testing.assert_array_equal(_bits(glr), _bits(lr_c))
    body = ctx.psis_body(mw, S, cut, x, lw)
    staged = ctx.psis_fit(glr, gll, body, mw, S)
    np.testing.assert_array_equal(_bits(staged), _bits(out))
    ms = ctx.psis_last_ms()
    assert ms.shape == (4,) and np.all(ms > 0.0)


@pytest.mark.parametrize("world", [2, 4])
def test_shards(world):
    """In-process shards of unequal size against one shard: the selection exact, the sums re-associated."""
    from smcnuts_amd.psis import loo_from_context
    from tests.test_sharding import _run_shards
    M = 1000
    edges = np.linspace(0, M, world + 1).astype(int)
    edges[1:-1] += 17
    _, m = pw.make("poisson_log", 70, 17, 9)
    x = pw.points(m, M, 4)
    lw = 2.0 * np.random.default_rng(8).standard_normal(M)
    lw[3:700:13] = -np.inf
    src = np.random.default_rng(1).integers(0, M, size=M)
    dup = np.random.default_rng(2).random(M) < 0.3                 # equal ratios on different ranks
    x[dup], lw[dup] = x[src[dup]], lw[src[dup]]
    one = pw.make("poisson_log", 70, 17, 9)[0].loo(x, lw)
    out = {}

    def drive(c):
        t = pw.make("poisson_log", 70, 17, 9)[0]
        a, b = edges[c.rank], edges[c.rank + 1]
        out[c.rank] = loo_from_context(t._context(b - a), c, x[a:b], lw[a:b])

    _run_shards(lambda c: c, world, drive, device=True)
    assert sorted(out) == list(range(world))
    ref = dict(pareto_k=one.pareto_k_i, elpd_psis=one.elpd_loo_i, psis_ess=one.psis_ess_i, sigma=one.sigma_i,
               tail_len=one.tail_len_i, cutoff=one.cutoff_i)
    for r in range(world):
        _assert_loo(out[r], ref, f"rank {r} of {world}", bound=ps.SHARD_BOUND)
        assert out[r].n_particles == one.n_particles
        for attr in ("pareto_k_i", "elpd_loo_i", "psis_ess_i", "sigma_i", "p_loo_i"):
            np.testing.assert_array_equal(_bits(getattr(out[r], attr)), _bits(getattr(out[0], attr)))


def test_sampler_loo_equals_target_loo_on_the_downloaded_state():
    from smcnuts_amd import SMCSampler, compare_loo
    t, m = pw.make("bernoulli_logit", 100, 5, 2)
    smc = SMCSampler(K=3, N=1024, target=t, step_size=0.05, seed=5)
    with pytest.raises(RuntimeError, match="sample"):
        smc.loo()
    smc.sample(show_progress=False)
    got = smc.loo()
    x, lw = smc.x_saved[-1], smc.logw_saved[-1]
    host = t.loo(x, lw)
    ref = dict(pareto_k=host.pareto_k_i, elpd_psis=host.elpd_loo_i, psis_ess=host.psis_ess_i, sigma=host.sigma_i,
               tail_len=host.tail_len_i, cutoff=host.cutoff_i)
    _assert_loo(got, ref, "resident against uploaded", exact_cutoff=False)
    close(got.cutoff_i, host.cutoff_i, rtol=ps.BOUND["elpd_psis"], atol=ps.BOUND["elpd_psis"], what="psis cutoff, resident")
    _assert_loo(got, ps.reference(t.pointwise_loglik(x), lw), "resident against the reference", exact_cutoff=False)
    assert got.n_particles == 1024 and got.n_obs == 100
    s = got.summary()
    assert s["k_threshold"] == min(1.0 - 1.0 / np.log10(1024), 0.7) and 0 <= s["n_high_k"] <= 100
    assert compare_loo(got, got)["elpd_loo_diff"] == 0.0


def test_errors():
    from smcnuts_amd import GaussianTarget, SMCSampler
    from smcnuts_amd._capi import SmcnError
    g = SMCSampler(K=2, N=1024, target=GaussianTarget(3), step_size=0.3, seed=1)
    g.sample(show_progress=False)
    with pytest.raises(NotImplementedError, match="GLMTarget"):
        g.loo()
    with pytest.raises(SmcnError, match="SMCN_MODEL_GLM"):
        g.samples.ctx.psis_loo()
    t, m = pw.make("bernoulli_logit", 5, 3, 5)
    ctx = t._context(64)
    with pytest.raises(SmcnError, match="1863225"):
        ctx.psis_candidates(0.0, 1863226, np.zeros((64, 3)))


def test_larger_case():
    """N = 65 536, n = 128, D = 16: T = 768, 1024 particle chunks in 32 slices."""
    t, m = pw.make("poisson_log", 128, 16, 9)
    x = pw.points(m, 65536, 13, scale=0.1)
    lw = 0.5 * np.random.default_rng(4).standard_normal(65536)
    ll = t.pointwise_loglik(x)
    ref = ps.reference(ll, lw)
    got = t.loo(x, lw)
    _assert_loo(got, ref, "N = 65536")
    assert np.all(got.tail_len_i == 768) and np.all(np.isfinite(got.pareto_k_i))
