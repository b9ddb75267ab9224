"""The calibration checks on the device (smcn_calibration_*) against tests/_calibration.py: the per-pair tails against 50
digits, the mixtures' partials across the lane, wavefront, slice and group edges, the iteration bound, the sampler's
calibration() on one, two and four shards, and that a Poisson fit of overdispersed counts shows a U-shaped PIT histogram.

Tolerances: per compared quantity 10 x the error of the fp64 restatement against 50 digits on the test's
own inputs, each tail as a relative error of itself (both are sums of non-negative terms), with a floor of 1e-14."""
import functools
import math

import numpy as np
import pytest

import _calibration as ref
from _tol import close

pytestmark = pytest.mark.gpu


def _check(dev, ref64, refmp, what):
    """|dev - 50 digits| <= tolerance x 50 digits, the tolerance measured on these inputs."""
    tol = ref.tolerance(ref64, refmp)
    used = ref.share(dev, refmp) / tol
    print(f"  {what}: tolerance {tol:.2e}, used {used:.3f}")
    sel = np.asarray(refmp) >= ref.TINY
    close(np.asarray(dev)[sel], np.asarray(refmp)[sel], rtol=tol, atol=0.0, what=what,
          err_msg=f"{what} (tolerance {tol:.2e}, used {used:.2f})")
    return tol


# ---- 1. the per-pair tails ---------------------------------------------------------------------------------------------------
# (n, M, Dc, offset): every n in {1, 63, 64, 65, 130}, M in {1, 63, 64, 65, 257}, Dc in {1, 16, 17, 33} (the three row
# capacities), once with an offset table; 50 digits are taken on at most 400 pairs of a case (ref.sample_pairs)
SHAPES = [(1, 257, 1, False), (63, 64, 16, False), (64, 65, 17, False), (65, 63, 33, False), (130, 1, 16, False),
          (130, 257, 17, True)]


@pytest.mark.parametrize("family", ref.FAMILIES)
@pytest.mark.parametrize("n,M,Dc,offset", SHAPES)
def test_points_against_50_digits(family, n, M, Dc, offset):
    key = (family, n, M, Dc, offset)
    c = ref.case(*key)
    t = ref.target(c)
    got = t.calibration_points(c["x"])
    assert got.shape == (M, n, 2)
    fin = c["finite"]
    assert np.all(np.isnan(got[~fin])) and not np.isnan(got[fin]).any()       # the NaN particle alone, between its neighbours
    lo64, up64, _, conv = ref.tails64(c)
    assert conv[fin].all()
    P = np.array(ref.sample_pairs(c))
    mp = ref.tails_mp(key, P)
    tol_lo = _check(got[P[:, 0], P[:, 1], 0], lo64[P[:, 0], P[:, 1]], mp[:, 0], f"{family} lo")
    tol_up = _check(got[P[:, 0], P[:, 1], 1], up64[P[:, 0], P[:, 1]], mp[:, 1], f"{family} up")
    assert np.all((got[fin] >= 0.0) & (got[fin] <= 1.0))
    # lo + pmf + up = 1 on every pair, pmf from the pointwise term (normal: lo + up = 1)
    pmf = np.exp(t.pointwise_loglik(c["x"][fin])) if family != "normal" else 0.0
    close(got[fin, :, 0] + pmf + got[fin, :, 1], 1.0, rtol=0.0, atol=max(tol_lo, tol_up), what=f"{family} lo + pmf + up")
    if family == "normal":
        z = np.abs(c["y"][None, :] - ref.eta64(c)[fin]) / np.exp(c["x"][fin, Dc:Dc + 1])
        assert M < 7 or z.max() >= 30.0


# ---- 2. the mixtures' partials -----------------------------------------------------------------------------------------------
# M across the lane, wavefront, slice and group-of-16 edges; n = 12 rows, Dc = 3; the particles repeat a pool of 64 (50 digits
# once per pool); moderate means, so that the leave-one-out ratios e^-ll stay inside the doubles
PARTIAL_CASES = [("poisson_log", 1), ("neg_binomial_2_log", 64), ("normal", 255), ("bernoulli_logit", 256), ("poisson_log", 257),
                 ("neg_binomial_2_log", 4097), ("poisson_log", 4097)]
POOL, ROWS, INF_ROW = 64, 12, 4
KEYS = ("pit_lo", "sf", "pit_lo_loo", "sf_loo")


@functools.lru_cache(maxsize=None)
def _pool(family):
    """The case, its target and (lo, up, term) [POOL][ROWS] at 50 digits and in fp64.  Count families: column 0 of X is
    in [-0.01, 0] except at INF_ROW, where it is 1, and the pool's last particle has the coefficient 720 on it, so its term
    is -inf at INF_ROW alone (e^720 overflows) and moderate elsewhere (eta in [-7.2, 0]: the ratios e^-ll stay in range)."""
    c = dict(ref.case(family, ROWS, POOL, 3, False, 1, False, True))
    count = c["fam"] in (1, 3)
    if count:
        X, x = c["X"].copy(), c["x"].copy()
        X[:, 0] = -0.01 * np.abs(X[:, 0])
        X[INF_ROW, 0] = 1.0
        x[POOL - 1, :3] = 0.0, 720.0, 0.0
        c["X"], c["x"] = X, x
    lo64, up64, t64, conv = ref.tails64(c)
    assert conv.all()
    mp = np.full((POOL, ROWS, 4), np.nan)
    for p in range(POOL):
        for i in range(ROWS):
            if not (count and p == POOL - 1 and i == INF_ROW):
                mp[p, i] = [ref._f(v) if k < 3 else float(v) for k, v in enumerate(ref.pair_mp(c, c["x"][p], i))]
    if count:
        assert t64[POOL - 1, INF_ROW] == -np.inf and np.isfinite(np.delete(t64[POOL - 1], INF_ROW)).all()
    return c, ref.target(c), (lo64, up64, t64), (mp[..., 0], mp[..., 1], mp[..., 3])


def _weights(M, seed):
    lw = np.random.default_rng(seed).normal(0.0, 2.0, M)
    if M > 8:
        lw[1], lw[5] = -np.inf, -790.0
    return lw


def _of(res):
    return {k: getattr(res, k) for k in KEYS}


def _check_mixture(got, idx, lw, family, what):
    c, _, r64, rmp = _pool(family)
    rows = np.ones(ROWS, dtype=bool)
    has_inf = c["fam"] in (1, 3) and np.any((idx == POOL - 1) & np.isfinite(lw))
    if has_inf:
        rows[INF_ROW] = False
    a64 = ref.mixture(*[v[idx][:, rows] for v in r64], lw)
    amp = ref.mixture(*[v[idx][:, rows] for v in rmp], lw, exact=True)
    for k in KEYS:
        _check(got[k][rows], a64[k], amp[k], f"{what} {k}")
    return rows, has_inf


@pytest.mark.parametrize("family,M", PARTIAL_CASES)
def test_partials_against_the_reference(family, M):
    from smcnuts_amd.calibration import QC, combine_calibration_partials
    c, t, _, _ = _pool(family)
    idx = (np.arange(M) * 5 + (POOL - 1 if M > 1 else 0)) % POOL if M < POOL else np.arange(M) % POOL
    x, lw = c["x"][idx], _weights(M, M)
    part = t.calibration_partials(x, lw)
    assert part.shape == (1 + ROWS, QC)
    assert part.tobytes() == t.calibration_partials(x, lw).tobytes()             # a repeated call: identical bits
    res = combine_calibration_partials([part])
    rows, has_inf = _check_mixture(_of(res), idx, lw, family, f"{family} M={M}")
    fin = np.isfinite(lw)
    assert res.n_particles == int(fin.sum()) and np.all(res.n_unconverged == 0)
    want_inf = np.zeros(ROWS)
    if has_inf:
        want_inf[INF_ROW] = np.sum((idx == POOL - 1) & fin)
        for k in KEYS + ("pit_hi", "pit_hi_loo"):
            assert np.isnan(getattr(res, k)[INF_ROW]) and not np.isnan(getattr(res, k)[rows]).any(), k
    np.testing.assert_array_equal(res.ninf, want_inf)
    close(res.pit_hi, 1.0 - res.sf, rtol=0.0, atol=0.0, what="pit_hi is 1 - sf")
    w = np.exp(lw[fin] - lw[fin].max())
    close(res.ess, w.sum() ** 2 / (w * w).sum(), rtol=(M + 16) * 4 * 2.0 ** -53, what="the weights' ESS")
    if M >= 2:
        # two calls on halves, merged on the host
        h = M // 2
        two = combine_calibration_partials([t.calibration_partials(x[:h], lw[:h]), t.calibration_partials(x[h:], lw[h:])])
        _check_mixture(_of(two), idx, lw, family, f"{family} M={M} two halves")
        np.testing.assert_array_equal(two.ninf, want_inf)
        assert two.n_particles == res.n_particles
    # equal weights: logw = None
    if M == 64:
        _check_mixture(_of(t.calibration(x)), idx, np.zeros(M), family, f"{family} equal weights")


def test_no_contributing_particle():
    c, t, _, _ = _pool("poisson_log")
    res = t.calibration(c["x"][:4], np.full(4, -np.inf))
    assert res.n_particles == 0 and res.ess == 0.0 and all(np.isnan(getattr(res, k)).all() for k in KEYS)


# ---- 3. the iteration bound --------------------------------------------------------------------------------------------------
def test_the_iteration_bound():
    """A Poisson row with y = mu = 4e5 needs about 8.2 sqrt(mu) = 5200 terms at its mode, beyond the bound of 2048: the pair is
    counted, its row is NaN, the ordinary rows beside it are what they are without it."""
    from smcnuts_amd import GLMTarget
    rng = np.random.default_rng(11)
    n, M, r = 6, 70, 3
    X = np.zeros((n, 1))
    X[r, 0] = 1.0
    y = np.array([3.0, 5.0, 8.0, 4e5, 0.0, 12.0])
    x = np.empty((M, 2))
    x[:, 0] = math.log(5.0) + 0.1 * rng.standard_normal(M)
    x[:, 1] = math.log(4e5) - x[:, 0] + 1e-4 * rng.standard_normal(M)
    lw = rng.normal(0.0, 1.0, M)
    t = GLMTarget(X, y, family="poisson_log")
    c = dict(family="poisson_log", fam=1, X=X, y=y, offset=None, x=x, Dc=2)
    lo64, up64, t64, conv = ref.tails64(c)
    others = np.arange(n) != r
    assert not conv[:, r].any() and conv[:, others].all()                        # (the restatement has the same bound)
    pts = t.calibration_points(x)
    assert np.isnan(pts[:, r]).all() and not np.isnan(pts[:, others]).any()
    res = t.calibration(x, lw)
    ms = t._context(M).calibration_last_ms()
    print(f"  the call with {M} unconverged pairs: {ms:.3f} ms on the device")
    assert ms < 1000.0          # (70 particles x 2048 iterations of a few dozen instructions: well below a millisecond's order)
    np.testing.assert_array_equal(res.n_unconverged, np.where(others, 0.0, float(M)))
    np.testing.assert_array_equal(res.ninf, np.zeros(n))
    for k in KEYS:
        assert np.isnan(getattr(res, k)[r]) and not np.isnan(getattr(res, k)[others]).any()
    # the other rows: bit for bit the same model without the row
    t2 = GLMTarget(X[others], y[others], family="poisson_log")
    res2 = t2.calibration(x, lw)
    for k in KEYS:
        assert getattr(res, k)[others].tobytes() == getattr(res2, k).tobytes(), k
    a64 = ref.mixture(lo64[:, others], up64[:, others], t64[:, others], lw)
    for k in KEYS:
        close(getattr(res, k)[others], a64[k], rtol=1e-11, what=f"iteration bound, ordinary rows {k}")   # (a sanity bound)


def test_abi_refusals():
    from smcnuts_amd import ArmaModel, GLMTarget
    from smcnuts_amd._capi import SmcnError
    ctx = ArmaModel()._context(64)
    for call in (ctx.calibration_dims, lambda: ctx.calibration_partials(np.zeros((64, 4)))):
        with pytest.raises(SmcnError, match="SMCN_MODEL_GLM"):
            call()
    rng = np.random.default_rng(0)
    X, y = rng.standard_normal((10, 2)), rng.poisson(3.0, 10).astype(np.float64)
    w = GLMTarget(X, y, family="poisson_log", weights=np.ones(10))
    with pytest.raises(SmcnError, match="weights"):
        w._context(64).calibration_dims()
    ok = GLMTarget(X, y, family="poisson_log")._context(64)
    assert ok.calibration_dims() == (10, 9)
    with pytest.raises(SmcnError, match="bad arguments"):
        ok.call("smcn_calibration_points", None, 4, None)


# ---- 4. the sampler ----------------------------------------------------------------------------------------------------------
def _counts(seed=4, n=40):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, 2)) / math.sqrt(2.0)
    y = rng.poisson(rng.gamma(2.0, np.exp(1.0 + X @ np.array([0.5, -0.3])) / 2.0)).astype(np.float64)
    return X, y


def _make(family):
    from smcnuts_amd import GLMTarget
    X, y = _counts()
    return GLMTarget(X, y, family=family, **({"dispersion_prior": (0.0, 2.0)} if family == "neg_binomial_2_log" else {}))


FIT = dict(K=3, N=256, step_size=0.05, seed=2)
ALL = KEYS + ("pit_hi", "pit_hi_loo")


def _same(a, b, N, what):
    """Two merges of the same N particles' sums of non-negative terms: 2 N u of each value."""
    for k in ALL:
        close(getattr(a, k), getattr(b, k), rtol=2.0 * N * 2.0 ** -53, what=f"{what} {k}")
    np.testing.assert_array_equal(a.ninf, b.ninf)
    np.testing.assert_array_equal(a.n_unconverged, b.n_unconverged)
    assert a.n_particles == b.n_particles


@pytest.mark.parametrize("family", ["poisson_log", "neg_binomial_2_log"])
def test_through_the_sampler(family):
    from smcnuts_amd import SMCSampler
    smc = SMCSampler(target=_make(family), **FIT)
    with pytest.raises(RuntimeError, match="sample"):
        smc.calibration()
    smc.sample(show_progress=False)
    res = smc.calibration()
    x, lw = smc.samples.ctx.get_state()[:2]
    _same(res, smc.target.calibration(x, lw), FIT["N"], f"{family}: resident against uploaded")
    assert res.n_obs == 40 and np.all(res.ninf == 0) and np.all(res.n_unconverged == 0) and len(res.summary()["rows"]) == 40
    assert np.all((res.pit_lo >= 0) & (res.pit_lo <= res.pit_hi) & (res.pit_hi <= 1))
    u = res.randomised(3)
    assert np.all((u >= res.pit_lo) & (u <= res.pit_hi)) and np.isfinite(res.quantile_residuals(3)).all()
    assert abs(res.pit_histogram().sum() - 1.0) < 1e-12


def test_sampler_refusals():
    from smcnuts_amd import ArmaModel, GLMTarget, SMCSampler
    asy = SMCSampler(K=2, N=256, target=_make("poisson_log"), step_size=0.05, seed=1, lkernel="asymptoticLKernel")
    with pytest.raises(NotImplementedError, match="asymptotic"):
        asy.calibration()
    with pytest.raises(NotImplementedError, match="GLMTarget"):
        SMCSampler(K=2, N=256, target=ArmaModel(), step_size=0.01, seed=1).calibration()
    X, y = _counts()
    with pytest.raises(NotImplementedError, match="weights"):
        SMCSampler(K=2, N=256, target=GLMTarget(X, y, family="poisson_log", weights=np.ones(40)), step_size=0.05,
                   seed=1).calibration()


@pytest.mark.parametrize("family", ["poisson_log", "neg_binomial_2_log"])
@pytest.mark.parametrize("world", [2, 4])
def test_shards(world, family):
    """In-process shards: every rank returns the one-shard result of the same particles."""
    from smcnuts_amd import SMCSampler
    from tests.test_sharding import _run_shards
    out = {}

    def drive(s):
        s.sample(show_progress=False)
        out[s.comm.rank] = (s.calibration(),) + s.samples.ctx.get_state()[:2]

    _run_shards(lambda c: SMCSampler(target=_make(family), comm=c, **FIT), world, drive, device=True)
    assert sorted(out) == list(range(world))
    x, lw = np.concatenate([out[r][1] for r in range(world)]), np.concatenate([out[r][2] for r in range(world)])
    one = _make(family).calibration(x, lw)
    for r in range(world):
        _same(out[r][0], one, len(lw), f"{family}: rank {r} of {world} against one shard")
        assert all(getattr(out[r][0], k).tobytes() == getattr(out[0][0], k).tobytes() for k in ALL)


# ---- 5. it detects what it is for ------------------------------------------------------------------------------------------
def _overdispersed(seed=7, n=130, phi=0.7):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, 2)) / math.sqrt(2.0)
    mu = np.exp(1.5 + X @ np.array([0.6, -0.4]))
    return X, rng.poisson(rng.gamma(phi, mu / phi)).astype(np.float64)


def test_a_poisson_fit_of_overdispersed_counts_is_u_shaped():
    """Counts from NB2 with phi = 0.7: the Poisson fit's predictive laws are too narrow, so its PIT mass piles up in the two
    outer bins of ten; the NB2 fit's histogram is flat up to the noise of n = 130 rows."""
    from smcnuts_amd import GLMTarget, SMCSampler
    X, y = _overdispersed()
    outer = {}
    for fam, kw in (("poisson_log", {}), ("neg_binomial_2_log", dict(dispersion_prior=(0.0, 2.5)))):
        smc = SMCSampler(K=12, N=4096, target=GLMTarget(X, y, family=fam, **kw), step_size=0.03, seed=21)
        smc.sample(show_progress=False)
        h = smc.calibration().pit_histogram(10)
        assert abs(h.sum() - 1.0) < 1e-12
        outer[fam] = float(h[0] + h[-1])
        print(f"  {fam}: histogram {np.round(h, 3)}, outer bins {outer[fam]:.3f}, final ESS {smc.ess[-1]:.0f}")
    # The NumPy restatement on 400 draws from the Laplace approximation of either posterior (tests/test_calibration.py,
    # test_the_u_shape_on_the_cpu, this seed) gives 0.527 for the Poisson fit and 0.206 for the NB2 fit (flat: 0.2).
    # Asserted with a margin of a third of that gap, 0.107, on either side.
    assert outer["poisson_log"] > 0.42 and outer["neg_binomial_2_log"] < 0.313
    assert outer["poisson_log"] > outer["neg_binomial_2_log"] + 0.107
