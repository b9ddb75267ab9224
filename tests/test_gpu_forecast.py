"""The arma forecasts on the device (smcn_forecast_*) against tests/_forecast.py: the per-point laws against 50 digits and
err_T bit for bit, the mixture's partials, the joint terms against the density's own log-likelihood, the paths, and the
sampler's forecast() / forecast_draws() on one and two shards.

Tolerances: per compared quantity 10 x the error of the fp64 restatement against 50 digits on the test's
own inputs, as a share of the quantity's magnitude (tests/_forecast.py: scales, mixture_scales), with a floor of 1e-14."""
import functools

import numpy as np
import pytest

import _forecast as ref
from _tol import close

pytestmark = pytest.mark.gpu


def _series(T):
    return ref.shipped_series()[:T] if T > 9 else ref.synthetic_series(T, 3)


def _target(T):
    from smcnuts_amd import ArmaModel
    return ArmaModel(y=_series(T))


def _ess_tol(M):
    """sw^2 / sw2 of M weights: each sum carries at most (M + 4) u relative (M - 1 additions, a 2 ulp exponential, a
    square), the quotient of the two 2 (M + 8) u."""
    return 2.0 * (M + 8) * ref.U


def _check(dev, ref64, refmp, scale, what):
    """|dev - 50 digits| <= tolerance x magnitude, the tolerance measured on these inputs -> "tolerance (share used)"."""
    tol = ref.tolerance(ref64, refmp, scale)
    scale = np.broadcast_to(scale, np.shape(refmp))
    used = ref.share(dev, refmp, scale) / tol
    with np.errstate(all="ignore"):
        close(np.asarray(dev) / scale, np.asarray(refmp) / scale, rtol=0.0, atol=tol, what=what,
              err_msg=f"{what} (tolerance {tol:.2e}, used {used:.2f})")
    return f"{tol:.1e} ({used:.2f})"


# ---- 1. the per-point laws -------------------------------------------------------------------------------------------------
POINT_CASES = [(1, 1, 1), (2, 2, 63), (9, 63, 65), (33, 65, 300), (200, 2, 65), (200, 65, 63)]


@pytest.mark.parametrize("T,H,M", POINT_CASES)
def test_points_against_50_digits(T, H, M):
    ser, t = _series(T), _target(T)
    X = ref.value_particles(M, T + H)
    odd = ref.odd_particles()
    allx = np.concatenate([X[:M // 2], odd, X[M // 2:]])              # the odd rows sit between their neighbours
    val = np.r_[0:M // 2, M // 2 + len(odd):M + len(odd)]
    yf = ref.synthetic_series(H, 7)
    got = t.forecast_points(allx, H, y_future=yf)
    plain = t.forecast_points(allx, H)
    assert set(plain) == {"err_T", "m", "v"}
    for k in plain:
        np.testing.assert_array_equal(plain[k], got[k])
    # err_T has the bits of the exact-fma chain, |theta| > 1 and overflowing rows included
    finite_rows = np.all(np.isfinite(allx), axis=1)
    ex = ref.err_T_exact(ser, allx[finite_rows])
    np.testing.assert_array_equal(got["err_T"][finite_rows], ex)
    # a row with a non-finite coordinate is NaN throughout
    for k in got:
        assert np.all(np.isnan(got[k][~finite_rows]))
    # sigma^2 = inf and sigma^2 = 0 are bad at every horizon: no marginal term
    o0 = M // 2
    assert np.all(np.isnan(got["marginal"][o0 + 2:o0 + 4])) and np.all(np.isinf(got["v"][o0 + 2])) and np.all(got["v"][o0 + 3] == 0.0)
    # the values
    e64, m64, v64, _ = ref.laws(ser, X, H)
    a64, J64 = ref.terms(ser, X, yf)
    emp, mmp, vmp, amp, Jmp = ref.points_mp(ser, X, H, yf)
    sc = ref.scales(ser, X, H, yf)
    tols = dict(err=_check(got["err_T"][val], e64, emp, sc["err"], "points err_T"),
                m=_check(got["m"][val], m64, mmp, sc["m"], "points m_h"),
                v=_check(got["v"][val], v64, vmp, sc["v"], "points v_h"),
                a=_check(got["marginal"][val], a64, amp, sc["a"], "points marginal term"),
                J=_check(got["joint"][val], J64, Jmp, sc["J"], "points joint term"))
    print(f"T={T} H={H} M={M}: tolerances {tols}")


# ---- 2. the mixture's partials ---------------------------------------------------------------------------------------------
PARTIAL_CASES = [(1, 1, 1, 1, True), (2, 2, 16, 63, True), (9, 2, 1, 600, True), (33, 65, 1, 40, False),
                 (200, 63, 0, 65, True), (9, 63, 0, 300, False)]


def _partial_inputs(T, H, Tn, M):
    rng = np.random.default_rng(T * 1000 + H)
    X = ref.value_particles(M, T + H + 1)
    lw = 2.0 * rng.standard_normal(M)
    if M > 2:
        lw[::5] = -np.inf
    at = np.sort(rng.normal(0.5, 1.5, (H, Tn)), axis=1) if Tn else None
    return X, lw, ref.synthetic_series(H, 9), at


def _check_forecast(f, ser, X, lw, H, yf, at, what):
    a, b = ref.mixture(ser, X, lw, H, yf, at), ref.mixture_mp(ser, X, lw, H, yf, at)
    sc = ref.mixture_scales(ser, X, lw, H, yf, at)
    keys = ["mean", "var"] + (["cdf"] if at is not None else []) + (["lpd_marginal", "lpd_joint"] if yf is not None else [])
    tols = {k: _check(getattr(f, k), a[k], b[k], sc[k], f"{what} {k}") for k in keys}
    assert f.n_particles == a["n_particles"] and np.all(f.n_bad == 0)
    close(f.ess, a["ess"], rtol=_ess_tol(X.shape[0]), what="forecast ess")
    return tols


@pytest.mark.parametrize("T,H,Tn,M,has_y", PARTIAL_CASES)
def test_partials_against_the_reference(T, H, Tn, M, has_y):
    from smcnuts_amd.forecast import combine_forecast_partials
    ser, t = _series(T), _target(T)
    X, lw, yf, at = _partial_inputs(T, H, Tn, M)
    yf = yf if has_y else None
    ctx = t._context(M)
    ctx.forecast_set(H, yf, at)
    assert ctx.forecast_dims() == (H, 10 + Tn, has_y, Tn)
    slices = ctx.forecast_slices(M)
    assert slices == -(-M // 256)
    p1 = t.forecast_partials(X, H, lw, yf, at)
    p2 = t.forecast_partials(X, H, lw, yf, at)
    assert p1.shape == (1 + H, 10 + Tn) and p1.tobytes() == p2.tobytes()
    f = combine_forecast_partials([p1], Tn, has_y, at)
    tols = _check_forecast(f, ser, X, lw, H, yf, at, "partials")
    print(f"T={T} H={H} Tn={Tn} M={M} slices={slices}: tolerances {tols}")
    assert (f.lpd_marginal is None) == (not has_y) and (f.cdf is None) == (Tn == 0)
    if not has_y:
        assert np.all(p1[1:, 0] == -np.inf) and np.all(p1[1:, 1] == 0) and np.all(p1[1:, 2] == -np.inf) and np.all(p1[1:, 3] == 0)
    if M > 1:
        # halves merged on the host
        k = M // 2 + 1
        halves = [t.forecast_partials(X[:k], H, lw[:k], yf, at), t.forecast_partials(X[k:], H, lw[k:], yf, at)]
        _check_forecast(combine_forecast_partials(halves, Tn, has_y, at), ser, X, lw, H, yf, at, "merged halves")
    # classification: bad particles with a weight, |theta| > 1 ones without
    odd = ref.odd_particles()
    Xb, lwb = np.concatenate([X, odd]), np.concatenate([np.where(np.isfinite(lw), lw, 0.1), [-np.inf, -np.inf, 0.3, -0.2, 0.0, 0.1, -0.1, 0.2]])
    g = t.forecast(Xb, H, logw=lwb, y_future=yf, at=at)
    want = ref.mixture(ser, Xb, lwb, H, yf, at)
    np.testing.assert_array_equal(g.n_bad, want["n_bad"])
    assert np.all(g.n_bad == 6) and g.n_particles == M + 6
    assert np.all(np.isnan(g.mean)) and np.all(np.isnan(g.var)) and (at is None or np.all(np.isnan(g.cdf)))
    if has_y:
        # the lpd runs over the other particles (their weights all finite here)
        lwc = lwb[:M]
        clean, clean_mp = ref.mixture(ser, X, lwc, H, yf, at), ref.mixture_mp(ser, X, lwc, H, yf, at)
        sc = ref.mixture_scales(ser, X, lwc, H, yf, at)
        fin = np.isfinite(lwb)
        shift = np.log(np.exp(lwb[fin] - lwb[fin].max()).sum()) - np.log(np.exp(lwc - lwb[fin].max()).sum())
        for key in ("lpd_marginal", "lpd_joint"):
            _check(getattr(g, key) + shift, clean[key], clean_mp[key], sc[key], f"bad particles present: {key}")
    # particles without a weight add nothing: the same bits with and without them
    p3 = t.forecast_partials(np.concatenate([X, odd[:2]]), H, np.concatenate([lw, [-np.inf, -np.inf]]), yf, at)
    if -(-(M + 2) // 256) == slices:
        assert p3.tobytes() == p1.tobytes()


def test_no_contributing_particle():
    t = _target(9)
    f = t.forecast(ref.value_particles(5, 1), 3, logw=np.full(5, -np.inf), y_future=[0.1, 0.2, 0.3], at=0.5)
    assert f.n_particles == 0 and np.all(np.isnan(f.mean)) and np.all(np.isnan(f.cdf)) and np.all(np.isnan(f.lpd_joint))


# ---- 3. the joint terms against the density's log-likelihood ---------------------------------------------------------------
def test_joint_terms_against_the_density():
    from smcnuts_amd import ArmaModel
    T, H, M = 33, 6, 65
    ser, t = _series(T), _target(T)
    X = ref.value_particles(M, 21)
    yf = ref.synthetic_series(H, 4)
    J = t.forecast_points(X, H, y_future=yf)["joint"]
    base = t.logpdf_parts(X)[1]
    _, J64 = ref.terms(ser, X, yf)
    Jmp = ref.points_mp(ser, X, H, yf)[4]
    sJ = ref.scales(ser, X, H, yf)["J"]
    b64 = ref.arma_llik(ser, X)
    for j in range(1, H + 1):
        longer = np.concatenate([ser, yf[:j]])
        full = ArmaModel(y=longer).logpdf_parts(X)[1]
        # the magnitude of a difference of two log-likelihoods: theirs, and the joint term's own
        f64 = ref.arma_llik(longer, X)
        scale = np.abs(f64) + np.abs(b64) + sJ[:, j - 1]
        _check(full - base, f64 - b64, Jmp[:, j - 1], scale, "llik difference against the joint term")
        _check(J[:, j - 1], J64[:, j - 1], Jmp[:, j - 1], scale, "joint term against the llik difference's reference")


# ---- 4. the paths ------------------------------------------------------------------------------------------------------------
def _check_paths(y, ser, X, anc, seed, H, s_first, what):
    want, bound = ref.paths(ser, X, anc, seed, H, s_first)
    assert np.array_equal(np.isnan(y), np.isnan(want)), what
    with np.errstate(all="ignore"):
        close((y - want) / bound, np.zeros_like(want), rtol=0.0, atol=1.0, what=f"{what}: |device - restatement| / bound")


def test_draws_against_the_reference():
    T, H, M, S, seed = 33, 9, 70, 200, 17
    ser, t = _series(T), _target(T)
    X = ref.value_particles(M, 5)
    rng = np.random.default_rng(2)
    anc = rng.integers(0, M, S)
    d = t.forecast_draws(X, H, S, seed=seed, ancestors=anc)
    assert d.y.shape == (S, H) and d.n_bad == 0 and np.array_equal(d.ancestors, anc)
    _check_paths(d.y, ser, X, anc, seed, H, 0, "given ancestors")
    # a window of slots reproduces the full call's rows; so does another S with the same ancestors there
    ctx = t._context(M)
    ctx.forecast_set(H)
    y_w, a_w, _ = ctx.forecast_draws(S, seed, X, None, anc, s_first=37, s_count=70)
    assert y_w.tobytes() == d.y[37:107].tobytes() and np.array_equal(a_w, anc[37:107])
    d2 = t.forecast_draws(X, H, S + 56, seed=seed, ancestors=np.concatenate([anc, anc[:56]]))
    assert d2.y[:S].tobytes() == d.y.tobytes()
    # the systematic ancestors
    lw = 2.0 * rng.standard_normal(M)
    lw[::6] = -np.inf
    ds = t.forecast_draws(X, H, S, seed=seed, logw=lw)
    want, amb = ref.ancestors(lw, M, S, seed)
    assert np.array_equal(ds.ancestors[~amb], want[~amb]) and amb.sum() <= 2 and np.all(np.isfinite(lw[ds.ancestors]))
    _check_paths(ds.y, ser, X, ds.ancestors, seed, H, 0, "systematic ancestors")
    assert not np.array_equal(t.forecast_draws(X, H, S, seed=seed + 1, logw=lw).y, ds.y)


def test_draws_match_their_laws():
    """S = 4096 paths from one particle under a fixed seed: the sample mean and variance of each y_{T+h} within 5 standard
    errors of m_h, v_h (tests/test_forecast_host.py asserts the same of the reference's own paths)."""
    ser = ref.shipped_series()
    t = _target(200)
    x = np.array([[0.35, 0.6, -0.3, -0.4]])
    S, H = 4096, 8
    d = t.forecast_draws(x, H, S, seed=11)
    assert d.n_bad == 0 and np.all(d.ancestors == 0)
    _, m, v, _ = ref.laws(ser, x, H)
    mean, var = d.y.mean(0), d.y.var(0, ddof=1)
    dm, dv = np.abs(mean - m[0]) / np.sqrt(v[0] / S), np.abs(var - v[0]) / (v[0] * np.sqrt(2.0 / (S - 1)))
    print(f"in standard errors: mean {np.round(dm, 2)}, variance {np.round(dv, 2)}")
    assert np.all(dm <= 5.0) and np.all(dv <= 5.0)
    lo, hi = d.interval(0.9)
    assert np.all(lo < m[0]) and np.all(m[0] < hi)


def test_draws_from_bad_ancestors_are_nan():
    T, H = 9, 5
    t = _target(T)
    odd = ref.odd_particles()
    X = np.concatenate([ref.value_particles(3, 1), [[0.3, 0.4, 0.2, 800.0]], odd[4:5], [[0.3, 1.3, 0.2, 709.0]]])   # sigma = inf, mu = NaN
    anc = np.array([0, 3, 1, 4, 2, 5, 3])
    d = t.forecast_draws(X, H, 7, seed=3, ancestors=anc)
    assert np.all(np.isnan(d.y[[1, 3, 6]])) and np.all(np.isfinite(d.y[[0, 2, 4]]))
    row = d.y[5]                                         # sigma = e^709: finite at first, NaN from the first overflow on
    k = int(np.argmax(np.isnan(row))) if np.isnan(row).any() else H
    assert np.all(np.isfinite(row[:k])) and np.all(np.isnan(row[k:]))
    assert d.n_bad == int(np.isnan(d.y).sum())


# ---- the C ABI's refusals -------------------------------------------------------------------------------------------------
def test_abi_refusals():
    import ctypes as C
    from smcnuts_amd import GaussianTarget
    from smcnuts_amd._capi import SmcnError, dptr
    ctx = _target(9)._context(4)
    with pytest.raises(SmcnError, match="smcn_forecast_set first"):
        ctx.call("smcn_forecast_partials", None, None, ctx.N, dptr(np.zeros(64)))
    one = np.ones(4)
    for args, msg in (((0, None, None, 0), "1..512"), ((513, None, None, 0), "1..512"), ((2, None, None, 17), "0..16"),
                      ((2, None, None, 1), "thresholds"), ((2, dptr(np.array([1.0, np.nan])), None, 0), "not finite"),
                      ((2, None, dptr(np.array([1.0, np.inf])), 1), "not finite")):
        with pytest.raises(SmcnError, match=msg):
            ctx.call("smcn_forecast_set", *args)
    ctx.forecast_set(2, one[:2])
    with pytest.raises(SmcnError, match="resident"):
        ctx.call("smcn_forecast_partials", None, None, 3, dptr(np.zeros(64)))
    with pytest.raises(SmcnError, match="slot range"):
        ctx.forecast_draws(5, 0, np.zeros((2, 4)), None, None, s_first=3, s_count=3)
    with pytest.raises(SmcnError, match="finite log-weight"):
        ctx.forecast_draws(5, 0, np.zeros((2, 4)), np.full(2, -np.inf))
    g = GaussianTarget(3)._context(4)
    for name, args in (("smcn_forecast_set", (2, None, None, 0)), ("smcn_forecast_dims", (None, None, None, None)),
                       ("smcn_forecast_slices", (4, None)), ("smcn_forecast_points", (None, 1, None)),
                       ("smcn_forecast_partials", (None, None, 4, None)),
                       ("smcn_forecast_draws", (None, None, 4, 3, 0, None, 0, 3, None, None, None))):
        with pytest.raises(SmcnError, match="SMCN_MODEL_ARMA"):
            g.call(name, *args)
    ms = ctx.forecast_last_ms()
    assert ms.shape == (2,) and np.all(ms >= 0.0)


# ---- 5. through the sampler -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fit():
    from smcnuts_amd import ArmaModel, SMCSampler
    smc = SMCSampler(K=3, N=1024, target=ArmaModel(), step_size=0.01, seed=1)
    with pytest.raises(RuntimeError, match="sample"):
        smc.forecast(4)
    with pytest.raises(RuntimeError, match="sample"):
        smc.forecast_draws(4)
    smc.sample(show_progress=False)
    return smc


def _same_forecast(a, b, sc, what):
    for k in ("mean", "var", "cdf", "lpd_marginal", "lpd_joint"):
        with np.errstate(all="ignore"):
            close(getattr(a, k) / sc[k], getattr(b, k) / sc[k], rtol=0.0, atol=ref.FLOOR, what=f"{what} {k}")
    np.testing.assert_array_equal(a.n_bad, b.n_bad)
    assert a.n_particles == b.n_particles
    close(a.ess, b.ess, rtol=_ess_tol(a.n_particles), what=f"{what} ess")


def test_through_the_sampler():
    smc = _fit()
    t = smc.target
    H, yf, at = 6, ref.synthetic_series(6, 2), [0.0, 0.8]
    before = smc.summary()
    f = smc.forecast(H, y_future=yf, at=at)
    x, lw = smc.samples.ctx.get_state()[:2]
    up = t.forecast(x, H, logw=lw, y_future=yf, at=at)
    ser = ref.shipped_series()
    A = np.tile(np.asarray(at), (H, 1))
    sc = ref.mixture_scales(ser, x, lw, H, yf, A)
    _same_forecast(f, up, sc, "resident against uploaded")
    assert f.horizon == H and f.cdf.shape == (H, 2) and np.all(np.diff(f.cdf, axis=1) > 0) and np.all(f.var > 0)
    assert np.all(np.diff(f.lpd_joint) != 0) and len(f.summary()) == H
    d = smc.forecast_draws(H, n_draws=500, seed=12)
    du = t.forecast_draws(x, H, 500, seed=12, logw=lw)
    assert d.y.tobytes() == du.y.tobytes() and np.array_equal(d.ancestors, du.ancestors) and d.n_bad == 0
    dev = np.abs(d.y.mean(0) - f.mean) / np.sqrt(f.var / 500)
    print(f"|mean of paths - forecast().mean| in standard errors: {np.round(dev, 2)}")
    assert np.all(dev <= 6.0)
    assert not np.array_equal(smc.forecast_draws(H, 20).y, smc.forecast_draws(H, 20).y)      # seed=None: a fresh seed per call
    # the fit's own results are untouched
    after = smc.summary()
    for k in ("mean", "sd", "quantiles"):
        assert np.asarray(getattr(before, k)).tobytes() == np.asarray(getattr(after, k)).tobytes()


def test_sampler_refusals():
    from smcnuts_amd import ArmaModel, GaussianTarget, SMCSampler
    asy = SMCSampler(K=2, N=256, target=ArmaModel(), step_size=0.01, seed=1, lkernel="asymptoticLKernel")
    with pytest.raises(NotImplementedError, match="asymptotic"):
        asy.forecast(3)
    with pytest.raises(NotImplementedError, match="asymptotic"):
        asy.forecast_draws(3)
    g = SMCSampler(K=2, N=256, target=GaussianTarget(3), step_size=0.1, seed=1)
    with pytest.raises(NotImplementedError, match="ArmaModel"):
        g.forecast(3)


def test_two_shards():
    """Two in-process shards: every rank returns the one-shard result of the same particles."""
    from smcnuts_amd import ArmaModel, SMCSampler
    from tests.test_sharding import _run_shards
    H, yf, at, S, seed = 5, ref.synthetic_series(5, 6), [0.2, 1.0], 333, 19
    out = {}

    def drive(s):
        s.sample(show_progress=False)
        out[s.comm.rank] = (s.forecast(H, y_future=yf, at=at), s.forecast_draws(H, n_draws=S, seed=seed)) + s.samples.ctx.get_state()[:2]

    _run_shards(lambda c: SMCSampler(target=ArmaModel(), comm=c, K=3, N=1024, step_size=0.01, seed=3), 2, drive, device=True)
    assert sorted(out) == [0, 1]
    x, lw = np.concatenate([out[0][2], out[1][2]]), np.concatenate([out[0][3], out[1][3]])
    t = ArmaModel()
    one = t.forecast(x, H, logw=lw, y_future=yf, at=at)
    sc = ref.mixture_scales(ref.shipped_series(), x, lw, H, yf, np.tile(np.asarray(at), (H, 1)))
    for r in (0, 1):
        _same_forecast(out[r][0], one, sc, f"rank {r} against one shard")
    for k in ("mean", "var", "cdf", "lpd_marginal", "lpd_joint"):
        assert getattr(out[0][0], k).tobytes() == getattr(out[1][0], k).tobytes()
    d0, d1 = out[0][1], out[1][1]
    assert d0.y.tobytes() == d1.y.tobytes() and np.array_equal(d0.ancestors, d1.ancestors)
    od = t.forecast_draws(x, H, S, seed=seed, logw=lw)
    _, amb = ref.ancestors(lw, x.shape[0], S, seed)
    same = od.ancestors == d0.ancestors
    assert (~same).sum() <= amb.sum() + 2
    np.testing.assert_array_equal(d0.y[same], od.y[same])
    assert d0.n_bad == int(np.isnan(d0.y).sum())


def test_draws_bit_for_bit_with_the_parent_of_the_draw_plan():
    """tests/_draws_golden.py: y (NaNs by position), ancestors and n_bad of Context.forecast_draws as recorded on an
    MI355X before smcn_predict_draws and smcn_forecast_draws shared their draw plan."""
    import _draws_golden as g
    g.assert_same_as_parent(g.forecast_results(), "forecast/")
