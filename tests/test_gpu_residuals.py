"""The arma one-step residual checks on the device (smcn_residuals_*) against tests/_residuals.py: the per-point chain
against 50 digits and nu_t bit for bit, the mixture's partials across the lane, wavefront, slice, group and window edges,
the ABI's refusals, and the sampler's residuals() on one, two and four shards.

Tolerances: per compared quantity 10 x the error of the fp64 restatement against 50 digits on the test's
own inputs, as a share of the quantity's magnitude (tests/_residuals.py: scales, mixture_scales), with a floor of 1e-14."""
import functools

import numpy as np
import pytest

import _forecast as fref
import _residuals as ref
from _tol import close

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _series(T):
    return fref.shipped_series()[:T] if 9 < T <= 200 else fref.synthetic_series(T, 3)


@functools.lru_cache(maxsize=None)
def _target(T):
    from smcnuts_amd import ArmaModel
    return ArmaModel(y=_series(T))


def _ess_tol(M):
    return 2.0 * (M + 8) * ref.U


def _check(dev, ref64, refmp, scale, what):
    """|dev - 50 digits| <= tolerance x magnitude, the tolerance measured on these inputs -> "tolerance (share used)"."""
    tol = ref.tolerance(ref64, refmp, scale)
    scale = np.broadcast_to(scale, np.shape(refmp))
    used = ref.share(dev, refmp, scale) / tol
    print(f"  {what}: tolerance {tol:.2e}, used {used:.3f}")
    with np.errstate(all="ignore"):
        close(np.asarray(dev) / scale, np.asarray(refmp) / scale, rtol=0.0, atol=tol, what=what,
              err_msg=f"{what} (tolerance {tol:.2e}, used {used:.2f})")
    return f"{tol:.1e} ({used:.2f})"


def _at_floor(dev, want, scale, what):
    """|dev - want| <= 1e-14 x magnitude: the floor of the tolerance, for the cases 50 digits are too slow for."""
    print(f"  {what}: tolerance {ref.FLOOR:.2e}, used {ref.share(dev, want, scale) / ref.FLOOR:.3f}")
    with np.errstate(all="ignore"):
        close(np.asarray(dev) / scale, np.asarray(want) / scale, rtol=0.0, atol=ref.FLOOR, what=what)


# ---- 1. the per-point chain ------------------------------------------------------------------------------------------------
# every T in {1, 2, 3, 65, 200} with every M in {1, 63, 64, 65, 257}; L = T - 1 for the short series, 32, 17 and 16 (the
# edges of the lag builds) and 10 once each, a few lags elsewhere (50 digits cost T M L products)
_POINT_LAGS = {(65, 65): 32, (65, 63): 17, (65, 64): 16, (200, 257): 10, (200, 1): 10}
POINT_CASES = [(T, M, _POINT_LAGS.get((T, M), min(T - 1, 3))) for T in (1, 2, 3, 65, 200) for M in (1, 63, 64, 65, 257)]


@pytest.mark.parametrize("T,M,L", POINT_CASES)
def test_points_against_50_digits(T, M, L):
    ser, t = _series(T), _target(T)
    X = fref.value_particles(M, T + M)
    odd = fref.odd_particles()
    allx = np.concatenate([X[:M // 2], odd, X[M // 2:]])              # the odd rows sit between their neighbours
    val = np.r_[0:M // 2, M // 2 + len(odd):M + len(odd)]
    got = t.residual_points(allx, lags=L)
    assert set(got) == ({"nu", "r", "rho", "Q"} if L else {"nu", "r"})
    assert got["nu"].shape == got["r"].shape == (len(allx), T) and (not L or got["rho"].shape == (len(allx), L))
    # nu_t has the bits of y_t - err_t of the exact-fma chain, |theta| > 1 included
    finite_rows = np.all(np.isfinite(allx), axis=1)
    np.testing.assert_array_equal(got["nu"][finite_rows], ref.nu_exact(ser, allx[finite_rows]))
    # classification: a row with a non-finite coordinate is NaN throughout, no other value of nu or r is
    for k in got:
        assert np.all(np.isnan(got[k][~finite_rows])), k
    assert not np.isnan(got["nu"][finite_rows]).any() and not np.isnan(got["r"][finite_rows]).any()
    o0 = M // 2
    assert np.all(np.abs(got["r"][o0 + 3]) > 1e100)                  # s = -400: finite residuals of an absurd size
    # the values
    p64, pmp, sc = ref.points(ser, X, L), ref.points_mp(ser, X, L), ref.scales(ser, X, L)
    _check(got["nu"][val], p64["nu"], pmp["nu"], sc["nu"], "points nu_t")
    _check(got["r"][val], p64["r"], pmp["r"], sc["r"], "points r_t")
    if L:
        _check(got["rho"][val], p64["rho"], pmp["rho"], sc["rho"], "points rho_k")
        _check(got["Q"][val], p64["Q"], pmp["Q"], sc["Q"], "points Q")
    # sum_t l_t from r is the density's log-likelihood
    r = got["r"][val]
    l_sum = ((-0.5 * ref.LOG2PI - X[:, 3])[:, None] - 0.5 * r * r).sum(1)
    s_llik = sc["l"].sum(1)
    b64 = fref.arma_llik(ser, X)
    _check(l_sum, b64, pmp["llik"], s_llik, "sum of the one-step terms")
    _check(t.logpdf_parts(X)[1], b64, pmp["llik"], s_llik, "the density's log-likelihood")


# ---- 2. the mixture's partials ---------------------------------------------------------------------------------------------
# (T, L, Tn, M): every L in {0, 1, 10, 32}, Tn in {0, 1, 8}, M across the lane, wavefront, slice and group-of-16 edges
PARTIAL_CASES = [(9, 0, 0, 1), (9, 1, 1, 64), (33, 10, 8, 255), (40, 32, 1, 256), (33, 10, 0, 257), (9, 1, 8, 4097),
                 (65, 32, 8, 65)]


def _partial_inputs(T, L, Tn, M):
    rng = np.random.default_rng(T * 1000 + M)
    X = fref.value_particles(M, T + L + M)
    lw = 2.0 * rng.standard_normal(M)
    if M > 2:
        lw[::5] = -np.inf
        lw[2::11] = -790.0                            # (exp(lw - max) underflows to 0)
    q_at = None
    if Tn:
        Q = ref.points(_series(T), X, L)["Q"][np.isfinite(lw)]
        q_at = np.quantile(Q, np.linspace(0.1, 0.9, Tn)) if len(Q) > 1 else np.linspace(0.5, 2.0, Tn) * Q[0]
    return X, lw, q_at


def _check_residuals(got, ser, X, lw, L, q_at, what):
    a, b, sc = ref.mixture(ser, X, lw, L, q_at), ref.mixture_mp(ser, X, lw, L, q_at), ref.mixture_scales(ser, X, lw, L, q_at)
    keys = ref.KEYS_T + ((ref.KEYS_L + ("ljung_box", "ljung_box_var")) if L else ())
    tols = {k: _check(got[k], a[k], b[k], sc[k], f"{what} {k}") for k in keys}
    assert got["n_particles"] == a["n_particles"] and np.all(got["n_bad"] == 0)
    close(got["ess"], a["ess"], rtol=_ess_tol(X.shape[0]), what=f"{what} ess")
    if L:
        assert got["n_bad_acf"] == 0
        if q_at is not None:
            # an indicator: a particle whose Q lies within rounding of a threshold may fall on either side
            M = X.shape[0]
            with np.errstate(all="ignore"):
                d = np.abs(got["exceed"] - b["exceed"])
            assert np.all(d <= ref.FLOOR * M + a["exceed_amb"]), (what, d, a["exceed_amb"])
    return tols


@pytest.mark.parametrize("T,L,Tn,M", PARTIAL_CASES)
def test_partials_against_the_reference(T, L, Tn, M):
    from smcnuts_amd.residuals import combine_residual_partials
    ser, t = _series(T), _target(T)
    X, lw, q_at = _partial_inputs(T, L, Tn, M)
    levels = tuple(np.linspace(0.9, 0.1, Tn)) if Tn else ()
    ctx = t._context(M)
    ctx.residuals_set(L, q_at)
    assert ctx.residuals_dims() == (T, L, 20, Tn)
    p1 = t.residual_partials(X, lw, L, q_at)
    p2 = t.residual_partials(X, lw, L, q_at)
    assert p1.shape == (1 + T + (L + 1 if L else 0), 20) and p1.tobytes() == p2.tobytes()
    res = combine_residual_partials([p1], L, levels)
    tols = _check_residuals(ref.of(res), ser, X, lw, L, q_at, "partials")
    print(f"T={T} L={L} Tn={Tn} M={M}: tolerances {tols}")
    assert (res.acf is None) == (L == 0) and res.lppd == res.lpd.sum()
    # the layout's constant columns
    assert np.all(p1[1:, 12:] == 0.0) if not Tn else np.all(p1[1:T + L + 1, 12:] == 0.0) and np.all(p1[T + L + 1, 12 + Tn:] == 0.0)
    if L:
        G = p1[1 + T:]
        assert np.all(G[:, 0] == -np.inf) and np.all(G[:, 1] == 0.0) and np.all(np.isnan(G[:, 8])) and np.all(G[:, [7, 9, 10, 11]] == 0.0)
    if M > 1:
        # halves merged on the host
        k = M // 2 + 1
        halves = [t.residual_partials(X[:k], lw[:k], L, q_at), t.residual_partials(X[k:], lw[k:], L, q_at)]
        _check_residuals(ref.of(combine_residual_partials(halves, L, levels)), ser, X, lw, L, q_at, "merged halves")
    # classification: bad particles with a weight, |theta| > 1 ones without
    odd = fref.odd_particles()
    Xb = np.concatenate([X, odd, [[0.3, 0.4, 0.2, 800.0], [0.3, 0.4, 0.2, -800.0]]])
    lwb = np.concatenate([np.where(np.isfinite(lw), lw, 0.1), [-np.inf, -np.inf, 0.3, -0.2, 0.0, 0.1, -0.1, 0.2, 0.0, 0.1]])
    g = t.residuals(Xb, logw=lwb, lags=L, levels=levels or (0.05,))
    want = ref.mixture(ser, Xb, lwb, L, q_at)
    np.testing.assert_array_equal(g.n_bad, want["n_bad"])
    # (theta = -inf is bad from t = 2 on: err_1 does not see theta)
    assert g.n_bad[0] == 5 and np.all(g.n_bad[1:] == 6) and g.n_particles == M + 8
    for k in ("mean", "var", "z", "z_sd", "pit"):
        assert np.all(np.isnan(getattr(g, k))), k
    if L:
        assert g.n_bad_acf == want["n_bad_acf"] and np.all(np.isnan(g.acf)) and np.isnan(g.ljung_box) and np.all(np.isnan(g.exceed))
    # particles without a weight add nothing: the same bits with and without them
    p3 = t.residual_partials(np.concatenate([X, odd[:2]]), np.concatenate([lw, [-np.inf, -np.inf]]), L, q_at)
    if -(-(M + 2) // 256) == -(-M // 256):
        assert p3.tobytes() == p1.tobytes()


def test_a_particle_that_goes_bad_midway():
    """|theta| = 1.6 on a series of 1600 values: err_t overflows near t = 1500.  The rows before stay clean, the rows from
    there on report NaN moments and their lpd over the other particles; the lag rows report NaN.  Between the step where
    the runaway err_t^2 stops being representable (about 1e154) and the step where err_t itself overflows the particle
    is not bad by the definition (include/smcnuts_hip.h says so): there n_bad is 0, the first moments are not NaN and
    the second moments (var, z_sd) are inf or NaN."""
    T, L = 1600, 1
    ser, t = _series(T), _target(T)
    X = np.concatenate([fref.value_particles(9, 3), [[0.2, 0.5, 1.6, -0.4]]])
    lw = np.linspace(-1.0, 1.0, 10)
    bad = ref.points(ser, X, L)["bad"]
    t0 = int(np.argmax(bad[9]))                                       # (0-based: the first bad step is t0 + 1)
    assert 1400 < t0 < T - 10 and not bad[:9].any() and bad[9, t0:].all()
    res = t.residuals(X, logw=lw, lags=L)
    np.testing.assert_array_equal(res.n_bad, (np.arange(T) >= t0).astype(float))
    # (a second moment is clean while the runaway particle's square is representable: 1.6^t below 1e140)
    pts = ref.points(ser, X, L)
    n2 = int(np.argmax(np.maximum(np.abs(pts["nu"][9]), np.abs(pts["r"][9])) >= 1e140))
    assert 600 < n2 < t0
    for k, n in (("mean", t0), ("var", n2), ("z", t0), ("z_sd", n2), ("pit", t0)):
        v = getattr(res, k)
        assert not np.isnan(v[:n]).any() and np.all(np.isfinite(v[:n2])) and np.all(np.isnan(v[t0:])), k
    assert np.all(np.isfinite(res.lpd)) and res.n_bad_acf == 1 and np.all(np.isnan(res.acf)) and np.isnan(res.ljung_box)
    # the values while the runaway particle is small, the lpd everywhere (its density underflows long before it is bad)
    a, b, sc = ref.mixture(ser, X, lw, 0), ref.mixture_mp(ser, X, lw, 0), ref.mixture_scales(ser, X, lw, 0)
    got = ref.of(res)
    n = 400
    for k in ("mean", "var", "z", "z_var", "pit"):
        _check(got[k][:n], a[k][:n], b[k][:n], sc[k][:n], f"going bad midway: {k}")
    _check(got["lpd"], a["lpd"], b["lpd"], sc["lpd"], "going bad midway: lpd")


def test_no_contributing_particle():
    t = _target(9)
    res = t.residuals(fref.value_particles(5, 1), logw=np.full(5, -np.inf), lags=2)
    assert res.n_particles == 0 and np.all(np.isnan(res.mean)) and np.all(np.isnan(res.lpd)) and np.all(np.isnan(res.acf))
    assert np.all(np.isnan(res.exceed)) and res.n_bad_acf == 0


def test_the_window_edge():
    """T = 13 000, L = 2, M = 8 193: 33 slices, at most 16 per window of the slab.  50 digits would cost minutes here, so
    the reference is the NumPy restatement in one pass over t (tests/_residuals.py: mixture_stream; the time rows at both
    ends and every 97th between), compared at the floor of the project's tolerance, 1e-14 of the magnitude."""
    T, L, M = 13000, 2, 8193
    ser = fref.synthetic_series(T, 11)
    from smcnuts_amd import ArmaModel
    t = ArmaModel(y=ser)
    rng = np.random.default_rng(5)
    X = fref.value_particles(M, 77)
    X[:, 2] *= 0.5                                                    # (|theta| <= 0.475: the chain forgets its rounding)
    lw = 2.0 * rng.standard_normal(M)
    lw[::5] = -np.inf
    q_at = [2000.0, 12000.0]                                          # (near the 30 % and 70 % points of these particles' Q)
    p1 = t.residual_partials(X, lw, L, q_at)
    assert p1.shape == (1 + T + L + 1, 20) and p1.tobytes() == t.residual_partials(X, lw, L, q_at).tobytes()
    from smcnuts_amd.residuals import combine_residual_partials
    got = ref.of(combine_residual_partials([p1], L, (0.5, 0.1)))
    at_rows = np.unique(np.r_[0:40, 40:T - 40:97, T - 40:T])
    a, sc = ref.mixture_stream(ser, X, lw, L, q_at, at_rows)
    tol = ref.FLOOR
    for k in ref.KEYS_T + ref.KEYS_L + ("ljung_box", "ljung_box_var"):
        sel = at_rows if k in ref.KEYS_T else slice(None)
        _at_floor(np.atleast_1d(got[k])[sel], np.atleast_1d(a[k])[sel], np.atleast_1d(sc[k])[sel], f"window edge {k}")
        assert np.all(np.isfinite(np.asarray(got[k])))
    print(f"  window edge exceed: |device - NumPy| {np.abs(got['exceed'] - a['exceed'])}, ambiguous {a['exceed_amb']}")
    assert np.all(np.abs(got["exceed"] - a["exceed"]) <= tol + a["exceed_amb"])
    assert got["n_particles"] == a["n_particles"] and np.all(got["n_bad"] == 0) and got["n_bad_acf"] == 0
    # the windows' slices in order: the first 4096 particles alone are the first window's 16 slices
    k = 16 * 256
    halves = [t.residual_partials(X[:k], lw[:k], L, q_at), t.residual_partials(X[k:], lw[k:], L, q_at)]
    m = ref.of(combine_residual_partials(halves, L, (0.5, 0.1)))
    for key in ref.KEYS_T + ref.KEYS_L:
        sel = at_rows if key in ref.KEYS_T else slice(None)
        _at_floor(m[key][sel], got[key][sel], sc[key][sel], f"window edge, merged {key}")


# ---- the C ABI's refusals -------------------------------------------------------------------------------------------------
def test_abi_refusals():
    from smcnuts_amd import ArmaModel, GaussianTarget
    from smcnuts_amd._capi import SmcnError, dptr
    ctx = ArmaModel(y=_series(9))._context(4)                         # (a context of its own: nothing set yet)
    big = np.zeros(20 * 64)                                           # (room for any block of this series)
    with pytest.raises(SmcnError, match="smcn_residuals_set first"):
        ctx.call("smcn_residuals_partials", None, None, ctx.N, dptr(big))
    with pytest.raises(SmcnError, match="smcn_residuals_set first"):
        ctx.residuals_dims()
    for args, msg in (((-1, None, 0), r"0\.\.32"), ((33, None, 0), r"0\.\.32"), ((9, None, 0), r"L = 9 lags need a series of at least L \+ 1"),
                      ((2, None, 9), r"0\.\.8"), ((2, None, 1), "thresholds"), ((0, dptr(np.ones(1)), 1), "L >= 1"),
                      ((2, dptr(np.array([1.0, np.nan])), 2), "not finite"), ((2, dptr(np.array([np.inf])), 1), "not finite")):
        with pytest.raises(SmcnError, match=msg):
            ctx.call("smcn_residuals_set", *args)
    ctx.residuals_set(2, [1.0])
    with pytest.raises(SmcnError, match="resident"):
        ctx.call("smcn_residuals_partials", None, None, 3, dptr(big))
    with pytest.raises(SmcnError, match="bad arguments"):
        ctx.call("smcn_residuals_points", None, 1, None)
    long = ArmaModel(y=np.zeros(13104))._context(4)
    long.residuals_set(0)                                             # (13104 + 0 + 2) * 20 = 2^18 - 24
    with pytest.raises(SmcnError, match=r"too long: \(T \+ L \+ 2\) \* 20 must not exceed 2\^18"):
        long.residuals_set(2)
    g = GaussianTarget(3)._context(4)
    for name, args in (("smcn_residuals_set", (2, None, 0)), ("smcn_residuals_dims", (None, None, None, None)),
                       ("smcn_residuals_points", (None, 1, None)), ("smcn_residuals_partials", (None, None, 4, None))):
        with pytest.raises(SmcnError, match=f"{name}: one-step residual checks cover SMCN_MODEL_ARMA contexts only"):
            g.call(name, *args)
    assert ctx.residuals_last_ms() >= 0.0


# ---- 3. through the sampler -------------------------------------------------------------------------------------------------
FIT = dict(K=8, N=4096, step_size=0.02, seed=1)


@functools.lru_cache(maxsize=None)
def _fit(seasonal=False):
    from smcnuts_amd import ArmaModel, SMCSampler
    y = ref.seasonal_series(200, 0) if seasonal else fref.synthetic_series(200, 0)
    smc = SMCSampler(target=ArmaModel(y=y), **FIT)
    with pytest.raises(RuntimeError, match="sample"):
        smc.residuals()
    smc.sample(show_progress=False)
    return smc, y


def _same_residuals(a, b, sc, what):
    for k in sc:
        if k == "exceed":
            continue
        with np.errstate(all="ignore"):
            close(np.asarray(a[k]) / sc[k], np.asarray(b[k]) / sc[k], rtol=0.0, atol=ref.FLOOR, what=f"{what} {k}")
    np.testing.assert_array_equal(a["n_bad"], b["n_bad"])
    assert a["n_particles"] == b["n_particles"] and a["n_bad_acf"] == b["n_bad_acf"]
    close(a["ess"], b["ess"], rtol=_ess_tol(a["n_particles"]), what=f"{what} ess")


def test_through_the_sampler():
    smc, y = _fit()
    before = smc.summary()
    res = smc.residuals()
    assert res.T == 200 and res.lags == 10 and res.levels == (0.05,) and res.lppd == res.lpd.sum()
    close(res.critical[0], 18.307038053275146, rtol=1e-12, what="the 5 % critical value on 10 degrees of freedom")
    x, lw = smc.samples.ctx.get_state()[:2]
    q_at = np.array(res.critical)
    got = ref.of(res)
    a, sc = ref.mixture(y, x, lw, 10, q_at), ref.mixture_scales(y, x, lw, 10, q_at)
    # against the reference applied to get_state(): 50 digits would cost a minute for 4096 particles, so the NumPy
    # restatement, at the floor of the project's tolerance, 1e-14 of the magnitude
    tol = ref.FLOOR
    for k in ref.KEYS_T + ref.KEYS_L + ("ljung_box", "ljung_box_var"):
        _at_floor(got[k], a[k], sc[k], f"sampler {k}")
    print(f"  sampler exceed: |device - NumPy| {abs(got['exceed'][0] - a['exceed'][0])}, ambiguous {a['exceed_amb'][0]}")
    assert abs(got["exceed"][0] - a["exceed"][0]) <= tol + a["exceed_amb"][0]
    _same_residuals(got, ref.of(smc.target.residuals(x, logw=lw)), sc, "resident against uploaded")
    print(f"Q = {res.ljung_box:.2f} +- {res.ljung_box_sd:.2f}, exceed {res.exceed[0]:.3f}, lppd {res.lppd:.2f}, ess {res.ess:.0f}")
    assert res.exceed[0] < 0.5
    assert np.all(res.n_bad == 0) and np.all((res.pit > 0) & (res.pit < 1)) and len(res.summary()["rows"]) == 200
    r2 = smc.residuals(lags=0)
    assert r2.acf is None and r2.lpd.tobytes() == res.lpd.tobytes()
    after = smc.summary()
    for k in ("mean", "sd", "quantiles"):
        assert np.asarray(getattr(before, k)).tobytes() == np.asarray(getattr(after, k)).tobytes()


def test_a_seasonal_series_is_flagged():
    smc, _ = _fit(True)
    res = smc.residuals()
    print(f"Q = {res.ljung_box:.1f} +- {res.ljung_box_sd:.1f}, exceed {res.exceed[0]:.3f}, acf {np.round(res.acf, 2)}")
    assert res.exceed[0] > 0.9 and abs(res.acf[3]) > res.acf_band


def test_sampler_refusals():
    from smcnuts_amd import ArmaModel, GaussianTarget, SMCSampler
    asy = SMCSampler(K=2, N=256, target=ArmaModel(), step_size=0.01, seed=1, lkernel="asymptoticLKernel")
    with pytest.raises(NotImplementedError, match="asymptotic"):
        asy.residuals()
    g = SMCSampler(K=2, N=256, target=GaussianTarget(3), step_size=0.1, seed=1)
    with pytest.raises(NotImplementedError, match="ArmaModel"):
        g.residuals()


@pytest.mark.parametrize("world", [2, 4])
def test_shards(world):
    """In-process shards: every rank returns the one-shard result of the same particles."""
    from smcnuts_amd import ArmaModel, SMCSampler
    from tests.test_sharding import _run_shards
    y = fref.synthetic_series(200, 0)
    out = {}

    def drive(s):
        s.sample(show_progress=False)
        out[s.comm.rank] = (s.residuals(levels=(0.05, 0.5)),) + s.samples.ctx.get_state()[:2]

    _run_shards(lambda c: SMCSampler(target=ArmaModel(y=y), comm=c, K=3, N=1024, step_size=0.02, seed=3), world, drive, device=True)
    assert sorted(out) == list(range(world))
    x, lw = np.concatenate([out[r][1] for r in range(world)]), np.concatenate([out[r][2] for r in range(world)])
    one = ref.of(ArmaModel(y=y).residuals(x, logw=lw, levels=(0.05, 0.5)))
    sc = ref.mixture_scales(y, x, lw, 10)
    for r in range(world):
        _same_residuals(ref.of(out[r][0]), one, sc, f"rank {r} against one shard")
        assert np.all(np.abs(out[r][0].exceed - one["exceed"]) <= ref.FLOOR * len(lw))
    for k in ("mean", "var", "lpd", "z", "pit", "acf", "exceed"):
        assert all(np.asarray(getattr(out[r][0], k)).tobytes() == np.asarray(getattr(out[0][0], k)).tobytes() for r in range(world))
