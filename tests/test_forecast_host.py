"""The arma forecasts without a GPU: the reference against 50 digits, the joint terms against the density's own
log-likelihood, the partials' merge rules, the argument refusals (before any context), ArmaModel(y=), the exports."""
import json

import numpy as np
import pytest

import _forecast as ref

from smcnuts_amd import forecast as fc


def _case(T, H, M, Tn, seed=3):
    ser = ref.shipped_series()[:T] if T > 9 else ref.synthetic_series(T, seed)
    rng = np.random.default_rng(seed + 10)
    X = ref.value_particles(M, seed)
    lw = 2.0 * rng.standard_normal(M)
    lw[::7] = -np.inf
    at = np.sort(rng.normal(0.5, 1.5, (H, Tn)), axis=1) if Tn else None
    return ser, X, lw, ref.synthetic_series(H, seed + 2), at


# ---- the fp64 restatement against 50 digits ------------------------------------------------------------------------------
@pytest.mark.parametrize("T,H,M", [(40, 12, 40), (1, 1, 5), (2, 63, 20), (200, 24, 16)])
def test_reference_laws_against_50_digits(T, H, M):
    ser, X, _, yf, _ = _case(T, H, M, 0)
    err, m, v, bad = ref.laws(ser, X, H)
    a, J = ref.terms(ser, X, yf)
    e_mp, m_mp, v_mp, a_mp, J_mp = ref.points_mp(ser, X, H, yf)
    sc = ref.scales(ser, X, H, yf)
    assert not bad.any()
    got = dict(err=ref.share(err, e_mp, sc["err"]), m=ref.share(m, m_mp, sc["m"]), v=ref.share(v, v_mp, sc["v"]),
               a=ref.share(a, a_mp, sc["a"]), J=ref.share(J, J_mp, sc["J"]))
    print(f"T={T} H={H} M={M}: fp64 against 50 digits, as shares of the magnitudes: {got}")
    assert max(got.values()) <= ref.FLOOR
    assert np.max(np.abs(v - v_mp) / v_mp) <= 4e-15          # (sums of positive terms: a plain relative error)


@pytest.mark.parametrize("T,H,M,Tn", [(40, 12, 40, 4), (9, 5, 65, 16)])
def test_reference_mixture_against_50_digits(T, H, M, Tn):
    ser, X, lw, yf, at = _case(T, H, M, Tn)
    a, b, sc = ref.mixture(ser, X, lw, H, yf, at), ref.mixture_mp(ser, X, lw, H, yf, at), ref.mixture_scales(ser, X, lw, H, yf, at)
    got = {k: ref.share(a[k], b[k], sc[k]) for k in sc}
    print(f"T={T} H={H} M={M} Tn={Tn}: {got}")
    assert max(got.values()) <= ref.FLOOR
    assert a["n_particles"] == int(np.isfinite(lw).sum()) and np.all(a["n_bad"] == 0)


def test_exact_err_T_is_the_rounded_chain():
    ser = ref.shipped_series()[:33]
    X = np.concatenate([ref.value_particles(20, 1), ref.odd_particles()])
    ex = ref.err_T_exact(ser, X)
    e64, _ = ref.err_chain(ser, X)
    mp_err = ref.points_mp(ser, X[:20], 1)[0]
    assert np.all(np.abs(ex[:20] - mp_err) <= 1e-14 * ref.scales(ser, X[:20], 1)["err"])
    assert np.array_equal(np.isnan(ex), np.isnan(e64)) and np.array_equal(np.isinf(ex), np.isinf(e64))


# ---- sum_{j<=h} l_j is a difference of the density's log-likelihoods ------------------------------------------------------
@pytest.mark.parametrize("T,H", [(1, 3), (9, 8), (40, 12)])
def test_joint_terms_are_loglik_differences(T, H):
    ser, X, _, yf, _ = _case(T, H, 30, 0)
    _, J = ref.terms(ser, X, yf)
    base = ref.arma_llik(ser, X)
    for h in range(1, H + 1):
        full = ref.arma_llik(np.concatenate([ser, yf[:h]]), X)
        # two sums of T + h terms each, rounded independently: (T + h + 8) u of their magnitudes
        np.testing.assert_allclose(J[:, h - 1], full - base, rtol=0,
                                   atol=float(np.max((T + h + 8) * 4 * ref.U * (np.abs(full) + np.abs(base) + ref.scales(ser, X, H, yf)["J"][:, h - 1]))))


# ---- merging and finishing the partials -----------------------------------------------------------------------------------
def _finish_equal(a, b, tol=1e-12):
    for k in ("mean", "var", "cdf", "lpd_marginal", "lpd_joint", "n_bad"):
        np.testing.assert_allclose(getattr(a, k), getattr(b, k), rtol=tol, atol=tol, err_msg=k)
    assert a.n_particles == b.n_particles
    np.testing.assert_allclose(a.ess, b.ess, rtol=1e-12)


@pytest.mark.parametrize("cuts", [(20,), (13, 27), (1, 39), (3, 4, 31)])
def test_split_partials_merge_to_the_whole(cuts):
    ser, X, lw, yf, at = _case(40, 6, 40, 3)
    lw[5] += 30.0                                    # the blocks' weight scales differ
    whole = fc.combine_forecast_partials([ref.partials(ser, X, lw, 6, yf, at)], 3, True, at)
    edges = [0, *cuts, 40]
    parts = [ref.partials(ser, X[i:j], lw[i:j], 6, yf, at) for i, j in zip(edges[:-1], edges[1:])]
    _finish_equal(fc.combine_forecast_partials(parts, 3, True, at), whole)
    want = ref.mixture(ser, X, lw, 6, yf, at)
    for k in ("mean", "var", "cdf", "lpd_marginal", "lpd_joint"):
        np.testing.assert_allclose(getattr(whole, k), want[k], rtol=1e-12, atol=1e-12, err_msg=k)
    assert whole.horizon == 6 and np.allclose(whole.sd ** 2, whole.var) and len(whole.summary()) == 6
    assert set(whole.summary()[0]) == {"h", "mean", "sd", "n_bad", "lpd_marginal", "lpd_joint", "cdf"}


def test_a_block_without_contributing_particles_is_neutral():
    ser, X, lw, yf, at = _case(40, 4, 24, 2)
    a = ref.partials(ser, X, lw, 4, yf, at)
    empty = ref.partials(ser, X[:5], np.full(5, -np.inf), 4, yf, at)
    for parts in ([a, empty], [empty, a], [empty, a, empty]):
        got = fc.combine_forecast_partials(parts, 2, True, at)
        _finish_equal(got, fc.combine_forecast_partials([a], 2, True, at), tol=0.0)
    none = fc.combine_forecast_partials([empty], 2, True, at)
    assert none.n_particles == 0 and np.all(np.isnan(none.mean)) and np.all(np.isnan(none.cdf))


def test_bad_particles_make_the_row_nan_and_leave_the_lpd():
    ser, X, lw, yf, at = _case(40, 5, 24, 2)
    lw = np.where(np.isfinite(lw), lw, 0.0)
    Xb = np.concatenate([X, ref.odd_particles()[2:4]])          # sigma = inf, sigma^2 = 0: bad at every horizon
    lwb = np.concatenate([lw, [0.3, -0.2]])
    got = fc.combine_forecast_partials([ref.partials(ser, Xb, lwb, 5, yf, at)], 2, True, at)
    clean = fc.combine_forecast_partials([ref.partials(ser, X, lw, 5, yf, at)], 2, True, at)
    assert np.all(got.n_bad == 2) and np.all(np.isnan(got.mean)) and np.all(np.isnan(got.var)) and np.all(np.isnan(got.cdf))
    # the lpd runs over the other particles; the two bad ones still count in the normalising sum of the weights
    shift = np.log(np.exp(lwb - lwb.max()).sum()) - np.log(np.exp(lw - lwb.max()).sum())
    np.testing.assert_allclose(got.lpd_marginal, clean.lpd_marginal - shift, rtol=1e-12)
    np.testing.assert_allclose(got.lpd_joint, clean.lpd_joint - shift, rtol=1e-12)


def test_combine_refuses_wrong_shapes():
    with pytest.raises(ValueError):
        fc.combine_forecast_partials([], 0, False)
    with pytest.raises(ValueError):
        fc.combine_forecast_partials([np.zeros((4, 11))], 0, False)
    with pytest.raises(ValueError):
        fc.merge_forecast_partials(np.zeros((4, 10)), np.zeros((5, 10)))


# ---- the reference's paths pass their own statistical check (the GPU test asserts the same on the device's) -------------
def test_reference_paths_match_their_laws():
    ser = ref.shipped_series()
    x = np.array([[0.35, 0.6, -0.3, -0.4]])
    S, H, seed = 4096, 8, 11
    y, _ = ref.paths(ser, x, np.zeros(S, dtype=np.int64), seed, H)
    _, m, v, _ = ref.laws(ser, x, H)
    mean, var = y.mean(0), y.var(0, ddof=1)
    assert np.all(np.abs(mean - m[0]) <= 5.0 * np.sqrt(v[0] / S))
    assert np.all(np.abs(var - v[0]) <= 5.0 * v[0] * np.sqrt(2.0 / (S - 1)))
    # a window of slots and another S give the same rows
    y2, _ = ref.paths(ser, x, np.zeros(10, dtype=np.int64), seed, H, s_first=100)
    assert np.array_equal(y2, y[100:110])


# ---- refusals, before any context is made ---------------------------------------------------------------------------------
def test_arguments_are_refused_before_any_context(monkeypatch):
    from smcnuts_amd import ArmaModel, _capi

    def no_context(*a, **k):
        raise AssertionError("a context was made before the refusal")
    monkeypatch.setattr(_capi, "Context", no_context)
    t = ArmaModel()
    x = np.zeros((3, 4))
    for kw in (dict(horizon=0), dict(horizon=513), dict(horizon=2.0), dict(horizon=True), dict(horizon="3"),
               dict(horizon=3, y_future=[1.0, 2.0]), dict(horizon=2, y_future=[1.0, np.nan]), dict(horizon=2, y_future=[1.0, np.inf]),
               dict(horizon=2, y_future=["a", "b"]), dict(horizon=2, at=np.zeros((3, 2))), dict(horizon=2, at=np.zeros(17)),
               dict(horizon=2, at=[0.0, np.nan]), dict(horizon=2, at=np.zeros((2, 2, 2))), dict(horizon=2, at=np.zeros((2, 0))),
               dict(horizon=2, logw=np.zeros(4))):
        with pytest.raises(ValueError):
            t.forecast(x, **kw)
    with pytest.raises(ValueError):
        t.forecast(np.zeros((3, 3)), 2)
    with pytest.raises(ValueError):
        t.forecast_points(x, 0)
    with pytest.raises(ValueError):
        t.forecast_points(x, 2, y_future=[1.0])
    for kw in (dict(n_draws=0), dict(n_draws=2 ** 31), dict(n_draws=1.5), dict(n_draws=2, ancestors=[0, 1, 2]),
               dict(n_draws=2, ancestors=[0, 3]), dict(n_draws=2, ancestors=[0.0, 1.0]), dict(n_draws=2, logw=np.zeros(2))):
        with pytest.raises(ValueError):
            t.forecast_draws(x, 2, **kw)
    with pytest.raises(ValueError):
        t.forecast_draws(x, 0, 4)
    assert t._ctx is None
    # at: a scalar and [Tn] repeat over the horizons
    assert fc.check_at("f", 0.5, 3).shape == (3, 1) and fc.check_at("f", [0.0, 1.0], 3).shape == (3, 2)
    assert fc.check_at("f", None, 3) is None


def test_only_the_arma_target_forecasts():
    from smcnuts_amd import ArmaModel, GaussianTarget, LogisticRegression, PRMwCDModel
    rng = np.random.default_rng(0)
    X = rng.standard_normal((20, 2))
    for t in (GaussianTarget(3), PRMwCDModel(), LogisticRegression(X, (rng.uniform(size=20) < 0.5).astype(float))):
        for name in ("forecast", "forecast_partials", "forecast_points", "forecast_draws"):
            assert not hasattr(t, name)
    for name in ("forecast", "forecast_partials", "forecast_points", "forecast_draws"):
        assert callable(getattr(ArmaModel(), name))


def test_sampler_forecast_preconditions():
    from smcnuts_amd import ArmaModel, GaussianTarget, SMCSampler
    smc = SMCSampler.__new__(SMCSampler)
    smc.lkernel, smc.target = "asymptoticLKernel", ArmaModel()
    with pytest.raises(NotImplementedError, match="asymptotic"):
        smc.forecast(4)
    with pytest.raises(NotImplementedError, match="asymptotic"):
        smc.forecast_draws(4)
    smc.lkernel, smc.target = "forwardsLKernel", GaussianTarget(3)
    with pytest.raises(NotImplementedError, match="ArmaModel"):
        smc.forecast(4)
    with pytest.raises(NotImplementedError, match="ArmaModel"):
        smc.forecast_draws(4)
    smc.target, smc._finalised = ArmaModel(), False
    with pytest.raises(ValueError, match="horizon"):
        smc.forecast(0)
    with pytest.raises(ValueError, match="y_future"):
        smc.forecast(3, y_future=[1.0])
    with pytest.raises(ValueError, match="n_draws"):
        smc.forecast_draws(3, n_draws=0)
    with pytest.raises(RuntimeError, match="finalise"):
        smc.forecast(3)
    with pytest.raises(RuntimeError, match="finalise"):
        smc.forecast_draws(3)
    smc._finalised, smc.K, smc.phi = True, 2, np.array([0.0, 0.5, 0.9])
    with pytest.raises(RuntimeError, match="phi"):
        smc.forecast(3)
    with pytest.raises(RuntimeError, match="phi"):
        smc.forecast_draws(3)


# ---- ArmaModel(y=) -----------------------------------------------------------------------------------------------------------
def test_arma_model_takes_a_series(tmp_path):
    from smcnuts_amd import ArmaModel
    y = ref.synthetic_series(17, 4)
    p = tmp_path / "series.json"
    p.write_text(json.dumps(dict(T=17, y=[float(v) for v in y])))
    a, b = ArmaModel(y=y), ArmaModel(str(p))
    assert a.model_data.tobytes() == b.model_data.tobytes() and a.model_data.dtype == b.model_data.dtype
    assert a.dim == 4 and a.param_names() == b.param_names()
    assert ArmaModel(y=list(y)).model_data.tobytes() == b.model_data.tobytes()
    assert ArmaModel(y=[1.5]).model_data.tolist() == [1.0, 1.5]
    for bad in ([], np.zeros((2, 2)), [1.0, np.nan], [1.0, np.inf], ["a"], 3.0):
        with pytest.raises(ValueError):
            ArmaModel(y=bad)
    with pytest.raises(ValueError, match="not both"):
        ArmaModel(str(p), y=y)
    assert ArmaModel().model_data.tobytes() == ArmaModel(None).model_data.tobytes()


def test_exports_and_bindings():
    import smcnuts_amd
    from smcnuts_amd import SMCSampler, _capi
    assert smcnuts_amd.Forecast is fc.Forecast
    assert smcnuts_amd.combine_forecast_partials is fc.combine_forecast_partials
    for name in ("forecast_set", "forecast_points", "forecast_partials", "forecast_draws"):
        assert callable(getattr(_capi.Context, name))
    for name in ("smcn_forecast_set", "smcn_forecast_dims", "smcn_forecast_points", "smcn_forecast_partials",
                 "smcn_forecast_draws", "smcn_forecast_last_ms"):
        assert name in _capi.SIGNATURES
    assert callable(SMCSampler.forecast) and callable(SMCSampler.forecast_draws)
    from smcnuts_amd import build
    assert "smcn_forecast.hip" in build.UNITS and len(build.UNITS) == 5
