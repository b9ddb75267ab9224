"""Pointwise criteria, host side (no GPU): the NumPy reference against mpmath, combine_pointwise_partials against the
reference on partials built in NumPy by the documented layout, compare(), and the unsupported targets."""
import numpy as np
import pytest

import _pointwise as pw


def _matrix(M, n, seed, ninf=0, spread=3.0):
    rng = np.random.default_rng(seed)
    ll = -np.abs(spread * rng.standard_normal((M, n))) - 0.5
    for k in range(ninf):
        ll[rng.integers(M), rng.integers(n)] = -np.inf
    lw = 3.0 * rng.standard_normal(M)
    mean = np.exp(rng.standard_normal((M, n)))
    return ll, lw, mean


def _mp_reference(ll, lw, mean):
    import mpmath as mp
    with mp.workdps(40):
        keep = np.isfinite(lw)
        w = [mp.exp(mp.mpf(float(v))) for v in lw[keep]]
        tot = mp.fsum(w)
        W = [v / tot for v in w]
        llk, mk = ll[keep], mean[keep]
        out = {k: [] for k in pw.FIELDS}
        for i in range(ll.shape[1]):
            col = llk[:, i]
            bad = bool(np.any(np.isneginf(col)))
            t = [mp.mpf(float(v)) if np.isfinite(v) else None for v in col]
            lik = mp.fsum(Wp * mp.exp(v) for Wp, v in zip(W, t) if v is not None)
            lppd = float(mp.log(lik)) if lik > 0 else -np.inf
            out["lppd_i"].append(lppd)
            if bad:
                for k, v in (("mean_loglik_i", -np.inf), ("p_waic_i", np.nan), ("elpd_waic_i", np.nan),
                             ("elpd_loo_i", -np.inf), ("loo_ess_i", 0.0), ("fitted_i", np.nan)):
                    out[k].append(v)
                continue
            mu = mp.fsum(Wp * v for Wp, v in zip(W, t))
            var = mp.fsum(Wp * (v - mu) ** 2 for Wp, v in zip(W, t))
            r = [Wp * mp.exp(-v) for Wp, v in zip(W, t)]
            out["mean_loglik_i"].append(float(mu))
            out["p_waic_i"].append(float(var))
            out["elpd_waic_i"].append(float(mp.log(lik) - var))
            out["elpd_loo_i"].append(float(-mp.log(mp.fsum(r))))
            out["loo_ess_i"].append(float(mp.fsum(r) ** 2 / mp.fsum(v * v for v in r)))
            out["fitted_i"].append(float(mp.fsum(Wp * mp.mpf(float(v)) for Wp, v in zip(W, mk[:, i]))))
        return {k: np.array(v) for k, v in out.items()}


def _same(got, want, rtol, what):
    for k in pw.FIELDS:
        g, w = np.asarray(got[k] if isinstance(got, dict) else getattr(got, k)), want[k]
        np.testing.assert_array_equal(np.isnan(g), np.isnan(w), err_msg=f"{what} {k}")
        fin = np.isfinite(w)
        np.testing.assert_array_equal(g[~fin & ~np.isnan(w)], w[~fin & ~np.isnan(w)], err_msg=f"{what} {k}")
        np.testing.assert_allclose(g[fin], w[fin], rtol=rtol, atol=rtol, err_msg=f"{what} {k}")


@pytest.mark.parametrize("M,n,ninf", [(1, 3, 0), (7, 5, 0), (40, 6, 3), (40, 4, 0)])
def test_reference_against_mpmath(M, n, ninf):
    ll, lw, mean = _matrix(M, n, 10 * M + n, ninf)
    if M == 40 and ninf == 0:
        lw[::3] = -np.inf                                       # a third of the particles do not contribute ..
        ll[0, :] = -np.inf                                      # .. and one of them sits where every term overflows
        ll = ll * 40.0                                          # |ll| of a few hundred: exp(ll) underflows unshifted
    ref = pw.criteria_reference(ll, lw, mean)
    _same(ref, _mp_reference(ll, lw, mean), 1e-12, "reference")
    assert ref["n_particles"] == int(np.sum(np.isfinite(lw)))


def test_reference_large_magnitudes():
    """|ll| of 1e6 and log-weights shifted by +-1e5: finite, and unchanged by the shift."""
    ll, lw, mean = _matrix(30, 4, 3)
    ll = ll - 1.0e6
    a = pw.criteria_reference(ll, lw, mean)
    for sh in (1.0e5, -1.0e5):
        b = pw.criteria_reference(ll, (lw + sh) - sh + sh, mean)
        _same(b, a, 1e-9, "shift")
    assert np.all(np.isfinite(a["lppd_i"])) and np.all(np.isfinite(a["elpd_loo_i"]))


SPLITS = [(1000,), (1, 999), (64, 936), (333, 333, 334)]


@pytest.mark.parametrize("ninf", [0, 5])
@pytest.mark.parametrize("split", SPLITS)
def test_combine_against_reference(split, ninf):
    """Partials built in NumPy by the documented column layout, per consecutive slice of the particles (each slice with its
    own weight maximum and shift), merged in order and finished: the reference on the whole matrix."""
    from smcnuts_amd import combine_pointwise_partials
    ll, lw, mean = _matrix(1000, 9, 5, ninf)
    ll = ll * 20.0
    lw[10:400:7] = -np.inf
    lw[500:] += 40.0                                             # the slices' weight maxima differ by many e-folds
    parts, m0 = [], 0
    for m in split:
        parts.append(pw.numpy_partials(ll[m0:m0 + m], lw[m0:m0 + m], mean[m0:m0 + m]))
        m0 += m
    got = combine_pointwise_partials(parts)
    ref = pw.criteria_reference(ll, lw, mean)
    _same(got, ref, 1e-10, f"split {split}")
    assert got.n_particles == ref["n_particles"]
    np.testing.assert_allclose(got.ess, ref["ess"], rtol=1e-12)
    fin = np.isfinite(ref["elpd_waic_i"])
    if ninf == 0:
        np.testing.assert_allclose(got.elpd_waic, np.sum(ref["elpd_waic_i"]), rtol=1e-12)
        np.testing.assert_allclose(got.se_elpd_loo, np.sqrt(9 * np.var(ref["elpd_loo_i"], ddof=1)), rtol=1e-12)
        assert got.summary()["n_nonfinite"] == 0
    else:
        assert not np.all(fin) and got.summary()["n_nonfinite"] == int(np.sum(~fin))


def test_combine_empty_shard_and_shape_errors():
    from smcnuts_amd import combine_pointwise_partials
    ll, lw, mean = _matrix(20, 3, 8)
    full = pw.numpy_partials(ll, lw, mean)
    none = pw.numpy_partials(ll[:5], np.full(5, -np.inf), mean[:5])
    a, b = combine_pointwise_partials([none, full, none]), combine_pointwise_partials([full])
    for k in pw.FIELDS:
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k))
    assert np.all(np.isnan(combine_pointwise_partials([none]).lppd_i))
    with pytest.raises(ValueError):
        combine_pointwise_partials([full, full[:-1]])
    with pytest.raises(ValueError):
        combine_pointwise_partials([])


def test_ill_conditioned_variance_merges():
    """Terms of size 1.8e6 with a spread of 1.8 (the GPU suite's case, here as numbers): the merged shifted moments give
    the exact variance to 1e-12 where sum W ll^2 - mean^2 is off by 1e-3."""
    from smcnuts_amd import combine_pointwise_partials
    rng = np.random.default_rng(2)
    col = -1.8e6 + 1.8 * rng.random(2000)
    ll = col[:, None]
    parts = [pw.numpy_partials(ll[:700]), pw.numpy_partials(ll[700:1400]), pw.numpy_partials(ll[1400:])]
    got = combine_pointwise_partials(parts).p_waic_i[0]
    exact = pw.exact_variance(col)
    assert abs(got - exact) < 1e-11 * exact
    assert abs(pw.naive_variance(col) - exact) > 1e-5


def test_compare():
    from smcnuts_amd import combine_pointwise_partials, compare
    la, wa, ma = _matrix(50, 12, 1)
    lb, wb, mb = _matrix(70, 12, 2, spread=5.0)
    a, b = (combine_pointwise_partials([pw.numpy_partials(*v)]) for v in ((la, wa, ma), (lb, wb, mb)))
    c = compare(a, b)
    d = a.elpd_waic_i - b.elpd_waic_i
    np.testing.assert_allclose(c["elpd_waic_diff"], a.elpd_waic - b.elpd_waic, rtol=1e-12)
    np.testing.assert_allclose(c["se_elpd_waic_diff"], np.sqrt(12 * np.var(d, ddof=1)), rtol=1e-12)
    dl = a.elpd_loo_i - b.elpd_loo_i
    np.testing.assert_allclose(c["elpd_loo_diff"], np.sum(dl), rtol=1e-12)
    np.testing.assert_allclose(c["se_elpd_loo_diff"], np.sqrt(12 * np.var(dl, ddof=1)), rtol=1e-12)
    assert compare(a, a)["elpd_waic_diff"] == 0.0
    short = combine_pointwise_partials([pw.numpy_partials(la[:, :5], wa, ma[:, :5])])
    with pytest.raises(ValueError, match="different numbers of observations"):
        compare(a, short)


def test_unsupported_targets_raise_before_any_context():
    from smcnuts_amd import (ArmaModel, CategoricalRegression, GaussianTarget, HierarchicalGLM, HostTarget,
                             OrdinalRegression, PRMwCDModel)
    import _glm
    rng = np.random.default_rng(0)
    X = rng.standard_normal((30, 2))
    yb = (rng.random(30) < 0.5).astype(float)
    targets = [GaussianTarget(3), ArmaModel(), PRMwCDModel(), HierarchicalGLM(X, yb, np.arange(30) % 3),
               CategoricalRegression(X, np.arange(30) % 3), OrdinalRegression(X, np.arange(30) % 3),
               HostTarget(_glm.GLMNumpy(X, yb))]
    for t in targets:
        x = np.zeros((2, t.dim))
        for call in (lambda: t.pointwise_loglik(x), lambda: t.pointwise(x), lambda: t.pointwise(x, np.zeros(2))):
            with pytest.raises(NotImplementedError, match="GLMTarget"):
                call()
        assert getattr(t, "_ctx", None) is None


def test_glm_argument_checks_come_first():
    from smcnuts_amd import LogisticRegression
    rng = np.random.default_rng(0)
    t = LogisticRegression(rng.standard_normal((10, 2)), (rng.random(10) < 0.5).astype(float))
    with pytest.raises(ValueError):
        t.pointwise_loglik(np.zeros((4, 7)))
    with pytest.raises(ValueError):
        t.pointwise(np.zeros((4, 7)))
    assert t._ctx is None
