"""Posterior predictive draws, the parts that need no GPU: predict_draws' argument checks (all before a context
exists), the PredictiveDraws helpers, and the NumPy restatement of the samplers (tests/_predict_draws.py) ALONE against
the exact moments of each law: the sample mean within 6 sqrt(var / n) of the exact mean and the sample variance within 6
of its own standard errors, sqrt((mu4 - var^2) / n) with mu4 the law's exact fourth central moment (a false alarm of
about 2e-9 per assertion under the normal approximation).  Seeds are fixed: the checks are deterministic."""
import math

import numpy as np
import pytest

import _predict_draws as dr

N = 20000


def _moments_ok(y, mean, var, mu4, what):
    y = np.asarray(y, dtype=np.float64)
    assert not np.any(np.isnan(y)), what
    n = y.size
    assert abs(np.mean(y) - mean) <= 6.0 * math.sqrt(var / n), f"{what}: mean {np.mean(y)} against {mean}"
    se_v = math.sqrt(max(mu4 - var * var, 0.0) / n)
    assert abs(np.var(y) - var) <= 6.0 * se_v + var / n, f"{what}: variance {np.var(y)} against {var}"


def _keys(n, m=4):
    return np.arange(n // m)[:, None] + np.zeros((1, m), dtype=np.int64), np.zeros((n // m, 1), dtype=np.int64) + np.arange(m)[None, :]


def test_philox_restated():
    from oracle import oracle as orc
    for seed, it, p, st in [(0, 0, 0, 16), (1234, 7, 3, 17), (2 ** 40 + 5, 199, 64, 18), (99, 2 ** 20, 2 ** 31 + 1, 19)]:
        want = orc.philox_uniforms(seed, it, p, st, 0, 11)
        got = dr.philox_uniform(seed, it, p, st, np.arange(11))
        np.testing.assert_array_equal(got, want)
    from smcnuts_amd.predict import _philox_uniform
    assert _philox_uniform(1234, 0, 0, 16, 0) == orc.philox_uniforms(1234, 0, 0, 16, 0, 1)[0]
    assert _philox_uniform(2 ** 40 + 5, 3, 9, 17, 5) == orc.philox_uniforms(2 ** 40 + 5, 3, 9, 17, 5, 1)[0]


def test_reference_bernoulli_and_normal():
    s, i = _keys(N)
    y, _ = dr.bernoulli(np.full(s.shape, 0.3), 0.0, 11, s, i)
    _moments_ok(y, 0.3, 0.21, 0.3 * 0.7 * (1 - 3 * 0.21), "bernoulli")
    y, _ = dr.normal(1.5, 0.0, 2.0, 0.0, 12, s, i)
    _moments_ok(y, 1.5, 4.0, 3 * 16.0, "normal")


@pytest.mark.parametrize("mu", [0.3, 9.99, 10.0, 37.5, 1.0e6])
def test_reference_poisson(mu):
    s, i = _keys(N)
    y, amb, att = dr.poisson(np.full(s.shape, mu), 0.0, 21, s, i)
    _moments_ok(y, mu, mu, mu + 3 * mu * mu, f"poisson {mu}")
    assert np.all(y == np.floor(y)) and np.all(y >= 0) and att.max() <= 16
    assert np.sum(amb) <= 2, "exact inputs: only a comparison within rounding of its threshold is ambiguous"


@pytest.mark.parametrize("phi", [0.5, 3.7, 1.0e8])
def test_reference_nb2(phi):
    s, i = _keys(N)
    mu = 12.5
    y, amb, (ng, npo) = dr.nb2(np.full(s.shape, mu), 0.0, phi, 0.0, 31, s, i)
    var = mu + mu * mu / phi
    # NB2 with r = phi, p = phi / (phi + mu): fourth central moment from the cumulants
    q = mu / (phi + mu)
    p = 1.0 - q
    k2, k4 = phi * q / p ** 2, phi * q * (1 + 4 * q + q * q) / p ** 4
    _moments_ok(y, mu, var, k4 + 3 * k2 * k2, f"nb2 {phi}")
    assert abs(k2 - var) <= 1e-9 * var and ng.max() <= 16 and npo.max() <= 16 and np.sum(amb) <= 2


def test_reference_gamma():
    s, i = _keys(N)
    for a in (0.5, 3.7):
        G, _, _, _ = dr.gamma(np.full(s.size, a), 0.0, 41, s.reshape(-1), i.reshape(-1))
        _moments_ok(G, a, a, 3 * a * a + 6 * a, f"gamma {a}")


def test_reference_ordinal_and_categorical():
    s, i = _keys(N)
    c = np.array([-1.0, 0.2, 0.2, 1.7])                     # (a collapsed pair: class 2 is empty)
    eta = 0.4
    sg = lambda a: 1.0 / (1.0 + np.exp(-a))
    P = np.diff(np.concatenate([[0.0], sg(c - eta), [1.0]]))
    y, _ = dr.ordinal(np.full(s.shape, eta), 0.0, np.broadcast_to(c, s.shape + (4,)), 0.0, 51, s, i)
    for k in range(5):
        _moments_ok(y == k, P[k], P[k] * (1 - P[k]), P[k] * (1 - P[k]) * (1 - 3 * P[k] * (1 - P[k])), f"ordinal class {k}")
    P = np.array([0.1, 0.0, 0.55, 0.35])
    y, _ = dr.categorical(np.broadcast_to(P, s.shape + (4,)), np.zeros(4), 52, s, i)
    for k in range(4):
        _moments_ok(y == k, P[k], P[k] * (1 - P[k]), P[k] * (1 - P[k]) * (1 - 3 * P[k] * (1 - P[k])), f"categorical class {k}")


def test_reference_bad_draws_are_nan():
    s, i = _keys(8)
    y, _, _ = dr.poisson(np.array([np.inf, np.nan, 2.0 ** 54, -1.0, 0.0, 5.0, 50.0, 2.0 ** 53]), 0.0, 1, s.reshape(-1), i.reshape(-1))
    assert np.all(np.isnan(y[:4])) and y[4] == 0.0 and not np.any(np.isnan(y[4:]))


def test_reference_ancestors():
    # dyadic weights: every cumulative sum is exact
    lw = np.array([-2.0, -np.inf, -1.0, -3.0, -3.0]) * math.log(2.0)
    a, amb = dr.ancestors(lw, 5, 8, 3)
    u0 = float(dr.philox_uniform(3, 0, 0, 16, 0))
    pos = (np.arange(8) + u0) / 8
    want = np.array([0 if p < 0.25 else (2 if p < 0.75 else (3 if p < 0.875 else 4)) for p in pos])
    np.testing.assert_array_equal(a, want)
    assert not amb.any() and 1 not in a


# ---- PredictiveDraws ---------------------------------------------------------------------------------------------------
def test_predictive_draws_helpers():
    from smcnuts_amd import PredictiveDraws
    y = np.array([[1.0, 10.0], [2.0, np.nan], [3.0, 30.0], [4.0, 20.0], [5.0, np.nan]])
    d = PredictiveDraws(y, np.arange(5), 2)
    assert d.n_draws == 5 and d.n_bad == 2 and d.ancestors.dtype == np.int64
    np.testing.assert_allclose(d.mean(), [3.0, 20.0])
    lo, hi = d.interval(0.5)
    np.testing.assert_allclose(lo, [2.0, 15.0])
    np.testing.assert_allclose(hi, [4.0, 25.0])
    with pytest.raises(ValueError, match="level"):
        d.interval(1.0)
    # the statistic of rows 1 and 4 is NaN: left out; of the three others, max >= 20 holds for two
    assert d.pvalue(np.max, np.array([20.0, 3.0])) == pytest.approx(2.0 / 3.0)
    assert d.pvalue(lambda r: r[0], np.array([3.0, 0.0])) == pytest.approx(3.0 / 5.0)
    e = PredictiveDraws(np.full((2, 1), np.nan), [0, 0], 2)
    assert np.isnan(e.mean()[0]) and np.isnan(e.interval()[0][0]) and np.isnan(e.pvalue(np.max, [1.0]))


# ---- argument checks, all before a context exists ------------------------------------------------------------------------
def _glm():
    from smcnuts_amd import GLMTarget
    rng = np.random.default_rng(0)
    X = rng.standard_normal((20, 2))
    return GLMTarget(X, (rng.random(20) < 0.5).astype(float), family="bernoulli_logit"), X


def _hier():
    from smcnuts_amd import HierarchicalGLM
    rng = np.random.default_rng(1)
    X = rng.standard_normal((20, 2))
    g = np.arange(20) % 4
    return HierarchicalGLM(X, rng.poisson(2.0, 20).astype(float), g, family="poisson_log"), X, g


def test_predict_draws_argument_checks():
    t, X = _glm()
    x = np.zeros((3, t.dim))
    for bad in (0, -5, 2.5, True, 2 ** 31):
        with pytest.raises(ValueError, match="n_draws"):
            t.predict_draws(x, X, bad)
    with pytest.raises(ValueError, match="ancestors"):
        t.predict_draws(x, X, 4, ancestors=[0, 1, 2])
    with pytest.raises(ValueError, match="ancestors"):
        t.predict_draws(x, X, 3, ancestors=[0, 1, 3])
    with pytest.raises(ValueError, match="ancestors"):
        t.predict_draws(x, X, 3, ancestors=[0, -1, 2])
    with pytest.raises(ValueError, match="ancestors"):
        t.predict_draws(x, X, 3, ancestors=[0.0, 1.0, 2.0])
    with pytest.raises(ValueError, match="HierarchicalGLM only"):
        t.predict_draws(x, X, 3, groups_new=np.zeros(20, dtype=int))
    with pytest.raises(ValueError, match="columns"):
        t.predict_draws(x, X[:, :1], 3)
    with pytest.raises(ValueError, match="logw"):
        t.predict_draws(x, X, 3, logw=np.zeros(2))
    with pytest.raises(ValueError, match="x must be"):
        t.predict_draws(np.zeros((3, t.dim + 1)), X, 3)
    assert t._ctx is None


def test_predict_draws_group_labels():
    t, X, g = _hier()
    x = np.zeros((3, t.dim))
    with pytest.raises(ValueError, match="groups_new is required"):
        t.predict_draws(x, X, 3)
    for bad in (-1, 2.5, np.nan, 2.0 ** 32):
        gg = g.astype(float)
        gg[3] = bad
        with pytest.raises(ValueError, match="groups_new must be labels"):
            t.predict_draws(x, X, 3, groups_new=gg)
    with pytest.raises(ValueError, match="vector of m"):
        t.predict_draws(x, X, 3, groups_new=g[:5])
    # predict() still refuses labels >= J, with its own message
    gg = g.copy()
    gg[0] = 4
    with pytest.raises(ValueError, match="new, unseen groups are not implemented"):
        t.predict(x, X, groups_new=gg)
    # the variant that admits them: such rows carry group 0 in the block, the labels travel beside it
    block, labels, S, anc = t._draws_args(X, 7, gg, None, 3)
    assert S == 7 and anc is None and labels[0] == 4 and np.array_equal(labels[1:], g[1:])
    m = X.shape[0]
    assert block[5 + m] == 0.0 and np.array_equal(block[5 + m + 1:5 + 2 * m], g[1:].astype(float))
    assert t._draws_args(X, 7, g, None, 3)[1] is None          # no new group among the labels
    assert t._ctx is None


def test_sampler_predict_draws_preconditions():
    from smcnuts_amd import ArmaModel, SMCSampler
    t, X = _glm()
    assert hasattr(SMCSampler, "predict_draws")
    smc = SMCSampler.__new__(SMCSampler)
    smc.lkernel, smc.target = "asymptoticLKernel", t
    with pytest.raises(NotImplementedError, match="asymptotic"):
        smc.predict_draws(X)
    smc.lkernel, smc.target = "forwardsLKernel", ArmaModel()
    with pytest.raises(NotImplementedError, match="GLMTarget"):
        smc.predict_draws()
    smc.target, smc._finalised = t, False
    with pytest.raises(ValueError, match="n_draws"):
        smc.predict_draws(X, n_draws=0)
    with pytest.raises(RuntimeError, match="finalise"):
        smc.predict_draws(X)


def test_shard_slots_cover_every_slot_once():
    """Two in-process ranks: the slot ranges partition 0..S-1 and the local ancestors are the one-shard ancestors."""
    from smcnuts_amd.predict import shard_slots
    rng = np.random.default_rng(5)
    lw = [3.0 * rng.standard_normal(40), 3.0 * rng.standard_normal(40) - 2.0]
    lw[0][::7] = -np.inf
    S, seed = 97, 8

    class Comm:
        world_size = 2

        def __init__(self, rank, rows):
            self.rank, self.rows = rank, rows

        def allgather(self, v):
            return np.stack(self.rows)

    rows = []
    for lwr in lw:
        fin = np.isfinite(lwr)
        mw = np.max(lwr[fin])
        rows.append(np.array([mw, np.sum(np.exp(lwr[fin] - mw)), 40.0]))
    one, amb = dr.ancestors(np.concatenate(lw), 80, S, seed)
    seen = np.zeros(S, dtype=int)
    for r in range(2):
        s0, n, anc, offs = shard_slots(lw[r], S, seed, Comm(r, rows))
        seen[s0:s0 + n] += 1
        ok = ~amb[s0:s0 + n]
        np.testing.assert_array_equal((anc[s0:s0 + n] + offs[r])[ok], one[s0:s0 + n][ok])
        assert np.all(np.isfinite(lw[r][anc[s0:s0 + n]]))
    assert np.all(seen == 1) and amb.sum() <= 2
