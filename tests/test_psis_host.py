"""Pareto-smoothed LOO without a GPU: the tail length, the NumPy reference of tests/_psis.py against known truth and its
edge rules, the host merge of the shards' candidates, the refusals and compare_loo."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _psis as ps  # noqa: E402


def test_tail_len():
    from smcnuts_amd import tail_len
    want = {20: 4, 24: 4, 25: 5, 64: 12, 100: 20, 1000: 95, 65536: 768}
    for S, M in want.items():
        assert tail_len(S) == M and ps.tail_len(S) == M
    # the integer form and the floating-point restatement agree, perfect squares and their neighbours included
    for S in list(range(1, 3000)) + [r * r + d for r in range(300, 1400, 37) for d in (-1, 0, 1)] + [1863225, 1863226]:
        assert tail_len(S) == ps.tail_len(S), S
    assert tail_len(0) == 0 and tail_len(1863225) == 4095 and tail_len(1863226) == 4096


@pytest.mark.parametrize("k", [-0.3, 0.0, 0.2, 0.7, 1.2])
def test_reference_recovers_known_shape(k):
    T = 768
    got, sigma = ps.gpdfit(ps.gpd_quantiles(T, k))
    assert abs(got - (T * k + 5.0) / (T + 10.0)) < 0.005
    assert abs(sigma - 1.0) < 0.01
    # the same through the whole definition: an observation whose tail is those quantiles
    lwp, ll = ps.gpd_tail_case(T, k)
    r = ps.psis_obs(lwp, ll)
    assert r["tail_len"] == T and r["cutoff"] == -3.0
    assert abs(r["pareto_k"] - (T * k + 5.0) / (T + 10.0)) < 0.005


def _plain_loo(lwp, ll):
    a = lwp - ll
    return -(np.max(a) + np.log(np.sum(np.exp(a - np.max(a)))) - np.log(np.sum(np.exp(lwp))))


def test_fewer_than_five_tail_entries_are_not_smoothed():
    rng = np.random.default_rng(1)
    lw, ll = rng.standard_normal(25), -np.abs(rng.standard_normal(25)) * 3
    lwp = lw - lw.max()
    r24 = ps.psis_obs(lwp[:24] - lwp[:24].max(), ll[:24])
    assert r24["pareto_k"] == np.inf and r24["tail_len"] == 4 and np.isnan(r24["sigma"])
    # elpd_psis is log sum r p / sum r of the unnormalised ratios; plain elpd_loo is the same number
    l24 = lwp[:24] - lwp[:24].max()
    np.testing.assert_allclose(r24["elpd_psis"], _plain_loo(l24, ll[:24]) , rtol=1e-13)
    r25 = ps.psis_obs(lwp, ll)
    assert np.isfinite(r25["pareto_k"]) and r25["tail_len"] == 5 and np.isfinite(r25["sigma"])


def test_constant_ratios_and_repeated_values():
    r = ps.psis_obs(np.zeros(200), np.full(200, -1.5))
    assert r["tail_len"] == 0 and r["pareto_k"] == np.inf and r["cutoff"] == 1.5
    np.testing.assert_allclose(r["elpd_psis"], -1.5, rtol=1e-14)
    np.testing.assert_allclose(r["psis_ess"], 200.0, rtol=1e-13)
    # fifty distinct values, four times each: S = 200, M = 40, c is the value of the 41st largest = the 11th distinct one,
    # and the tail holds the ten distinct values above it
    ll = -np.repeat(np.linspace(0.0, 5.0, 50), 4)
    r = ps.psis_obs(np.zeros(200), np.random.default_rng(0).permutation(ll))
    assert r["tail_len"] == 40 and np.isfinite(r["pareto_k"])


def test_inf_rule():
    ll = -np.abs(np.random.default_rng(2).standard_normal(100))
    ll[17] = -np.inf
    r = ps.psis_obs(np.zeros(100), ll)
    assert (r["pareto_k"], r["elpd_psis"], r["psis_ess"], r["tail_len"]) == (np.inf, -np.inf, 0.0, 0)


@pytest.mark.parametrize("split", [(100, 200), (1, 299), (150,), (60, 120, 180, 240)])
def test_merge_candidates_equals_unsplit_selection(split):
    from smcnuts_amd import merge_candidates, tail_len
    rng = np.random.default_rng(5)
    S, n = 300, 7
    lwp = -np.abs(rng.standard_normal(S))
    ll = -np.abs(rng.standard_normal((S, n))) * 2
    # ties: duplicated particles on both sides of every split point, so that equal values straddle the cutoff and the ranks
    src = rng.integers(0, S, size=S)
    dup = rng.random(S) < 0.6
    lwp[dup], ll[dup] = lwp[src[dup]], ll[src[dup]]
    cap = tail_len(S) + 1
    want_lr, want_ll = ps.candidates(lwp, ll, cap)
    edges = [0, *split, S]
    parts = [ps.candidates(lwp[a:b], ll[a:b], cap) for a, b in zip(edges[:-1], edges[1:])]
    lr, llc, cut = merge_candidates(parts)
    np.testing.assert_array_equal(lr, want_lr)
    np.testing.assert_array_equal(llc, want_ll)
    ref = [ps.psis_obs(lwp, ll[:, i]) for i in range(n)]
    np.testing.assert_array_equal(cut, [r["cutoff"] for r in ref])
    assert any(np.sum(want_lr[i] == want_lr[i, -1]) > 1 for i in range(n)), "no tie at the cutoff: the case is too easy"
    # the tail the merged list implies is the reference's
    for i, r in enumerate(ref):
        assert int(np.sum(lr[i] > cut[i])) == r["tail_len"]


def test_unsupported_targets_raise_before_any_context():
    from smcnuts_amd import (ArmaModel, CategoricalRegression, GaussianTarget, HierarchicalGLM, HostTarget,
                             OrdinalRegression, SMCSampler)
    import _glm
    rng = np.random.default_rng(0)
    X = rng.standard_normal((30, 2))
    yb = (rng.random(30) < 0.5).astype(float)
    targets = [HierarchicalGLM(X, yb, np.arange(30) % 3), CategoricalRegression(X, np.arange(30) % 3),
               OrdinalRegression(X, np.arange(30) % 3), ArmaModel(), GaussianTarget(3), HostTarget(_glm.GLMNumpy(X, yb))]
    for t in targets:
        x = np.zeros((2, t.dim))
        for call in (lambda: t.loo(x), lambda: t.loo(x, np.zeros(2))):
            with pytest.raises(NotImplementedError, match="GLMTarget"):
                call()
        assert getattr(t, "_ctx", None) is None
        smc = SMCSampler.__new__(SMCSampler)
        smc.lkernel, smc.target = "forwardsLKernel", t
        with pytest.raises(NotImplementedError, match="GLMTarget"):
            smc.loo()
    smc.lkernel = "asymptoticLKernel"
    with pytest.raises(NotImplementedError, match="asymptotic"):
        smc.loo()


def test_glm_argument_checks_come_first():
    from smcnuts_amd import LogisticRegression
    rng = np.random.default_rng(0)
    t = LogisticRegression(rng.standard_normal((10, 2)), (rng.random(10) < 0.5).astype(float))
    with pytest.raises(ValueError):
        t.loo(np.zeros((4, 7)))
    assert t._ctx is None


def _fake(elpd, k, S=1000):
    from smcnuts_amd import PsisLoo
    from smcnuts_amd.criteria import Pointwise
    n = len(elpd)
    z = np.zeros(n)
    plain = Pointwise(z + 0.25, z, z, z, z, z, z, S, S)
    out = np.stack([np.asarray(k, float), np.asarray(elpd, float), z + 10, z + 5, z, z + 1], axis=1)
    return PsisLoo(out, plain, S)


def test_psisloo_and_compare_loo_by_hand():
    from smcnuts_amd import compare_loo
    a = _fake([-1.0, -2.0, -4.0], [0.1, 0.69, 0.71])
    b = _fake([-1.5, -1.0, -6.0], [np.inf, 0.2, 0.3])
    assert a.elpd_loo == -7.0 and a.k_threshold == min(1 - 1 / 3.0, 0.7) and a.n_high_k == 2 and b.n_high_k == 1
    np.testing.assert_allclose(a.p_loo_i, [1.25, 2.25, 4.25])
    # n var(ddof = 1) of [-1, -2, -4]: mean -7/3, squares 16/9 + 1/9 + 25/9 = 42/9, / 2 * 3 = 7
    np.testing.assert_allclose(a.se_elpd_loo, np.sqrt(7.0), rtol=1e-14)
    assert _fake([0.0] * 3, [0.5] * 3, S=10 ** 9).k_threshold == 0.7
    c = compare_loo(a, b)
    # differences 0.5, -1, 2: sum 1.5, mean 0.5, squares 0 + 2.25 + 2.25 = 4.5, / 2 * 3 = 6.75
    assert c["elpd_loo_diff"] == 1.5 and c["n_obs"] == 3
    np.testing.assert_allclose(c["se_elpd_loo_diff"], np.sqrt(6.75), rtol=1e-14)
    s = a.summary()
    assert s["n_high_k"] == 2 and s["max_pareto_k"] == 0.71 and s["elpd_loo"] == -7.0
    with pytest.raises(ValueError, match="different numbers of observations"):
        compare_loo(a, _fake([-1.0], [0.1]))
