"""The exact references of tests/test_gpu_reductions.py are themselves tested (no GPU): the long-double and fsum
paths against mpmath at 40 digits on small inputs, and the vectorised right-search against the oracle's bisection."""
import math

import numpy as np
import pytest

import _exact as ex
from oracle import oracle as orc


def small_sets(rng, n=3000):
    tiles = 3.0 * rng.standard_normal(n)
    tiles[1024:2048] = -np.inf
    tiles[0] = tiles[-1] = -np.inf
    single = np.full(n, -np.inf)
    single[17] = 0.5
    ties = rng.standard_normal(n)
    ties[::10] = 4.0
    return {"gauss3": 3.0 * rng.standard_normal(n), "uniform_2000": rng.uniform(-2000.0, 0.0, n),
            "offset_1e6": -1e6 + rng.standard_normal(n), "tiles": tiles, "single": single, "ties": ties}


@pytest.mark.parametrize("wide_ld", [True, False])
def test_exact_references_agree_with_mpmath(monkeypatch, wide_ld):
    pytest.importorskip("mpmath")
    rng = np.random.default_rng(11)
    x = 1e4 + 1e-2 * rng.standard_normal((3000, 3))
    for name, logw in small_sets(rng).items():
        want = (ex.lse_exact(logw), ex.ess_exact(logw), ex.wn_exact(logw), ex.moments_exact(logw, x))
        with monkeypatch.context() as m:
            m.setattr(ex, "MP_MAX", 0)                      # the large-N path on the same inputs
            if not wide_ld:
                m.setattr(ex, "WIDE_LD", False)
            got = (ex.lse_exact(logw), ex.ess_exact(logw), ex.wn_exact(logw), ex.moments_exact(logw, x))
        np.testing.assert_allclose(got[0], want[0], rtol=2 * ex.EPS, atol=4 * ex.EPS, err_msg=name)
        np.testing.assert_allclose(got[1], want[1], rtol=4 * ex.EPS, err_msg=name)
        np.testing.assert_allclose(got[2], want[2], rtol=4 * ex.EPS if wide_ld else 4 * ex.EPS * 2000, err_msg=name)
        np.testing.assert_allclose(got[3][0], want[3][0], rtol=2 * ex.EPS, err_msg=name)
        np.testing.assert_allclose(got[3][1], want[3][1], rtol=4 * ex.EPS if wide_ld else 1e-9, err_msg=name)
    # the reference against a plain statement of the definition
    a = np.array([0.0, math.log(2.0), -np.inf, math.log(5.0)])
    assert ex.lse_exact(a) == pytest.approx(math.log(8.0), rel=1e-16)
    assert ex.ess_exact(a) == pytest.approx(64.0 / 30.0, rel=1e-15)
    np.testing.assert_allclose(ex.wn_exact(a), [1 / 8, 2 / 8, 0.0, 5 / 8], rtol=1e-16)
    assert ex.lse_exact(np.full(5, -np.inf)) == -np.inf and np.all(ex.wn_exact(np.full(5, -np.inf)) == 0.0)


def test_vectorised_search_is_the_oracle_bisection():
    rng = np.random.default_rng(12)
    for n in (1, 1023, 1025, 5000):
        w = np.exp(3.0 * rng.standard_normal(n))
        if n > 3000:
            w[1000:2100] = 0.0
            w[-300:] = 0.0
        wn = w / w.sum()
        u = rng.random(n)
        u[0] = 1.0 - 2.0 ** -53
        if n > 1:
            u[1] = 0.0
        np.testing.assert_array_equal(ex.indices_exact(wn, u, orc.blocked_cumsum), orc.multinomial_indices(wn, u, "blocked"))
        keys = (np.arange(n, dtype=np.float64) + 0.37) / n
        np.testing.assert_array_equal(ex.indices_exact(wn, keys, orc.blocked_cumsum),
                                      orc.systematic_indices(wn, 0.37, "blocked"))
