"""Posterior summaries, the parts that need no GPU: the exact reference of tests/_summary.py against NumPy, argument
validation, PosteriorSummary, the key map and the host side of the shard protocol (thresholds, pick_digits)."""
import math
from fractions import Fraction

import numpy as np
import pytest

import _summary as S
from smcnuts_amd import summary as sm

MS = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 4097)


@pytest.mark.parametrize("M", MS)
def test_reference_against_numpy_and_order_statistic(M):
    rng = np.random.default_rng(M)
    v = S.dup_values(rng, M, 3)
    lw = 3.0 * rng.standard_normal(M)
    w = S.weights(lw, M)
    ref = S.quantiles(v, lw, S.DEFAULT)
    for c in range(3):
        want = np.quantile(v[:, c], S.DEFAULT, method="inverted_cdf", weights=w)
        np.testing.assert_array_equal(ref[c], want)
    eq = S.quantiles(v, None, S.DEFAULT)
    for c in range(3):
        sv = np.sort(v[:, c])
        want = [sv[math.ceil(Fraction(p) * M) - 1] for p in S.DEFAULT]
        np.testing.assert_array_equal(eq[c], want)
        # NumPy forms p * M in doubles: where the exact product lies an ulp above an integer (0.025 * 1000 = 25 + 1.4e-15
        # with the double 0.025) it rounds to the integer and takes the particle before; compare everywhere else
        clear = [j for j, p in enumerate(S.DEFAULT)
                 if abs(Fraction(p) * M - round(Fraction(p) * M)) > Fraction(1, 10 ** 9) or Fraction(p) * M == round(Fraction(p) * M)]
        got_np = np.quantile(v[:, c], S.DEFAULT, method="inverted_cdf", weights=np.ones(M))
        np.testing.assert_array_equal(eq[c][clear], got_np[clear])


def test_reference_masses_and_special_values():
    v = np.array([[-np.inf], [-0.0], [0.0], [1.0], [np.inf], [np.nan]])
    lw = np.array([0.0, 0.0, 0.0, 0.0, 0.0, -np.inf])
    col = S.columns(v, lw)[0]
    assert not col.nan and col.W == 5 * col.cum[0]
    assert col.mass_lt(0.0) == col.cum[0] and col.mass_le(-0.0) == 3 * col.cum[0]      # the zeros are equal
    assert col.quantile(0.19)[0] == -np.inf and col.quantile(1.0)[0] == np.inf and col.quantile(0.5)[0] == 0.0
    assert S.columns(v, np.zeros(6))[0].nan                                             # a NaN of positive weight
    assert np.all(np.isnan(S.quantiles(v, np.full(6, -np.inf), (0.5,))))                # all weights zero


@pytest.mark.parametrize("probs,word", [((0.0, 0.5), "probs"), ((0.5, 1.5), "probs"), ((-0.1,), "probs"),
                                         ((0.5, float("nan")), "probs"), (tuple(np.linspace(0.01, 0.99, 17)), "probs"),
                                         ((), "probs"), ("abc", "probs")])
def test_probs_are_validated(probs, word):
    with pytest.raises(ValueError, match=word):
        sm.check_probs(probs)


def test_probs_edges_pass():
    np.testing.assert_array_equal(sm.check_probs((1.0, 1e-300)), [1.0, 1e-300])
    assert sm.check_probs(0.5).shape == (1,)
    assert sm.check_probs(np.linspace(0.01, 0.99, 16)).size == 16


@pytest.mark.parametrize("at", [np.zeros((2, 3)), np.zeros((3, 17)), np.zeros(17), np.zeros((3, 0)), np.zeros((3, 2, 2)), "x"])
def test_at_is_validated(at):
    with pytest.raises(ValueError, match="at"):
        sm.check_at(at, 3)


def test_at_shapes():
    assert sm.check_at(None, 3) is None
    np.testing.assert_array_equal(sm.check_at(0.0, 3), np.zeros((3, 1)))
    np.testing.assert_array_equal(sm.check_at([0.0, 1.0], 3), np.tile([0.0, 1.0], (3, 1)))
    a = np.arange(6.0).reshape(3, 2)
    np.testing.assert_array_equal(sm.check_at(a, 3), a)


def test_targets_validate_before_any_launch():
    """Every ValueError is raised from the arguments alone: no context exists yet (and none can be made here)."""
    from smcnuts_amd import GaussianTarget, HostTarget
    t = GaussianTarget(3)
    x = np.zeros((5, 3))
    for kw, word in ((dict(probs=(0.0,)), "probs"), (dict(probs=(float("nan"),)), "probs"), (dict(probs=(2.0,)), "probs"),
                     (dict(probs=np.linspace(0.1, 0.9, 17)), "probs"), (dict(at=np.zeros((2, 1))), "at"),
                     (dict(at=np.zeros(17)), "at"), (dict(logw=np.zeros(4)), "logw"),
                     (dict(logw=np.array([0, 0, np.nan, 0, 0.0])), "logw")):
        with pytest.raises(ValueError, match=word):
            t.summary(x, **kw)
        assert t._ctx is None
    with pytest.raises(ValueError, match="x must be"):
        t.summary(np.zeros((5, 4)))

    class M:
        dim = 3
        def logpdf(self, x, phi=1.0): return -0.5 * np.sum(np.square(x), axis=-1)
        def logpdfgrad(self, x, phi=1.0): return -np.asarray(x)

    h = HostTarget(M())
    with pytest.raises(ValueError, match="probs"):
        h.summary(x, probs=(0.0,))
    with pytest.raises(ValueError, match="at"):
        h.summary(x, at=np.zeros((4, 1)))
    assert getattr(h, "_sum_ctx", None) is None


def _summary_object(probs=S.DEFAULT, cdf=True):
    q = np.array([[-1.0, -0.5, 0.0, 0.5, 1.0], [0.1, 0.5, 1.0, 2.0, 9.0]])[:, :len(probs)]
    at = np.zeros((2, 1)) if cdf else None
    return sm.PosteriorSummary(["Intercept", "sigma"], [0.0, 1.5], [0.5, 2.0], probs, q,
                               np.array([[0.5], [0.0]]) if cdf else None, at, 812.3, 1024)


def test_interval_and_table():
    s = _summary_object()
    np.testing.assert_array_equal(s.interval(0.95), [[-1.0, 1.0], [0.1, 9.0]])
    np.testing.assert_array_equal(s.interval(0.5), [[-0.5, 0.5], [0.5, 2.0]])
    np.testing.assert_array_equal(s.quantile(0.5), [0.0, 1.0])
    with pytest.raises(ValueError, match=r"0\.05 and 0\.95"):
        s.interval(0.9)
    with pytest.raises(ValueError, match="level"):
        s.interval(1.0)
    with pytest.raises(ValueError, match="not requested"):
        s.quantile(0.1)
    text = str(s)
    lines = text.splitlines()
    assert len(lines) == 4 and lines[-1] == "1024 particles, ESS 812.3"
    for word in ("mean", "sd", "2.5%", "25%", "50%", "75%", "97.5%", "P(<=0)"):
        assert word in lines[0]
    assert lines[1].startswith("Intercept") and lines[2].startswith("sigma")
    assert "P(<=" not in str(_summary_object(cdf=False))
    two = sm.PosteriorSummary(["a"], [0.0], [1.0], (0.025, 0.975), np.array([[-2.0, 2.0]]), None, None, 10.0, 10)
    np.testing.assert_array_equal(two.interval(0.95), [[-2.0, 2.0]])


def test_key_map_orders_like_less_than():
    vals = [-np.inf, -1.0, -2.0 ** -1074, -0.0, 0.0, 2.0 ** -1074, 1.0, np.inf]
    keys = [sm.key_of(v) for v in vals]
    for i in range(len(vals)):
        for j in range(len(vals)):
            if vals[i] < vals[j]:
                assert keys[i] < keys[j], (vals[i], vals[j])
    assert keys == sorted(keys) and len(set(keys)) == len(keys)      # (-0.0 directly below +0.0: neighbours, not equal keys)
    assert keys[4] == keys[3] + 1
    rng = np.random.default_rng(0)
    r = rng.standard_normal(200) * 10.0 ** rng.integers(-300, 300, 200)
    assert list(np.argsort(r)) == sorted(range(200), key=lambda i: sm.key_of(r[i]))


def _select_on_host(v, f, probs, world):
    """The shard protocol of summary.device_summary with NumPy in the place of the device: `world` shards' histograms of
    the keys' digits, summed, pick_digits, descend; returns the selected values."""
    keys = np.array([sm.key_of(a) for a in v], dtype=np.uint64)
    shard = np.arange(len(v)) % world
    mass = int(f.sum())
    nq = len(probs)
    thr = np.array(sm.thresholds(probs, mass), dtype=np.int64)[None, :]
    prefix = np.zeros(nq, dtype=np.uint64)
    for k in range(8):
        hist = np.zeros((1, 1 if k == 0 else nq, 256), dtype=np.int64)
        for r in range(world):
            for q in range(hist.shape[1]):
                m = (shard == r) & (f > 0)
                if k:
                    m &= (keys >> np.uint64(64 - 8 * k)) == prefix[q]
                d = ((keys[m] >> np.uint64(56 - 8 * k)) & np.uint64(255)).astype(np.int64)
                hist[0, q] += np.bincount(d, weights=None if not len(d) else f[m], minlength=256).astype(np.int64)
        digit, thr = sm.pick_digits(hist, thr)
        prefix = (prefix << np.uint64(8)) | digit[0].astype(np.uint64)
    return np.array([np.uint64(p ^ (1 << 63) if p >> 63 else ~p & (2 ** 64 - 1)) for p in prefix.tolist()],
                    dtype=np.uint64).view(np.float64)


@pytest.mark.parametrize("world", [1, 3])
def test_host_side_of_the_shard_protocol(world):
    """Integer weights (exactly representable masses): the protocol's answer IS the reference's."""
    rng = np.random.default_rng(7)
    M = 257
    v = S.dup_values(rng, M, 1)[:, 0]
    v[:4] = [-np.inf, np.inf, 0.0, -0.0]
    f = rng.integers(0, 1 << 20, M).astype(np.int64)
    probs = np.sort(np.concatenate([S.DEFAULT, [1e-300, 1.0]]))
    got = _select_on_host(v, f, probs, world)
    with np.errstate(divide="ignore"):
        want = S.quantiles(v[:, None], np.log(f.astype(np.float64)), probs)[0]
    np.testing.assert_array_equal(got, want)
