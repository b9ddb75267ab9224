"""CategoricalRegression (SMCN_MODEL_CATEGORICAL) on the CPU: input validation, the data block it packs, and the numpy
reference density of tests/_cat.py against mpmath at 40 digits -- benign points, logits of +-800, ties, one dominating
class -- against logistic regression at K = 2, and under permuted observations and relabelled classes."""
import math

import numpy as np
import pytest

import _cat as ct
import _glm as gl

U = ct.U


def test_packing_and_names():
    from smcnuts_amd import CategoricalRegression, _capi
    X = np.arange(8.0).reshape(4, 2) / 10.0
    y = np.array([0, 2, 1, 2])
    t = CategoricalRegression(X, y, prior_sd=[1.0, 2.0, 3.0])
    assert t.model_id == _capi.MODEL_CATEGORICAL == 6
    assert t.n_classes == 3
    assert t.dim == t.constrained_dim == 2 * 3
    assert t.param_names() == ["Intercept.1", "beta.1.1", "beta.1.2", "Intercept.2", "beta.2.1", "beta.2.2"]
    want = np.concatenate([[3, 4, 2, 1], [1.0, 2.0, 3.0, 1.0, 2.0, 3.0], [0, 2, 1, 2], X.reshape(-1)])
    np.testing.assert_array_equal(t.model_data, want)
    # no intercept, an empty class beyond the largest label, a (K - 1, Dc) prior, float labels
    sd = np.array([[0.5, 0.6], [0.7, 0.8], [0.9, 1.0], [1.1, 1.2]])
    t = CategoricalRegression(X, [0.0, 1.0, 1.0, 0.0], n_classes=5, prior_sd=sd, intercept=False)
    assert t.dim == 4 * 2
    assert t.param_names() == ["beta.1.1", "beta.1.2", "beta.2.1", "beta.2.2", "beta.3.1", "beta.3.2", "beta.4.1",
                               "beta.4.2"]
    want = np.concatenate([[5, 4, 2, 0], sd.reshape(-1), [0, 1, 1, 0], X.reshape(-1)])
    np.testing.assert_array_equal(t.model_data, want)
    # intercept only; the default prior
    t = CategoricalRegression(np.zeros((3, 0)), [1, 0, 3])
    assert t.dim == 3 and t.param_names() == ["Intercept.1", "Intercept.2", "Intercept.3"]
    np.testing.assert_array_equal(t.model_data[:7], [4, 3, 0, 1, 2.5, 2.5, 2.5])
    # the limits exactly: K = 16 with Dc = 4, and D = 64
    assert CategoricalRegression(np.zeros((3, 3)), [0, 15, 1]).dim == 60
    assert CategoricalRegression(np.zeros((3, 31)), [0, 2, 1]).dim == 64


def test_validation():
    from smcnuts_amd import CategoricalRegression
    X = np.zeros((4, 2))
    y = [0, 1, 2, 1]
    cases = [
        (dict(X=np.zeros((2, 2, 2))), "X must be an (n, p) matrix"),
        (dict(X=np.zeros((0, 2)), y=[]), "at least one observation"),
        (dict(y=[0, 1, 1]), "y must be a vector of the n = 4"),
        (dict(y=[0, 1.5, 1, 0]), "the labels y must be integers"),
        (dict(y=[0, np.nan, 1, 0]), "the labels y must be integers"),
        (dict(y=["a", "b", "a", "b"]), "the labels y must be integers"),
        (dict(y=[True, False, True, False]), "the labels y must be integers"),
        (dict(y=[0, -1, 1, 0]), "the labels y must be >= 0"),
        (dict(y=[0, 0, 0, 0]), "K = n_classes must be >= 2"),
        (dict(n_classes=1, y=[0, 0, 0, 0]), "K = n_classes must be >= 2"),
        (dict(n_classes=2.0), "n_classes must be an integer"),
        (dict(n_classes=2), "the labels y must be in 0..n_classes - 1 = 1"),
        (dict(y=[0, 1, 16, 0]), "K = 17 classes; the device functor holds K <= 16"),
        (dict(n_classes=20), "K = 20 classes; the device functor holds K <= 16"),
        (dict(X=np.zeros((4, 32))), "the device functor covers D <= 64"),
        (dict(X=np.zeros((4, 7)), n_classes=10), "D = (K - 1) Dc = 9 x 8 = 72"),
        (dict(X=np.zeros((4, 0)), intercept=False), "no coefficients"),
        (dict(X=np.array([[0, 1], [np.inf, 0], [0, 0], [1, 1]])), "X must be finite"),
        (dict(prior_sd=0.0), "prior_sd must be finite and > 0"),
        (dict(prior_sd=[1.0, np.nan, 1.0]), "prior_sd must be finite and > 0"),
        (dict(prior_sd=[1.0, 2.0]), "prior_sd must be a scalar, one value per column (3) or a (K - 1, Dc) = (2, 3)"),
        (dict(prior_sd=np.ones((3, 3))), "prior_sd must be a scalar, one value per column (3)"),
    ]
    for kw, msg in cases:
        kw = dict(kw)
        args = (kw.pop("X", X), kw.pop("y", y))
        with pytest.raises(ValueError) as ei:
            CategoricalRegression(*args, **kw)
        assert msg in str(ei.value), (str(ei.value), msg)


@pytest.mark.parametrize("K,p,ic", [(2, 3, 1), (3, 2, 1), (5, 3, 0), (16, 1, 1)])
def test_reference_against_mpmath(K, p, ic):
    X, y = ct.synthetic(K, 23, p, 10 * K + p)
    m = ct.CategoricalNumpy(X, y, n_classes=K, prior_sd=np.linspace(0.7, 2.0, p + ic), intercept=bool(ic))
    pts = ct.points(m, np.random.default_rng(K))
    lpri, llik, gpri, glik = ct.exact_parts(m, pts)
    b_lpri, b_llik, b_glik = ct.device_bounds(m, pts)
    for i, x in enumerate(pts):
        mp_lpri, mp_llik, mp_g = ct.mp_parts(m, x)
        assert np.isfinite(llik[i])                     # (every finite x: a finite density)
        # the reference is itself one such evaluation: within the device's bound of the exact value
        assert abs(lpri[i] - mp_lpri) <= b_lpri[i], (i, lpri[i] - mp_lpri, b_lpri[i])
        assert abs(llik[i] - mp_llik) <= b_llik[i], (i, llik[i] - mp_llik, b_llik[i])
        assert np.all(np.abs(glik[i] - mp_g) <= b_glik[i]), (i, np.max(np.abs(glik[i] - mp_g) - b_glik[i]))
        np.testing.assert_array_equal(gpri[i], -x / m.s ** 2)
    # at +-800 nothing cancels: the bound is a few u of the magnitudes, and the terms are exact to it
    assert np.all(b_llik[3:5] <= 1e-9 * (np.abs(llik[3:5]) + 1.0))


def test_overflowing_logits_give_minus_inf():
    X = np.array([[1e300], [0.5], [-1.0]])
    m = ct.CategoricalNumpy(X, [1, 0, 2], n_classes=3)
    x = np.array([0.0, 1e10, 0.0, 1.0])                  # eta_01 = 1e310: not finite
    lpri, llik, _, _ = ct.exact_parts(m, x)
    assert np.isfinite(lpri[0]) and llik[0] == -np.inf
    assert m.logpdf(x) == -np.inf and np.all(m.logpdfgrad(x) == -np.inf)
    x = np.array([0.0, 1e-10, 0.0, 1.0])
    assert np.isfinite(m.logpdf(x))


def test_two_classes_are_logistic_regression():
    """K = 2: the categorical terms are bernoulli_logit's, value and gradient, within both references' bounds."""
    rng = np.random.default_rng(3)
    X, y = ct.synthetic(2, 40, 4, 5)
    m = ct.CategoricalNumpy(X, y, prior_sd=1.7)
    g = gl.GLMNumpy(X, y.astype(np.float64), "bernoulli_logit", prior_sd=1.7)
    assert m.dim == g.dim == 5
    assert m.param_names() == ["Intercept.1"] + [f"beta.1.{j + 1}" for j in range(4)]
    pts = np.vstack([rng.standard_normal((4, 5)), rng.standard_normal((2, 5)) * 200.0])
    a = ct.exact_parts(m, pts)
    b = gl.exact_parts(g, pts)
    ba, bb = ct.device_bounds(m, pts), gl.device_bounds(g, pts)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[2], b[2])
    assert np.all(np.abs(a[1] - b[1]) <= ba[1] + bb[1])
    assert np.all(np.abs(a[3] - b[3]) <= ba[2] + bb[2])


def test_permuting_observations():
    X, y = ct.synthetic(4, 50, 3, 8)
    m = ct.CategoricalNumpy(X, y)
    perm = np.random.default_rng(1).permutation(50)
    mp = ct.CategoricalNumpy(X[perm], y[perm])
    pts = np.random.default_rng(2).standard_normal((5, m.dim))
    for u, v in zip(ct.exact_parts(m, pts), ct.exact_parts(mp, pts)):
        np.testing.assert_array_equal(u, v)             # (fsum: exactly rounded, whatever the order)


def test_relabelling_classes_permutes_the_blocks():
    """A permutation pi of the non-reference classes 1..K-1 relabels y; the density at x is the density of the
    relabelled model at x with block k moved to block pi(k)."""
    K, p = 5, 2
    X, y = ct.synthetic(K, 60, p, 4)
    Dc = p + 1
    sd = np.linspace(0.5, 2.0, (K - 1) * Dc).reshape(K - 1, Dc)
    m = ct.CategoricalNumpy(X, y, prior_sd=sd)
    pi = np.array([0, 3, 1, 4, 2])                        # class k -> pi[k], class 0 stays
    sd2 = np.empty_like(sd)
    sd2[pi[1:] - 1] = sd
    m2 = ct.CategoricalNumpy(X, pi[y], n_classes=K, prior_sd=sd2)
    pts = np.random.default_rng(6).standard_normal((6, m.dim))
    pts2 = np.empty_like(pts)
    for k in range(1, K):
        pts2[:, (pi[k] - 1) * Dc:pi[k] * Dc] = pts[:, (k - 1) * Dc:k * Dc]
    a, b = ct.exact_parts(m, pts), ct.exact_parts(m2, pts2)
    bnd = ct.device_bounds(m, pts)
    np.testing.assert_array_equal(a[0], b[0])
    assert np.all(np.abs(a[1] - b[1]) <= 2 * bnd[1])
    g2 = np.empty_like(b[3])
    for k in range(1, K):
        g2[:, (k - 1) * Dc:k * Dc] = b[3][:, (pi[k] - 1) * Dc:pi[k] * Dc]
    assert np.all(np.abs(a[3] - g2) <= 2 * bnd[2])
    np.testing.assert_allclose(m.logpdf(pts), m2.logpdf(pts2), rtol=1e-13)
    assert math.isfinite(m.logpdf(pts[0]))
