"""Posterior covariance, host side (no GPU): the references of tests/_cov.py against exact rational arithmetic and
np.cov, combine_cov_partials on NumPy-made partials, PosteriorCovariance, argument checks and the sampler's guards."""
import numpy as np
import pytest

import _cov as CV
from smcnuts_amd.covariance import PosteriorCovariance, check_centre, combine_cov_partials

# the GPU grid's cases that rational arithmetic reaches in a second or two
SMALL = [(Dc, M) for Dc in (1, 2, 15, 16, 17) for M in (1, 2, 63, 64, 65, 257)]


def _inside(mean, cov, v, w, n, centre, what):
    em, ec = CV.exact_floats(v, w)
    absmean = np.abs(v[w > 0]).T @ w[w > 0] / w.sum()
    bm, bc = CV.bounds(em, ec, absmean, centre, n)
    assert np.all(CV.share(mean, em, bm) <= 1.0), f"{what}: mean"
    assert np.all(CV.share(cov, ec, bc) <= 1.0), f"{what}: cov"
    return em, ec


@pytest.mark.parametrize("Dc,M", SMALL)
def test_float_reference_against_exact(Dc, M):
    for weighted in (True, False):
        v, lw = CV.population(Dc, M, weighted)
        w = CV.weights(lw, M)
        for route in ("fsum",) + (("ld",) if CV.HAVE_LD else ()):
            m, c, _ = CV.reference(v, w, route=route)
            # about the exact mean itself (d = 0): the tightest form of the bound
            _inside(m, c, v, w, M, CV.exact_floats(v, w)[0], f"Dc={Dc} M={M} weighted={weighted} {route}")


def test_both_routes_agree():
    if not CV.HAVE_LD:          # no extended precision on this platform: the reference is the fsum route everywhere
        return
    v, lw = CV.population(33, 257, True)
    w = CV.weights(lw, 257)
    a, b = CV.reference(v, w, route="fsum"), CV.reference(v, w, route="ld")
    scale = np.sqrt(np.outer(np.diagonal(a[1]), np.diagonal(a[1])))
    assert np.max(np.abs(a[1] - b[1]) / scale) <= 8 * CV.U
    assert np.max(np.abs(a[0] - b[0]) / a[2]) <= 8 * CV.U


def test_ill_conditioned_reference():
    rng = np.random.default_rng(5)
    M = 4097
    v = 1e8 + 1e-4 * rng.standard_normal((M, 2)) @ np.array([[1.0, 0.6], [0.0, 0.8]])
    w = CV.weights(3.0 * rng.standard_normal(M), M)
    m, c, _ = CV.reference(v, w)
    em, ec = _inside(m, c, v, w, M, CV.exact_floats(v, w)[0], "ill-conditioned")
    wn = w / w.sum()
    naive = (v * wn[:, None]).T @ v - np.outer(wn @ v, wn @ v)
    assert np.all(np.abs(naive - ec) > 0.5 * np.abs(ec))          # no correct digit


@pytest.mark.parametrize("Dc,M", [(3, 65), (17, 257), (64, 130)])
def test_reference_agrees_with_numpy_cov(Dc, M):
    v, lw = CV.population(Dc, M, True)
    w = CV.weights(lw, M)
    m, c, _ = CV.reference(v, w)
    want = np.atleast_2d(np.cov(v, rowvar=False, ddof=0, aweights=w))
    sd = np.sqrt(np.diagonal(want))
    np.testing.assert_allclose(c, want, rtol=0.0, atol=1e-12 * np.max(np.outer(sd, sd)))
    np.testing.assert_allclose(m, np.average(v, axis=0, weights=w), rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("shards", [1, 2, 4])
def test_combine_partials_of_shards(shards):
    Dc, M = 17, 1000
    v, lw = CV.population(Dc, M, True)
    lw[::7] = -np.inf
    w = CV.weights(lw, M)
    centre = np.average(v, axis=0, weights=w) + 0.01
    cuts = np.linspace(0, M, shards + 1).astype(int)
    parts = [CV.numpy_partial(v[a:b], w[a:b], centre) for a, b in zip(cuts[:-1], cuts[1:])]
    mean, cov, corr, W = combine_cov_partials(parts, centre)
    m, c, am = CV.reference(v, w)
    bm, bc = CV.bounds(m, c, am, centre, CV.contributing(lw, M))
    assert np.all(CV.share(mean, m, bm) <= 1.0) and np.all(CV.share(cov, c, bc) <= 1.0)
    assert abs(W - w.sum()) <= CV.TOL(M) * w.sum()
    assert cov.tobytes() == cov.T.copy().tobytes()
    CV.check_corr(corr, cov, f"{shards} shards")


def test_recentring_is_exact_on_integers():
    rng = np.random.default_rng(2)
    M, Dc = 64, 5                                           # W = 64: every division is exact
    v = rng.integers(-8, 9, (M, Dc)).astype(np.float64)
    w = np.ones(M)
    em, ec = CV.exact_floats(v, w)
    got = []
    for centre in (np.zeros(Dc), np.array([3.0, -2.0, 0.0, 7.0, -8.0])):
        halves = [CV.numpy_partial(v[:40], w[:40], centre), CV.numpy_partial(v[40:], w[40:], centre)]
        mean, cov, _, W = combine_cov_partials(halves, centre)
        assert W == 64.0
        np.testing.assert_array_equal(mean, em)
        np.testing.assert_array_equal(cov, ec)
        got.append(cov)
    assert got[0].tobytes() == got[1].tobytes()


def test_finishing_rules():
    Dc = 4
    rng = np.random.default_rng(3)
    v = rng.standard_normal((50, Dc))
    v[:, 2] = 0.25                                          # a constant column
    w = np.ones(50)
    centre = np.array([0.1, -0.1, 0.25, 0.0])
    A = CV.numpy_partial(v, w, centre)
    mean, cov, corr, _ = combine_cov_partials([A], centre)
    assert cov[2, 2] == 0.0 and np.all(np.isnan(corr[2])) and np.all(np.isnan(corr[:, 2]))
    assert np.all(np.diagonal(corr)[[0, 1, 3]] == 1.0) and np.all(np.isfinite(cov))
    B = A.copy()
    B[1, :] = B[:, 1] = np.nan                              # a non-finite value in coordinate 1
    mean, cov, corr, _ = combine_cov_partials([B], centre)
    bad = np.zeros((Dc, Dc), dtype=bool)
    bad[1, :] = bad[:, 1] = True
    assert np.all(np.isnan(cov[bad])) and np.all(np.isfinite(cov[~bad])) and np.isnan(mean[1])
    assert np.all(np.isfinite(mean[[0, 2, 3]]))
    C = A.copy()
    C[0, 0] = C[Dc, 0] = C[0, Dc] = np.inf
    _, cov, _, _ = combine_cov_partials([C], centre)
    assert np.all(np.isnan(cov[0])) and np.all(np.isnan(cov[:, 0])) and np.all(np.isfinite(cov[1:, 1:]))
    mean, cov, corr, W = combine_cov_partials([np.zeros((Dc + 1, Dc + 1))], centre)
    assert W == 0.0 and np.all(np.isnan(mean)) and np.all(np.isnan(cov)) and np.all(np.isnan(corr))


def _pc():
    names = ["a", "b", "c"]
    mean = np.array([1.0, 2.0, -1.0])
    cov = np.array([[4.0, 1.0, -3.0], [1.0, 1.0, 0.0], [-3.0, 0.0, 9.0]])
    sd = np.sqrt(np.diagonal(cov))
    return PosteriorCovariance(names, mean, cov, cov / np.outer(sd, sd), 123.4, 1000)


def test_contrast_pairs_and_str():
    pc = _pc()
    np.testing.assert_array_equal(pc.sd, [2.0, 1.0, 3.0])
    m, s = pc.contrast([1.0, -1.0, 0.0])
    assert m == -1.0 and s == np.sqrt(4.0 + 1.0 - 2.0)
    for i in range(3):
        assert pc.contrast(np.eye(3)[i]) == (pc.mean[i], pc.sd[i])
    mm, ss = pc.contrast(np.array([[1.0, -1.0, 0.0], [1.0, 0.0, 1.0]]))
    np.testing.assert_array_equal(mm, [-1.0, 0.0])
    np.testing.assert_allclose(ss, [np.sqrt(3.0), np.sqrt(4.0 + 9.0 - 6.0)], rtol=1e-15)
    assert pc.pairs() == [("a", "b", 0.5), ("a", "c", -0.5), ("b", "c", 0.0)]      # (ties keep their index order)
    assert pc.pairs(0.4) == [("a", "b", 0.5), ("a", "c", -0.5)] and pc.pairs(0.6) == []
    text = str(pc)
    assert "correlation" in text and "1000 particles, ESS 123.4" in text and text.splitlines()[1].startswith("a")
    wide = PosteriorCovariance([f"x.{i}" for i in range(12)], np.zeros(12), np.eye(12), np.eye(12), 5.0, 10)
    assert "largest correlations of 66 pairs" in str(wide)


def test_argument_checks():
    pc = _pc()
    for bad in (np.zeros(2), np.zeros((2, 2)), np.zeros((1, 2, 3)), "abc"):
        with pytest.raises(ValueError, match="contrast"):
            pc.contrast(bad)
    with pytest.raises(ValueError, match="min_abs_corr"):
        pc.pairs(1.5)
    with pytest.raises(ValueError, match="names"):
        PosteriorCovariance(["a"], np.zeros(2), np.eye(2), np.eye(2), 1.0, 1)
    with pytest.raises(ValueError, match="centre"):
        check_centre(np.zeros(3), 4)
    with pytest.raises(ValueError, match="centre"):
        check_centre("abc", 3)
    assert check_centre(None, 3) is None
    with pytest.raises(ValueError, match="partial"):
        combine_cov_partials([np.zeros((3, 3))], np.zeros(3))
    with pytest.raises(ValueError, match="partial"):
        combine_cov_partials([], np.zeros(3))


def test_targets_check_their_arguments_first():
    from smcnuts_amd import GaussianTarget
    t = GaussianTarget(3)
    with pytest.raises(ValueError, match="x must be"):
        t.covariance(np.zeros((4, 2)))
    with pytest.raises(ValueError, match="logw"):
        t.covariance(np.zeros((4, 3)), np.zeros(5))
    with pytest.raises(ValueError, match="logw"):
        t.covariance(np.zeros((4, 3)), np.array([0.0, np.nan, 0.0, 0.0]))
    assert getattr(t, "_ctx", None) is None


def test_sampler_guards():
    from smcnuts_amd import GaussianTarget, SMCSampler
    smc = SMCSampler.__new__(SMCSampler)
    smc.lkernel, smc.target, smc.K = "asymptoticLKernel", GaussianTarget(3), 2
    with pytest.raises(NotImplementedError, match="asymptotic"):
        smc.covariance()
    smc.lkernel, smc._finalised = "forwardsLKernel", False
    with pytest.raises(RuntimeError, match="sample"):
        smc.covariance()
    smc._finalised, smc.phi = True, np.array([0.0, 0.4, 0.8])
    with pytest.raises(RuntimeError, match="temperature"):
        smc.covariance()


def test_exports():
    import smcnuts_amd
    for name in ("PosteriorCovariance", "combine_cov_partials", "device_covariance"):
        assert hasattr(smcnuts_amd, name)
    from smcnuts_amd import _capi
    for name in ("smcn_cov_partials", "smcn_cov_dims", "smcn_cov_last_ms"):
        assert name in _capi.SIGNATURES
