"""smcnuts_amd/calibration.py on the host (no GPU): the merge of partials, the PIT histogram, the randomisation, the
inverse normal cdf against mpmath, argument checks and refusals -- and tests/_calibration.py itself: the fp64 restatement
of the device's tails against 50 digits on the GPU tests' inputs, with no unconverged pair among them."""
import math

import numpy as np
import pytest

import _calibration as ref
from smcnuts_amd import calibration as cal


def _block(rng, n, M, mw):
    """A partials block of M random (w, lo, up, ll) per row, formed as the device forms it."""
    lw = rng.normal(0.0, 2.0, M) + mw
    lo, pm = rng.uniform(0.0, 0.6, (M, n)), rng.uniform(0.0, 0.4, (M, n))
    up, ll = 1.0 - lo - pm, rng.normal(-3.0, 2.0, (M, n))
    m = lw.max()
    w = np.exp(lw - m)
    out = np.zeros((1 + n, cal.QC))
    out[0, :4] = m, w.sum(), (w * w).sum(), M
    v = (lw - m)[:, None] - ll
    mb = v.max(0)
    e = np.exp(v - mb)
    out[1:, cal.SW] = w.sum()
    out[1:, cal.LO], out[1:, cal.UP] = (w[:, None] * lo).sum(0), (w[:, None] * up).sum(0)
    out[1:, cal.MB], out[1:, cal.SB] = mb, e.sum(0)
    out[1:, cal.LOB], out[1:, cal.UPB] = (e * lo).sum(0), (e * up).sum(0)
    return out, (lw, lo, up, ll)


def _finish(parts):
    r = cal.combine_calibration_partials(parts)
    return np.stack([r.pit_lo, r.pit_hi, r.sf, r.pit_lo_loo, r.pit_hi_loo, r.sf_loo])


def test_merge_is_associative_and_rescales():
    rng = np.random.default_rng(0)
    n = 7
    (a, ra), (b, rb), (c, rc) = _block(rng, n, 30, 0.0), _block(rng, n, 5, -40.0), _block(rng, n, 17, 25.0)     # differing mw
    left = cal.merge_calibration_partials(cal.merge_calibration_partials(a, b), c)
    right = cal.merge_calibration_partials(a, cal.merge_calibration_partials(b, c))
    np.testing.assert_allclose(left, right, rtol=1e-13, atol=0.0)
    np.testing.assert_allclose(_finish([a, b, c]), _finish([left]), rtol=0.0, atol=0.0)
    # against the definitions on the union
    lw, lo, up, ll = (np.concatenate(v) for v in zip(ra, rb, rc))
    m = ref.mixture(lo, up, ll, lw)
    got = cal.combine_calibration_partials([a, b, c])
    for k in m:
        np.testing.assert_allclose(getattr(got, k), m[k], rtol=1e-13)
    assert got.n_particles == 52
    w = np.exp(lw - lw.max())
    assert got.ess == pytest.approx(w.sum() ** 2 / (w * w).sum(), rel=1e-13)
    # counts add and make their rows NaN, the others stay
    b2 = b.copy()
    b2[2, cal.NINF], b2[4, cal.NUNC] = 1.0, 2.0
    bad = cal.combine_calibration_partials([a, b2, c])
    assert bad.ninf[1] == 1 and bad.n_unconverged[3] == 2
    assert np.isnan(bad.pit_lo[[1, 3]]).all() and np.isnan(bad.sf_loo[[1, 3]]).all()
    keep = np.array([0, 2, 4, 5, 6])
    assert bad.pit_lo[keep].tobytes() == got.pit_lo[keep].tobytes()


def test_merge_with_an_empty_block_and_bad_shapes():
    rng = np.random.default_rng(1)
    a, _ = _block(rng, 4, 9, 0.0)
    empty = np.zeros_like(a)
    empty[0, 0], empty[1:, cal.MB] = -np.inf, -np.inf
    assert cal.merge_calibration_partials(a, empty).tobytes() == a.tobytes()
    assert cal.merge_calibration_partials(empty, a).tobytes() == a.tobytes()
    none = cal.combine_calibration_partials([empty])
    assert none.n_particles == 0 and none.ess == 0.0 and np.isnan(none.pit_lo).all() and np.isnan(none.sf_loo).all()
    with pytest.raises(ValueError, match="same shape"):
        cal.merge_calibration_partials(a, a[:-1])
    with pytest.raises(ValueError, match="no partials"):
        cal.combine_calibration_partials([])
    with pytest.raises(ValueError, match=r"\[1 \+ n\]\[9\]"):
        cal.combine_calibration_partials([np.zeros((5, 11))])


def _cal(lo, hi):
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    z = np.zeros(lo.shape)
    return cal.Calibration(lo, hi, 1.0 - hi, lo.copy(), hi.copy(), 1.0 - hi, z, z.copy(), 10, 10.0)


def test_pit_histogram():
    rng = np.random.default_rng(2)
    lo = rng.uniform(0.0, 0.7, 50)
    c = _cal(lo, lo + rng.uniform(0.0, 0.3, 50))
    for bins in (1, 4, 10):
        h = c.pit_histogram(bins)
        assert h.shape == (bins,) and abs(h.sum() - 1.0) < 1e-14 and np.all(h >= 0.0)
    np.testing.assert_allclose(_cal([0.0, 0.0], [1.0, 1.0]).pit_histogram(10), np.full(10, 0.1), rtol=1e-15)     # flat
    # the step hi == lo: the whole row in the bin that holds the point; an interval inside one bin likewise
    np.testing.assert_array_equal(_cal([0.25], [0.25]).pit_histogram(10), np.eye(10)[2])
    np.testing.assert_array_equal(_cal([0.0], [0.0]).pit_histogram(10), np.eye(10)[0])
    np.testing.assert_array_equal(_cal([1.0], [1.0]).pit_histogram(10), np.eye(10)[9])
    np.testing.assert_allclose(_cal([0.21], [0.29]).pit_histogram(10), np.eye(10)[2], atol=1e-15)
    np.testing.assert_allclose(_cal([0.1], [0.4]).pit_histogram(10), [0, 1 / 3, 1 / 3, 1 / 3, 0, 0, 0, 0, 0, 0], atol=1e-15)
    # NaN rows are left out
    np.testing.assert_array_equal(_cal([0.25, np.nan], [0.25, np.nan]).pit_histogram(10), np.eye(10)[2])
    assert np.isnan(_cal([np.nan], [np.nan]).pit_histogram(3)).all()
    assert c.pit_histogram(10, loo=True).tobytes() == c.pit_histogram(10).tobytes()
    for bad in (0, 2.5, True, 1001):
        with pytest.raises(ValueError, match="bins"):
            c.pit_histogram(bad)


def test_randomised_depends_on_seed_and_row_only():
    lo = np.linspace(0.0, 0.8, 40)
    a, b = _cal(lo, lo + 0.2), _cal(lo[:13], lo[:13] + 0.2)
    u, v = a.randomised(5), b.randomised(5)
    assert u[:13].tobytes() == v.tobytes() and np.all((u >= lo) & (u <= lo + 0.2))
    assert a.randomised(6).tobytes() != u.tobytes() and a.randomised(5).tobytes() == u.tobytes()
    assert a.quantile_residuals(5)[:13].tobytes() == b.quantile_residuals(5).tobytes()
    for bad in (-1, 1.5, None, True):
        with pytest.raises(ValueError, match="seed"):
            a.randomised(bad)


def test_quantile_residuals_use_the_smaller_tail():
    import mpmath
    mpmath.mp.dps = 50
    # a continuous row far in the upper tail: u = 1 - 1e-16 would round to +8.2 or inf; sf keeps it
    lo = np.array([1.0, 0.5, 1e-250])
    c = cal.Calibration(lo, lo.copy(), np.array([6.22096057427178e-16, 0.5, 1.0]), lo, lo, np.zeros(3), np.zeros(3), np.zeros(3), 1, 1.0)
    r = c.quantile_residuals(0)
    assert r[0] == pytest.approx(8.0, rel=1e-13) and r[1] == 0.0
    assert r[2] == cal.norm_ppf(p=1e-250) and r[2] < -33.0            # (norm_ppf itself: the next test)
    assert abs(float(mpmath.ncdf(mpmath.mpf(r[0]))) - (1.0 - 6.22096057427178e-16)) < 1e-16
    # NaN rows stay NaN
    n = _cal([np.nan, 0.2], [np.nan, 0.3]).quantile_residuals(1)
    assert np.isnan(n[0]) and np.isfinite(n[1])


def test_inverse_normal_cdf_against_mpmath():
    import mpmath
    mpmath.mp.dps = 50

    def want(p):        # Phi^-1 at 50 digits, by its own Newton iteration from the double's value
        p = mpmath.mpf(p)
        return mpmath.findroot(lambda x: mpmath.ncdf(x) - p, float(cal.norm_ppf(p=float(p))), tol=1e-45, maxsteps=50) \
            if p != 0.5 else mpmath.mpf(0)

    ps = [10.0 ** -k for k in (300, 200, 100, 50, 20, 16, 10, 5, 3, 2, 1)] + [0.074, 0.075, 0.3, 0.5, 0.7, 0.925, 0.926, 0.99,
                                                                             1 - 1e-10, 1 - 1e-15, 1 - 1e-16]
    for p in ps:
        got, w = cal.norm_ppf(p=p), float(want(p))
        # one ulp of p moves x by u p / pdf(x) <= u max(1 / |x|, 1.26); x itself rounds by u |x|: 1e-15 (1 + |x|) is ~5 x that
        assert abs(got - w) <= 1e-15 * (1.0 + abs(w)), (p, got, w)
        # through the upper tail: the same values mirrored, and beyond what p can hold
        assert cal.norm_ppf(sf=p) == -got
    for s in (1e-17, 1e-40, 1e-300):
        assert cal.norm_ppf(sf=s) == -cal.norm_ppf(p=s) and cal.norm_ppf(sf=s) > 8.0
    v = cal.norm_ppf(p=np.array([[0.0, 1.0, 0.5], [-0.1, 1.1, np.nan]]))
    assert v[0, 0] == -np.inf and v[0, 1] == np.inf and v[0, 2] == 0.0 and np.isnan(v[1]).all()
    assert cal.norm_ppf(sf=0.0) == np.inf and isinstance(cal.norm_ppf(p=0.3), float)
    with pytest.raises(ValueError, match="p or sf"):
        cal.norm_ppf()


def test_summary_rows():
    c = _cal([0.1, 0.2], [0.3, 0.2])
    s = c.summary()
    assert s["n_obs"] == 2 and s["n_particles"] == 10 and s["n_nonfinite"] == 0 and len(s["rows"]) == 2
    assert s["rows"][1] == dict(i=1, pit_lo=0.2, pit_hi=0.2, sf=0.8, pit_lo_loo=0.2, pit_hi_loo=0.2, sf_loo=0.8, ninf=0,
                                n_unconverged=0)
    assert c.pit is c.pit_lo and c.pit_loo is c.pit_lo_loo


def test_argument_checks_and_refusals():
    from smcnuts_amd import ArmaModel, Calibration, GLMTarget, HierarchicalGLM
    assert Calibration is cal.Calibration
    rng = np.random.default_rng(3)
    X, y = rng.standard_normal((12, 2)), rng.poisson(3.0, 12).astype(np.float64)
    t = GLMTarget(X, y, family="poisson_log")
    with pytest.raises(ValueError):
        t.calibration_points(np.zeros((4, 5)))                       # D is 3
    with pytest.raises(ValueError, match="one log-weight per row"):
        t.calibration_partials(np.zeros((4, 3)), np.zeros(5))
    w = GLMTarget(X, y, family="poisson_log", weights=np.ones(12))
    for call in (lambda: w.calibration(np.zeros((4, 3))), lambda: w.calibration_points(np.zeros(3)),
                 lambda: w.calibration_partials(np.zeros((4, 3)))):
        with pytest.raises(NotImplementedError, match="weights"):
            call()
    h = HierarchicalGLM(X, y, groups=np.arange(12) % 3, family="poisson_log")
    for tgt, D in ((h, h.dim), (ArmaModel(), 4)):
        for call in (lambda: tgt.calibration(np.zeros((2, D))), lambda: tgt.calibration_points(np.zeros(D)),
                     lambda: tgt.calibration_partials(np.zeros((2, D)))):
            with pytest.raises(NotImplementedError, match="GLMTarget"):
                call()


# ---- tests/_calibration.py itself ------------------------------------------------------------------------------------------------
def test_the_reference_against_mpmath_betainc():
    """_betainc_mp (a continued fraction) against mpmath's own betainc (a hypergeometric series) where that converges."""
    mp = ref._mp()
    for a, b, x in ((8.0, 20.0, 0.2), (0.5, 7.0, 0.05), (21.0, 8.0, 0.6), (1000.0, 30.0, 0.95), (3.0, 0.05, 0.3)):
        a, b, x = mp.mpf(a), mp.mpf(b), mp.mpf(x)
        assert x < (a + 1) / (a + b + 2)
        got, want = ref._betainc_mp(a, b, x, 1 - x), mp.betainc(a, b, 0, x, regularized=True)
        assert abs(got / want - 1) < mp.mpf(10) ** -50


@pytest.mark.parametrize("family", ref.FAMILIES)
def test_the_restatement_on_the_gpu_tests_inputs(family):
    """On every case of tests/test_gpu_calibration.py's first test: no unconverged pair (a condition on the inputs), the
    kinds the issue lists are met, and the restatement agrees with 50 digits (its error is what the tolerance is made of)."""
    from test_gpu_calibration import SHAPES
    worst = 0.0
    for n, M, Dc, offset in SHAPES:
        key = (family, n, M, Dc, offset)
        c = ref.case(*key)
        lo, up, term, conv = ref.tails64(c)
        fin = c["finite"]
        assert conv[fin].all(), f"{key}: {int((~conv[fin]).sum())} unconverged pairs"
        assert np.isnan(lo[~fin]).all() and not np.isnan(lo[fin]).any() and not np.isnan(up[fin]).any()
        P = np.array(ref.sample_pairs(c))
        mp = ref.tails_mp(key, P)
        e = max(ref.share(lo[P[:, 0], P[:, 1]], mp[:, 0]), ref.share(up[P[:, 0], P[:, 1]], mp[:, 1]))
        worst = max(worst, e)
    print(f"  {family}: the restatement's largest relative error of a tail {worst:.2e}")
    # the term's own rounding bounds it: |term's parts| <= 3e6 (y log mu, lgamma(y + 1) at y = 2e5) times a few u, 3e-9;
    # where the tail formed as a complement is the smaller one (NB2 at phi = 0.05, y = 10 mu + 3: up = 0.03 beside
    # lo = 0.97) that error is divided by the tail
    assert worst < 3e6 * 8 * 2.0 ** -53 / 0.03
    if family in ("poisson_log", "neg_binomial_2_log"):
        c = ref.case(family, 130, 257, 17, True)
        assert {0.0, 1.0} <= set(c["y"]) and c["y"].max() >= 10 * 2e4 + 3
        mu = np.exp(c["x"][c["finite"], 0])
        assert mu.min() <= 1.001e-3 and mu.max() >= 1.999e4
        if family == "neg_binomial_2_log":
            phi = np.exp(c["x"][c["finite"], 17])
            assert phi.min() <= 0.0501 and phi.max() >= 0.999e6


def test_the_restatement_reports_the_iteration_bound():
    c = dict(family="poisson_log", fam=1, X=np.zeros((2, 0)), y=np.array([4e5, 7.0]), offset=None,
             x=np.array([[math.log(4e5)], [math.log(7.0)]]), Dc=1)
    lo, up, _, conv = ref.tails64(c)
    np.testing.assert_array_equal(conv, [[False, True], [True, True]])
    assert np.isnan(lo[0, 0]) and np.isnan(up[0, 0]) and not np.isnan(lo[1]).any()
    assert 8.2 * math.sqrt(4e5) > ref.MAXIT > 8.2 * math.sqrt(2e4)


def _laplace_draws(model, S, rng):
    from test_gpu_pointwise import _laplace
    mode, _ = _laplace(model)
    D = model.dim
    H = np.empty((D, D))
    for j in range(D):
        e = np.zeros(D)
        e[j] = 1e-5
        H[:, j] = (model.logpdfgrad(mode + e) - model.logpdfgrad(mode - e)) / 2e-5
    cov = np.linalg.inv(-0.5 * (H + H.T))
    return rng.multivariate_normal(mode, cov, size=S)


def test_the_u_shape_on_the_cpu():
    """The inequality of test_a_poisson_fit_of_overdispersed_counts_is_u_shaped, fixed here before any GPU run: the NumPy
    restatement on 400 draws from the Laplace approximation of either posterior (the NumPy models of tests/_glm.py and
    tests/_glm_disp.py)."""
    import _glm
    import _glm_disp as gd
    from test_gpu_calibration import _overdispersed
    X, y = _overdispersed()
    rng = np.random.default_rng(0)
    outer = {}
    for fam, model in (("poisson_log", _glm.GLMNumpy(X, y, "poisson_log", 2.5)),
                       ("neg_binomial_2_log", gd.GLMDispNumpy(X, y, "neg_binomial_2_log", 2.5, (0.0, 2.5)))):
        x = _laplace_draws(model, 400, rng)
        c = dict(family=fam, fam=ref.FAMILIES.index(fam), X=X, y=y, offset=None, x=x, Dc=3)
        lo, up, term, conv = ref.tails64(c)
        assert conv.all()
        m = ref.mixture(lo, up, term, np.zeros(400))
        r = cal.Calibration(m["pit_lo"], 1.0 - m["sf"], m["sf"], m["pit_lo_loo"], 1.0 - m["sf_loo"], m["sf_loo"],
                            np.zeros(130), np.zeros(130), 400, 400.0)
        h = r.pit_histogram(10)
        outer[fam] = float(h[0] + h[-1])
        print(f"  {fam}: histogram {np.round(h, 3)}, outer bins {outer[fam]:.3f}")
    # 0.527 and 0.206 (flat: 0.2); the GPU test asserts them with a margin of a third of their gap
    assert abs(outer["poisson_log"] - 0.527) < 0.002 and abs(outer["neg_binomial_2_log"] - 0.206) < 0.002
