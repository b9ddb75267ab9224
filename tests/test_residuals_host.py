"""The host side of the arma one-step residual checks (smcnuts_amd/residuals.py) against tests/_residuals.py, without a
device: merging and finishing the partials, the chi-square tails, the argument checks, and what SMCSampler.residuals
refuses before it reaches the device, in which order.

Tolerances: per compared quantity 10 x the error of the fp64 restatement against 50 digits on the test's
own inputs, as a share of the quantity's magnitude (tests/_residuals.py: mixture_scales), with a floor of 1e-14."""
import functools
import math

import numpy as np
import pytest

import _forecast as fref
import _residuals as ref
from _tol import close

from smcnuts_amd import residuals as R

T, L, M = 12, 3, 45
Q_AT = [0.5, 3.0]


@functools.lru_cache(maxsize=None)
def _inputs():
    ser = fref.synthetic_series(T, 5)
    X = fref.value_particles(M, 31)
    rng = np.random.default_rng(8)
    lw = 2.0 * rng.standard_normal(M)
    lw[::7] = -np.inf
    lw[3] = -800.0                                   # (its weight underflows to 0)
    return ser, X, lw


@functools.lru_cache(maxsize=None)
def _refs():
    ser, X, lw = _inputs()
    return ref.mixture(ser, X, lw, L, Q_AT), ref.mixture_mp(ser, X, lw, L, Q_AT), ref.mixture_scales(ser, X, lw, L, Q_AT)


def _check_all(got, what):
    a, b, sc = _refs()
    for k in ref.KEYS_T + ref.KEYS_L + ("ljung_box", "ljung_box_var"):
        tol = ref.tolerance(a[k], b[k], sc[k])
        with np.errstate(all="ignore"):
            close(np.asarray(got[k]) / sc[k], np.asarray(b[k]) / sc[k], rtol=0.0, atol=tol, what=f"{what} {k}")
    assert np.all(a["exceed_amb"] == 0.0)
    close(got["exceed"], b["exceed"], rtol=0.0, atol=ref.FLOOR * M, what=f"{what} exceed")
    assert got["n_particles"] == a["n_particles"] and np.all(got["n_bad"] == 0) and got["n_bad_acf"] == 0
    close(got["ess"], a["ess"], rtol=2.0 * (M + 8) * ref.U, what=f"{what} ess")


def test_one_block_finishes_to_the_definitions():
    ser, X, lw = _inputs()
    p = ref.partials(ser, X, lw, L, Q_AT)
    assert p.shape == (R.block_rows(T, L), R.QC) == (1 + T + L + 1, 20)
    res = R.combine_residual_partials([p], L, (0.3, 0.1))
    _check_all(ref.of(res), "one block")
    assert res.T == T and res.lags == L and res.lppd == float(np.sum(res.lpd)) and res.acf_band == 1.96 / math.sqrt(T)
    assert res.critical == tuple(R.chi2_isf(v, L) for v in (0.3, 0.1)) and res.levels == (0.3, 0.1)
    s = res.summary()
    assert len(s["rows"]) == T and s["rows"][2]["t"] == 3 and s["lags"] == L and len(s["acf"]) == L


def test_merging_equals_the_union_and_is_associative():
    ser, X, lw = _inputs()
    cuts = [0, 1, 17, 18, M]                          # (a block of one particle; one whose first particle has no weight)
    blocks = [ref.partials(ser, X[a:b], lw[a:b], L, Q_AT) for a, b in zip(cuts, cuts[1:])]
    m = R.merge_residual_partials
    left = m(m(m(blocks[0], blocks[1]), blocks[2]), blocks[3])
    right = m(blocks[0], m(blocks[1], m(blocks[2], blocks[3])))
    for name, acc in (("left", left), ("right", right)):
        _check_all(ref.of(R.combine_residual_partials([acc], L, (0.3, 0.1))), f"merged ({name})")
    _check_all(ref.of(R.combine_residual_partials(blocks, L, (0.3, 0.1))), "combined in list order")
    np.testing.assert_array_equal(left[:, R.NBAD], right[:, R.NBAD])
    assert left[0, 3] == right[0, 3] == np.isfinite(lw).sum()
    # a block without a contributing particle changes nothing, on either side
    none = ref.partials(ser, X[:4], np.full(4, -np.inf), L, Q_AT)
    assert m(left, none).tobytes() == left.tobytes() and m(none, left).tobytes() == left.tobytes()
    with pytest.raises(ValueError, match="same shape"):
        m(left, left[:-1])


def test_the_one_pass_reference_is_the_reference():
    """tests/_residuals.py: mixture_stream (what the longest series of the device tests is compared with) against
    mixture and mixture_scales on the inputs above."""
    ser, X, lw = _inputs()
    a, _, sc = _refs()
    b, sb = ref.mixture_stream(ser, X, lw, L, Q_AT)
    for k in ref.KEYS_T + ref.KEYS_L + ("ljung_box", "ljung_box_var"):
        close(np.asarray(b[k]) / sc[k], np.asarray(a[k]) / sc[k], rtol=0.0, atol=ref.FLOOR, what=f"one pass {k}")
        close(sb[k], sc[k], rtol=1e-12, what=f"one pass, magnitude of {k}")
    np.testing.assert_array_equal(b["exceed"], a["exceed"])
    part, _ = ref.mixture_stream(ser, X, lw, L, Q_AT, at_rows=[0, T - 1])
    assert np.all(np.isnan(part["mean"][1:T - 1])) and part["mean"][0] == b["mean"][0] and part["acf"].tobytes() == b["acf"].tobytes()


def test_bad_particles_give_nan_rows_and_counts():
    ser, X, lw = _inputs()
    Xb = np.concatenate([X, [[0.3, 0.4, 0.2, 800.0], [0.3, 0.4, 0.2, -800.0]]])      # sigma = inf, sigma = 0: bad at every t
    lwb = np.concatenate([lw, [0.1, -np.inf]])                                        # ... the second has no weight
    res = R.combine_residual_partials([ref.partials(ser, Xb, lwb, L, Q_AT)], L, (0.3, 0.1))
    assert np.all(res.n_bad == 1) and res.n_bad_acf == 1 and res.n_particles == np.isfinite(lw).sum() + 1
    for k in ("mean", "var", "sd", "z", "z_sd", "pit", "acf", "acf_sd", "exceed"):
        assert np.all(np.isnan(getattr(res, k))), k
    assert math.isnan(res.ljung_box) and math.isnan(res.ljung_box_sd)
    # the lpd runs over the other particles: the clean result, re-normalised by the bad particle's weight
    a, b, sc = _refs()
    fin = np.isfinite(lwb)
    shift = math.log(np.exp(lwb[fin] - lwb[fin].max()).sum()) - math.log(np.exp(lw[np.isfinite(lw)] - lwb[fin].max()).sum())
    tol = ref.tolerance(a["lpd"], b["lpd"], sc["lpd"])
    close((res.lpd + shift) / sc["lpd"], b["lpd"] / sc["lpd"], rtol=0.0, atol=tol, what="lpd over the other particles")
    # a particle that is bad from t = 6 on: the rows before stay clean
    p = ref.partials(ser, X, lw, L, Q_AT)
    p[6:1 + T, R.NBAD] = 1.0
    res = R.combine_residual_partials([p], L, (0.3, 0.1))
    assert np.all(np.isfinite(res.mean[:5])) and np.all(np.isnan(res.mean[5:])) and np.all(np.isfinite(res.lpd))
    assert np.all(np.isfinite(res.acf))


def test_no_contributing_particle_and_no_lags():
    ser, X, lw = _inputs()
    res = R.combine_residual_partials([ref.partials(ser, X, np.full(M, -np.inf), L, Q_AT)], L, (0.3, 0.1))
    assert res.n_particles == 0 and res.ess == 0.0 and np.all(res.n_bad == 0) and res.n_bad_acf == 0
    for k in ("mean", "var", "lpd", "z", "z_sd", "pit", "acf", "acf_sd", "exceed"):
        assert np.all(np.isnan(getattr(res, k))), k
    assert math.isnan(res.ljung_box) and math.isnan(res.lppd) and len(res.exceed) == 2
    p0 = ref.partials(ser, X, lw, 0)
    assert p0.shape == (1 + T, 20)
    res = R.combine_residual_partials([p0], 0, (0.05,))
    for k in ("acf", "acf_sd", "acf_band", "ljung_box", "ljung_box_sd", "levels", "critical", "exceed", "n_bad_acf"):
        assert getattr(res, k) is None, k
    assert res.lags == 0 and "ljung_box" not in res.summary() and np.all(np.isfinite(res.mean))
    with pytest.raises(ValueError, match="no partials"):
        R.combine_residual_partials([], 0)
    with pytest.raises(ValueError, match=r"3 lags is \[1 \+ T \+ 4\]\[20\]"):
        R.combine_residual_partials([np.zeros((3, 20))], 3)


def test_chi_square_tails_against_scipy():
    st = pytest.importorskip("scipy.stats")
    worst_sf = worst_isf = 0.0
    for df in range(1, 33):
        for x in np.geomspace(1e-3, 200.0, 40):
            want = st.chi2.sf(x, df)
            worst_sf = max(worst_sf, abs(R.chi2_sf(x, df) - want) / want)
        for p in (1e-12, 1e-6, 1e-3, 0.01, 0.05, 0.1, 0.5, 0.9, 0.99, 0.999):
            want = st.chi2.isf(p, df)
            worst_isf = max(worst_isf, abs(R.chi2_isf(p, df) - want) / want)
    print(f"largest relative difference: sf {worst_sf:.1e}, isf {worst_isf:.1e}")
    assert worst_sf <= 1e-12 and worst_isf <= 1e-12


def test_chi_square_tails_on_their_own():
    assert R.chi2_sf(0.0, 3) == 1.0 and R.chi2_sf(math.inf, 3) == 0.0 and R.chi2_isf(1.0, 3) == 0.0
    assert R.chi2_isf(0.0, 3) == math.inf
    close(R.chi2_sf(2.0, 2), math.exp(-1.0), rtol=1e-14, what="chi2_sf(2, df = 2) = e^-1")
    close(R.chi2_isf(0.05, 10), 18.307038053275146, rtol=1e-12, what="the 5 % critical value on 10 degrees of freedom")
    for df in (1, 7, 32):
        for p in (1e-9, 0.05, 0.7):
            close(R.chi2_sf(R.chi2_isf(p, df), df), p, rtol=1e-11, what="chi2_sf(chi2_isf(p))")
    with pytest.raises(ValueError, match="df"):
        R.chi2_sf(1.0, 0)
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        R.chi2_isf(1.5, 2)


def test_argument_checks():
    assert R.MAX_LAGS == 32 and R.MAX_LEVELS == 8
    assert [R.check_lags("f", None, n) for n in (1, 4, 5, 49, 50, 4000)] == [0, 0, 1, 9, 10, 10]
    assert R.check_lags("f", 0, 1) == 0 and R.check_lags("f", 32, 33) == 32 and R.check_lags("f", np.int64(4), 9) == 4
    for bad in (-1, 33, 2.0, True, "3"):
        with pytest.raises(ValueError, match=r"f: lags must be an integer in 0\.\.32"):
            R.check_lags("f", bad, 100)
    with pytest.raises(ValueError, match=r"f: lags = 9 needs a series of at least 10 values \(T = 9\)"):
        R.check_lags("f", 9, 9)
    assert R.check_levels("f", 0.1) == (0.1,) and R.check_levels("f", [0.05, 0.01]) == (0.05, 0.01) and R.check_levels("f", ()) == ()
    for bad in ([0.0], [1.0], [0.05, -0.1], [np.nan]):
        with pytest.raises(ValueError, match=r"f: every level must lie in \(0, 1\)"):
            R.check_levels("f", bad)
    with pytest.raises(ValueError, match="f: levels must be a scalar or a vector of at most 8 values"):
        R.check_levels("f", [0.1] * 9)
    with pytest.raises(ValueError, match="f: levels must be numeric"):
        R.check_levels("f", ["a"])
    from smcnuts_amd import ArmaModel
    t = ArmaModel(y=fref.synthetic_series(9, 1))
    with pytest.raises(ValueError, match=r"ArmaModel.residuals: lags = 9 needs"):
        t.residuals(np.zeros((2, 4)), lags=9)
    with pytest.raises(ValueError, match="ArmaModel.residuals: every level"):
        t.residuals(np.zeros((2, 4)), levels=[2.0])
    with pytest.raises(ValueError, match="ArmaModel.residuals: logw must hold one log-weight per row of x"):
        t.residuals(np.zeros((2, 4)), logw=np.zeros(3))
    # residual_partials, called on its own, reports under its own name
    with pytest.raises(ValueError, match="ArmaModel.residual_partials: logw must hold one log-weight per row of x"):
        t.residual_partials(np.zeros((2, 4)), logw=np.zeros(3))
    with pytest.raises(ValueError, match=r"ArmaModel.residual_partials: lags = 9 needs"):
        t.residual_partials(np.zeros((2, 4)), lags=9)
    for bad in ([np.inf], [1.0] * 9, [], [[1.0]]):
        with pytest.raises(ValueError, match="ArmaModel.residual_partials: q_at must hold 1 to 8 finite thresholds"):
            t.residual_partials(np.zeros((2, 4)), q_at=bad)
    with pytest.raises(ValueError, match="ArmaModel.residual_partials: q_at must be numeric"):
        t.residual_partials(np.zeros((2, 4)), q_at=["a"])
    with pytest.raises(ValueError, match="ArmaModel.residual_partials: q_at holds thresholds .* lags = 0 does not compute"):
        t.residual_partials(np.zeros((2, 4)), lags=0, q_at=[1.0])
    with pytest.raises(ValueError, match="ArmaModel.residual_points: lags must be"):
        t.residual_points(np.zeros((2, 4)), lags=40)
    # the default of a short series has no lag rows, whatever the levels
    assert ArmaModel(y=[0.1, 0.2, 0.3])._residual_args("f", None, (0.05,))[:2] == (0, ())


# ---- what SMCSampler.residuals refuses before it reaches the device (the tripwire of tests/test_postfit_guards_host.py) ----
class ReachedDevice(Exception):
    pass


class _Tripwire:
    @property
    def ctx(self):
        raise ReachedDevice("the guards passed")


class _OneRank:
    world_size, rank = 1, 0


def _sampler(target):
    from smcnuts_amd.smc_sampler import SMCSampler
    s = object.__new__(SMCSampler)
    s.lkernel, s.target, s._finalised, s.K = "forwardsLKernel", target, True, 3
    s.phi = np.array([0.0, 0.3, 0.7, 1.0])
    s.mean_estimate = np.zeros((4, getattr(target, "constrained_dim", target.dim)))
    s.rng, s.seed, s.comm, s.samples = None, 1234, _OneRank(), _Tripwire()
    return s


def _arma():
    from smcnuts_amd import ArmaModel
    return ArmaModel(y=fref.synthetic_series(30, 2))


def _asymptotic(s, kw):
    s.lkernel = "asymptoticLKernel"


def _other_target(s, kw):
    from smcnuts_amd import GaussianTarget
    s.target = GaussianTarget(3)


def _bad_lags(s, kw):
    kw["lags"] = 30


def _bad_levels(s, kw):
    kw["levels"] = [1.5]


def _not_finalised(s, kw):
    s._finalised = False


def _phi_half(s, kw):
    s.phi = np.array([0.0, 0.2, 0.4, 0.5])


MESSAGES = {
    _asymptotic: (NotImplementedError, "residuals(): the asymptotic L-kernel's estimates pool generations; residual diagnostics "
                                       "over the pooled generations are not implemented"),
    _other_target: (NotImplementedError, "GaussianTarget: one-step residual diagnostics are implemented for ArmaModel"),
    _bad_lags: (ValueError, "residuals: lags = 30 needs a series of at least 31 values (T = 30)"),
    _bad_levels: (ValueError, "residuals: every level must lie in (0, 1)"),
    _not_finalised: (RuntimeError, "residuals(): run sample() (or step() K times and finalise()) first"),
    _phi_half: (RuntimeError, "residuals(): the final temperature is phi = 0.5, not 1: the particles do not target the posterior"),
}
ORDER = [[_asymptotic], [_other_target], [_bad_lags, _bad_levels], [_not_finalised], [_phi_half]]


def _outcome(*faults):
    s, kw = _sampler(_arma()), {}
    for f in faults:
        f(s, kw)
    try:
        s.residuals(**kw)
    except Exception as e:      # noqa: BLE001 -- the class is what is compared
        return type(e), str(e)
    return None


def test_guards_and_their_order():
    assert _outcome() == (ReachedDevice, "the guards passed")
    for pos in ORDER:
        for f in pos:
            assert _outcome(f) == MESSAGES[f], f.__name__
    # of two faults the one checked first is reported (an unsupported target has no arguments to check)
    for i, pos0 in enumerate(ORDER):
        for pos1 in ORDER[i + 1:]:
            for f0 in pos0:
                for f1 in pos1:
                    assert _outcome(f0, f1) == MESSAGES[f0], (f0.__name__, f1.__name__)
                    assert _outcome(f1, f0) == MESSAGES[f0], (f1.__name__, f0.__name__)


def test_every_other_target_is_refused():
    import smcnuts_amd
    from smcnuts_amd.model import targets as Tm
    X = (np.arange(12, dtype=np.float64).reshape(6, 2) % 7.0 - 3.0) / 4.0
    y01 = np.array([0.0, 1.0, 1.0, 0.0, 1.0, 0.0])
    made = [Tm.GaussianTarget(3), Tm.IsoGaussian(2), Tm.GLMTarget(X, y01), Tm.LogisticRegression(X, y01), Tm.PRMwCDModel()]
    for t in made:
        with pytest.raises(NotImplementedError, match=f"{type(t).__name__}: one-step residual diagnostics are implemented for ArmaModel"):
            _sampler(t).residuals()
    # ... and no other target class has the method the sampler looks for
    for name in dir(smcnuts_amd):
        cls = getattr(smcnuts_amd, name)
        if isinstance(cls, type) and issubclass(cls, Tm.DeviceTarget | Tm.HostTarget):
            assert hasattr(cls, "residual_partials") == (cls is Tm.ArmaModel), name
    assert smcnuts_amd.OneStepResiduals is R.OneStepResiduals and smcnuts_amd.combine_residual_partials is R.combine_residual_partials
