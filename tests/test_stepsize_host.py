"""Host side of the step-size probe (smcnuts_amd/stepsize.py): the choice from an acceptance curve, the combination of
shards' partials, the ladders, the refusals that come before any device context is made -- and the condition the GPU
comparison rests on, asserted on the NumPy restatement alone: at most a quarter of a case's entries lie beyond the
exactness band (tests/_stepsize.py).  No GPU."""
import numpy as np
import pytest

import _stepsize as ref
from smcnuts_amd import stepsize as ss


# ---- choose_step_size -------------------------------------------------------------------------------------------------
def test_choose_interpolates_in_log_eps():
    lad = 2.0 ** np.arange(-4.0, 0.0)
    eps, br = ss.choose_step_size(lad, [0.99, 0.9, 0.7, 0.2], 0.8)
    assert br
    assert eps == pytest.approx(2.0 ** (-3.0 + 0.5), rel=1e-14)          # halfway between 0.9 and 0.7, in log2
    eps, br = ss.choose_step_size(lad, [0.99, 0.9, 0.85, 0.05], 0.8)
    assert br and eps == pytest.approx(2.0 ** (-2.0 + 0.05 / 0.8), rel=1e-14)


def test_choose_takes_the_first_crossing_of_a_non_monotone_curve():
    lad = 2.0 ** np.arange(-5.0, 0.0)
    eps, br = ss.choose_step_size(lad, [0.95, 0.7, 0.9, 0.95, 0.1], 0.8)
    assert br and lad[0] < eps < lad[1]
    assert eps == pytest.approx(2.0 ** (-5.0 + 0.15 / 0.25), rel=1e-14)


def test_choose_unbracketed_ends():
    lad = np.array([0.01, 0.1, 1.0])
    assert ss.choose_step_size(lad, [0.99, 0.95, 0.9], 0.8) == (1.0, False)
    assert ss.choose_step_size(lad, [0.5, 0.4, 0.1], 0.8) == (0.01, False)
    assert ss.choose_step_size(lad, [np.nan, np.nan, np.nan], 0.8) == (0.01, False)
    assert ss.choose_step_size([0.3], [0.9], 0.8) == (0.3, False)


def test_choose_target_exactly_an_entry():
    lad = np.array([0.01, 0.1, 1.0])
    # an entry AT the target is not below it: the crossing lies between it and its successor, at the entry itself
    eps, br = ss.choose_step_size(lad, [0.9, 0.8, 0.3], 0.8)
    assert br and eps == pytest.approx(0.1, rel=1e-15)
    eps, br = ss.choose_step_size(lad, [0.9, 0.85, 0.8], 0.8)
    assert (eps, br) == (1.0, False)
    with pytest.raises(ValueError):
        ss.choose_step_size(lad, [0.9, 0.8], 0.8)


# ---- ladders ----------------------------------------------------------------------------------------------------------
def test_ladders():
    lad = ss.default_ladder()
    assert lad.shape == (16,) and lad[0] == 2.0 ** -12 and lad[-1] == 8.0
    np.testing.assert_array_equal(lad[1:] / lad[:-1], 2.0)
    fine = ss.refine_ladder(0.1, 0.2)
    assert fine.shape == (16,) and fine[0] == 0.1 and fine[-1] == 0.2 and np.all(np.diff(fine) > 0)
    np.testing.assert_allclose(fine[1:] / fine[:-1], 2.0 ** (1 / 15), rtol=1e-14)
    ss.check_ladder(fine)
    for bad in ((0.2, 0.1), (0.0, 1.0), (0.1, np.inf), (0.1, 0.1)):
        with pytest.raises(ValueError):
            ss.refine_ladder(*bad)
    for bad in ([], np.ones(17).cumsum(), [0.1, 0.1], [0.2, 0.1], [-1.0, 1.0], [0.1, np.nan], [0.0, 1.0]):
        with pytest.raises(ValueError):
            ss.check_ladder(bad)


# ---- combine_stepsize_partials ------------------------------------------------------------------------------------------
def _partials(lw, a, d, excl):
    """One shard's partials from per-particle values, as the device forms them."""
    L = a.shape[0]
    fin = np.isfinite(lw)
    m = lw[fin].max() if fin.any() else -np.inf
    with np.errstate(all="ignore"):
        w = np.where(excl, 0.0, np.exp(lw - m))
    p = np.zeros((1 + L, 4))
    p[0] = (m, lw.size, excl.sum(), 0.0)
    for j in range(L):
        dj = d[j] & ~excl
        p[1 + j] = (np.sum(w * a[j]), np.sum(w * dj), np.sum(w), dj.sum())
    return p


@pytest.mark.parametrize("ways", [1, 2, 8])
def test_combine_equals_one_shard(ways):
    rng = np.random.default_rng(5)
    M, L = 64, 7
    lw = 30.0 * rng.standard_normal(M)
    lw[8:16] = -np.inf                      # (8 ways: a whole shard without weight)
    lw[3] = -np.inf
    excl = ~np.isfinite(lw)
    a = np.where(excl, 0.0, rng.random((L, M)))
    d = rng.random((L, M)) < 0.2
    one = ss.combine_stepsize_partials([_partials(lw, a, d, excl)])
    sl = [slice(k * M // ways, (k + 1) * M // ways) for k in range(ways)]
    parts = [_partials(lw[s], a[:, s], d[:, s], excl[s]) for s in sl]
    if ways == 8:
        assert not np.isfinite(parts[1][0, 0]) and parts[1][0, 2] == 8
    got = ss.combine_stepsize_partials(parts)
    assert got[0, 0] == one[0, 0]
    np.testing.assert_array_equal(got[0, 1:], one[0, 1:])
    np.testing.assert_array_equal(got[1:, 3], one[1:, 3])
    np.testing.assert_allclose(got[1:, :3], one[1:, :3], rtol=1e-13, atol=0.0)
    acc, div = ss.curves_from_partials(got)
    acc1, div1 = ss.curves_from_partials(one)
    np.testing.assert_allclose(acc, acc1, rtol=1e-13)
    np.testing.assert_allclose(div, div1, rtol=1e-13, atol=1e-300)


def test_combine_all_excluded_and_bad_shapes():
    p = np.zeros((3, 4))
    p[0] = (-np.inf, 5, 5, 0)
    got = ss.combine_stepsize_partials([p, p])
    assert got[0, 0] == -np.inf and got[0, 1] == 10 and got[0, 2] == 10
    assert np.all(np.isnan(ss.curves_from_partials(got)[0]))
    res = ss.probe_from_partials(np.array([0.1, 0.2]), got, 0.8, 0.0)
    assert not res.bracketed and res.step_size == 0.1 and res.n_excluded == 10
    with pytest.raises(ValueError):
        ss.combine_stepsize_partials([])
    with pytest.raises(ValueError):
        ss.combine_stepsize_partials([p, np.zeros((4, 4))])


def test_run_probe_refines_between_the_bracketing_neighbours():
    """The driver on a synthetic acceptance curve a(eps) = 1 / (1 + (eps / 0.3)^4): both passes, common to every caller."""
    seen = []

    def one_pass(lad):
        seen.append(lad.copy())
        a = 1.0 / (1.0 + (lad / 0.3) ** 4)
        part = np.zeros((1 + lad.size, 4))
        part[0] = (0.0, 10, 0, 0)
        part[1:, 0], part[1:, 2] = 10 * a, 10.0
        return part, 0.5
    res = ss.run_probe(one_pass, ss.default_ladder(), 0.8, True)
    want = 0.3 * 0.25 ** 0.25
    assert res.bracketed and res.coarse is not None and res.ms == 1.0
    assert seen[1][0] == 0.125 and seen[1][-1] == 0.25 and len(seen) == 2
    assert abs(res.step_size / want - 1.0) < 2e-3 < abs(res.coarse.step_size / want - 1.0)
    assert isinstance(res, ss.StepSizeProbe) and res.n_particles == 10 and res.target_accept == 0.8
    res = ss.run_probe(one_pass, ss.default_ladder(), 0.8, False)
    assert res.coarse is None and len(seen) == 3


# ---- refusals, before any context is made ---------------------------------------------------------------------------------
def test_probe_arguments_are_refused_before_any_context():
    from smcnuts_amd import GaussianTarget
    t = GaussianTarget(3)
    x = np.zeros((4, 3))
    for kw in (dict(target_accept=0.0), dict(target_accept=1.0), dict(target_accept="high"), dict(n_leapfrog=0),
               dict(n_leapfrog=65), dict(n_leapfrog=2.5), dict(max_particles=0), dict(ladder=[0.2, 0.1]),
               dict(ladder=np.arange(1.0, 18.0)), dict(ladder=[]), dict(phi=1.5), dict(phi=np.nan), dict(delta_max=0.0)):
        with pytest.raises(ValueError):
            t.probe_step_size(x, **kw)
    assert t._ctx is None
    with pytest.raises(ValueError):
        t.probe_step_size(np.zeros((4, 2)))
    assert t._ctx is None


def test_host_target_names_the_reason():
    from smcnuts_amd import HostTarget

    class T:
        dim = 2
        logpdf = logpdfgrad = staticmethod(lambda x, phi=1.0: None)
    with pytest.raises(NotImplementedError, match="device functor"):
        HostTarget(T()).probe_step_size(np.zeros((1, 2)))


def test_sampler_refuses_bad_step_size_strings_before_any_context(monkeypatch):
    from smcnuts_amd import ArmaModel, HostTarget, SMCSampler, _capi
    from smcnuts_amd.proposal.nuts import NUTSProposal

    def no_context(*a, **k):
        raise AssertionError("a context was made before the refusal")
    monkeypatch.setattr(_capi, "Context", no_context)
    t = ArmaModel()
    with pytest.raises(ValueError, match="auto"):
        SMCSampler(K=2, N=64, target=t, step_size="x")
    with pytest.raises(ValueError, match="forward_kernel"):
        SMCSampler(K=2, N=64, target=t, step_size="auto", forward_kernel=NUTSProposal(t, None, 0.01))

    class T:
        dim = 2
        logpdf = logpdfgrad = staticmethod(lambda x, phi=1.0: None)
    with pytest.raises(ValueError, match="host-evaluated"):
        SMCSampler(K=2, N=64, target=HostTarget(T()), step_size="auto")


def test_exports():
    import smcnuts_amd
    assert smcnuts_amd.StepSizeProbe is ss.StepSizeProbe
    assert smcnuts_amd.choose_step_size is ss.choose_step_size
    assert smcnuts_amd.combine_stepsize_partials is ss.combine_stepsize_partials


# ---- the NumPy restatement: its own properties, and the cap the GPU comparison rests on -------------------------------
def test_reference_on_the_standard_normal():
    lp, grad = ref.gaussian(4)
    rng = np.random.default_rng(0)
    x, r = rng.standard_normal((30, 4)), rng.standard_normal((30, 4))
    out = ref.probe_reference(lp, grad, x, r, [2.0 ** -8, 1.0, 2.0 ** 1.5], n=64)
    assert np.all(out["accept"][0] > 0.999) and np.all(out["first_bad"][:2] == 0)
    assert np.all(out["first_bad"][2] > 0)                     # beyond the stability limit eps = 2: every pair diverges
    lw = rng.standard_normal(30)
    lw[4] = -np.inf
    x[7] = np.inf
    out = ref.probe_reference(lp, grad, x, r[:10], [0.5], logw=lw, max_particles=10)
    np.testing.assert_array_equal(out["index"], np.arange(10) * 3)
    assert out["excluded"].sum() == 0 and out["partials"][0, 1] == 10
    out = ref.probe_reference(lp, grad, x, r, [0.5], logw=lw)
    assert out["excluded"].sum() == 2 and out["partials"][0, 2] == 2 and np.all(out["accept"][0, [4, 7]] == 0.0)


@pytest.mark.parametrize("name", ref.ANALYTIC)
def test_entries_beyond_the_band_stay_under_the_cap(name):
    case = ref.CASES[name][0]()
    lp, grad = case["callbacks"]
    x, r = ref.case_points(name, case["D"])
    out = ref.probe_reference(lp, grad, x, r, ref.case_ladder(name))
    share = float(np.mean(ref.beyond_band(out)))
    print(f"{name}: share beyond the band {share:.3f}")
    assert share <= ref.CAP
