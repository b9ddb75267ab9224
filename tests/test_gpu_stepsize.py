"""The step-size probe on the device (smcn_stepsize_probe) against its NumPy restatement (tests/_stepsize.py), particle by
particle, for every device functor; its weighted reduction, subsampling and determinism; the properties it must have
(scaling, divergence); that it leaves a sampler's state alone; resident against host points; shards; step_size="auto"
and retune_step_size() end to end.

Comparison of a case (tests/_stepsize.compare_entries): entries whose reference |dH| stays within 20 are compared in the
exact class; beyond it by the divergent flag where the reference says divergent, by accept <= exp(-20) where every step
lies beyond the band, and otherwise by the exact steps in front of the first one beyond it (a trajectory whose energy
error leaves the band at its last step has a statistic near 7/8, not near 0).  At most a quarter of a case's entries
may lie beyond the band -- asserted on the reference before anything is compared."""

import numpy as np
import pytest

import _stepsize as ref
from _tol import close

pytestmark = pytest.mark.gpu

# accept is a mean of n terms in [0, 1]; its error is the energy error's.  Every call site started in the project's 1e-11
# class (tests/_tol.py) and is now set to at most 10x what the first GPU runs recorded there (DESIGN.md 4.5's table):
TOL = dict(rtol=4.9e-13, atol=4.9e-13)          # per particle against NumPy: largest difference 9.8e-14 (gauss_d257)
TOL_SHAPES = dict(rtol=1e-13, atol=1e-13)       # the further call shapes: largest difference 2.0e-14
TOL_SUBSAMPLE = dict(rtol=1.4e-14, atol=1.4e-14)   # N(0, I), D = 5: largest difference 2.8e-15
TOL_SAME = dict(rtol=2e-15, atol=2e-15)         # the same trajectories, summed over shards in another order: largest difference 3.3e-16


def _case(name, tmp_path):
    build = ref.CASES[name][0]
    if build is None:
        target = ref.SPECIAL[name](tmp_path)
        return target, ref.target_callbacks(target), target.dim
    case = build()
    target = case["make"]()
    return target, case["callbacks"] or ref.target_callbacks(target), case["D"]


def _device(target, ladder, x, r, **kw):
    ctx = target._context(x.shape[0])
    return ctx.stepsize_probe(ladder, x=x, r=r, n_leapfrog=kw.pop("n", ref.N_LEAP), want_particles=True, **kw)


@pytest.mark.parametrize("name", list(ref.CASES))
def test_particles_against_numpy(name, tmp_path):
    target, (lp, grad), D = _case(name, tmp_path)
    assert target.dim == D
    x, r = ref.case_points(name, D)
    ladder = ref.case_ladder(name)
    want = ref.probe_reference(lp, grad, x, r, ladder)
    part, acc, fb = _device(target, ladder, x, r)
    share = ref.compare_entries(want, acc, fb, close, **TOL)
    print(f"{name}: share beyond the band {share:.3f}")
    assert part[0, 0] == 0.0 and part[0, 1] == x.shape[0] and part[0, 2] == 0
    close(part[1:, 0], acc.sum(axis=1), rtol=4e-15)       # unit weights: the reduction of the device's own values
    np.testing.assert_array_equal(part[1:, 2], x.shape[0])
    np.testing.assert_array_equal(part[1:, 3], (fb != 0).sum(axis=1))


@pytest.mark.parametrize("name,M,L,n", [("gauss_d5", 1, 16, 8), ("logistic_d5", 37, 1, 8), ("logistic_d5", 37, 16, 1),
                                        ("gauss_d5", 37, 16, 64), ("logistic_d17", 5, 3, 64)])
def test_call_shapes(name, M, L, n, tmp_path):
    target, (lp, grad), D = _case(name, tmp_path)
    x, r = ref.case_points(name, D)
    x, r = x[:M], r[:M]
    base = ref.case_ladder(name) / (4.0 if n > 8 else 1.0)       # (longer trajectories: a ladder two octaves lower)
    ladder = base if L == 16 else base[8:8 + L]
    want = ref.probe_reference(lp, grad, x, r, ladder, n=n)
    part, acc, fb = _device(target, ladder, x, r, n=n)
    assert acc.shape == (L, M) and part.shape == (1 + L, 4)
    far = ref.beyond_band(want)
    near = ~far
    np.testing.assert_array_equal(fb[near], 0)
    close(acc[near], want["accept"][near], **TOL_SHAPES)
    assert np.all(fb[want["first_bad"] != 0] != 0)


def test_weighted_reduction_subsample_and_repeat():
    """Random log-weights with -inf among them and one particle started at a non-finite density; max_particles < M picks
    particles (k M) / Mp; two identical calls give identical bits."""
    from smcnuts_amd import GaussianTarget
    D, M = 5, 101
    target = GaussianTarget(D)
    lp, grad = ref.gaussian(D)
    rng = np.random.default_rng(3)
    x, lw = rng.standard_normal((M, D)), 20.0 * rng.standard_normal(M)
    lw[[0, 17, 50]] = -np.inf
    x[33] = 1e200                                   # |x|^2 overflows: log density -inf
    ladder = ref.OCTAVES[4:]
    ctx = target._context(M)
    for Mp in (M, 40, 1):
        r = rng.standard_normal((min(M, Mp), D))
        want = ref.probe_reference(lp, grad, x, r, ladder, logw=lw, max_particles=Mp)
        part, acc, fb = ctx.stepsize_probe(ladder, x=x, logw=lw, r=r, max_particles=Mp, want_particles=True)
        again = ctx.stepsize_probe(ladder, x=x, logw=lw, r=r, max_particles=Mp, want_particles=True)
        for a, b in zip((part, acc, fb), again):
            np.testing.assert_array_equal(a, b)
        ex = want["excluded"]
        assert part[0, 0] == want["partials"][0, 0] and part[0, 1] == min(M, Mp) and part[0, 2] == ex.sum()
        assert np.all(acc[:, ex] == 0.0) and np.all(fb[:, ex] == 0)
        if Mp == M:
            assert ex.sum() == 4
        near = ~ref.beyond_band(want)
        close(acc[near], want["accept"][near], **TOL_SUBSAMPLE)          # (the subsample's indices: another particle, another value)
        # the reduction from the device's own per-particle values, in the reference's weights
        with np.errstate(all="ignore"):
            w = np.where(ex, 0.0, np.exp(lw[want["index"]] - part[0, 0]))
        d = (fb != 0) & ~ex
        close(part[1:, 0], (w * acc).sum(axis=1), rtol=4e-15, atol=1e-300)
        close(part[1:, 1], (w * d).sum(axis=1), rtol=2e-15, atol=1e-300)
        close(part[1:, 2], np.full(ladder.size, w.sum()), rtol=2e-15)
        np.testing.assert_array_equal(part[1:, 3], d.sum(axis=1))
    # Philox momenta: a function of (seed, particle) alone
    a = ctx.stepsize_probe(ladder, x=x, logw=lw, seed=7, want_particles=True)
    b = ctx.stepsize_probe(ladder, x=x, logw=lw, seed=7, want_particles=True)
    c = ctx.stepsize_probe(ladder, x=x, logw=lw, seed=8, want_particles=True)
    np.testing.assert_array_equal(a[1], b[1])
    assert np.any(a[1] != c[1])
    assert ctx.stepsize_last_ms() > 0.0


def test_scaling_is_exact_for_powers_of_two():
    """x = s u on N(0, s^2 I) with the ladder multiplied by s, s in {1/8, 1, 8}: the same trajectories in units of s, bit
    for bit -- positions, momenta and gradients scale exactly by powers of two, and the probe evaluates the Gaussian
    functors' energy without the normalising constant -D log s (probe_logp, smcn_stepsize.hpp), whose rounding would
    otherwise differ with s."""
    from smcnuts_amd import GaussianTarget
    D, M = 6, 40
    rng = np.random.default_rng(4)
    u, r = rng.standard_normal((M, D)), rng.standard_normal((M, D))
    out = []
    for s in (0.125, 1.0, 8.0):
        t = GaussianTarget(D, prior_sd=s)
        out.append(t._context(M).stepsize_probe(ref.OCTAVES * s, x=s * u, r=r, want_particles=True))
    assert out[0][1].min() < 0.5 and out[0][1].max() > 0.99 and np.any(out[0][2] != 0)    # the ladder crosses the limit
    for s, o in zip((1.0, 8.0), out[1:]):
        print(f"s = {s}: largest |accept - accept(s = 1/8)| = {np.abs(o[1] - out[0][1]).max():.3e}")
        np.testing.assert_array_equal(o[1], out[0][1])
        np.testing.assert_array_equal(o[2], out[0][2])
        np.testing.assert_array_equal(o[0][1:], out[0][0][1:])


def test_divergence_on_the_standard_normal():
    from smcnuts_amd import GaussianTarget
    D, M = 4, 64
    rng = np.random.default_rng(5)
    x, r = rng.standard_normal((M, D)), rng.standard_normal((M, D))
    ladder = np.array([2.0 ** -6, 0.25, 1.0, 2.0 ** 1.5])
    part, acc, fb = GaussianTarget(D)._context(M).stepsize_probe(ladder, x=x, r=r, n_leapfrog=64, want_particles=True)
    assert np.all(fb[3] > 0) and part[4, 3] == M and part[4, 1] == part[4, 2]
    assert np.all(fb[:3] == 0) and np.all(part[1:4, 3] == 0)
    assert np.all(acc[0] > 0.999)


def test_library_refuses_bad_arguments():
    from smcnuts_amd import GaussianTarget, _capi
    ctx = GaussianTarget(3)._context(4)
    x = np.zeros((4, 3))
    for kw, msg in ((dict(ladder=np.arange(1.0, 18.0)), "ladder entries"), (dict(ladder=[0.2, 0.1]), "strictly increasing"),
                    (dict(ladder=[0.1], n_leapfrog=65), "leapfrogs"), (dict(ladder=[0.1], n_leapfrog=0), "leapfrogs"),
                    (dict(ladder=[np.nan]), "strictly increasing"), (dict(ladder=[0.1], max_particles=0), "bad arguments"),
                    (dict(ladder=[0.1], delta_max=0.0), "delta_max")):
        with pytest.raises(_capi.SmcnError, match=msg):
            ctx.stepsize_probe(x=x, **kw)
    host = _capi.Context(4, _capi.MODEL_HOST, np.array([3.0]))
    with pytest.raises(_capi.SmcnError, match="host-evaluated"):
        host.stepsize_probe([0.1], x=x)
    host.close()


def test_probe_leaves_the_sampler_alone():
    """run_fused(upto=3), probe_step_size(), sample(): x_saved, logw_saved and ess of an uninterrupted run, in every bit."""
    from smcnuts_amd import ArmaModel, SMCSampler
    kw = dict(K=6, N=256, step_size=0.01, seed=11, wide_eval=False)
    one = SMCSampler(target=ArmaModel(), **kw)
    one.sample(show_progress=False)
    two = SMCSampler(target=ArmaModel(), **kw)
    two.run_fused(upto=3)
    p = two.probe_step_size()
    assert two.step_size == 0.01 and two.samples.forward_kernel.step_size == 0.01 and two.step_size_probe is None
    assert np.isfinite(p.step_size) and p.n_particles == 256
    two.sample(show_progress=False)
    np.testing.assert_array_equal(two.x_saved, one.x_saved)
    np.testing.assert_array_equal(two.logw_saved, one.logw_saved)
    np.testing.assert_array_equal(two.ess, one.ess)
    for kw2 in (dict(target_accept=1.0), dict(n_leapfrog=0), dict(ladder=[2.0, 1.0]), dict(max_particles=0)):
        with pytest.raises(ValueError):
            two.probe_step_size(**kw2)


def test_resident_equals_host_points():
    from smcnuts_amd import LogisticRegression, SMCSampler
    case = ref.CASES["logistic_d5"][0]()
    s = SMCSampler(K=3, N=512, target=case["make"](), step_size=0.05, seed=2)
    s.run_fused(upto=2)
    a = s.probe_step_size(seed=99)
    s.samples.ctx.call("smcn_synchronize")
    x, lw, _ = s.samples.ctx.get_state()
    b = case["make"]().probe_step_size(x, lw, seed=99)
    assert a.step_size == b.step_size and a.bracketed and b.bracketed
    np.testing.assert_array_equal(a.accept, b.accept)
    np.testing.assert_array_equal(a.ladder, b.ladder)
    np.testing.assert_array_equal(a.coarse.accept, b.coarse.accept)
    np.testing.assert_array_equal(a.divergent_share, b.divergent_share)
    assert (a.n_particles, a.n_excluded) == (b.n_particles, b.n_excluded) == (512, 0)


@pytest.mark.parametrize("world", [2, 8])
def test_shards_choose_the_same_step_size(world):
    from smcnuts_amd import SMCSampler
    from tests.test_sharding import _run_shards
    case = ref.CASES["logistic_d5"][0]()
    kw = dict(K=2, N=1024, step_size=0.05, seed=6)
    one = SMCSampler(target=case["make"](), **kw)
    p1 = one.probe_step_size(seed=5)
    got = {}

    def drive(s):
        got[s.comm.rank] = s.probe_step_size(seed=5)
    _run_shards(lambda c: SMCSampler(target=case["make"](), comm=c, **kw), world, drive, device=True)
    assert len(got) == world
    for p in got.values():
        assert p.step_size == got[0].step_size and p.bracketed
        np.testing.assert_array_equal(p.accept, got[0].accept)
        np.testing.assert_array_equal(p.ladder, p1.ladder)
        assert (p.n_particles, p.n_excluded) == (1024, 0)
        close(p.accept, p1.accept, **TOL_SAME)
        close(p.step_size, p1.step_size, **TOL_SAME)


def _scaled_logistic(col_scale):
    rng = np.random.default_rng(8)
    n, p = 200, 4
    Z = rng.standard_normal((n, p))
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-(Z @ np.array([1.0, -0.5, 0.5, 0.25]))))).astype(np.float64)
    X = Z.copy()
    X[:, 0] *= col_scale
    return X, y


def test_auto_end_to_end():
    """One column in other units: step_size="auto" constructs, brackets a value inside the ladder, samples, and the same
    data at unit scale gets a larger step size."""
    from smcnuts_amd import LogisticRegression, SMCSampler
    out = {}
    for scale in (100.0, 1.0):
        X, y = _scaled_logistic(scale)
        s = SMCSampler(K=5, N=1024, target=LogisticRegression(X, y), step_size="auto", seed=4)
        p = s.step_size_probe
        assert p is not None and p.bracketed and s.step_size == p.step_size == s.samples.forward_kernel.step_size
        assert np.isfinite(s.step_size) and 2.0 ** -12 < s.step_size < 8.0
        s.sample(show_progress=False)
        assert s.ess[-1] > 0.0 and np.all(np.isfinite(s.mean_estimate[-1]))
        out[scale] = s.step_size
    assert out[1.0] > out[100.0]


def test_retune_sets_the_step_size_of_the_next_launch():
    from smcnuts_amd import ArmaModel, SMCSampler
    s = SMCSampler(K=4, N=512, target=ArmaModel(), step_size=1e-4, seed=9, wide_eval=False)
    s.run_fused(upto=2)
    p = s.retune_step_size(seed=3)
    assert p is s.step_size_probe and s.samples.forward_kernel.step_size == p.step_size == s.step_size != 1e-4
    s.run_fused(upto=3)
    t = SMCSampler(K=4, N=512, target=ArmaModel(), step_size=1e-4, seed=9, wide_eval=False)
    t.run_fused(upto=3)
    s.samples.ctx.call("smcn_synchronize")
    t.samples.ctx.call("smcn_synchronize")
    xs, _, _ = s.samples.ctx.get_state()
    xt, _, _ = t.samples.ctx.get_state()
    assert np.any(xs != xt)         # generation 3 was proposed with another step size
