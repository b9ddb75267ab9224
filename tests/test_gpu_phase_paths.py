"""smcn_set_phase_paths: the lane kernel passes over the tree bookkeeping no lane of a wavefront needs in an iteration (every
leaf an even one that only parks at level 0; no lane starting a tree or a doubling) in one scalar branch.  The schedule, the
draws and the arithmetic are untouched, so every case below runs twice in one process, switch on and off, from the same
seed, and must give the same bits: particles, log-weights, leapfrog and draw counts, and the scalar history.

Trees take 2^depth loop iterations when they run to a U-turn at the top, so lanes that start together stay in step; the
cases are chosen for what breaks that: trees of 2 iterations (large steps, max_depth = 0), depth caps, divergent leaves
(an odd number of iterations: the only trees that put a lane's even leaves into its wave mates' odd iterations),
non-finite start points, short series, the lane queue with its hand-overs, and the recorded tapes.

The shares asserted on tree lengths were checked on the CPU oracle (Philox mode, 6 transitions, same starts) before they
were fixed: from the posterior (arma.params) at step 0.01, 1.6 % (N = 64) and 0.75 % (N = 200) of the trees do not last a
multiple of 4 iterations, none an odd number; from N(0, I) at step 0.01 47-49 % and 1.8-2.1 % odd (without the loop's
resampling, which takes such a population to its best particles at once); at steps 0.2 / 0.5 every tree lasts 2 iterations;
with the first 20 values of the series at step 0.2, 82 % and 24 % odd."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 6            # fused transitions: the whole run is one launch
SEED = 7


def posterior_start(N, rng):
    """Particles around the posterior of the shipped series (arma.params: mean and spread of mu, beta, theta, sigma)."""
    p = np.loadtxt(os.path.join(ROOT, "smcnuts_amd", "model", "data", "arma.params"), usecols=(1, 2))
    m = np.array([p[0, 0], p[1, 0], p[2, 0], np.log(p[3, 0])])
    s = np.array([p[0, 1], p[1, 1], p[2, 1], p[3, 1] / p[3, 0]])
    return m + s * rng.normal(size=(N, 4))


def fused_run(on, N, eps, x0, wide=False, max_depth=10, y=None, grid=None, segments=0):
    """B transitions in ONE launch of the lane kernel; everything a run leaves behind."""
    from smcnuts_amd import ArmaModel, SMCSampler
    s = SMCSampler(K=B, N=N, target=ArmaModel(y=y), step_size=eps, seed=SEED, x0=x0, logq0=np.zeros(N), wide_eval=wide)
    ctx = s.samples.ctx
    ctx.call("smcn_set_phase_paths", 1 if on else 0)
    if grid is not None:
        ctx.call("smcn_set_lane_grid", grid)
        ctx.call("smcn_set_lane_segments", segments)
    s.samples.forward_kernel.max_depth = max_depth
    s._fuse_B = s._spec_hint = B          # (the driver would otherwise work up to blocks of this length: 1, 2, 4 ..)
    s.run_fused(fuse_max=B)
    s.finalise_async()
    out = dict(x=s.x_saved.copy(), logw=s.logw_saved.copy(), leapfrogs=s.leapfrogs.copy(), ess=s.ess.copy(),
               log_likelihood=s.log_likelihood.copy(), mean=s.mean_estimate.copy(), var=s.variance_estimate.copy(),
               acceptance=s.acceptance_rate.copy(), resampled=np.array(s.resampled), **ctx.tree_stats())
    ctx.close()
    return out


def tree_iterations(N, eps, x0, max_depth=10, y=None):
    """Loop iterations (leapfrogs + 1) of every tree of the same chain, run one transition per launch: the fused run is
    that chain bit for bit with wide_eval=False (test_fused_transitions_equal_one_launch_per_iteration)."""
    from smcnuts_amd import ArmaModel, SMCSampler
    s = SMCSampler(K=B, N=N, target=ArmaModel(y=y), step_size=eps, seed=SEED, x0=x0, logq0=np.zeros(N), wide_eval=False)
    s.samples.forward_kernel.max_depth = max_depth
    its = []
    for _ in range(B):
        s.step_async()
        s.samples.ctx.call("smcn_synchronize")
        its.append(s.samples.ctx.tree_stats()["nleap"].astype(np.int64) + 1)
    s.finalise_async()
    s.samples.ctx.close()
    return np.concatenate(its), s.leapfrogs.copy()


def assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")


def on_and_off(what, *args, **kw):
    a, b = fused_run(True, *args, **kw), fused_run(False, *args, **kw)
    assert_same(a, b, what)
    return a


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("N", [64, 200])
def test_in_phase_throughout(N, wide):
    """From the posterior at step 0.01 almost every tree lasts a multiple of 4 iterations (N = 200: a ragged last
    wavefront)."""
    x0 = posterior_start(N, np.random.default_rng(N))
    a = on_and_off(f"N={N} wide={wide}", N, 0.01, x0, wide=wide)
    its, leaps = tree_iterations(N, 0.01, x0)
    share = np.mean(its % 4 != 0)
    print(f"N={N}: {share * 100:.2f}% of {its.size} trees do not last a multiple of 4 iterations")
    assert share < 0.02
    if not wide:
        np.testing.assert_array_equal(a["leapfrogs"], leaps)


@pytest.mark.parametrize("eps", [0.2, 0.5])
def test_large_steps_trees_of_two_iterations(eps):
    """Divergent leaves, two-leaf U-turns, one-leapfrog trees: no lane stays in step with its wave mates."""
    N = 200
    rng = np.random.default_rng(int(eps * 10))
    for start, x0 in (("posterior", posterior_start(N, rng)), ("N(0, I)", rng.normal(size=(N, 4)))):
        a = on_and_off(f"eps={eps} from {start}", N, eps, x0)
        its, leaps = tree_iterations(N, eps, x0)
        print(f"eps={eps} from {start}: {np.mean(its % 4 != 0) * 100:.1f}% not a multiple of 4, {np.mean(its % 2 != 0) * 100:.1f}% odd")
        assert np.any(its % 4 != 0)
        np.testing.assert_array_equal(a["leapfrogs"], leaps)


@pytest.mark.parametrize("wide", [False, True])
def test_divergent_leaves_from_the_prior(wide):
    """From N(0, I) at step 0.01, far from the posterior: trees that stop early in every doubling.  (The loop resamples at
    once from such a start, so the population is not the oracle's N(0, I) one for long: 5.5 % of the trees do not last a
    multiple of 4 iterations, none an odd number.  Trees of an odd number of iterations are test_short_series'.)"""
    N = 200
    x0 = np.random.default_rng(11).normal(size=(N, 4))
    on_and_off(f"from N(0, I), wide={wide}", N, 0.01, x0, wide=wide)
    its, _ = tree_iterations(N, 0.01, x0)
    print(f"from N(0, I): {np.mean(its % 4 != 0) * 100:.1f}% not a multiple of 4, {np.mean(its % 2 != 0) * 100:.1f}% odd")
    assert np.any(its % 4 != 0)


@pytest.mark.parametrize("max_depth", [0, 1, 2, 3])
def test_depth_caps(max_depth):
    """max_depth = 0: every tree lasts 2 iterations; 1 .. 3: the cap ends trees where a merge was due.  From N(0, I),
    where trees stop early in every doubling."""
    N = 200
    x0 = np.random.default_rng(max_depth).normal(size=(N, 4))
    for wide in (False, True):
        a = on_and_off(f"max_depth={max_depth} wide={wide}", N, 0.01, x0, wide=wide, max_depth=max_depth)
    its, leaps = tree_iterations(N, 0.01, x0, max_depth=max_depth)
    print(f"max_depth={max_depth}: {np.mean(its % 4 != 0) * 100:.1f}% not a multiple of 4, {np.mean(its % 2 != 0) * 100:.1f}% odd")
    assert np.any(its % 4 != 0)
    assert its.max() <= 2 ** (max_depth + 1)      # (max_depth + 1 doublings, 2^doublings iterations)


def test_non_finite_start_points():
    """Every ninth lane starts where the density is -inf (sigma overflows): its first leaf diverges and each of its trees
    lasts 2 iterations, beside wave mates whose trees last multiples of 4.  (Its log-weight is NaN from the first update on,
    so nothing resamples: the particle stays where it is.)"""
    N = 200
    x0 = posterior_start(N, np.random.default_rng(3))
    x0[::9] = [0.0, 0.0, 0.0, 800.0]
    for wide in (False, True):
        a = on_and_off(f"non-finite starts wide={wide}", N, 0.01, x0, wide=wide)
    its, _ = tree_iterations(N, 0.01, x0)
    assert np.all(its.reshape(B, N)[:, ::9] == 2)
    np.testing.assert_array_equal(a["x"][-1][::9], x0[::9])


@pytest.mark.parametrize("T", [20, 64])
def test_short_series(T):
    """A series below the wide evaluation's shortest (T < 33) and one of 64 values; step 0.2 takes both out of phase, with
    trees of an odd number of iterations among them."""
    import json
    y = np.asarray(json.load(open(os.path.join(ROOT, "smcnuts_amd", "model", "data", "arma.json")))["y"], dtype=np.float64)[:T]
    N = 200
    x0 = posterior_start(N, np.random.default_rng(T))
    for eps in (0.01, 0.2):
        for wide in (False, True):
            on_and_off(f"T={T} eps={eps} wide={wide}", N, eps, x0, wide=wide, y=y)
    its, _ = tree_iterations(N, 0.2, x0, y=y)
    print(f"T={T} eps=0.2: {np.mean(its % 4 != 0) * 100:.1f}% not a multiple of 4, {np.mean(its % 2 != 0) * 100:.1f}% odd")
    assert np.any(its % 4 != 0)
    if T == 20:      # (CPU oracle: 24 % of these trees end on a leaf that diverges, after an odd number of iterations)
        assert np.any(its % 2 != 0)


@pytest.mark.parametrize("N", [192, 300])
def test_lane_queue(N):
    """Fewer lanes than particles (one and two wavefronts): the lanes take their wavefront's ready jobs, a block worked off
    in 2, 4 and 5 segments; in step (posterior, step 0.01) and out of it (N(0, I))."""
    rng = np.random.default_rng(N)
    for start, x0 in (("posterior", posterior_start(N, rng)), ("N(0, I)", rng.normal(size=(N, 4)))):
        ref = None
        for grid in (1, 2):
            for segments in (2, 4, 5):
                a = on_and_off(f"N={N} from {start}, {grid} wavefronts, {segments} segments", N, 0.01, x0, grid=grid, segments=segments)
                if ref is None:
                    ref = a
                assert_same(a, ref, f"N={N} from {start}: schedule ({grid}, {segments})")   # (wide_eval off: any schedule, same bits)


@pytest.mark.parametrize("grid", [0, 1])
def test_reference_tapes(golden_dir, grid):
    """The reference's recorded draws for its 128 particles, two wavefronts of a lane per particle (0) and one wavefront whose
    lanes run two particles each (1): draws consumed equal draws recorded, switch on and off, and the states are the same
    bits."""
    from smcnuts_amd import ArmaModel, _capi
    g = np.load(os.path.join(golden_dir, "arma_fwd.npz"), allow_pickle=False)
    t = ArmaModel()
    N = int(g["N"])
    assert N == 128
    got = {}
    for on in (1, 0):
        ctx = _capi.Context(N, t.model_id, t.model_data)
        ctx.call("smcn_set_phase_paths", on)
        ctx.call("smcn_set_lane_grid", grid)
        runs = []
        for k in range(int(g["K"])):
            ctx.set_state(x=g[f"x_in_{k}"], logw=np.zeros(N))
            ctx.call("smcn_set_momentum", _capi.dptr(np.ascontiguousarray(g[f"r_{k}"])))
            ctx.propose_nuts(float(g["eps"]), float(g[f"phi_prop_{k}"]), k, tape=g[f"tape_{k}"], tape_off=g[f"tape_off_{k}"])
            _, xn, rn, _ = ctx.get_proposal(r=False)
            st = ctx.tree_stats()
            assert not st["flags"].any()
            np.testing.assert_array_equal(st["ndraws"], np.diff(g[f"tape_off_{k}"]))
            runs.append((xn, rn, st["nleap"], st["depth"], st["ndraws"]))
        ctx.close()
        got[on] = runs
    for a, b in zip(got[1], got[0]):
        for u, v in zip(a, b):
            np.testing.assert_array_equal(u, v)
