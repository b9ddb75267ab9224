"""smcn_set_tree_align: in the lane kernel with a lane per particle, a lane whose tree ended starts its next one in the first
loop iteration whose number is a multiple of the alignment (1, 2, 4 or 8), sitting out the iterations in between, so that
the trees of a wavefront stay in step.  Only WHEN a tree runs changes -- Philox is keyed by the particle, the records are
taken and written in the same order --, so with wide_eval=False every alignment must give the same bits: particles,
log-weights, leapfrog and draw counts, and the scalar history.  With wide_eval=True the number of lanes at work in an
iteration decides which evaluations run wide: the runs then agree to rounding (same_run_to_rounding of test_gpu_parity).

The schedule itself is asserted too.  The model, per lane: a tree of n leapfrogs lasts n + 1 loop iterations (the iteration
that evaluates its start, then one per leaf); the first tree starts in iteration 0; a tree that starts in iteration s and
lasts L ends at e = s + L, and the next one starts at the smallest multiple of the alignment not before e; nothing waits
behind the last tree.  A wavefront leaves its loop at the bottom of the iteration in which its last lane's last tree ended,
so the count smcn_get_wave_iterations reports is the largest e of its live lanes, with no constant on top.  The tree
lengths come from the same chain run one transition per launch, which does not depend on the schedule.  The model is per
launch: the driver cuts a block where a generation has to resample and launches again from there, so each launch's counts
are read behind it and every launch whose transitions were all kept is held against the model (fused_run).

Shapes and harness follow test_gpu_phase_paths.py (fused blocks of up to B = 6 transitions, N = 64 and 200 -- a ragged last
wavefront of 8 lanes); every case also runs with smcn_set_phase_paths 0 and 1."""
import ctypes as C
import json
import os
import types

import numpy as np
import pytest

from test_gpu_parity import same_run_to_rounding
from test_gpu_phase_paths import posterior_start

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 6            # fused transitions: the whole run is one launch unless a generation resamples
SEED = 7
ALIGNS = (1, 2, 4, 8)


def fused_run(align, N, eps, x0, wide=False, max_depth=10, y=None, grid=None, paths=1, nb=B, logq0=None):
    """nb transitions in one launch of the lane kernel, unless a generation resamples: (what the run leaves behind, its
    launches -- first transition k0, length B, each wavefront's loop iterations wi, whole or not --, the sampler's own
    results as same_run_to_rounding reads them)."""
    from smcnuts_amd import ArmaModel, SMCSampler
    s = SMCSampler(K=nb, N=N, target=ArmaModel(y=y), step_size=eps, seed=SEED, x0=x0, logq0=np.zeros(N) if logq0 is None else logq0, wide_eval=wide)
    ctx = s.samples.ctx
    ctx.call("smcn_set_tree_align", align)
    ctx.call("smcn_set_phase_paths", paths)
    waves = (N + 63) // 64
    if grid is not None:
        ctx.call("smcn_set_lane_grid", grid)
        waves = min(waves, grid)
    s.samples.forward_kernel.max_depth = max_depth
    if not s._fast_started:
        s._fast_start()
    s._fuse_setup(nb)                     # (sets the block length to 1: before the next line)
    s._fuse_B = s._spec_hint = nb         # (the driver would otherwise work up to blocks of this length: 1, 2, 4 ..)
    # The driver cuts a block at a generation that has to resample and launches again from there, and it launches the next
    # block before it knows (smc_sampler._run_blocks).  Every launch's loop counts are read behind it; a launch counts for
    # the schedule ("whole") if it started from the chain's true state and all its transitions were kept.
    launches, pending, call = [], [], ctx.call

    def recording_call(name, *args):
        call(name, *args)
        if name == "smcn_block_launch":
            wi = (C.c_uint32 * waves)()
            call("smcn_get_wave_iterations", wi, waves)
            pending.append(len(launches))
            launches.append(dict(k0=int(args[0]), B=int(args[1]), wi=np.array(list(wi), dtype=np.int64), whole=False))
        elif name == "smcn_block_wait":       # (B, &n_ok, &resample_next) of the oldest launch in flight
            whole = args[1]._obj.value == args[0]
            launches[pending[0]]["whole"] = whole
            if whole and not args[2]._obj.value:
                pending.pop(0)
            else:
                pending.clear()               # (a launch behind it started from a state that was not to be)

    ctx.call = recording_call
    s.run_fused(fuse_max=nb)
    s.finalise_async()
    ctx.call = call
    out = dict(x=s.x_saved.copy(), logw=s.logw_saved.copy(), leapfrogs=s.leapfrogs.copy(), ess=s.ess.copy(),
               log_likelihood=s.log_likelihood.copy(), mean=s.mean_estimate.copy(), var=s.variance_estimate.copy(),
               acceptance=s.acceptance_rate.copy(), resampled=np.array(s.resampled), **ctx.tree_stats())
    res = types.SimpleNamespace(resampled=list(s.resampled), x_saved=s.x_saved.copy(), leapfrogs=s.leapfrogs.copy(),
                                ess=s.ess.copy(), variance_estimate=s.variance_estimate.copy(),
                                mean_estimate=s.mean_estimate.copy())
    ctx.close()
    return out, launches, res


def tree_iterations(N, eps, x0, max_depth=10, y=None, nb=B, logq0=None):
    """[nb][N] loop iterations (leapfrogs + 1) of every tree of the same chain, run one transition per launch: the fused run
    is that chain bit for bit with wide_eval=False (test_fused_transitions_equal_one_launch_per_iteration)."""
    from smcnuts_amd import ArmaModel, SMCSampler
    s = SMCSampler(K=nb, N=N, target=ArmaModel(y=y), step_size=eps, seed=SEED, x0=x0, logq0=np.zeros(N) if logq0 is None else logq0, wide_eval=False)
    s.samples.forward_kernel.max_depth = max_depth
    its = []
    for _ in range(nb):
        s.step_async()
        s.samples.ctx.call("smcn_synchronize")
        its.append(s.samples.ctx.tree_stats()["nleap"].astype(np.int64) + 1)
    s.finalise_async()
    s.samples.ctx.close()
    return np.stack(its), s.leapfrogs.copy()


def wave_iterations_model(its, align):
    """The module docstring's model for one launch: each wavefront's loop count from the launch's [B][N] tree lengths."""
    nb, N = its.shape
    end = np.zeros(N, dtype=np.int64)
    for b in range(nb):
        start = (end + align - 1) // align * align        # (b = 0: iteration 0)
        end = start + its[b]
    return np.array([end[w:w + 64].max() for w in range(0, N, 64)], dtype=np.int64)


def assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")


def every_alignment(what, N, eps, x0, nb=B, **kw):
    """wide_eval=False: all four alignments, phase paths on and off: the same bits, and every whole launch's schedule the one
    the model gives.  Returns ([nb][N] tree lengths, {alignment: [(k0, B, wave iterations) of the whole launches]})."""
    its, leaps = tree_iterations(N, eps, x0, nb=nb, **kw)
    ref, ref_plan, waves = None, None, {}
    for paths in (1, 0):
        for align in ALIGNS:
            out, launches, _ = fused_run(align, N, eps, x0, paths=paths, nb=nb, **kw)
            if ref is None:
                ref, ref_plan = out, [(l["k0"], l["B"], l["whole"]) for l in launches]
                np.testing.assert_array_equal(out["leapfrogs"], leaps, err_msg=what)
            assert_same(out, ref, f"{what}: tree_align={align} phase_paths={paths}")
            assert [(l["k0"], l["B"], l["whole"]) for l in launches] == ref_plan      # (the same bits: the same decisions)
            whole = [l for l in launches if l["whole"]]
            assert whole
            for l in whole:
                want = wave_iterations_model(its[l["k0"]:l["k0"] + l["B"]], align)
                print(f"{what}: tree_align={align} phase_paths={paths}, transitions {l['k0']}..{l['k0'] + l['B'] - 1}: "
                      f"wave iterations {l['wi'].tolist()}, model {want.tolist()}")
                np.testing.assert_array_equal(l["wi"], want, err_msg=f"{what}: schedule, tree_align={align} phase_paths={paths}")
            waves[align] = [(l["k0"], l["B"], l["wi"]) for l in whole]
    return its, waves


def test_two_transitions_wake():
    """The smallest case in which a lane has to sit out and be woken: one wavefront, two transitions in one launch.  From the
    posterior with max_depth = 1 a tree lasts 4 iterations (its start and three leaves), so alignment 8 makes every lane
    wait 4 iterations for its second tree."""
    N = 64
    x0 = posterior_start(N, np.random.default_rng(2))
    its, waves = every_alignment("two transitions", N, 0.01, x0, nb=2, max_depth=1)
    assert np.any(its[0] % 8 != 0)
    assert [(k0, nb) for k0, nb, _ in waves[8]] == [(0, 2)]       # (nothing resampled: the launch is the whole run)
    assert np.any(waves[8][0][2] != waves[1][0][2])


@pytest.mark.parametrize("N", [64, 200])
def test_posterior_start(N):
    """From the posterior at step 0.01 few trees stop early (0.75-1.6 % do not last a multiple of 4 iterations); N = 200 has
    a ragged last wavefront."""
    x0 = posterior_start(N, np.random.default_rng(N))
    every_alignment(f"posterior N={N}", N, 0.01, x0)


def test_from_the_prior_in_the_loop():
    """From N(0, I) at step 0.01 inside the SMC loop: it resamples at once to the start's best particles and again a few
    generations on, so the launches are short (1, 1, 2 .. transitions) and 3-6 % of the trees are out of step."""
    N = 200
    x0 = np.random.default_rng(11).normal(size=(N, 4))
    its, waves = every_alignment("from N(0, I)", N, 0.01, x0)
    assert np.any(its % 4 != 0)


def direct_launches(align, N, eps, x0, lengths, paths=1):
    """The kernel without the SMC loop around it: launches of `lengths` transitions one behind the other from x0 as it is
    (smcn_block_launch / _post / _commit and nothing else: no generation resamples).  Per launch: each wavefront's loop
    iterations, and the tree statistics of its last transition."""
    from smcnuts_amd import ArmaModel, SMCSampler
    s = SMCSampler(K=sum(lengths), N=N, target=ArmaModel(), step_size=eps, seed=SEED, x0=x0, logq0=np.zeros(N), wide_eval=False)
    ctx, fk = s.samples.ctx, s.samples.forward_kernel
    ctx.call("smcn_set_tree_align", align)
    ctx.call("smcn_set_phase_paths", paths)
    s._fast_start()
    s._fuse_setup(max(lengths))
    waves, k, out = (N + 63) // 64, 0, []
    for nb in lengths:
        ctx.call("smcn_block_launch", k, nb, float(eps), 1.0, fk.max_depth, fk.delta_max)
        wi = (C.c_uint32 * waves)()
        ctx.call("smcn_get_wave_iterations", wi, waves)
        ctx.call("smcn_block_post", k, nb, 1)
        out.append((np.array(list(wi), dtype=np.int64), ctx.tree_stats()))
        ctx.call("smcn_block_commit", k, nb)
        k += nb
    ctx.call("smcn_synchronize")
    ctx.close()
    return out


def test_prior_population_the_switch_is_live():
    """An N(0, I) population as it is, far from the posterior at step 0.01 (47-49 % of its trees do not last a multiple of 4
    iterations on the CPU oracle): B transitions in one launch against the same chain one transition per launch.  Lanes
    wait in every wavefront, and the loop counts of alignment 4 are not those of alignment 1."""
    N = 200
    x0 = np.random.default_rng(11).normal(size=(N, 4))
    ref = direct_launches(1, N, 0.01, x0, [1] * B)
    its = np.stack([st["nleap"].astype(np.int64) + 1 for _, st in ref])
    for b, (wi, _) in enumerate(ref):             # (one transition per launch: nothing can wait)
        np.testing.assert_array_equal(wi, wave_iterations_model(its[b:b + 1], 1))
    print(f"N(0, I) as it is: {np.mean(its % 4 != 0) * 100:.1f}% of the trees do not last a multiple of 4 iterations, "
          f"{np.mean(its % 2 != 0) * 100:.1f}% an odd number")
    assert np.any(its % 4 != 0)
    got = {}
    for paths in (1, 0):
        for align in ALIGNS:
            (wi, st), = direct_launches(align, N, 0.01, x0, [B], paths=paths)
            want = wave_iterations_model(its, align)
            print(f"N(0, I) as it is: tree_align={align} phase_paths={paths}: wave iterations {wi.tolist()}, model {want.tolist()}")
            np.testing.assert_array_equal(wi, want, err_msg=f"schedule, tree_align={align} phase_paths={paths}")
            for key in st:                        # (the last transition's trees: the same bits as the chain's)
                np.testing.assert_array_equal(st[key], ref[-1][1][key], err_msg=f"{key}, tree_align={align} phase_paths={paths}")
            got[align] = wi
    assert np.any(got[4] != got[1])


@pytest.mark.parametrize("eps", [0.2, 0.5])
def test_trees_of_two_iterations_every_end_waits(eps):
    """max_depth = 0: every tree lasts 2 iterations, so with alignments 4 and 8 every tree end waits."""
    N = 200
    x0 = np.random.default_rng(int(eps * 10)).normal(size=(N, 4))
    its, waves = every_alignment(f"eps={eps} max_depth=0", N, eps, x0, max_depth=0)
    assert np.all(its == 2)
    for align in ALIGNS:
        assert any(nb > 1 for _, nb, _ in waves[align])
        for _, nb, wi in waves[align]:      # (a launch of nb transitions: nb - 1 periods of max(align, 2), then the last tree)
            np.testing.assert_array_equal(wi, max(align, 2) * (nb - 1) + 2)


def test_short_series_odd_tree_lengths():
    """The first 20 values of the series at step 0.2: 24 % of the trees end on a leaf that diverges, after an odd number of
    iterations: waits of 1 and 3 iterations."""
    y = np.asarray(json.load(open(os.path.join(ROOT, "smcnuts_amd", "model", "data", "arma.json")))["y"], dtype=np.float64)[:20]
    N = 200
    x0 = posterior_start(N, np.random.default_rng(20))
    its, _ = every_alignment("T=20 eps=0.2", N, 0.2, x0, y=y)
    assert np.any(its % 2 != 0)


def test_non_finite_start_row():
    """Every ninth lane starts where the density is -inf: each of its trees lasts 2 iterations, beside wave mates whose trees
    last multiples of 4."""
    N = 200
    x0 = posterior_start(N, np.random.default_rng(3))
    x0[::9] = [0.0, 0.0, 0.0, 800.0]
    its, _ = every_alignment("non-finite starts", N, 0.01, x0)
    assert np.all(its[:, ::9] == 2)


@pytest.mark.parametrize("start", ["posterior", "prior"])
def test_wide_eval_to_rounding(start):
    """wide_eval=True: how many lanes are at work in an iteration decides which evaluations run wide, and waiting lanes are
    not at work: every alignment against alignment 1, to rounding."""
    N = 200
    rng = np.random.default_rng(5)
    x0 = posterior_start(N, rng) if start == "posterior" else rng.normal(size=(N, 4))
    for paths in (1, 0):
        _, _, ref = fused_run(1, N, 0.01, x0, wide=True, paths=paths)
        for align in ALIGNS[1:]:
            _, _, got = fused_run(align, N, 0.01, x0, wide=True, paths=paths)
            same_run_to_rounding(got, ref, f"wide, from the {start}: tree_align={align} phase_paths={paths}")


def test_reference_tapes(golden_dir):
    """The tape instantiation: the reference's recorded draws for its 128 particles, a lane per particle, alignment 4: draws
    consumed equal draws recorded, and the states are the bits alignment 1 gives."""
    from smcnuts_amd import ArmaModel, _capi
    g = np.load(os.path.join(golden_dir, "arma_fwd.npz"), allow_pickle=False)
    t = ArmaModel()
    N = int(g["N"])
    assert N == 128
    got = {}
    for align in (4, 1):
        ctx = _capi.Context(N, t.model_id, t.model_data)
        ctx.call("smcn_set_tree_align", align)
        runs = []
        for k in range(int(g["K"])):
            ctx.set_state(x=g[f"x_in_{k}"], logw=np.zeros(N))
            ctx.call("smcn_set_momentum", _capi.dptr(np.ascontiguousarray(g[f"r_{k}"])))
            ctx.propose_nuts(float(g["eps"]), float(g[f"phi_prop_{k}"]), k, tape=g[f"tape_{k}"], tape_off=g[f"tape_off_{k}"])
            _, xn, rn, _ = ctx.get_proposal(r=False)
            st = ctx.tree_stats()
            assert not st["flags"].any()
            np.testing.assert_array_equal(st["ndraws"], np.diff(g[f"tape_off_{k}"]))
            wi = (C.c_uint32 * 2)()
            ctx.call("smcn_get_wave_iterations", wi, 2)
            np.testing.assert_array_equal(np.array(list(wi)), (st["nleap"].astype(np.int64) + 1).reshape(2, 64).max(axis=1))
            runs.append((xn, rn, st["nleap"], st["depth"], st["ndraws"]))
        ctx.close()
        got[align] = runs
    for a, b in zip(got[4], got[1]):
        for u, v in zip(a, b):
            np.testing.assert_array_equal(u, v)


@pytest.mark.parametrize("start", ["posterior", "prior"])
def test_lane_queue_is_untouched(start):
    """Fewer lanes than particles (smcn_set_lane_grid): the queue has its own rule (seg_align) and the setter does not reach
    it: alignments 1 and 4 give the same bits and the same loop counts."""
    N = 192
    rng = np.random.default_rng(N)
    x0 = posterior_start(N, rng) if start == "posterior" else rng.normal(size=(N, 4))
    a, la, _ = fused_run(1, N, 0.01, x0, grid=1)
    b, lb, _ = fused_run(4, N, 0.01, x0, grid=1)
    assert_same(a, b, f"lane queue from the {start}")
    assert [(l["k0"], l["B"], l["whole"], l["wi"].tolist()) for l in la] == [(l["k0"], l["B"], l["whole"], l["wi"].tolist()) for l in lb]
    c, _, _ = fused_run(4, N, 0.01, x0)          # (a lane per particle: the same chain, wide_eval off)
    assert_same(a, c, f"lane queue against a lane per particle, from the {start}")


@pytest.mark.parametrize("n", [0, 3, 16, -1])
def test_setter_refuses(n):
    from smcnuts_amd import ArmaModel, _capi
    from smcnuts_amd._capi import SmcnError
    t = ArmaModel()
    ctx = _capi.Context(64, t.model_id, t.model_data)
    try:
        with pytest.raises(SmcnError, match="smcn_set_tree_align"):
            ctx.call("smcn_set_tree_align", n)
        ctx.call("smcn_set_tree_align", 2)       # (and takes what it should)
    finally:
        ctx.close()
