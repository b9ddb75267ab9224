"""The population reductions and the resampling against EXACT references (tests/_exact.py), past 262 144 particles
and at the weights where log-sum-exp kernels go wrong.

Sizes: beyond 262 144 elements the block reductions clamp at kMaxPart = 1024 blocks and every grid-stride loop takes
more than one trip per thread; beyond 256 tiles of 1024 (N > 262 144) the resampling takes its tile offsets from
scan_offsets_kernel / scan_offsets_if_kernel in global memory and cdf_search its plain element bisection.  The
generation statistics of the device-resident loop (gen_partials_kernel) keep a particle's weight in registers up to
N = 4 * blocks * 256, re-read it from work[] for D > 8 with one coordinate group, and recompute it otherwise.

Tolerances are not tuned: each one is the worst-case bound of the summation it checks.  A sum of positive terms
taken as t sequential adds per thread, an 8-level block tree, then ceil(blocks / 256) sequential adds and another
8-level tree has relative error at most (that chain length + 2) eps; forming a term exp(a - max) adds eps |a - max|.
"""
import math

import numpy as np
import pytest

import _exact as ex
from _tol import close
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

EPS = ex.EPS
SUB = float(np.finfo(np.float64).smallest_subnormal)   # absolute rounding of a result in the subnormal range
TILE = 1024
RED_BLOCK, MAX_PART = 256, 1024


def red_grid(n):
    return max(1, min(MAX_PART, -(-n // RED_BLOCK)))


def weight_sets(N, rng):
    """The weights of every test here: benign, underflowing, offset, tied, single, -inf tiles, late maximum, none."""
    base = 3.0 * rng.standard_normal(N)
    ties = base.copy()
    ties[rng.choice(N, max(1, N // 10), replace=False)] = float(base.max()) + 1.0
    single = np.full(N, -np.inf)
    single[rng.integers(N)] = 5.0 * rng.standard_normal()
    tiles = base.copy()
    for t0 in range(1, -(-N // TILE), 3):
        tiles[t0 * TILE:(t0 + 1) * TILE] = -np.inf       # whole tiles (and whole 256-blocks) of -inf
    tiles[0] = tiles[-1] = -np.inf
    late = base - 10.0
    late[-1] = 20.0                                       # the maximum only in the last, partial block
    return {
        "gauss3": base,
        "uniform_2000": rng.uniform(-2000.0, 0.0, N),
        "offset_1e6": -1e6 + rng.standard_normal(N),
        "ties_10pc": ties,
        "single_finite": single,
        "inf_tiles": tiles,
        "max_last": late,
        "all_inf": np.full(N, -np.inf),
    }


def lse_bound(logw, wn_x, depth, exp_terms=1):
    """Relative error of sum exp(a - max) (chain `depth`, each term's exponent rounded `exp_terms` times: eps |a - max|
    each, weighted by the term) and the absolute error of log-sum-exp (+ the roundings of log1p, log and the adds)."""
    fin = np.isfinite(logw)
    m = float(logw[fin].max())
    spread = float(np.sum(wn_x[fin] * np.abs(logw[fin] - m)))
    s_rel = (depth + 2 + 2 * exp_terms) * EPS + exp_terms * EPS * spread
    n = int(fin.sum())
    ll_abs = s_rel + 2 * EPS * (math.log(n) + 1.0)
    return s_rel, ll_abs


def step_normalise(ctx):
    from smcnuts_amd import _capi
    ll, ess = np.empty(1), np.empty(1)
    ctx.call("smcn_normalise", _capi.dptr(ll), _capi.dptr(ess))
    return float(ll[0]), float(ess[0])


# ---- B. smcn_normalise / smcn_moment_sums (step path) -----------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 255, 256, 257, 1025, 262143, 262144, 262145, 1048579])
def test_normalise_and_moments_against_exact(N):
    """log-likelihood, wn and ESS of smcn_normalise and the weighted moments of smcn_moment_sums against exact
    references, on every weight set; wn exactly 0 at -inf; invariant under a constant shift of the weights.  The
    moments at x = 1e4 + 1e-2 z: around the exact mean (two-pass accuracy) and around a point 1e3 away, where the
    derived variance S - (mean - s)^2 can only be trusted to r (V + d^2) + 2 |d| |mean| r_mean -- the cost of the
    shifted form, asserted as that bound."""
    from smcnuts_amd import GaussianTarget, _capi
    D, C0 = 4, 700.25
    t = GaussianTarget(D)
    ctx = _capi.Context(N, t.model_id, t.model_data)
    rng = np.random.default_rng(1000 + N)
    x = 1e4 + np.arange(D) + 1e-2 * rng.standard_normal((N, D))
    depth = ex.sum_depth(N, red_grid(N))
    try:
        for name, logw in weight_sets(N, rng).items():
            msg = f"N={N} weights={name}"
            fin = np.isfinite(logw)
            ctx.set_state(x=x, logw=logw)
            ll, ess = step_normalise(ctx)
            wn = ctx.get_state(x=False, logw=False, wn=True)[2]
            assert np.all(wn[~fin] == 0.0), msg
            if not fin.any():                       # oracle.normalise_weights: loglik -inf, wn = 0
                assert ll == -np.inf and np.all(wn == 0.0), msg
                continue
            ll_x, ess_x, wn_x = ex.lse_exact(logw), ex.ess_exact(logw), ex.wn_exact(logw)
            s_rel, ll_abs = lse_bound(logw, wn_x, depth)
            close(ll, ll_x, rtol=2 * EPS, atol=ll_abs, err_msg=msg, what="smcn_normalise loglik vs exact")
            ll_err = ll_abs + 2 * EPS * abs(ll_x)                         # |ll - ll_exact| at most
            wn_rtol = ll_err + EPS * float(np.max(np.abs(logw[fin] - ll_x))) + 2 * EPS
            close(wn, wn_x, rtol=wn_rtol, atol=2 * SUB, err_msg=msg, what="smcn_normalise wn vs exact")
            m = float(logw[fin].max())
            ess_rtol = 2 * s_rel + 2 * (ll_err + EPS * abs(m - ll_x)) + 4 * EPS
            close(ess, ess_x, rtol=ess_rtol, err_msg=msg, what="smcn_normalise ESS vs exact")

            # a constant shift of the weights: the same result, up to the rounding of logw + C0
            ctx.set_state(logw=logw + C0)
            ll2, ess2 = step_normalise(ctx)
            wn2 = ctx.get_state(x=False, logw=False, wn=True)[2]
            assert np.all(wn2[~fin] == 0.0), msg
            r_in = EPS * (float(np.max(np.abs(logw[fin]))) + C0)
            close(ll2 - C0, ll, rtol=2 * EPS, atol=2 * ll_abs + r_in + EPS * abs(ll2), err_msg=msg,
                  what="loglik under a constant shift")
            close(wn2, wn, rtol=2 * wn_rtol + 2 * r_in, atol=2 * SUB, err_msg=msg, what="wn under a constant shift")
            close(ess2, ess, rtol=2 * ess_rtol + 4 * r_in, err_msg=msg, what="ESS under a constant shift")

            # weighted moments of the (normalised) particles, on the wn of the unshifted weights
            ctx.set_state(x=x, logw=logw)
            step_normalise(ctx)
            mean_x, var_x = ex.moments_exact(logw, x)
            mean_rtol = wn_rtol + (depth + 3) * EPS
            mean = ctx.moment_sums()
            close(mean, mean_x, rtol=mean_rtol, err_msg=msg, what="smcn_moment_sums mean vs exact")
            s_rtol = wn_rtol + (depth + 5) * EPS
            # around the exact mean rounded to float64 (two-pass accuracy); that rounding, at most half a spacing of the
            # mean, adds its square
            half = np.spacing(np.abs(mean_x)) / 2
            var = ctx.moment_sums(mean_x)
            close(var, var_x, rtol=s_rtol, atol=float(np.max(half)) ** 2 * (1 + s_rtol), err_msg=msg,
                  what="smcn_moment_sums variance around the mean")
            far = mean_x + 1e3
            S = ctx.moment_sums(far)
            d = mean_x - far
            close(S, var_x + d * d, rtol=s_rtol + 2 * EPS + float(np.max(2 * half / np.abs(d))), err_msg=msg,
                  what="smcn_moment_sums around a far shift")
            derived = S - (mean - far) ** 2
            cost = s_rtol * (var_x + d * d) + 2 * np.abs(d) * np.abs(mean_x) * mean_rtol + 4 * EPS * d * d
            close(derived, var_x, rtol=0.0, atol=float(np.max(cost)), err_msg=msg,
                  what="variance derived from a shift 1e3 away (bound of the shifted form)")
    finally:
        ctx.close()


# ---- C. device-resident generation statistics ---------------------------------------------------------------------
def gen_grid(N, D):
    """enqueue_partials' block count for one generation.  (Its halving loop, which keeps blocks x (4 + 3 D) block
    partials x generations within the partials buffer of kMaxPart x (4 D^2 + 2 D + 8), never acts on one generation.)"""
    g = red_grid(N)
    return min(g, 128) if D >= 64 else g


def device_generation(ctx, N):
    """The first generation of the device-resident loop: its shard partials (the shift is 0 at generation 0) and
    history row 0 [LL, ESS, resampled, leaps, moved, phi, mean.., var..]."""
    ctx.fast_begin(1, False)
    ctx.step_begin(0)
    p = ctx.partials_get()
    ctx.step_finish(0, 1, 0, float(N), 0.0, 1.0, last=True)
    hist = ctx.fast_read(1, False)[0]
    D = (p.size - 4) // 2
    return p, np.zeros(D), hist[0]


@pytest.mark.parametrize("D,N", [(4, 1048576), (4, 1048577), (13, 1048576), (13, 1048577),
                                 (70, 131072), (70, 131073), (256, 131072), (256, 131073)])
def test_generation_statistics_against_exact(D, N):
    """gen_partials_kernel + gen_reduce_blocks_kernel + combine_ranks_body (per-block maxima, combined like shards)
    against the exact log-likelihood, ESS, mean and variance, and against smcn_normalise on the same state.  The
    shapes straddle the kernel's branches: weights in registers up to N = 4 * blocks * 256 (1 048 576 at 1024 blocks;
    131 072 at 128 blocks x 8 coordinate groups for D >= 64), re-read from work[] at D = 13, recomputed at D = 4.
    x = 1e4 + 1e-2 z (mean / sd = 1e6): the variance of generation 0 needs the two-pass accuracy."""
    from smcnuts_amd import GaussianTarget, _capi, parallel
    t = GaussianTarget(D)
    ctx = _capi.Context(N, t.model_id, t.model_data)
    rng = np.random.default_rng(2000 + N + D)
    x = 1e4 + 1e-2 * rng.standard_normal((N, D))
    nb = gen_grid(N, D)
    depth = ex.sum_depth(N, nb)
    step_depth = ex.sum_depth(N, red_grid(N))
    try:
        for name, logw in weight_sets(N, rng).items():
            msg = f"D={D} N={N} weights={name}"
            fin = np.isfinite(logw)
            ctx.set_state(x=x, logw=logw)
            p, shift, h = device_generation(ctx, N)
            wn = ctx.get_state(x=False, logw=False, wn=True)[2]
            assert np.all(wn[~fin] == 0.0), msg
            if not fin.any():
                assert h[0] == -np.inf and p[0] == -np.inf and np.all(wn == 0.0), msg
                continue
            ll_h, sum_wn2 = parallel.combine_lse_partials(p[:4])
            W = p[1] + p[2]
            mean_h = shift + p[4:4 + D] / W           # combine_ranks_body, one shard: A around the shift,
            var_h = p[4 + D:] / W                     # B around the shard's own mean
            ll_x, ess_x = ex.lse_exact(logw), ex.ess_exact(logw)
            wn_x = ex.wn_exact(logw)
            mean_x, var_x = ex.moments_exact(logw, x)
            # a block's terms exp(a - max_b), scaled by exp(max_b - max): two rounded exponents per term
            s_rel, ll_abs = lse_bound(logw, wn_x, depth, exp_terms=3)
            m = float(logw[fin].max())
            ll_err = ll_abs + 2 * EPS * abs(ll_x)
            ess_rtol = 2 * s_rel + 2 * (ll_err + EPS * abs(m - ll_x)) + 4 * EPS
            mean_rtol = 2 * s_rel + 2 * EPS
            var_rtol = 2 * s_rel + 6 * EPS + 4 * float(np.max((mean_rtol * mean_x) ** 2 / np.maximum(var_x, 1e-300)))
            for got, what in ((h, "history row"), (None, "host combine of the partials")):
                g_ll, g_ess, g_mean, g_var = ((got[0], got[1], got[6:6 + D], got[6 + D:6 + 2 * D]) if got is not None
                                              else (ll_h, 1.0 / sum_wn2, mean_h, var_h))
                close(g_ll, ll_x, rtol=2 * EPS, atol=ll_abs, err_msg=f"{msg} {what}", what="generation loglik vs exact")
                close(g_ess, ess_x, rtol=ess_rtol, err_msg=f"{msg} {what}", what="generation ESS vs exact")
                close(g_mean, mean_x, rtol=mean_rtol, err_msg=f"{msg} {what}", what="generation mean vs exact")
                close(g_var, var_x, rtol=var_rtol, atol=0.0, err_msg=f"{msg} {what}",
                      what="generation-0 variance vs exact (two-pass accuracy)")
            # the wn the loop wrote (exp(logw - LL)) and the step path on the same state, to rounding
            wn_rtol = ll_err + EPS * float(np.max(np.abs(logw[fin] - ll_x))) + 2 * EPS
            close(wn, wn_x, rtol=wn_rtol, atol=2 * SUB, err_msg=msg, what="generation wn vs exact")
            ll_s, ess_s = step_normalise(ctx)
            _, ll_abs_s = lse_bound(logw, wn_x, step_depth)
            close(h[0], ll_s, rtol=4 * EPS, atol=ll_abs + ll_abs_s, err_msg=msg, what="generation loglik vs step path")
            close(h[1], ess_s, rtol=2 * ess_rtol, err_msg=msg, what="generation ESS vs step path")
            # (the step path's mean is sum wn c(x), not divided by sum wn: off by its wn error times |mean|, and its
            #  variance, taken around that mean, by the square of that)
            mean_s = ctx.moment_sums()
            var_s = ctx.moment_sums(mean_s)
            mean_rtol_s = wn_rtol + (step_depth + 3) * EPS
            close(h[6:6 + D], mean_s, rtol=mean_rtol + mean_rtol_s, err_msg=msg, what="generation mean vs step path")
            off_s = float(np.max((mean_rtol_s * mean_x) ** 2 / np.maximum(var_x, 1e-300)))
            close(h[6 + D:6 + 2 * D], var_s, rtol=var_rtol + wn_rtol + (step_depth + 5) * EPS + 2 * off_s, err_msg=msg,
                  what="generation variance vs step path")
    finally:
        ctx.close()


def test_generation_variance_after_the_mean_moved_far():
    """The shift of a later generation's moment sums is the previous generation's mean.  Here the population jumps
    by 1e4 between two generations at sd 1e-2: the second moments are still taken around points of the population
    (each block's reference particle, then the shard mean), so generation 1 keeps the two-pass accuracy of
    generation 0.  (Around the shift, B / W - (mean - shift)^2 lost eps (1e4 / 1e-2)^2 -- 1e-4 relative.)"""
    from smcnuts_amd import GaussianTarget, _capi
    N, D = 262145, 4
    t = GaussianTarget(D)
    ctx = _capi.Context(N, t.model_id, t.model_data)
    rng = np.random.default_rng(7)
    z = 1e-2 * rng.standard_normal((N, D))
    logw = 3.0 * rng.standard_normal(N)
    depth = ex.sum_depth(N, gen_grid(N, D))
    try:
        ctx.set_state(x=z, logw=logw)
        ctx.fast_begin(1, False)
        ctx.step_begin(0)
        ctx.step_finish(0, 1, 0, float(N), 0.0, 1.0, last=True)
        x1 = 1e4 + z
        ctx.set_state(x=x1, logw=logw)
        ctx.step_begin(1)
        ctx.step_finish(1, 1, 0, float(N), 0.0, 1.0, last=True)
        hist = ctx.fast_read(1, False)[0]
        wn_x = ex.wn_exact(logw)
        s_rel, _ = lse_bound(logw, wn_x, depth, exp_terms=3)
        mean0, var0 = ex.moments_exact(logw, z)
        mean1, var1 = ex.moments_exact(logw, x1)
        mean_rtol = 2 * s_rel + 2 * EPS
        for k, (mk, vk) in enumerate(((mean0, var0), (mean1, var1))):
            var_rtol = 2 * s_rel + 6 * EPS + 4 * float(np.max((mean_rtol * mk) ** 2 / vk))
            xk = z if k == 0 else x1                 # (terms of both signs at generation 0: bound on sum wn |x|)
            close(hist[k, 6:6 + D], mk, rtol=mean_rtol, atol=mean_rtol * float(np.max(wn_x @ np.abs(xk))),
                  what="mean before and after a jump of 1e4")
            close(hist[k, 6 + D:6 + 2 * D], vk, rtol=var_rtol, what="variance before and after a jump of 1e4 (two-pass)")
    finally:
        ctx.close()


# ---- D. resampling beyond 256 tiles ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,D", [(262144, 4), (262145, 4), (300001, 4), (1048579, 4), (300001, 16), (300001, 70)])
def test_resampling_beyond_256_tiles(N, D):
    """smcn_resample_multinomial (multinomial and systematic, recorded uniforms and Philox) at the last fused size,
    the first unfused one and beyond: ancestors exactly the blocked-scan right-search, every particle its ancestor's
    row, no ancestor of zero weight (runs of -inf across a tile boundary, across the fused-tile limit and at the end),
    a key of 1 - 2^-53 clamped, systematic counts within 1 of N wn."""
    from smcnuts_amd import GaussianTarget, _capi
    seed, it = 4242, 5
    t = GaussianTarget(D)
    ctx = _capi.Context(N, t.model_id, t.model_data)
    ctx.set_seed(seed)
    rng = np.random.default_rng(3000 + N + D)
    x = rng.standard_normal((N, D))
    logw = 3.0 * rng.standard_normal(N)
    logw[5 * TILE - 300:7 * TILE + 300] = -np.inf            # across two tile boundaries
    logw[256 * TILE - 100:256 * TILE + 100] = -np.inf        # across the last fused tile (where N reaches it)
    logw[-2000:] = -np.inf                                   # the end
    u = rng.random(N)
    u[7] = 1.0 - 2.0 ** -53
    u[8] = 0.0
    philox = orc.philox_particle_uniforms(seed, it, 0, N, 2, 0)   # stream 2 = resampling, draw 0 of every slot
    try:
        for scheme in (0, 1):
            ctx.call("smcn_set_resample_scheme", scheme)
            for tape in (u, None):
                msg = f"N={N} D={D} scheme={scheme} {'recorded' if tape is not None else 'philox'}"
                ctx.set_state(x=x, logw=logw)
                ll, _ = step_normalise(ctx)
                wn = ctx.get_state(x=False, logw=False, wn=True)[2]
                idx = ctx.resample(ll, np.log(N), it, u=tape, want_idx=True)
                draws = tape if tape is not None else philox
                keys = draws if scheme == 0 else (np.arange(N, dtype=np.float64) + draws[0]) / N
                np.testing.assert_array_equal(idx, ex.indices_exact(wn, keys, orc.blocked_cumsum), err_msg=msg)
                src = np.minimum(idx, N - 1)
                assert np.all(wn[src] > 0.0), msg
                xr, lw, _ = ctx.get_state()
                np.testing.assert_array_equal(xr, x[src], err_msg=msg)
                close(lw, ll - np.log(N), rtol=1e-15, err_msg=msg)
                if scheme == 1:
                    assert np.all(np.diff(idx) >= 0), msg
                    counts = np.bincount(src, minlength=N)
                    assert np.all(np.abs(counts - N * wn) < 1.0 + 1e-6), msg
    finally:
        ctx.call("smcn_set_resample_scheme", 0)
        ctx.close()


def test_device_resident_equals_stepwise_beyond_256_tiles():
    """test_device_resident_equals_stepwise_philox at N > 262 144: the device-resident resampling
    (enqueue_resample_if: scan_offsets_if_kernel) and the stepwise one (scan_offsets_kernel) pick the same ancestors."""
    from smcnuts_amd import ArmaModel, SMCSampler
    N, K = 262145 + 40000, 8
    a = SMCSampler(K=K, N=N, target=ArmaModel(), step_size=0.01, seed=3, wide_eval=False)
    a.sample(show_progress=False)
    b = SMCSampler(K=K, N=N, target=ArmaModel(), step_size=0.01, seed=3, wide_eval=False)
    for _ in range(K):
        b.step()
    b.finalise()
    assert a.resampled == b.resampled and any(a.resampled)
    np.testing.assert_array_equal(a.x_saved, b.x_saved)
    np.testing.assert_array_equal(a.leapfrogs, b.leapfrogs)
    close(a.logw_saved, b.logw_saved, rtol=1e-14, atol=1e-15)
    close(a.ess, b.ess, rtol=1e-13)
    close(a.mean_estimate, b.mean_estimate, rtol=1e-13, atol=1e-15)
    close(a.variance_estimate, b.variance_estimate, rtol=5e-9, atol=5e-15)
    close(a.acceptance_rate, b.acceptance_rate)


def test_sampler_variance_at_mean_over_sd_1e6():
    """SMCSampler.sample() itself (device-resident loop) on a posterior at 1e4 with sd 1e-2, started there: the mean
    and variance estimate of every generation against the exact moments of that generation's saved particles and
    weights, with the two-pass bound of test_generation_statistics_against_exact."""
    from smcnuts_amd import GaussianTarget, SMCSampler
    N, D, K = 262145, 4, 3
    rng = np.random.default_rng(8)
    x0 = 1e4 + 1e-2 * rng.standard_normal((N, D))
    target = GaussianTarget(D, prior_sd=1e5, lik_mean=1e4, lik_sd=1e-2)
    smc = SMCSampler(K=K, N=N, target=target, step_size=1e-3, seed=9, x0=x0, logq0=np.zeros(N))
    smc.sample(show_progress=False)
    assert smc.device_resident
    depth = ex.sum_depth(N, gen_grid(N, D))
    for k in range(K + 1):
        logw, xk = smc.logw_saved[k], smc.x_saved[k]
        mean_x, var_x = ex.moments_exact(logw, xk)
        s_rel, _ = lse_bound(logw, ex.wn_exact(logw), depth, exp_terms=3)
        mean_rtol = 2 * s_rel + 2 * EPS
        var_rtol = 2 * s_rel + 6 * EPS + 4 * float(np.max((mean_rtol * mean_x) ** 2 / var_x))
        close(smc.mean_estimate[k], mean_x, rtol=mean_rtol, err_msg=f"k={k}", what="sampler mean at mean/sd 1e6")
        close(smc.variance_estimate[k], var_x, rtol=var_rtol, err_msg=f"k={k}", what="sampler variance at mean/sd 1e6")
