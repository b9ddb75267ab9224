"""The fused post pass of a pipelined arma block (smcn_set_block_post 1: block_stream_kernel + block_tail_kernel,
smcnuts_amd/csrc/smcn_block_post.hpp) against the separate launches it replaces (smcn_set_block_post 0), bit for bit.

One NUTS launch per block, then the sequence smcn_block_post -> smcn_block_stats -> smcn_block_wait -> smcn_block_commit
twice from the same context state and the same records -- fused first (so that an array it failed to write could not
pass on the reference's values), then the reference -- and every array the sequence leaves is compared: the last
transition's arrays, the generations and the scalar history rows of the block, the shard partials (lpB, gathB), what the
host reads back, and the committed state."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BLOCKS = (1, 2, 5, 20)     # 1: no compact records; 5: no multiple of the post kernel's unroll of 4


def _sampler(N, wide, history=True, seed=5, K=40):
    from smcnuts_amd import ArmaModel, SMCSampler
    s = SMCSampler(K=K, N=N, target=ArmaModel(), step_size=0.01, seed=seed, wide_eval=wide, save_history=history)
    s._fast_start()
    s._fuse_setup(max(BLOCKS))
    return s


def _buf(ctx, ptr, n):
    out = np.empty(n)
    ctx.call("smcn_buf_get", C.c_void_p(ptr), n, out.ctypes.data_as(C.POINTER(C.c_double)))
    return out


def _after_launch(s, k0, B, mode, history, probe=False):
    """post .. commit under `mode`, then everything the sequence leaves behind.  Nothing but the block's own entry points
    runs before the commit (the fused sequence then swaps the last generation in instead of copying it); probe: a getter
    in between, after which it has to copy."""
    ctx, N = s.samples.ctx, s.N
    phi = float(s.samples.phi_new)
    ctx.call("smcn_set_block_post", mode)
    ctx.call("smcn_block_post", k0, B, 1)
    ctx.call("smcn_block_stats", k0, B, 1, 0, float(N), phi, 0)
    n_ok, res = C.c_int(0), C.c_int(0)
    ctx.call("smcn_block_wait", B, C.byref(n_ok), C.byref(res))
    ess = np.empty(B)
    ctx.call("smcn_block_ess", B, ess.ctypes.data_as(C.POINTER(C.c_double)))
    if probe:
        ctx.get_state()
    ctx.call("smcn_block_commit", k0, n_ok.value)
    got = {"ess": ess, "n_ok": np.array(n_ok.value), "resample_next": np.array(res.value)}
    got["x"], got["logw"], _ = ctx.get_state()
    got["lpB"], got["gathB"] = _buf(ctx, s._fuse_lp, B * ctx.nq), _buf(ctx, s._fuse_gath, B * ctx.nq)
    got["r"], got["x_new"], got["r_new"], got["logw_new"] = ctx.get_proposal(logw_new=True)
    got.update(ctx.tree_stats())
    got["lpri0"], got["llik0"], got["lpri1"], got["llik1"] = ctx.density_parts()
    hist, xs, lw = ctx.fast_read(s.K, history)
    got["hist"] = hist[k0:k0 + B + 1].copy()
    if history:
        got["gen_x"], got["gen_logw"] = xs[k0 + 1:k0 + B + 1].copy(), lw[k0 + 1:k0 + B + 1].copy()
    # the committed state is the generation the history holds
    if history:
        np.testing.assert_array_equal(got["x"], xs[k0 + n_ok.value])
        np.testing.assert_array_equal(got["logw"], lw[k0 + n_ok.value])
    return got


def _block(s, k0, B, history=True, probe=False):
    """Generation k0 the classic way, one launch of B transitions, then both sequences; returns n_ok."""
    ctx, fk, N = s.samples.ctx, s.samples.forward_kernel, s.N
    phi = float(s.samples.phi_new)
    ctx.step_begin(k0)
    flag = C.c_int(0)
    ctx.call("smcn_fuse_decide", k0, 1, 0, float(N), phi, C.byref(flag))
    if flag.value:
        ctx.call("smcn_block_resample_local", k0)
    ctx.call("smcn_synchronize")
    x0, logw0, _ = ctx.get_state()
    ctx.call("smcn_block_launch", k0, B, float(fk.step_size), phi, fk.max_depth, fk.delta_max)
    fused = _after_launch(s, k0, B, 1, history, probe)
    ctx.set_state(x=x0, logw=logw0)        # the commit moved the state on: back to the block's start
    ref = _after_launch(s, k0, B, 0, history)
    ctx.call("smcn_set_block_post", 1)
    assert sorted(fused) == sorted(ref)
    for name in ref:
        np.testing.assert_array_equal(fused[name], ref[name], err_msg=f"{name}, N = {N}, B = {B}, k0 = {k0}")
    return int(ref["n_ok"])


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 1000, 4097])
def test_fused_post_equals_separate_launches(N, wide):
    """Ragged last blocks (63, 65, 1000, 4097), fewer particles than reduction blocks (1), more than one block; blocks
    of 1, 2, 5 and 20 transitions one after the other along one chain."""
    s = _sampler(N, wide)
    k = 0
    for B in BLOCKS:
        k += _block(s, k, B)


@pytest.mark.parametrize("N", [20000, 70000, 131073])
def test_fused_post_with_several_particles_per_thread(N):
    """Blocks of 4 and more transitions run on 64 cells per generation: 20 000 particles are 2 per thread, 70 000 are 5
    (the kernel's 8-slot instance, slots and cells ragged), and 131 073 are more than 8 -- there both settings run the
    separate launches, the counters cleared in front of them."""
    s = _sampler(N, False, K=6)
    assert _block(s, 0, 5) >= 1


def test_fused_post_without_kept_history():
    """save_history off: the generations live in the block's own buffers (the commit copies out of them)."""
    s = _sampler(1000, False, history=False)
    k = 0
    for B in BLOCKS:
        k += _block(s, k, B, history=False)


def test_fused_commit_copies_after_a_foreign_call():
    """An entry point that is not the block's own between the post pass and the commit: the commit copies the generation
    out of the history, as the separate launches' does."""
    s = _sampler(1000, False)
    k = 0
    for B in (2, 5):
        k += _block(s, k, B, probe=True)


def test_fused_post_when_a_generation_inside_the_block_resamples():
    """Few particles: the ESS falls below N / 2 inside a block of 20, so n_ok < B and the commit takes an inner
    generation."""
    for seed in range(3, 12):
        s = _sampler(256, False, seed=seed)
        if _block(s, 0, 20) < 20:
            return
    pytest.fail("no seed gave a block that resamples inside")


def test_fused_post_with_non_finite_weights():
    """A particle started at NaN, its weight NaN (so that no resampling in front of the block drops it): NaN weights in
    every generation of the block -- NaN block maxima, NaN partials, NaN history rows."""
    s = _sampler(1000, False)
    ctx = s.samples.ctx
    x, logw, _ = ctx.get_state()
    x[7] = np.nan
    logw[7] = np.nan
    ctx.set_state(x=x, logw=logw)
    _block(s, 0, 5)
    x, logw, _ = ctx.get_state()
    assert np.isnan(logw[7])
