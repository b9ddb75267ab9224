"""The Gaussian-approximation L-kernel on the device against the 50-digit reference of tests/_glk.py: the moment sums
(glk_sums_kernel + sum_final_kernel), the conditional log-density (glk_logpdf_kernel), the whole one-shard call
(smcn_gauss_lkernel_device: both passes, glk_mean_kernel, glk_algebra_kernel's two Cholesky factorisations, its condition
estimates and its decision) and the staged form over shards (smcn_gauss_lkernel_stage with glk_combine_kernel).

TOLERANCE OF AN L VALUE.  Errors are relative to scale_i = |c0| + maha_i / 2 of the reference.  Per population,
yard = max(err(host_L), err(chol_L), 16 u): what the reference's own float64 calls and a plain NumPy Cholesky route lose
against the 50-digit value on the same inputs -- cond x u, the cancellation of the Schur complement where fewer than
2 D + 1 distinct particles leave it to the ridge, |mean| / sd x u far from the origin.  The device -- one more float64
formulation, with fused multiply-adds and its own summation order -- must stay within MARGIN = 8 yard: two float64
formulations differ from each other by up to 4x either way on these populations, 8 is twice that.  The yardstick is
never the kernel.  Observed share of the tolerance (the `used` that tests/_tol.py records per call site): DESIGN.md section 2.

THE DECISION.  From the exact condition numbers a population is one the device must accept, must refuse, or may do either
with (_glk.decision; the classes are asserted on the CPU in test_glk_host.py).  No particle is masked or dropped anywhere.
"""
import ctypes as C
import math
import types

import numpy as np
import pytest

import _glk as G
from _tol import close

pytestmark = pytest.mark.gpu

U = G.U64
NAMES = list(G.CASES)
NOT_SET = "call smcn_gauss_lkernel_logpdf first"


def _capi():
    from smcnuts_amd import _capi
    return _capi


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _loaded(r, x):
    ctx = G.gauss_ctx(*x.shape)
    G.load(ctx, r, x)
    return ctx


def _device(ctx):
    info = np.zeros(4)
    ctx.call("smcn_gauss_lkernel_device", _capi().dptr(info))
    return info


def _check_L(L, ex, yard, what):
    assert np.all(np.isfinite(L)), what
    print(f"{what}: yardstick {yard / U:.3g} u, device {G.rel_err(L, ex) / U:.3g} u, allowed {G.MARGIN * yard / U:.3g} u")
    close(L / ex["scale"], ex["L"] / ex["scale"], rtol=0, atol=G.MARGIN * yard, err_msg=what, what="L / scale vs exact")


# ---- 1. the moment sums ------------------------------------------------------------------------------------------------------
SUM_SHAPES = [(D, N) for D in (1, 16, 17, 32, 33, 64) for N in (1, 63, 65, 257, 1000)] + \
             [(17, 64 * 1024 + 65), (2, 256 * 1024 + 257)]       # more tiles than kMaxPart blocks: the grid-stride loop


@pytest.mark.parametrize("D,N", SUM_SHAPES)
def test_moment_sums(D, N):
    """smcn_gauss_lkernel_sums, un-shifted and shifted by the float64 mean, against exact_sums: every sum within
    (depth + 5) u of the sum of its terms' magnitudes.  depth: the longest chain of additions the two kernels' loops give
    the shape (_glk.sums_depth, derived next to the loop structure); + 5: the two shift subtractions, the product and the
    final store, one more for the negation-and-shift of r being one rounding each.  Shapes: one column and kGlkMaxD..64
    (the E x TP tile next to nq = 8384 accumulators in LDS, sum_final_kernel striding over more vectors than blocks),
    both sides of the TP switch at D = 16 / 17, N of 1, below, above and far from a multiple of either tile."""
    capi = _capi()
    rng = np.random.default_rng(1000 * D + N % 1000)
    x = rng.standard_normal((N, D)) * rng.uniform(0.3, 3.0, D) + rng.uniform(-4.0, 4.0, D)
    r = 0.5 * x[:, ::-1] + rng.standard_normal((N, D)) - 1.5
    ctx = _loaded(r, x)
    E = 2 * D
    nq = E + E * (E + 1) // 2
    depth = G.sums_depth(N, D)
    for shift in (np.zeros(E), np.hstack([-r, x]).mean(axis=0)):
        dev = np.full(nq, np.nan)
        ctx.call("smcn_gauss_lkernel_sums", capi.dptr(np.ascontiguousarray(shift)), capi.dptr(dev))
        want, mag = G.exact_sums(r, x, shift)
        assert np.all(np.isfinite(dev))
        assert np.all(dev[mag == 0.0] == 0.0)                       # (N = 1 around its own mean: every term is exactly 0)
        m = np.where(mag > 0.0, mag, 1.0)
        print(f"D={D} N={N} depth {depth}: worst {np.max(np.abs(dev - want) / m) / U:.3g} u of sum|term|, allowed {depth + 5} u")
        close(dev / m, want / m, rtol=0, atol=(depth + 5) * U, err_msg=f"D={D} N={N} shifted={bool(shift.any())}",
              what="moment sums / sum|term| vs exact")


# ---- 2. the conditional log-density ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["d1", "d3", "d13_s2", "d8_far", "d32_70", "d5_255", "d5_256", "d5_257"])
def test_logpdf_kernel(name):
    """smcn_gauss_lkernel_logpdf fed the reference's (mu_x, m0, B, U, c0) rounded to float64, against exact().  Yardstick:
    the same formula in NumPy from the same rounded parameters (what rounding the parameters alone costs)."""
    capi = _capi()
    r, x = G.population(name)
    ex = G.exact_case(name)
    ctx = _loaded(r, x)
    ctx.call("smcn_gauss_lkernel_logpdf", *(capi.dptr(np.ascontiguousarray(ex[k])) for k in ("mu_x", "m0", "B", "U")),
             float(ex["c0"]))
    yard = max(G.rel_err(G.logpdf_np(r, x, ex["mu_x"], ex["m0"], ex["B"], ex["U"], ex["c0"]), ex), G.YARD_FLOOR)
    _check_L(G.read_L(ctx), ex, yard, f"logpdf {name}")


# ---- 3. the whole device path ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_device_path(name):
    """smcn_gauss_lkernel_device on every population: the decision the exact condition numbers force; where it answers,
    L and c0 against exact() and both condition estimates within [cond, D^1.5 cond] of the exact 2-norm condition numbers
    (an upper bound, and no looser than trace x Frobenius norm has to be); where it refuses, no L value is left behind
    for smcn_reweight, and GaussianApproxLKernel.apply ends on the host path."""
    capi = _capi()
    r, x = G.population(name)
    N, D = x.shape
    ex = G.exact_case(name)
    cls = G.decision(ex, D)
    ctx = _loaded(r, x)
    info = _device(ctx)
    print(f"{name}: class {cls}, info {info.tolist()}, exact cond {ex['cond_xx']:.4g} {ex['cond_cov']:.4g}")
    assert info[0] in (0.0, 1.0, 2.0)
    if cls == "accept":
        assert info[0] == 0.0, f"{name}: refused (status {info[0]}) with estimates {info[2]:.3g}, {info[3]:.3g}"
    elif cls == "refuse":
        assert info[0] != 0.0, f"{name}: answered with estimates {info[2]:.3g}, {info[3]:.3g}"
    if info[0] == 0.0:
        yard = G.yardstick(r, x, ex)
        _check_L(G.read_L(ctx), ex, yard, f"device {name}")
        s0 = float(np.min(ex["scale"]))                     # c0 is a part of every L_i: the tightest of their scales
        close(info[1] / s0, ex["c0"] / s0, rtol=0, atol=G.MARGIN * yard, err_msg=name, what="c0 / scale vs exact")
        for what, est, cond in (("c_xx", info[2], ex["cond_xx"]), ("cov", info[3], ex["cond_cov"])):
            assert cond * (1 - 1e-6) <= est <= D ** 1.5 * cond * (1 + 1e-6), \
                f"{name}: estimate {est!r} of cond({what}) = {cond!r}, D^1.5 = {D ** 1.5:.4g}"
        return
    with pytest.raises(capi.SmcnError, match=NOT_SET):
        G.read_L(ctx)
    if name not in G.HOST_ANSWERS:
        return
    # the reference's own calls decide: the host path of apply(), its sums from the device
    from smcnuts_amd.lkernel.gaussian_lkernel import GaussianApproxLKernel
    G.load(ctx, r, x)
    k = GaussianApproxLKernel(types.SimpleNamespace(dim=D), N)
    assert k.apply(ctx, types.SimpleNamespace(native_momentum=True)) == capi.LKERNEL_GAUSSIAN
    assert k.last_path == "host"
    L = G.read_L(ctx)
    assert np.all(np.isfinite(L))
    if not ex["singular"]:
        # same calls as host_L on moment sums from the device instead of np.cov: one more float64 formulation
        yard = G.yardstick(r, x, ex)
        close(L / ex["scale"], G.host_L(r, x) / ex["scale"], rtol=0, atol=G.MARGIN * yard, err_msg=name,
              what="host path / scale vs calculate_L")


# ---- 4. a non-finite particle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,value", [("x", math.nan), ("r", math.inf)])
def test_non_finite_particle_is_refused(which, value):
    """One NaN in x' (c_xx is NaN: the first pivot test fails) or one +inf in r' (its mean is inf, the centred column NaN:
    c_xx factorises, cov does not): the device refuses, and smcn_reweight finds no L value -- none from this call, and the
    values an earlier L-kernel call had set on the same proposal no longer count."""
    capi = _capi()
    r, x = (a.copy() for a in G.population("d5_2d2"))
    ex = G.exact_case("d5_2d2")
    (x if which == "x" else r)[7, 2] = value
    ctx = _loaded(r, x)
    ctx.call("smcn_gauss_lkernel_logpdf", *(capi.dptr(np.ascontiguousarray(ex[k])) for k in ("mu_x", "m0", "B", "U")),
             float(ex["c0"]))                                   # L values are set now: the refusal must unset them
    info = _device(ctx)
    assert info[0] in (1.0, 2.0), info
    with pytest.raises(capi.SmcnError, match=NOT_SET):
        G.read_L(ctx)


# ---- 5. over shards ----------------------------------------------------------------------------------------------------------
def _staged(r, x, sizes):
    """smcn_gauss_lkernel_stage 0 / 1 / 2 on one context per shard, from one thread, the all-gather done by hand through
    smcn_buf_get / smcn_buf_set.  -> (info per rank, the shards' L values concatenated)."""
    capi = _capi()
    N, D = x.shape
    assert sum(sizes) == N
    E = 2 * D
    nq = E + E * (E + 1) // 2
    world = len(sizes)
    edges = np.concatenate([[0], np.cumsum(sizes)])
    ctxs, bufs = [], []
    for a, b in zip(edges[:-1], edges[1:]):
        ctx = _loaded(r[a:b], x[a:b])
        loc, gat = C.c_void_p(), C.c_void_p()
        ctx.call("smcn_gauss_lkernel_buffers", world, C.byref(loc), C.byref(gat))
        ctxs.append(ctx)
        bufs.append((loc.value, gat.value))

    def gather():
        if world == 1:
            return
        rows = np.empty((world, nq))
        for w, (ctx, (loc, _)) in enumerate(zip(ctxs, bufs)):
            ctx.call("smcn_buf_get", loc, nq, capi.dptr(rows[w]))
        for ctx, (_, gat) in zip(ctxs, bufs):
            ctx.call("smcn_buf_set", gat, rows.size, capi.dptr(rows.reshape(-1)))

    infos = [np.zeros(4) for _ in ctxs]
    for stage in (0, 1, 2):
        for ctx, info in zip(ctxs, infos):
            ctx.call("smcn_gauss_lkernel_stage", stage, world, float(N), capi.dptr(info) if stage == 2 else None)
        if stage < 2:
            gather()
    return infos, np.concatenate([G.read_L(ctx) for ctx in ctxs])


def test_staged_path():
    """d5 at N = 257 as one shard, as (129, 128) and as (200, 56, 1): every rank holds the same info bits, the concatenated
    L values meet the tolerance of the one-shard call against exact() of the union, and the one-shard staged run is the
    one-shard call bit for bit."""
    name = "d5_257"
    r, x = G.population(name)
    ex = G.exact_case(name)
    yard = G.yardstick(r, x, ex)
    ctx = _loaded(r, x)
    info1 = _device(ctx)
    assert info1[0] == 0.0
    L1 = G.read_L(ctx)
    for sizes in ((257,), (129, 128), (200, 56, 1)):
        infos, L = _staged(r, x, sizes)
        for info in infos[1:]:
            np.testing.assert_array_equal(_bits(info), _bits(infos[0]))
        assert infos[0][0] == 0.0
        _check_L(L, ex, yard, f"staged {sizes}")
        s0 = float(np.min(ex["scale"]))
        close(infos[0][1] / s0, ex["c0"] / s0, rtol=0, atol=G.MARGIN * yard, what="staged c0 / scale vs exact")
        if len(sizes) == 1:
            np.testing.assert_array_equal(_bits(infos[0]), _bits(info1))
            np.testing.assert_array_equal(_bits(L), _bits(L1))
