"""The weight path on the device against the exact references of tests/_weights.py: smcn_reweight (both kernels behind it),
smcn_accept_reject, smcn_reweight_asymptotic, smcn_set_logw_density_ratio, smcn_init_weights, smcn_temper_partials, the
device bisection (smcn_temper_bisect and its staged form) and the moved count of smcn_commit and of the device-resident step.

How the tests get at the kernels: a SMCN_MODEL_HOST context puts the callback's (lpri, llik) into device memory as returned,
so a callback that looks the two parts of a row up in a table -- the row's first coordinate is its index -- injects any
density parts, non-finite ones included; device-native contexts (Gaussians of 4..300 coordinates, arma) cover the same calls
behind real functors and the particle-major momenta of the wide targets.  The parts are always read back with
density_parts() and the reference is built from what was read back.

Every comparison is device against the exact reference (class exact, finite values within the derived bound, printed as
"bound (share used)") unless it says "bits".  No test skips or filters rows: inputs that would land on a decision threshold
are refused by the builders (ValueError), on the CPU."""
import ctypes as C
import math

import numpy as np
import pytest

import _weights as W

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

INF, NAN = math.inf, math.nan
ELEM = [(1, 1), (1, 2), (4, 255), (4, 257), (64, 1000), (4, 4097)]       # (D, N): ragged last blocks, one and many blocks
PHIS = (0.0, 0.37, 1.0)


def _capi():
    from smcnuts_amd import _capi
    return _capi


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def host_ctx(N, D, tl, tk, particle_base=0):
    """A host-evaluated context whose density parts are table rows: (lpri, llik) of a row = (tl, tk)[int(row[0])]."""
    capi = _capi()
    ctx = capi.Context(N, capi.MODEL_HOST, np.array([float(D)]), particle_base=particle_base)
    tl, tk = np.ascontiguousarray(tl, dtype=np.float64), np.ascontiguousarray(tk, dtype=np.float64)

    def cb(user, n, d, x, want_grad, lpri, llik, gpri, glik):
        try:
            idx = np.ctypeslib.as_array(x, shape=(n, d))[:, 0].astype(np.int64)
            np.ctypeslib.as_array(lpri, shape=(n,))[:] = tl[idx]
            np.ctypeslib.as_array(llik, shape=(n,))[:] = tk[idx]
            return 0
        except Exception:
            return 1

    ctx._cb = capi.HOST_TARGET_FN(cb)            # (the trampoline must outlive the context)
    ctx.call("smcn_set_host_target", ctx._cb, None)
    return ctx


def gauss_ctx(N, D, seed, particle_base=0):
    from smcnuts_amd import GaussianTarget
    t = GaussianTarget(D, prior_sd=3.0, lik_mean=0.3, lik_sd=0.8)
    ctx = _capi().Context(N, t.model_id, t.model_data, particle_base=particle_base)
    ctx.set_seed(seed)
    return ctx


def arma_ctx(N):
    from smcnuts_amd import ArmaModel
    t = ArmaModel()
    return _capi().Context(N, t.model_id, t.model_data)


def arma_rows(N, rng):
    x = rng.standard_normal((N, 4)) * np.array([0.3, 0.3, 0.3, 0.5]) + np.array([0.0, 0.9, 0.0, -1.8])
    if N > 8:
        x[5, 3] = 900.0                      # sigma = e^900: the density is -inf
    return x


def logw_new(ctx):
    return ctx.get_proposal(r=False, x_new=False, r_new=False, logw_new=True)[3]


# ---- what becomes of injected non-finite parts -------------------------------------------------------------------------------
def test_injected_parts_arrive_as_returned():
    """The mapping the library applies to a callback's NaN, +inf and -inf: none -- the parts sit in device memory bit for
    bit as returned, and it is combine (log pi_phi not finite -> -inf) that handles them wherever they are used."""
    tl = np.array([-1.5, NAN, INF, -INF, -2.0, -2.5, -3.0, 0.0])
    tk = np.array([-0.5, -1.0, -1.0, -1.0, NAN, INF, -INF, -0.0])
    N = tl.size
    ctx = host_ctx(N, 4, tl, tk)
    x = W.rows(np.arange(N), 4, np.random.default_rng(0))
    ctx.set_state(x=x, logw=np.zeros(N))
    ctx.call("smcn_eval_proposed_parts", 0)
    _, _, c, d = ctx.density_parts()
    np.testing.assert_array_equal(_bits(c), _bits(tl))
    np.testing.assert_array_equal(_bits(d), _bits(tk))
    zero = np.zeros(N)
    ctx.call("smcn_init_weights", 1.0, _capi().dptr(zero))               # logw = log pi_1 - 0
    np.testing.assert_array_equal(ctx.get_state(x=False)[1], W.combine64(tl, tk, 1.0))
    ctx.call("smcn_init_weights", 0.0, _capi().dptr(zero))
    lp0 = ctx.get_state(x=False)[1]
    np.testing.assert_array_equal(lp0, W.combine64(tl, tk, 0.0))         # 0 * -inf and 0 * +inf are NaN, hence -inf
    assert lp0[5] == -INF and lp0[6] == -INF and lp0[0] == -1.5


# ---- 1. smcn_reweight --------------------------------------------------------------------------------------------------------
def _reweight_inputs(D, N, seed):
    rng = np.random.default_rng(seed)
    tl, tk = W.benign_table(2 * N, rng)
    logw = 3.0 * rng.standard_normal(N)
    if N >= 16:
        tl[1] = -INF                                    # p_x = -inf
        tk[N + 2] = -INF                                # p_xn = -inf
        tl[3] = tl[N + 3] = -INF                        # both
        logw[4], logw[5] = -INF, NAN
        tl[6], tk[6] = 1e300, -1e300                    # parts of magnitude 1e300 that cancel, at x ...
        tl[N + 7], tk[N + 7] = -1e300, 1e300            # ... and at x'
        tk[8] = INF                                     # a +inf part: log pi is not finite, hence -inf
        tl[N + 9] = NAN
    elif N == 2:
        tk[N + 1] = -INF
    x, x_new = W.rows(np.arange(N), D, rng), W.rows(N + np.arange(N), D, rng)
    r, r_new = rng.standard_normal((N, D)), rng.standard_normal((N, D))
    return tl, tk, logw, x, x_new, r, r_new, rng


@pytest.mark.parametrize("D,N", ELEM)
def test_reweight_forward_and_plug_in_values(D, N):
    """smcn_reweight plain, with L, with q, with both, as SMCN_LKERNEL_GAUSSIAN with L supplied, and in the call sequence of
    a tempered run (samples.py: the proposal, the bisection for phi_new on the parts at x', then the re-weighting -- which
    asks logpdf with its default phi = 1 whatever phi_new is)."""
    capi = _capi()
    tl, tk, logw, x, x_new, r, r_new, rng = _reweight_inputs(D, N, 100 + N)
    L, q = 5.0 * rng.standard_normal(N) - D, 5.0 * rng.standard_normal(N) - D
    if N >= 16:
        L[10], q[11] = -INF, -INF
    ctx = host_ctx(N, D, tl, tk)
    kin = (W.kinetic_mp(r), W.kinetic_mp(r_new))
    out = {}
    for mode, (Lm, qm, code) in dict(plain=(None, None, 0), L=(L, None, 0), q=(None, q, 0), Lq=(L, q, 0), gaussL=(L, None, 1),
                                     tempered=(None, None, 0)).items():
        ctx.set_state(x=x, logw=logw)
        ctx.call("smcn_set_proposal", capi.dptr(r), capi.dptr(x_new), capi.dptr(r_new))
        if Lm is not None or qm is not None:
            ctx.call("smcn_set_lkernel_values", capi.dptr(Lm), capi.dptr(qm))
        if mode == "tempered":
            phi, st = C.c_double(0.0), C.c_int(9)
            ctx.call("smcn_temper_bisect", 0.0, 0.5 * N, C.byref(phi), C.byref(st))
        ctx.call("smcn_reweight", code)
        a, b, c, d = ctx.density_parts()
        for got, want in ((a, tl[:N]), (b, tk[:N]), (c, tl[N:]), (d, tk[N:])):
            np.testing.assert_array_equal(_bits(got), _bits(want))
        ref = W.reweight_ref(logw, a, b, c, d, r, r_new, L=Lm, q=qm, kin=kin)
        out[mode] = W.check(logw_new(ctx), ref, "reweight")
    # the plug-in values are consumed by the call that used them
    ctx.call("smcn_reweight", 0)
    out["after"] = W.check(logw_new(ctx), W.reweight_ref(logw, a, b, c, d, r, r_new, kin=kin), "reweight")
    print(f"reweight D={D} N={N}: bound (share used) {out}")


# ---- 2. forward re-weighting after a real NUTS launch of a wide target ---------------------------------------------------------
@pytest.mark.parametrize("D", [65, 100, 300])
def test_reweight_and_moved_count_of_the_resident_step_for_wide_targets(D):
    """D > 64: the NUTS kernel leaves |r|^2, |r'|^2 and a moved flag per particle, and the device-resident step re-weights
    from those (the kernel that takes the kinetic energies) and counts the flags.  The reference is built from the
    downloaded r, r', density parts and previous log-weights; the moved count from the downloaded positions.  Then the same
    proposal is uploaded with smcn_set_proposal, which selects the pass over r and r': both device results meet the
    reference, and they agree within the sum of their bounds.  Particle 11 starts at 1e200 (density -inf): it stays."""
    capi = _capi()
    N = 257
    rng = np.random.default_rng(D)
    ctx = gauss_ctx(N, D, 7 + D)
    x0 = 0.3 + 0.8 * rng.standard_normal((N, D))
    x0[11, 0] = 1e200
    lw0 = 0.3 * rng.standard_normal(N)                      # ESS = 0.9 N: the step does not resample
    ctx.set_state(x=x0, logw=lw0)
    ctx.fast_begin(1, False)
    ctx.step_begin(0)
    ctx.step_finish(0, 1, 0, float(N), 0.15, 1.0, max_depth=4)
    hist, _, _ = ctx.fast_read(1, False)
    assert hist[0, 2] == 0.0                                 # not resampled
    x1, lw1, _ = ctx.get_state()
    r, xold, r_new, lwold = ctx.get_proposal(logw_new=True)   # (the step swapped the buffers: "new" now holds the old state)
    np.testing.assert_array_equal(_bits(xold), _bits(x0))
    np.testing.assert_array_equal(_bits(lwold), _bits(lw0))
    a, b, c, d = ctx.density_parts()
    kin = (W.kinetic_mp(r), W.kinetic_mp(r_new))
    refA = W.reweight_ref(lw0, a, b, c, d, r, r_new, kin=kin)
    mA = W.check(lw1, refA, "reweight (kinetic energies of the NUTS launch)")
    assert refA.cls[11] == W.NAN                             # -inf - -inf
    moved = int(np.sum(np.all(x1 != x0, axis=1)))
    assert int(hist[0, 4]) == moved and 0 < moved < N
    np.testing.assert_array_equal(_bits(x1[11]), _bits(x0[11]))
    # the same proposal, uploaded: the pass over r and r'
    ctx.set_state(x=x0, logw=lw0)
    ctx.call("smcn_set_proposal", capi.dptr(r), capi.dptr(x1), capi.dptr(r_new))
    ctx.call("smcn_reweight", 0)
    a2, b2, c2, d2 = ctx.density_parts()
    refB = W.reweight_ref(lw0, a2, b2, c2, d2, r, r_new, kin=kin)
    lwB = logw_new(ctx)
    mB = W.check(lwB, refB, "reweight")
    fin = refA.cls == W.FINITE
    np.testing.assert_array_equal(refA.cls, refB.cls)
    shift = (refA.hi - refB.hi) + (refA.lo - refB.lo)        # the density parts of the two routes may differ in their last bits
    assert np.all(np.abs((lw1 - lwB)[fin] - shift[fin]) <= (refA.bound + refB.bound)[fin])
    assert ctx.commit() == moved                             # the count over x and x' of smcn_commit, same proposal
    print(f"wide reweight D={D}: from the launch's kinetic energies {mA}, from r and r' {mB}, moved {moved} of {N}")


# ---- 3. smcn_accept_reject with supplied u -----------------------------------------------------------------------------------
def _check_accept(ctx, dec, x, r, x_new, r_new, parts, what):
    """Decisions exact on every row, read off the state: a rejected row holds (x, r, lpri0, llik0) bit for bit in
    (x', r', lpri1, llik1), an accepted row the proposal's bits; r itself is untouched."""
    a, b, c, d = parts
    r2, xn2, rn2, _ = ctx.get_proposal()
    a2, b2, c2, d2 = ctx.density_parts()
    acc = dec.accept
    np.testing.assert_array_equal(_bits(r2), _bits(r), err_msg=what)
    for got, if_acc, if_rej, name in ((xn2, x_new, x, "x'"), (rn2, r_new, r, "r'"), (c2, c, a, "lpri1"), (d2, d, b, "llik1")):
        want = np.where(acc.reshape((-1,) + (1,) * (np.ndim(got) - 1)), _bits(if_acc), _bits(if_rej))
        bad = np.nonzero((_bits(got) != want).reshape(len(acc), -1).any(axis=1))[0]
        assert bad.size == 0, f"{what}: {name} of rows {bad[:8].tolist()} (reference accepts: {acc[bad[:8]].tolist()}, " \
                              f"prob {[float(dec.prob[i]) for i in bad[:8]]})"
    np.testing.assert_array_equal(_bits(a2), _bits(a))
    np.testing.assert_array_equal(_bits(b2), _bits(b))
    return int(acc.sum())


@pytest.mark.parametrize("phi", PHIS)
@pytest.mark.parametrize("D,N", [(1, 2), (4, 257), (64, 1000)])
def test_accept_reject_with_supplied_uniforms(D, N, phi):
    capi = _capi()
    tl, tk, x, x_new, r, r_new, u, near = W.accept_inputs(D, N, phi, 300 + N)
    ctx = host_ctx(N, D, tl, tk)
    ctx.set_state(x=x, logw=np.zeros(N))
    ctx.call("smcn_set_proposal", capi.dptr(r), capi.dptr(x_new), capi.dptr(r_new))
    parts = ctx.density_parts()
    W.set_near(W.decisions_ref(*parts, r, r_new, x_new, phi, u), u, near)
    dec = W.require_margins(W.decisions_ref(*parts, r, r_new, x_new, phi, u))
    if N >= 32:
        assert dec.accept[0] and dec.accept[1] and not dec.accept[2] and dec.accept[6] and dec.accept[10]
        assert not dec.accept[11] and dec.accept[12] and (D == 1 or (not dec.accept[7] and not dec.accept[8] and dec.accept[9]))
        assert [bool(dec.accept[i]) for i in near] == [True, False, True, False]
    ctx.call("smcn_accept_reject", float(phi), capi.dptr(u), 0)
    n_acc = _check_accept(ctx, dec, x, r, x_new, r_new, parts, f"accept D={D} N={N} phi={phi}")
    fin = np.isfinite(dec.margin)
    print(f"accept/reject D={D} N={N} phi={phi}: {n_acc} accepted, every decision exact; smallest margin "
          f"{dec.margin.min():.1e} against a bound of {dec.bound[fin].max() if fin.any() else 0.0:.1e} on prob")


def test_accept_reject_after_a_real_launch_of_a_wide_target():
    """D = 100: the launch leaves r and r' particle-major; smcn_accept_reject converts them in place first.  r and r' are
    downloaded before and after the call and compared bit for bit."""
    capi = _capi()
    N, D, phi = 257, 100, 0.37
    rng = np.random.default_rng(5)
    ctx = gauss_ctx(N, D, 21)
    x = 0.3 + 1.2 * rng.standard_normal((N, D))
    ctx.set_state(x=x, logw=np.zeros(N))
    ctx.propose_nuts(0.15, phi, 3, max_depth=4)
    r, x_new, r_new, _ = ctx.get_proposal()
    parts = ctx.density_parts()
    u = rng.uniform(size=N)
    u[0] = 1.0 - 2.0 ** -53
    dec0 = W.decisions_ref(*parts, r, r_new, x_new, phi, u)
    near = [int(i) for i in np.nonzero(np.array([0.0 < float(p) < 1.0 for p in dec0.prob]))[0][:4]]
    assert len(near) == 4
    W.set_near(dec0, u, near)
    dec = W.require_margins(W.decisions_ref(*parts, r, r_new, x_new, phi, u))
    ctx.call("smcn_accept_reject", phi, capi.dptr(u), 3)
    n_acc = _check_accept(ctx, dec, x, r, x_new, r_new, parts, "accept after a launch, D=100")
    assert 0 < n_acc < N
    print(f"accept/reject after a launch D=100: {n_acc} of {N} accepted, every decision exact")


# ---- 4. smcn_accept_reject with the library's own uniforms -------------------------------------------------------------------
def test_accept_reject_with_philox_uniforms_and_two_shards():
    """u = NULL draws Philox stream 4, keyed by the global particle index: the decisions are the reference's on the
    oracle's uniforms of that stream, and two contexts of N / 2 particles with particle_base 0 and N / 2 make the decisions
    of the one context row for row."""
    capi = _capi()
    D, N, seed, it, phi = 4, 1000, 424242, 5, 1.0
    tl, tk, x, x_new, r, r_new, _, _ = W.accept_inputs(D, N, phi, 77)
    u = orc.philox_particle_uniforms(seed, it, 0, N, 4, 0)
    one = host_ctx(N, D, tl, tk)
    one.set_seed(seed)
    one.set_state(x=x, logw=np.zeros(N))
    one.call("smcn_set_proposal", capi.dptr(r), capi.dptr(x_new), capi.dptr(r_new))
    parts = one.density_parts()
    dec = W.require_margins(W.decisions_ref(*parts, r, r_new, x_new, phi, u))
    one.call("smcn_accept_reject", phi, None, it)
    n_acc = _check_accept(one, dec, x, r, x_new, r_new, parts, "accept, Philox")
    assert 100 < n_acc < N - 100
    h = N // 2
    for base, sl in ((0, slice(0, h)), (h, slice(h, N))):
        sh = host_ctx(h, D, tl, tk, particle_base=base)
        sh.set_seed(seed)
        sh.set_state(x=x[sl], logw=np.zeros(h))
        sh.call("smcn_set_proposal", capi.dptr(np.ascontiguousarray(r[sl])), capi.dptr(np.ascontiguousarray(x_new[sl])),
                capi.dptr(np.ascontiguousarray(r_new[sl])))
        ps = sh.density_parts()
        sub = W.Decisions(dec.prob[sl], dec.accept[sl], dec.margin[sl], dec.bound[sl], dec.dH_cls[sl], dec.dH[sl])
        sh.call("smcn_accept_reject", phi, None, it)
        _check_accept(sh, sub, x[sl], r[sl], x_new[sl], r_new[sl], ps, f"accept, Philox, shard at {base}")
    print(f"accept/reject Philox: {n_acc} of {N} accepted; two shards row for row")


# ---- 5. the two-temperature differences --------------------------------------------------------------------------------------
PAIRS = [(0.0, 1e-4), (0.3, 0.3000001), (0.999, 1.0), (0.0, 1.0), (0.37, 0.37), (0.0, 0.0), (1.0, 1.0)]     # (old, new)


def _edge_table(n, rng):
    tl, tk = W.benign_table(n, rng)
    if n >= 16:
        tk[1] = -INF                       # 0 * -inf at phi = 0
        tl[2] = tk[2] = -INF
        tk[3] = INF
        tl[4] = NAN
        tl[6], tk[6] = 1e300, -1e300       # cancels at phi = 1 only
        tl[7] = -INF
    return tl, tk


@pytest.mark.parametrize("D,N", ELEM)
def test_asymptotic_reweight_and_density_ratio_on_injected_parts(D, N):
    capi = _capi()
    rng = np.random.default_rng(500 + N)
    tl, tk = _edge_table(2 * N, rng)
    logw = 3.0 * rng.standard_normal(N)
    if N >= 16:
        logw[8], logw[9] = -INF, NAN
    x, x_new = W.rows(np.arange(N), D, rng), W.rows(N + np.arange(N), D, rng)
    r = rng.standard_normal((N, D))
    ctx = host_ctx(N, D, tl, tk)
    ctx.set_state(x=x, logw=logw)
    ctx.call("smcn_set_proposal", capi.dptr(r), capi.dptr(x_new), capi.dptr(r))
    a, b, _, _ = ctx.density_parts()
    out = {}
    for po, pn in PAIRS:
        ctx.call("smcn_reweight_asymptotic", po, pn)
        out[(po, pn)] = W.check(logw_new(ctx), W.tempered_difference_ref(logw, a, b, pn, po), "reweight_asymptotic")
    for po, pn in PAIRS:
        ctx.call("smcn_set_logw_density_ratio", pn, po)              # re-evaluates the parts at the resident x
        _, _, c, d = ctx.density_parts()
        np.testing.assert_array_equal(_bits(c), _bits(tl[:N]))
        got = ctx.get_state(x=False)[1]
        out[("ratio", pn, po)] = W.check(got, W.tempered_difference_ref(None, c, d, pn, po), "density_ratio")
    print(f"two-temperature differences D={D} N={N}: absolute bound (share used) {out}")


def test_asymptotic_reweight_and_density_ratio_on_arma():
    N = 257
    rng = np.random.default_rng(9)
    ctx = arma_ctx(N)
    x = arma_rows(N, rng)
    logw = rng.standard_normal(N)
    ctx.set_state(x=x, logw=logw)
    out = {}
    for po, pn in PAIRS:
        ctx.call("smcn_set_logw_density_ratio", pn, po)
        _, _, c, d = ctx.density_parts()
        ref = W.tempered_difference_ref(None, c, d, pn, po)
        assert ref.cls[5] == W.NAN                                   # -inf - -inf at the row whose density is -inf
        out[(pn, po)] = W.check(ctx.get_state(x=False)[1], ref, "density_ratio")
    print(f"density ratio on arma: {out}")


# ---- 6. smcn_init_weights ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("phi", PHIS)
@pytest.mark.parametrize("D,N", ELEM)
def test_init_weights_on_injected_parts(D, N, phi):
    capi = _capi()
    rng = np.random.default_rng(600 + N)
    tl, tk = _edge_table(N, rng)
    x = W.rows(np.arange(N), D, rng)
    logq0 = -2.0 + rng.standard_normal(N)
    if N >= 16:
        logq0[10] = -INF
    ctx = host_ctx(N, D, tl, tk)
    ctx.set_state(x=x, logw=np.full(N, 7.0))
    ctx.call("smcn_init_weights", float(phi), capi.dptr(logq0))
    _, _, c, d = ctx.density_parts()
    m1 = W.check(ctx.get_state(x=False)[1], W.init_weights_ref(c, d, phi, logq0=logq0), "init_weights")
    ctx.call("smcn_init_weights", float(phi), None)
    _, _, c, d = ctx.density_parts()
    m2 = W.check(ctx.get_state(x=False)[1], W.init_weights_ref(c, d, phi, x=x), "init_weights")
    print(f"init_weights D={D} N={N} phi={phi}: with logq0 {m1}, N(x; 0, I) {m2}")


@pytest.mark.parametrize("phi", PHIS)
def test_init_weights_behind_device_functors(phi):
    capi = _capi()
    rng = np.random.default_rng(66)
    out = {}
    for name, ctx, x in (("gauss4", gauss_ctx(257, 4, 1), 0.3 + rng.standard_normal((257, 4))),
                         ("gauss100", gauss_ctx(255, 100, 1), 0.3 + rng.standard_normal((255, 100))),
                         ("arma", arma_ctx(257), arma_rows(257, rng))):
        if name == "gauss4":
            x[3, 2] = 1e200                                          # the density overflows: -inf
        N = x.shape[0]
        logq0 = -2.0 + rng.standard_normal(N)
        ctx.set_state(x=x, logw=np.zeros(N))
        for lq in (logq0, None):
            ctx.call("smcn_init_weights", float(phi), capi.dptr(lq))
            _, _, c, d = ctx.density_parts()
            ref = W.init_weights_ref(c, d, phi, x=x, logq0=lq)
            if name == "arma":
                assert ref.cls[5] == W.NINF
            if name == "gauss4":             # (|x|^2 overflows with the density: -inf - -inf under the closed form)
                assert ref.cls[3] == (W.NAN if lq is None else W.NINF)
            out[(name, lq is None)] = W.check(ctx.get_state(x=False)[1], ref, "init_weights")
    print(f"init_weights behind functors phi={phi}: {out}")


# ---- 7. smcn_temper_partials -------------------------------------------------------------------------------------------------
PHI_NEW = {0.0: (0.0, 0.25, 0.5, 1.0), 1e-4: (0.25, 0.5, 1.0), 0.3: (0.3000001, 0.5, 1.0)}


def temper_ctx(lpri, llik):
    """Parts resident at x' (lpri1, llik1): what the NUTS kernel / smcn_eval_proposed_parts leaves."""
    N = len(lpri)
    ctx = host_ctx(N, 1, lpri, llik)
    ctx.set_state(x=np.arange(N, dtype=np.float64).reshape(N, 1), logw=np.zeros(N))
    ctx.call("smcn_eval_proposed_parts", 0)
    _, _, c, d = ctx.density_parts()
    np.testing.assert_array_equal(_bits(c), _bits(lpri))
    np.testing.assert_array_equal(_bits(d), _bits(llik))
    return ctx, c, d


@pytest.mark.parametrize("N", W.TEMPER_N)
@pytest.mark.parametrize("kind", W.TEMPER_KINDS)
def test_temper_partials(kind, N):
    """[max, count at the max, sum over the others, sum of squares] against the exact ones: the count exact, the maximum
    within the v-error and BIT FOR BIT where the expression is exactly computable (the exact maximum is then itself a
    double), the sums within their bounds, the ESS they give within its bound -- N for identical rows --, and NaN for
    the population with a NaN weight."""
    ctx, c, d = temper_ctx(*W.population(kind, N))
    out, nbits = {}, 0
    for po in W.PHI_OLD:
        T = W.Tempered(c, d, po)
        for pn in PHI_NEW[po]:
            dev = ctx.temper_partials(po, pn)
            what = f"{kind} N={N} phi_old={po} phi={pn}"
            exact = T.exactly_computable(pn)
            cls = T.rows_cls(pn)
            if np.any(cls == W.NAN):
                assert kind in ("nan", "overflow") and np.isnan(dev[0]), what      # (overflow rows: 0 * -inf at phi = 0)
                ess = (dev[1] + dev[2]) ** 2 / dev[3]
                assert np.isnan(ess), what
                continue
            assert kind != "nan"
            p = T.partials(pn, strict=not (exact and pn == po))
            assert dev[1] == p["cnt"], f"{what}: count at the maximum {dev[1]} != {p['cnt']}"
            if exact:
                assert _bits(dev[0]) == _bits(p["mx64"]), f"{what}: maximum {dev[0]!r} != {p['mx64']!r}"
                nbits, mm = nbits + 1, "bits"
            else:
                mm = W.check_scalar(dev[0], p["mx"], p["bv"], "temper max")
            e1, e2 = T.sum_bounds(p)
            m1 = W.check_scalar(dev[2], p["s1x"], e1 * p["s1"], "temper s1") if p["s1"] > 0 else "0"
            if p["s1"] == 0:
                assert dev[2] == 0.0, what
            m2 = W.check_scalar(dev[3], p["s2x"], e2 * p["s2"], "temper s2")
            ess = (dev[1] + dev[2]) ** 2 / dev[3]
            me = W.check_scalar(ess, p["essx"], T.ess_bound(p, log_space=False), "temper ESS")
            if kind == "identical":
                assert abs(ess - N) <= T.ess_bound(p, log_space=False), what
            out[(po, pn)] = dict(max=mm, s1=m1, s2=m2, ess=me)
    if kind in ("distinct", "repeated", "identical"):
        assert nbits >= 3                                    # phi_old = 0 with phi = 0.25, 0.5, 1: the maximum bit for bit
    print(f"temper partials {kind} N={N}: bound (share used) {out}")


# ---- 8. / 9. smcn_temper_bisect ----------------------------------------------------------------------------------------------
def _bisect(ctx, po, target):
    phi, st = C.c_double(-1.0), C.c_int(9)
    ctx.call("smcn_temper_bisect", float(po), float(target), C.byref(phi), C.byref(st))
    return phi.value, st.value


@pytest.mark.parametrize("N", W.TEMPER_N)
@pytest.mark.parametrize("kind", W.TEMPER_KINDS + ("masked",))
def test_temper_bisect(kind, N):
    """Targets 0.5 N and 0.9 N from phi_old = 0, 1e-4 and 0.3 on every population: the root property where f_exact has a
    root; otherwise the outcome of the reference's bisection on f_exact -- phi = 1 where ESS(1) >= target (identical rows,
    N = 1), status 2 where both ends are negative (more than half the rows masked) or both NaN, and for a NaN f(phi_old)
    with f(1) < 0 whatever bisect.c's tests make of it."""
    if kind == "masked" and N == 1:
        kind = "distinct"                                    # (one row cannot be half masked)
    ctx, c, d = temper_ctx(*W.population(kind, N))
    out = {}
    for po in W.PHI_OLD:
        T = W.Tempered(c, d, po)
        for alpha in (0.5, 0.9):
            phi, st = _bisect(ctx, po, alpha * N)
            out[(po, alpha)] = W.check_outcome(T, alpha * N, phi, st, f"{kind} N={N} phi_old={po} target={alpha} N")
    print(f"temper bisect {kind} N={N}: {out}")


@pytest.mark.parametrize("N", [2, 257, 1000])
def test_temper_bisect_root_at_the_left_end(N):
    """Target exactly N with every row finite: f(phi_old) = 0, and bisect.c returns the left end.  (At phi = phi_old every
    tempered weight of these populations is an exact 0 on the device too: the count at the maximum is N and the sum over the
    others 0.  Before the ESS of such weights was taken as their count, the rounding of e^(-2 log N) decided: N = 257 returned
    3.7e-9 from phi_old = 0, N = 1000 status 2.)"""
    ctx, c, d = temper_ctx(*W.population("distinct", N))
    for po in W.PHI_OLD:
        T = W.Tempered(c, d, po)
        assert T.f(float(N))(po) == 0.0 and T.f(float(N))(1.0) < 0
        phi, st = _bisect(ctx, po, float(N))
        assert (st, phi) == (0, po), f"N={N} phi_old={po}: status {st}, phi {phi!r}"


def test_temper_bisect_in_a_bracket_narrower_than_1000_xtol():
    """phi_old = 1 - 1e-9 with likelihoods of order 1e9: a root inside a bracket of 500 xtol."""
    N, po = 1000, 1.0 - 1e-9
    ctx, c, d = temper_ctx(*W.population("steep", N))
    T = W.Tempered(c, d, po)
    out = {}
    for alpha in (0.5, 0.9):
        assert W.has_root(T, alpha * N)
        phi, st = _bisect(ctx, po, alpha * N)
        out[alpha] = W.check_outcome(T, alpha * N, phi, st, f"steep target={alpha} N")
        assert po < phi < 1.0
    print(f"temper bisect in [1 - 1e-9, 1]: {out}")


# ---- 10. the staged API ------------------------------------------------------------------------------------------------------
def _staged(ctxs, po, target):
    """ESSTempering.calculate_phi_device's loop over passes on `ctxs` as the shards of one population: the [world][15][4]
    block is gathered on the host (smcn_buf_get) and handed to every shard (smcn_buf_set)."""
    world = len(ctxs)
    bufs = []
    for ctx in ctxs:
        loc, gat = C.c_void_p(), C.c_void_p()
        ctx.call("smcn_temper_bisect_buffers", world, C.byref(loc), C.byref(gat))
        bufs.append((loc, gat))
    capi = _capi()
    p, upto = 0, 1
    while True:
        while p < upto:
            block = np.empty((world, 15, 4))
            for k, ctx in enumerate(ctxs):
                ctx.call("smcn_temper_bisect_pass", p, float(po))
                ctx.call("smcn_buf_get", bufs[k][0], 60, capi.dptr(block[k]))
            for k, ctx in enumerate(ctxs):
                if world > 1:
                    ctx.call("smcn_buf_set", bufs[k][1], 60 * world, capi.dptr(block))
                ctx.call("smcn_temper_bisect_decide", p, world, float(target), float(po))
            p += 1
        res = []
        for ctx in ctxs:
            phi, st = C.c_double(-1.0), C.c_int(9)
            ctx.call("smcn_temper_bisect_result", C.byref(phi), C.byref(st))
            res.append((phi.value, st.value))
        if res[0][1] != 1 or p >= 26:
            return res
        upto = 11 if upto == 1 else min(26, upto + 4)


@pytest.mark.parametrize("kind,N", [("distinct", 4097), ("repeated", 1000)])
def test_staged_bisection_with_one_shard_has_the_bits_of_the_whole(kind, N):
    ctx, c, d = temper_ctx(*W.population(kind, N))
    for po in W.PHI_OLD:
        for alpha in (0.5, 0.9):
            whole = _bisect(ctx, po, alpha * N)
            (phi, st), = _staged([ctx], po, alpha * N)
            assert st == whole[1] == 0 and _bits(phi) == _bits(whole[0]), f"{kind} phi_old={po} target={alpha} N"


@pytest.mark.parametrize("case", ["tied maximum", "masked shard"])
def test_staged_bisection_over_two_unequal_shards(case):
    """Two contexts of one process as shards of 300 and 157 particles: the result is bit-identical on both and has the
    root property against the reference over the union.  "tied maximum": every distinct row, the heaviest included, sits in
    both shards; "masked shard": the second shard's weights are all -inf."""
    N1, N2 = 300, 157
    lpri, llik = W.population("repeated", N1 + N2)
    pos = W.PHI_OLD
    if case == "masked shard":
        lpri[N1:], llik[N1:] = -1e308, -1e308
        pos = (1e-4, 0.3)                                    # (at phi_old = 0 the masked rows are 0 * -inf = NaN)
    else:
        top = int(np.argmax(llik[:N1]))
        assert np.any(llik[N1:] == llik[top])
    a, b = temper_ctx(lpri[:N1], llik[:N1]), temper_ctx(lpri[N1:], llik[N1:])
    out = {}
    for po in pos:
        T = W.Tempered(np.concatenate([a[1], b[1]]), np.concatenate([a[2], b[2]]), po)
        for target in (0.5 * N1, 0.9 * N1) if case == "masked shard" else (0.5 * (N1 + N2), 0.9 * (N1 + N2)):
            (p1, s1), (p2, s2) = _staged([a[0], b[0]], po, target)
            assert s1 == s2 and _bits(p1) == _bits(p2)
            assert W.has_root(T, target)
            out[(po, target)] = W.check_outcome(T, target, p1, s1, f"{case} phi_old={po} target={target}")
    print(f"staged bisection, two shards, {case}: {out}")


# ---- 11. the moved count of smcn_commit --------------------------------------------------------------------------------------
def test_commit_counts_the_rows_whose_every_coordinate_changed():
    """smc_sampler.py:97 on the downloaded x and x': rows with every coordinate changed count; rows with exactly one
    coordinate unchanged do not; NaN != NaN is true.  After the commit x = x' and logw = logw_new bit for bit."""
    capi = _capi()
    for D, N in ((4, 257), (4, 4097), (1, 2)):
        rng = np.random.default_rng(N)
        tl, tk = W.benign_table(2 * N, rng)
        ctx = host_ctx(N, D, tl, tk)
        x, x_new = W.rows(np.arange(N), D, rng), W.rows(N + np.arange(N), D, rng)
        r = rng.standard_normal((N, D))
        if D > 1:
            for i in range(5, N, 7):
                x_new[i, 1 + i % (D - 1)] = x[i, 1 + i % (D - 1)]        # exactly one coordinate unchanged
            x[10, 2] = x_new[10, 2] = NAN                                # "unchanged" NaN: counts as changed
            x_new[13] = x[13]
            x_new[13, 0] = N + 13                                        # only the first coordinate changed
        ctx.set_state(x=x, logw=rng.standard_normal(N))
        ctx.call("smcn_set_proposal", capi.dptr(r), capi.dptr(x_new), capi.dptr(r))
        ctx.call("smcn_reweight", 0)
        xd, xnd, lwn = ctx.get_state()[0], ctx.get_proposal(r=False, r_new=False)[1], logw_new(ctx)
        want = int(np.sum(np.all(xnd != xd, axis=1)))
        assert want == (N - len(range(5, N, 7)) - 1 if D > 1 else N)
        assert ctx.commit() == want
        x2, lw2, _ = ctx.get_state()
        np.testing.assert_array_equal(_bits(x2), _bits(xnd))
        np.testing.assert_array_equal(_bits(lw2), _bits(lwn))


def test_commit_after_a_real_launch_of_a_wide_target():
    """D = 100 after smcn_propose_nuts and smcn_reweight; the particle started at 1e200 keeps its position."""
    N, D = 257, 100
    rng = np.random.default_rng(8)
    ctx = gauss_ctx(N, D, 31)
    x = 0.3 + 0.8 * rng.standard_normal((N, D))
    x[11, 0] = 1e200
    ctx.set_state(x=x, logw=np.zeros(N))
    ctx.propose_nuts(0.15, 1.0, 2, max_depth=4)
    ctx.call("smcn_reweight", 0)
    r, xnd, r_new, lwn = ctx.get_proposal(logw_new=True)
    a, b, c, d = ctx.density_parts()
    m = W.check(lwn, W.reweight_ref(np.zeros(N), a, b, c, d, r, r_new), "reweight")
    xd = ctx.get_state()[0]
    np.testing.assert_array_equal(_bits(xnd[11]), _bits(x[11]))
    want = int(np.sum(np.all(xnd != xd, axis=1)))
    assert 0 < want < N
    assert ctx.commit() == want
    x2, lw2, _ = ctx.get_state()
    np.testing.assert_array_equal(_bits(x2), _bits(xnd))
    np.testing.assert_array_equal(_bits(lw2), _bits(lwn))
    print(f"commit after a launch D=100: moved {want} of {N}; reweight {m}")


def test_zz_report_the_shares_used():
    """The largest share of each derived bound the device used in this session (the figures of the summary)."""
    for what, (bound, share) in sorted(W.SHARES.items()):
        print(f"SHARE {what}: bound {bound:.2e} (per row: the largest median of a call), largest share used {share:.3f}")
    assert all(share <= 1.0 for _, share in W.SHARES.values())
