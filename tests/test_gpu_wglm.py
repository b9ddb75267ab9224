"""The wide GLM target on the device (WideGLMTarget; SMCN_MODEL_WGLM; GlmWideModel<64, 2 | 4>) against exact references,
against GLMTarget on the same data, and against the same model evaluated on the host (the numpy densities of
tests/_glm.py / tests/_glm_disp.py through HostTarget / oracle/pynuts.PyNUTS).

Shapes.  The functor puts coordinate c on lane c % 64, slot c / 64, two slots for D <= 128 and four above, and takes the
observations in chunks of 64.  The column counts below put one coordinate in slot 1, an odd count with its pad column,
both sides of the two / four slot switch, a slot exactly full or empty and full capacity; the dispersion families take
one column fewer, so that tau falls on lane 0 and on lane 63 of slot 1, on lane 0 of slot 2 and on the last lane of the
last slot.  n and M sit on both sides of a chunk / of the 64 rows a block of the evaluation kernel takes per trip.
Every value tolerance is the worst-case bound of the evaluation it checks (_glm.device_bounds / _glm_disp.device_bounds:
worst-case in D and n, whatever the summation order); the trajectory tolerance is measured on the host (_wglm.py)."""
import numpy as np
import pytest

import _glm
import _glm_disp as gd
import _summary as S
import _wglm
from _tol import close
from test_gpu_glm import _points as glm_points
from test_gpu_glm_disp import _points as disp_points

pytestmark = pytest.mark.gpu

FAMILIES = ("bernoulli_logit", "poisson_log", "normal", "neg_binomial_2_log")
DISP = _wglm.DISP
U = _glm.U
DC_LIST = (65, 66, 127, 128, 129, 191, 192, 255, 256)
N_LIST = (1, 7, 64, 65, 130)
M_LIST = (1, 7, 64, 65, 200)


def _models(family, n, Dc, seed, intercept):
    """WideGLMTarget and the numpy model of one synthetic data set with Dc coefficients."""
    p = Dc - intercept
    X, y = _wglm.synthetic(family, n, p, seed)
    sd = np.linspace(0.8, 2.5, Dc)
    return (_wglm.wide_target(X, y, family, sd, (0.2, 1.5), intercept),
            _wglm.numpy_model(X, y, family, sd, (0.2, 1.5), intercept))


def _pts(model, rng, M):
    """M points: benign ones and, where M has room for them, the extreme points of the narrow targets' tests."""
    if M < 16:
        return rng.standard_normal((M, model.dim)) * 0.5
    x = (disp_points if model.family in DISP else glm_points)(model, rng, True)
    return np.vstack([x, rng.standard_normal((M - len(x), model.dim)) * 0.5])


def _value_cases():
    out = []
    for f, family in enumerate(FAMILIES):
        for i, Dc in enumerate(DC_LIST):
            out.append((family, Dc - (family in DISP), N_LIST[(i + f) % 5], M_LIST[(i + 2 * f + 2) % 5], (i + f) % 2 == 0))
    # every n with every M once more, at the first column count past two slots
    for i, n in enumerate(N_LIST):
        for j, M in enumerate(M_LIST):
            family = FAMILIES[(i + j) % 4]
            case = (family, 129 - (family in DISP), n, M, True)
            if case not in out:
                out.append(case)
    return out


@pytest.mark.parametrize("family,Dc,n,M,intercept", _value_cases())
def test_values_against_exact_reference(family, Dc, n, M, intercept):
    """logpdf_parts, and the gradient at phi = 0 (the prior's part) and phi = 1, against math.fsum over the float64
    terms; the non-finite pattern element by element."""
    disp = family in DISP
    ref = gd if disp else _glm
    t, m = _models(family, n, Dc, 1000 * Dc + n, intercept)
    assert t.dim == m.dim == Dc + disp
    x = _pts(m, np.random.default_rng(Dc + n + M), M)
    lpri, llik, gpri, glik = ref.exact_parts(m, x)
    b_lpri, b_llik, b_glik = ref.device_bounds(m, x)
    a, b = t.logpdf_parts(x)
    print(f"lpri: max |err| / bound {np.max(np.abs(a - lpri) / (b_lpri.max() + 1e-300)):.3g}")
    close(a, lpri, rtol=0.0, atol=b_lpri.max() + 1e-300)
    fin = np.isfinite(llik)
    assert np.array_equal(np.isfinite(b), fin), (b, llik)
    assert np.all(b[~fin] == -np.inf)
    print(f"llik: max |err| / bound {np.max(np.abs(b[fin] - llik[fin]) / b_llik[fin], initial=0.0):.3g}")
    assert np.all(np.abs(b[fin] - llik[fin]) <= b_llik[fin]), (b[fin] - llik[fin], b_llik[fin])
    for phi in (0.0, 1.0):
        lp = t.logpdf(x, phi)
        g = t.logpdfgrad(x, phi)
        assert np.all(lp[~fin] == -np.inf) and np.all(g[~fin] == -np.inf)
        assert np.all(np.isfinite(lp[fin])) and np.all(np.isfinite(g[fin]))
        want = lpri[fin] + phi * llik[fin]
        bound = b_lpri[fin] + phi * b_llik[fin] + 2 * U * (np.abs(lpri[fin]) + phi * np.abs(llik[fin]))
        assert np.all(np.abs(lp[fin] - want) <= bound), (lp[fin] - want, bound)
        gw = gpri[fin] + phi * glik[fin]
        gb = phi * b_glik[fin] + 2 * U * (np.abs(gpri[fin]) + phi * np.abs(glik[fin])) + 1e-300
        print(f"grad, phi = {phi}: max |err| / bound {np.max(np.abs(g[fin] - gw) / gb, initial=0.0):.3g}")
        assert np.all(np.abs(g[fin] - gw) <= gb), np.max(np.abs(g[fin] - gw) - gb)


_narrow = {}


def _narrow_reference(family):
    """The 64-coefficient GLMTarget, its points and its device values: computed once per family."""
    if family not in _narrow:
        from smcnuts_amd import GLMTarget
        X, y = _glm.synthetic(family, 130, 63, 77)
        g = GLMTarget(X, y, family=family, prior_sd=2.0)
        m = _glm.GLMNumpy(X, y, family, 2.0)
        x = np.random.default_rng(3).standard_normal((65, 64)) * 0.5
        _narrow[family] = (X, y, m, x, g.logpdf_parts(x), g.logpdfgrad(x, 1.0), _glm.device_bounds(m, x))
    return _narrow[family]


@pytest.mark.parametrize("family", ("bernoulli_logit", "poisson_log"))
@pytest.mark.parametrize("added", (1, 64, 192))
def test_zero_columns_against_glmtarget(family, added):
    """The same data with all-zero columns appended is the same likelihood whatever the added coefficients are: llik and
    the first 64 gradient entries agree with GLMTarget's within the two evaluations' bounds, and the likelihood's
    gradient in the added coordinates is exactly 0.  (The entry points return fma(phi, glik, gpri), rounded once in each
    call: 4 u |gradient| beside the two bounds.  With prior_sd = 2, gpri = -x / 4 exactly, and at phi = 2^500 any
    non-zero glik, however small, would show against it.)"""
    X, y, m, x, (_, llik_n), grad_n, (_, bl_n, bg_n) = _narrow_reference(family)
    Xw = np.hstack([X, np.zeros((X.shape[0], added))])
    t = _wglm.wide_target(Xw, y, family, 2.0)
    mw = _glm.GLMNumpy(Xw, y, family, 2.0)
    assert t.dim == 64 + added
    xw = np.hstack([x, 3.0 * np.random.default_rng(added).standard_normal((len(x), added))])
    _, bl_w, bg_w = _glm.device_bounds(mw, xw)
    _, llik_w = t.logpdf_parts(xw)
    assert np.all(np.abs(llik_w - llik_n) <= bl_n + bl_w), (llik_w - llik_n, bl_n + bl_w)
    grad_w = t.logpdfgrad(xw, 1.0)
    tol = bg_n + bg_w[:, :64] + 4 * U * np.abs(grad_n)
    assert np.all(np.abs(grad_w[:, :64] - grad_n) <= tol), np.max(np.abs(grad_w[:, :64] - grad_n) - tol)
    gpri = t.logpdfgrad(xw, 0.0)[:, 64:]
    np.testing.assert_array_equal(gpri, -0.25 * xw[:, 64:])
    np.testing.assert_array_equal(grad_w[:, 64:], gpri)
    np.testing.assert_array_equal(t.logpdfgrad(xw, 2.0 ** 500)[:, 64:], gpri)


# (family, D, step, seed): the step is small enough for trees of 63 leapfrogs and more; the seed is the data's
TAPE_CASES = [("bernoulli_logit", 65, 0.1, 0), ("poisson_log", 128, 0.1, 0), ("normal", 129, 0.05, 0),
              ("neg_binomial_2_log", 256, 0.1, 0)]


@pytest.mark.parametrize("family,D,eps,seed", TAPE_CASES)
def test_nuts_on_tapes_against_pynuts(family, D, eps, seed):
    """NUTSProposal(WideGLMTarget).rvs on drawn tapes: draws consumed, leapfrogs and depth exact for every particle, x'
    and r' within 10 times the spread of two correct host evaluations of the same trajectories (_wglm.tape_reference)."""
    from smcnuts_amd.proposal.nuts import NUTSProposal
    ref = _wglm.tape_reference(family, D, eps, seed)
    t = _wglm.wide_target(ref["X"], ref["y"], family)
    assert t.dim == D
    tape = np.concatenate(ref["tapes"])
    tape_off = np.concatenate([[0], np.cumsum([len(v) for v in ref["tapes"]])]).astype(np.int64)
    prop = NUTSProposal(t, None, eps)
    xn, rn = prop.rvs(ref["x"], ref["r"], 1.0, tape=tape, tape_off=tape_off)
    st = prop.last_stats
    assert not st["flags"].any()
    assert ref["nleap"].max() >= 63
    print(f"host spread {ref['spread']:.3g}, tolerance {ref['tol']:.3g}; device: x' {np.max(np.abs(xn - ref['want_x'])):.3g}, "
          f"r' {np.max(np.abs(rn - ref['want_r'])):.3g}; leapfrogs {ref['nleap'].tolist()}")
    np.testing.assert_array_equal(st["ndraws"], ref["ndraws"])
    np.testing.assert_array_equal(st["nleap"], ref["nleap"])
    np.testing.assert_array_equal(st["depth"], ref["depth"])
    close(xn, ref["want_x"], rtol=0.0, atol=ref["tol"], what=f"wide GLM, D = {D}: x' on tapes against PyNUTS")
    close(rn, ref["want_r"], rtol=0.0, atol=ref["tol"], what=f"wide GLM, D = {D}: r' on tapes against PyNUTS")


@pytest.mark.parametrize("family,D,eps,tape", [("bernoulli_logit", 65, 0.1, TAPE_CASES[0]), ("normal", 130, 0.05, TAPE_CASES[2])])
def test_philox_mode_against_host_target(family, D, eps, tape):
    """Production RNG: the device-native target and HostTarget(numpy model) on the same seed and state -- the same
    momenta, trees and draws for every particle, x' and r' to the tolerance measured for the family's tape case."""
    from smcnuts_amd import HostTarget, _capi
    N, seed, it = 2000, 4242, 5
    disp = family in DISP
    X, y = _wglm.synthetic(family, 65, D - 1 - disp, 11 * D, scale=0.5)
    t = _wglm.wide_target(X, y, family)
    h = HostTarget(_wglm.numpy_model(X, y, family))
    x = np.random.default_rng(D).standard_normal((N, D)) * 0.1
    if disp:
        x[:, -1] += np.log(0.7)
    out = []
    for tgt in (t, h):
        ctx = _capi.Context(N, tgt.model_id, tgt.model_data)
        if tgt is h:
            h.attach(ctx)
        ctx.set_seed(seed)
        ctx.set_state(x=x, logw=np.zeros(N))
        ctx.propose_nuts(eps, 1.0, it, max_depth=5)         # (the host side evaluates in lock step: trees of <= 63 leapfrogs)
        r, xn, rn, _ = ctx.get_proposal()
        out.append((r, xn, rn, ctx.tree_stats(), ctx.last_leapfrogs()))
        ctx.close()
    (r0, x0, q0, s0, l0), (r1, x1, q1, s1, l1) = out
    np.testing.assert_array_equal(r0, r1)
    mism = np.flatnonzero((s0["ndraws"] != s1["ndraws"]) | (s0["nleap"] != s1["nleap"]))
    assert mism.size == 0, f"particles {mism.tolist()} took a different tree (ndraws {s0['ndraws'][mism].tolist()} vs {s1['ndraws'][mism].tolist()})"
    assert l0 == l1 == int(s0["nleap"].sum())
    assert s0["nleap"].mean() >= 4
    tol = _wglm.tape_reference(*tape)["tol"]
    print(f"tolerance {tol:.3g}; x' {np.max(np.abs(x0 - x1)):.3g}, r' {np.max(np.abs(q0 - q1)):.3g}; mean leapfrogs {s0['nleap'].mean():.1f}")
    close(x0, x1, rtol=0.0, atol=tol, what=f"wide GLM, D = {D}: x' against HostTarget")
    close(q0, q1, rtol=0.0, atol=tol, what=f"wide GLM, D = {D}: r' against HostTarget")


@pytest.mark.parametrize("lkernel,tempering,family,D", [("forwardsLKernel", False, "bernoulli_logit", 65),
                                                        ("forwardsLKernel", True, "normal", 130),
                                                        ("asymptoticLKernel", False, "poisson_log", 65)])
def test_full_loop_against_host_target(lkernel, tempering, family, D):
    """The device-native target and the same model on the host give the same phi ladder, leapfrogs, resampling and
    particles.  No divergent particle is tolerated."""
    from smcnuts_amd import SMCSampler
    disp = family in DISP
    X, y = _wglm.synthetic(family, 120, D - 1 - disp, 3 * D, scale=0.5)
    kw = dict(K=4, N=512, step_size=0.2, seed=9, lkernel=lkernel, tempering=tempering)
    dev = SMCSampler(target=_wglm.wide_target(X, y, family), **kw)
    if lkernel == "forwardsLKernel" and not tempering:
        assert dev.device_resident
    dev.sample(show_progress=False)
    host = SMCSampler(target=_wglm.numpy_model(X, y, family), **kw)
    assert not host.device_resident
    host.sample(show_progress=False)
    np.testing.assert_array_equal(dev.leapfrogs, host.leapfrogs)
    assert list(dev.resampled) == list(host.resampled)
    close(dev.phi, host.phi, rtol=1e-12, atol=1e-15)
    close(dev.x_saved, host.x_saved, rtol=1e-10, atol=1e-11)
    close(dev.ess, host.ess, rtol=1e-10)
    close(dev.mean_estimate, host.mean_estimate, rtol=1e-10, atol=1e-12)


def test_constrained_space_and_summary():
    """A normal fit at Dc = 65: constrain(), the moments and summary() report sigma = e^tau, the coefficients as they are."""
    from smcnuts_amd import SMCSampler
    Dc = 65
    X, y = gd.synthetic("normal", 100, Dc - 1, 5, scale=0.5)
    t = _wglm.wide_target(X, y, "normal")
    x = np.random.default_rng(1).standard_normal((300, Dc + 1))
    c = t.constrain(x)
    np.testing.assert_array_equal(c[:, :Dc], x[:, :Dc])
    close(c[:, Dc], np.exp(x[:, Dc]), rtol=1e-15, atol=0.0)
    kw = dict(K=4, N=1024, step_size=0.1, seed=2)
    dev = SMCSampler(target=t, **kw)
    dev.sample(show_progress=False)
    host = SMCSampler(target=_wglm.numpy_model(X, y, "normal"), **kw)    # (its constrain() exps the last coordinate)
    host.sample(show_progress=False)
    close(dev.x_saved, host.x_saved, rtol=1e-10, atol=1e-11)
    close(dev.mean_estimate, host.mean_estimate, rtol=1e-10, atol=1e-12)
    close(dev.variance_estimate, host.variance_estimate, rtol=1e-8, atol=1e-12)
    assert dev.mean_estimate.shape[1] == Dc + 1 and np.all(dev.mean_estimate[:, -1] > 0.0)
    # sigma, not tau: the weighted mean of e^tau of the downloaded particles
    xs, lw = dev.x_saved[-1], dev.logw_saved[-1]
    w = S.weights(lw, dev.N)
    w = w / w.sum()
    close(dev.mean_estimate[-1, -1], w @ np.exp(xs[:, -1]), rtol=1e-11)
    assert abs(dev.mean_estimate[-1, -1] - w @ xs[:, -1]) > 1e-3
    s = dev.summary()
    assert s.names == t.param_names() and len(s.names) == Dc + 1 and s.names[-1] == "sigma"
    assert s.quantiles.shape == (Dc + 1, 5)
    v = t.constrain(xs)
    close(v[:, -1], np.exp(xs[:, -1]), rtol=1e-15, atol=0.0)
    S.check(s.quantiles, v, lw, S.DEFAULT, False, "wide GLM, resident")
    # the median of sigma is the weighted median of e^tau: e^(the weighted median of tau), one of the particles' values
    tau_med, margin = S.columns(xs[:, -1:], lw)[0].quantile(0.5)
    assert margin > 2 * S.TOL(dev.N)                       # (the reference's choice is unambiguous for this seed)
    close(s.quantile(0.5)[-1], np.exp(tau_med), rtol=1e-15, atol=0.0)
    np.testing.assert_array_equal(s.mean, dev.mean_estimate[dev.K])


def test_two_shards_equal_one_and_runs_repeat():
    """Two InProcessComm shards make the run one shard makes, particle for particle; two runs with one seed are
    bit-identical."""
    from smcnuts_amd import SMCSampler
    from tests.test_sharding import _run_shards
    X, y = _glm.synthetic("bernoulli_logit", 150, 64, 65, scale=0.5)
    make_t = lambda: _wglm.wide_target(X, y, "bernoulli_logit")
    kw = dict(K=4, N=2048, step_size=0.1, seed=3, lkernel="forwardsLKernel", tempering=False)
    one = SMCSampler(target=make_t(), **kw)
    one.sample(show_progress=False)
    again = SMCSampler(target=make_t(), **kw)
    again.sample(show_progress=False)
    np.testing.assert_array_equal(again.x_saved, one.x_saved)
    np.testing.assert_array_equal(again.logw_saved, one.logw_saved)
    np.testing.assert_array_equal(again.phi, one.phi)
    sh = _run_shards(lambda c: SMCSampler(target=make_t(), comm=c, **kw), 2, lambda s: s.sample(show_progress=False),
                     device=True)
    for s in sh:
        assert list(s.resampled) == list(one.resampled)
        close(s.phi, one.phi, rtol=1e-12, atol=1e-15)
        close(s.ess, one.ess, rtol=1e-11)
        close(s.mean_estimate, one.mean_estimate, rtol=1e-10, atol=1e-13)
    close(np.concatenate([s.x_saved for s in sh], axis=1), one.x_saved, rtol=1e-10, atol=1e-13)
    assert sum(int(s.leapfrogs.sum()) for s in sh) == int(one.leapfrogs.sum())


def test_creation_errors():
    """What WideGLMTarget refuses in Python, the library refuses at context creation with a message of its own."""
    from smcnuts_amd import _capi
    n = 3

    def data(family, p, ic, y, X=None, s=1.0, mt=0.0, st=1.0):
        Dc = p + ic
        X = np.zeros((n, p)) if X is None else X
        return np.concatenate([[family, n, p, ic], np.full(Dc, s), [mt, st] if family >= 2 else [],
                               np.asarray(y, dtype=np.float64), X.reshape(-1)])

    def X_with(p, v):
        X = np.zeros((n, p))
        X[1, p - 1] = v
        return X

    small = "65 <= D <= 256 coordinates (D counts tau for families 2 and 3); D <= 64 is SMCN_MODEL_GLM's (GLMTarget)"
    big = "65 <= D <= 256 coordinates; larger models run host-evaluated (SMCN_MODEL_HOST + smcn_set_host_target"
    cases = [
        (data(0, 64, 0, [0, 1, 0]), small),
        (data(1, 63, 1, [0, 1, 0]), small),
        (data(2, 63, 0, [0, 1, 0]), small),
        (data(3, 2, 1, [0, 1, 0]), small),
        (data(0, 257, 0, [0, 1, 0]), big),
        (data(1, 256, 1, [0, 1, 0]), big),
        (data(2, 255, 1, [0, 1, 0]), big),
        (data(0, 70, 1, [0, 2, 1]), "wide GLM target: bernoulli_logit needs y in {0, 1}"),
        (data(1, 70, 1, [0, -1, 1]), "wide GLM target: poisson_log needs y in {0, 1, 2, ..}"),
        (data(2, 70, 1, [0, np.nan, 1]), "wide GLM target: normal needs finite y"),
        (data(3, 70, 1, [0, 0.5, 1]), "wide GLM target: neg_binomial_2_log needs y in {0, 1, 2, .., 2^53}"),
        (data(0, 70, 1, [0, 1, 0], s=0.0), "wide GLM target: prior sds must be finite and > 0"),
        (data(2, 70, 1, [0, 1, 0], mt=np.inf), "wide GLM target: m_tau must be finite"),
        (data(3, 70, 1, [0, 1, 0], st=0.0), "wide GLM target: s_tau must be finite and > 0"),
        (data(0, 70, 1, [0, 1, 0], X=X_with(70, np.inf)), "wide GLM target: X must be finite"),
        (data(3, 70, 1, [0, 1, 0], X=X_with(70, np.nan)), "wide GLM target: X must be finite"),
        (data(4, 70, 1, [0, 1, 0]), "wide GLM target: family must be 0 (bernoulli_logit) or 1 (poisson_log), or 2 (normal) or 3"),
        (data(0, 70, 1, [0, 1, 0])[:-1], "wide GLM target: data = [family, n, p, intercept, s_1..s_D"),
        (data(3, 70, 1, [0, 1, 0])[:-1], "wide GLM target: data = [family, n, p, intercept, s_1..s_Dc, m_tau, s_tau"),
        (np.delete(data(2, 70, 1, [0, 1, 0]), [75, 76]), "wide GLM target: family must be 0 (bernoulli_logit) or 1 (poisson_log) "
                                                         "for a block without m_tau, s_tau"),
        (data(0, 0, 0, [0, 1, 0]), "wide GLM target: no coefficients"),
    ]
    for md, msg in cases:
        with pytest.raises(_capi.SmcnError) as ei:
            _capi.Context(64, _capi.MODEL_WGLM, md)
        assert msg in str(ei.value), (str(ei.value), msg)
    # the narrow model's own refusal is untouched
    with pytest.raises(_capi.SmcnError, match="GLM target: the device functor covers D <= 64 coefficients; larger models run "
                                              "host-evaluated"):
        _capi.Context(64, _capi.MODEL_GLM, data(0, 65, 0, [0, 1, 0]))
    for fam, p, ic, D in ((1, 65, 0, 65), (0, 64, 1, 65), (2, 63, 1, 65), (3, 64, 0, 65), (0, 255, 1, 256), (1, 256, 0, 256),
                          (2, 254, 1, 256), (3, 255, 0, 256)):
        ok = _capi.Context(64, _capi.MODEL_WGLM, data(fam, p, ic, [0, 3, 1] if fam else [0, 1, 1]))
        assert ok.D == ok.Dc == D
        ok.close()


def test_what_stays_refused():
    """The Gaussian L-kernel's sums, the pointwise criteria, LOO and prediction are not implemented for wide rows: each
    ends in an error, none in a result."""
    from smcnuts_amd import SMCSampler, _capi
    X, y = _glm.synthetic("bernoulli_logit", 40, 64, 1, scale=0.5)
    kw = dict(K=2, N=256, step_size=0.2, seed=1)
    with pytest.raises(_capi.SmcnError, match="smcn_gauss_lkernel_sums: D > 64 not supported"):
        SMCSampler(target=_wglm.wide_target(X, y, "bernoulli_logit"), lkernel="GaussianApproxLKernel", **kw).sample(
            show_progress=False)
    smc = SMCSampler(target=_wglm.wide_target(X, y, "bernoulli_logit"), **kw)
    smc.sample(show_progress=False)
    with pytest.raises(NotImplementedError, match="WideGLMTarget: pointwise log-likelihood"):
        smc.pointwise()
    with pytest.raises(NotImplementedError, match="WideGLMTarget: pointwise log-likelihood"):
        smc.loo()
    with pytest.raises(NotImplementedError, match="WideGLMTarget: held-out prediction is implemented for GLMTarget"):
        smc.predict(X)
    with pytest.raises(NotImplementedError, match="WideGLMTarget: posterior predictive draws"):
        smc.predict_draws(X)
    # the C entry points refuse the model id with their scope messages
    ctx = smc.samples.ctx
    for call in (lambda: ctx.pointwise_partials(), lambda: ctx.predict_set_data(np.zeros(4), False)):
        with pytest.raises(_capi.SmcnError, match="SMCN_MODEL_GLM"):
            call()
