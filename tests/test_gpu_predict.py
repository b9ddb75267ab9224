"""Held-out prediction of the five device regression targets against the NumPy references of tests/_predict.py.  Every
bound is derived there (module docstring); per-element bounds are asserted element by element, no element left out, and
recorded through _tol.close with the largest bound as atol."""
import math
import time

import numpy as np
import pytest

import _cat
import _glm
import _glm_disp as gd
import _hglm
import _ord
import _pointwise as pw
import _predict as pr
from _tol import close

pytestmark = pytest.mark.gpu

MS = (1, 65, 700)          # particles: below, across and many chunks of 64
USED = {}                  # the largest share of each bound that any case used (printed per test)


# ---- cases: (device target fitted to training rows, NumPy model AT THE NEW ROWS, new rows) ------------------------------
def glm_case(family, D, n, m, seed):
    from smcnuts_amd import GLMTarget
    ic = bool(D % 2)
    disp = family in gd.DISP_FAMILIES
    Dc = D - (1 if disp else 0)
    p = Dc - ic
    X, y = pw.synthetic(family, n, p, seed)
    Xn, yn = pw.synthetic(family, m, p, seed + 1)
    sd = np.linspace(0.8, 2.5, Dc)
    if disp:
        t = GLMTarget(X, y, family=family, prior_sd=sd, intercept=ic, dispersion_prior=(0.0, 1.0))
        mn = gd.GLMDispNumpy(Xn, yn, family, sd, (0.0, 1.0), intercept=ic)
        mt = gd.GLMDispNumpy(X, y, family, sd, (0.0, 1.0), intercept=ic)
    else:
        t = GLMTarget(X, y, family=family, prior_sd=sd, intercept=ic)
        mn = _glm.GLMNumpy(Xn, yn, family, sd, intercept=ic)
        mt = _glm.GLMNumpy(X, y, family, sd, intercept=ic)
    return t, mn, (Xn, yn, None), mt


def hier_case(family, Dc, J, n, m, seed):
    from smcnuts_amd import HierarchicalGLM
    ic = bool(Dc % 2) and Dc >= 1
    p = Dc - ic
    X, y, g = _hglm.synthetic(family, n, p, J, seed)
    Xn, yn, gn = _hglm.synthetic(family, m, p, J, seed + 1)
    sd = np.linspace(0.8, 2.5, Dc)
    kw = dict(dispersion_prior=(0.0, 1.0)) if family in gd.DISP_FAMILIES else {}
    t = HierarchicalGLM(X, y, g, family=family, prior_sd=sd, group_sd_prior=1.5, intercept=ic, n_groups=J, **kw)
    mk = lambda A, b, c: _hglm.HGLMNumpy(A, b, c, family, sd, 1.5, (0.0, 1.0), intercept=ic, n_groups=J)
    return t, mk(Xn, yn, gn), (Xn, yn, gn), mk(X, y, g)


def cat_case(K, Dc, n, m, seed):
    from smcnuts_amd import CategoricalRegression
    ic = bool(Dc % 2)
    p = Dc - ic
    X, y = _cat.synthetic(K, n, p, seed)
    Xn, yn = _cat.synthetic(K, m, p, seed + 1)
    t = CategoricalRegression(X, y, n_classes=K, prior_sd=2.0, intercept=ic)
    return t, _cat.CategoricalNumpy(Xn, yn, K, 2.0, intercept=ic), (Xn, yn, None), _cat.CategoricalNumpy(X, y, K, 2.0, intercept=ic)


def ord_case(K, p, n, m, seed):
    from smcnuts_amd import OrdinalRegression
    X, y = _ord.synthetic(K, n, p, seed)
    Xn, yn = _ord.synthetic(K, m, p, seed + 1)
    t = OrdinalRegression(X, y, n_classes=K)
    return t, _ord.OrdinalNumpy(Xn, yn, K), (Xn, yn, None), _ord.OrdinalNumpy(X, y, K)


def points(mn, M, seed):
    """Random points, and for the categorical and ordinal models their own extreme points (as many as fit in M)."""
    rng = np.random.default_rng(seed)
    x = 0.3 * rng.standard_normal((M, mn.dim))
    if isinstance(mn, _hglm.HGLMNumpy):
        x[:, mn.lt] = -0.5 + 0.3 * rng.standard_normal(M)
    if isinstance(mn, _ord.OrdinalNumpy):
        x[:, mn.p] -= 1.0
        ex = _ord.points(mn, rng)
    elif isinstance(mn, _cat.CategoricalNumpy):
        ex = _cat.points(mn, rng)
    else:
        ex = np.empty((0, mn.dim))
    k = min(M - 1, ex.shape[0])
    if k > 0:
        x[M - k:] = ex[:k]
    return x


def _check(t, mn, new, x, lw, what):
    Xn, yn, gn = new
    kind, K = pr.kind_of(mn), getattr(mn, "K", 0)
    T = pr.terms(mn, x)
    ref = pr.reference(T, lw)
    b = pr.bounds(T, lw, ref)
    got = t.predict(x, Xn, yn, gn, lw)
    pr.assert_prediction(got, ref, b, what=what, close=close, report=USED)
    assert got.n_particles == ref["n_particles"] and got.n_new == Xn.shape[0]
    close(got.ess, ref["ess"], rtol=(x.shape[0] + 16) * 4 * _glm.U, what="weights' ESS")
    if got.prob is not None:
        rows = np.sum(got.prob, axis=1)
        fin = np.isfinite(rows)
        assert np.all(np.abs(rows[fin] - 1.0) <= np.sum(b["prob"], axis=1)[fin] + 4 * K * _glm.U), what + ": prob rows"
    # without y_new: the same summaries, bit for bit, and no lpd
    g0 = t.predict(x, Xn, None, gn, lw)
    assert g0.lpd_i is None and g0.n_inf_i is None
    for k in ("mean_i", "var_i", "prob"):
        a, c = getattr(g0, k), getattr(got, k)
        assert (a is None) == (c is None)
        if a is not None:
            np.testing.assert_array_equal(a, c, err_msg=f"{what} {k}: changed by y_new")
    return got, T, ref, b


def _check_all_weights(t, mn, new, M, seed, what):
    rng = np.random.default_rng(seed)
    x = points(mn, M, seed)
    T = pr.terms(mn, x)
    mat = t.predict_loglik(x, new[0], new[1], new[2])
    assert mat.shape == T["ll"].shape
    pr.assert_loglik(mat, T, close=close, what=what + " predict_loglik")
    lw = 3.0 * rng.standard_normal(M)
    got, _, ref, b = _check(t, mn, new, x, lw, what + " random logw")
    _check(t, mn, new, x, None, what + " equal weights")
    for sh in (1.0e5, -1.0e5):
        g2, _, _, b2 = _check(t, mn, new, x, lw + sh, what + f" logw {sh:+g}")
        bs = pr.weight_shift_bounds(T, lw, ref, _glm.U * float(np.max(np.abs(lw + sh))))
        as_ref = {k: np.asarray(getattr(got, k)) for k in pr.FIELDS if getattr(got, k) is not None}
        pr.assert_prediction(g2, as_ref, pr.add_bounds(b, b2, bs), what=what + f" logw {sh:+g} against unshifted")
    if M > 1:
        lw3 = lw.copy()
        lw3[::3] = -np.inf
        _check(t, mn, new, x, lw3, what + " a third of the weights -inf")


def _report(name):
    print(f"{name}: largest share of a bound used: { {k: round(v, 4) for k, v in USED.items()} }")


# D on both sides of the row capacities 16 / 32 of the GLM walk; every family
@pytest.mark.parametrize("family", pw.FAMILIES)
@pytest.mark.parametrize("D,m", [(2, 1), (3, 65), (16, 130), (17, 64), (32, 7), (33, 65), (64, 70)])
def test_parity_glm(family, D, m):
    t, mn, new, _ = glm_case(family, D, 40, m, 10 * D + m)
    for M in MS:
        _check_all_weights(t, mn, new, M, D + M, f"{family} D={D} m={m} M={M}")
    _report(f"glm {family} D={D}")


# Dc on both sides of the row capacities 16 / 32; J up to the model's capacity D = Dc + J + 1 (+ 1) = 64
@pytest.mark.parametrize("family", _hglm.FAMILIES)
@pytest.mark.parametrize("Dc,J,m", [(0, 3, 65), (3, 4, 1), (16, 10, 66), (17, 33, 64), (32, 5, 7), (33, 28, 65), (40, 22, 70)])
def test_parity_hierarchical(family, Dc, J, m):
    t, mn, new, _ = hier_case(family, Dc, J, 50, m, 7 * Dc + J)
    assert t.dim <= 64
    for M in MS:
        _check_all_weights(t, mn, new, M, Dc + M, f"hier {family} Dc={Dc} J={J} m={m} M={M}")
    _report(f"hier {family} Dc={Dc}")


# K = 2, 3, 16 and Dc on both sides of the row capacities 4 / 8 / 16 / 32 of the categorical walk
@pytest.mark.parametrize("K,Dc,m", [(2, 4, 65), (2, 5, 1), (2, 32, 64), (2, 33, 66), (2, 64, 7), (3, 8, 65), (3, 9, 70),
                                    (3, 16, 64), (3, 17, 3), (3, 32, 65), (16, 1, 65), (16, 4, 130), (8, 9, 65),
                                    (13, 5, 64)])
def test_parity_categorical(K, Dc, m):
    t, mn, new, _ = cat_case(K, Dc, 60, m, 3 * K + Dc)
    for M in MS:
        _check_all_weights(t, mn, new, M, K + Dc + M, f"cat K={K} Dc={Dc} m={m} M={M}")
    _report(f"cat K={K} Dc={Dc}")


# K = 3, 10 and K > 16 (no prob); p on both sides of the row capacities 16 / 32; K = 65 at p = 0 is the model's limit
# and the largest LDS area any predict kernel asks for (2 (K - 1) x 512 B = 65 536 B)
@pytest.mark.parametrize("K,p,m", [(3, 0, 65), (3, 3, 1), (3, 16, 65), (3, 17, 64), (3, 33, 7), (3, 62, 66), (10, 2, 65),
                                   (10, 16, 70), (10, 17, 64), (10, 55, 65), (16, 5, 65), (17, 5, 65), (20, 45, 64),
                                   (64, 1, 65), (65, 0, 65), (2, 4, 65)])
def test_parity_ordinal(K, p, m):
    t, mn, new, _ = ord_case(K, p, 80, m, 5 * K + p)
    for M in MS:
        _check_all_weights(t, mn, new, M, K + p + M, f"ord K={K} p={p} m={m} M={M}")
    got = t.predict(points(mn, 5, 1), new[0])
    assert (got.prob is None) == (K > 16) and got.mean_i is not None and got.var_i is None
    _report(f"ord K={K} p={p}")


@pytest.mark.parametrize("family", ["poisson_log", "neg_binomial_2_log"])
def test_inf_and_nan_rules(family):
    """One positive-weight particle whose e^eta overflows in some rows: its term is -inf there (counted, lpd finite) and
    its mean is not finite (the row's mean and variance are NaN); the other rows are unaffected."""
    from smcnuts_amd import GLMTarget
    X, y = pw.synthetic(family, 90, 2, 5)
    Xn, yn = pw.synthetic(family, 200, 2, 6)
    Xn[:, 0] = np.random.default_rng(6).random(200) < 0.3
    if family == "neg_binomial_2_log":
        t = GLMTarget(X, y, family=family, prior_sd=2.0, intercept=False, dispersion_prior=(0.0, 1.0))
        mn = gd.GLMDispNumpy(Xn, yn, family, 2.0, (0.0, 1.0), intercept=False)
    else:
        t = GLMTarget(X, y, family=family, prior_sd=2.0, intercept=False)
        mn = _glm.GLMNumpy(Xn, yn, family, 2.0, intercept=False)
    x = pw.points(mn, 50, 1)
    x[17, 0], x[17, 1] = 1500.0, 0.0
    lw = np.random.default_rng(3).standard_normal(50)
    got, T, ref, _ = _check(t, mn, (Xn, yn, None), x, lw, f"{family} -inf rule")
    bad = np.isneginf(T["ll"][17])
    assert 10 < np.sum(bad) < 190
    np.testing.assert_array_equal(got.n_inf_i, bad.astype(np.float64))
    assert np.all(np.isfinite(got.lpd_i))
    for k in ("mean_i", "var_i"):
        assert np.all(np.isnan(getattr(got, k)[bad])) and np.all(np.isfinite(getattr(got, k)[~bad]))
    # the same particle with a -inf weight: as if it were not there
    lw2 = lw.copy()
    lw2[17] = -np.inf
    g2 = t.predict(x, Xn, yn, None, lw2)
    g3 = t.predict(np.delete(x, 17, axis=0), Xn, yn, None, np.delete(lw, 17))
    assert np.all(g2.n_inf_i == 0) and np.all(np.isfinite(g2.mean_i)) and g2.n_particles == 49
    for k in ("lpd_i", "mean_i", "var_i"):
        np.testing.assert_allclose(getattr(g2, k), getattr(g3, k), rtol=1e-12, atol=1e-300)


@pytest.mark.parametrize("family", pw.FAMILIES)
def test_tie_to_pointwise_at_the_training_rows(family):
    """X_new, y_new = the training data: lpd_i is pointwise()'s lppd_i and mean_i its fitted_i, within both bounds."""
    t, m = pw.make(family, 130, 9, 21)
    x = pw.points(m, 1000, 4)
    lw = 3.0 * np.random.default_rng(8).standard_normal(1000)
    lw[5:900:11] = -np.inf
    ll, e_term, mean, e_mean = pw.terms(m, x)
    _, bp = pw.criteria_bounds(ll, lw, e_term, mean, e_mean)
    pwise = t.pointwise(x, lw)
    T = pr.terms(m, x)
    ref = pr.reference(T, lw)
    b = pr.bounds(T, lw, ref)
    got = t.predict(x, t.X, t.y, None, lw)
    pr.assert_prediction(got, ref, b, what=f"{family} at the training rows", close=close)
    d1, d2 = np.abs(got.lpd_i - pwise.lppd_i), np.abs(got.mean_i - pwise.fitted_i)
    assert np.all(d1 <= b["lpd_i"] + bp["lppd_i"]), f"lpd_i vs lppd_i: {np.max(d1):.3e}"
    assert np.all(d2 <= b["mean_i"] + bp["fitted_i"]), f"mean_i vs fitted_i: {np.max(d2):.3e}"
    close(got.lpd_i, pwise.lppd_i, rtol=0.0, atol=float(np.max(b["lpd_i"] + bp["lppd_i"])), what="lpd_i against lppd_i")
    close(got.mean_i, pwise.fitted_i, rtol=0.0, atol=float(np.max(b["mean_i"] + bp["fitted_i"])),
          what="mean_i against fitted_i")


def _train_cases():
    return [("glm bernoulli", lambda: glm_case("bernoulli_logit", 9, 150, 5, 1), _glm.device_bounds),
            ("glm poisson", lambda: glm_case("poisson_log", 20, 150, 5, 2), _glm.device_bounds),
            ("glm normal", lambda: glm_case("normal", 6, 150, 5, 3), gd.device_bounds),
            ("glm nb", lambda: glm_case("neg_binomial_2_log", 24, 150, 5, 4), gd.device_bounds),
            ("hier poisson", lambda: hier_case("poisson_log", 5, 8, 150, 5, 5), _hglm.device_bounds),
            ("hier normal", lambda: hier_case("normal", 18, 6, 150, 5, 6), _hglm.device_bounds),
            ("cat", lambda: cat_case(5, 6, 150, 5, 7), _cat.device_bounds),
            ("ord", lambda: ord_case(6, 7, 150, 5, 8), _ord.device_bounds)]


@pytest.mark.parametrize("name,mk,dev_bounds", _train_cases(), ids=[c[0] for c in _train_cases()])
def test_row_sums_at_the_training_rows_are_the_density(name, mk, dev_bounds):
    """predict_loglik at the training data: its row sums are the llik of smcn_target_eval, within the terms' bounds plus
    the density tests' bound of llik (which holds the summation's share).  The ordinal density sums the middle classes'
    log(1 - e^-delta) as count x term, the matrix per row: the bound of the terms covers both."""
    t, _, _, mt = mk()
    x = points(mt, 200, 3)
    groups = t.groups if hasattr(t, "groups") else None
    got = t.predict_loglik(x, t.X, t.y, groups)
    T = pr.terms(mt, x)
    pr.assert_loglik(got, T, what=name)
    llik = t.logpdf_parts(x)[1]
    rows = np.all(np.isfinite(T["ll"]), axis=1)
    assert np.all(np.isneginf(llik[~rows])), name
    rows &= np.isfinite(llik)
    with np.errstate(all="ignore"):
        b = np.sum(np.where(np.isfinite(T["ll"]), T["e_ll"], 0.0), axis=1) + dev_bounds(mt, x)[1]
    s = np.array([math.fsum(r.tolist()) for r in got[rows]])
    assert np.sum(rows) > 100
    assert np.all(np.abs(s - llik[rows]) <= b[rows]), f"{name}: {np.max(np.abs(s - llik[rows]) - b[rows]):.3e}"
    close(s, llik[rows], rtol=0.0, atol=float(np.max(b[rows])), what="row sums of predict_loglik against llik")


RESIDENT = [("glm nb", lambda: glm_case("neg_binomial_2_log", 12, 150, 77, 4)),
            ("hier bernoulli", lambda: hier_case("bernoulli_logit", 4, 6, 150, 77, 5)),
            ("cat", lambda: cat_case(4, 3, 150, 77, 7)),
            ("ord", lambda: ord_case(5, 3, 150, 77, 8))]


def _same_bits(a, b, what):
    for k in pr.FIELDS + ("n_inf_i",):
        u, v = getattr(a, k), getattr(b, k)
        assert (u is None) == (v is None), f"{what} {k}"
        if u is not None:
            np.testing.assert_array_equal(u, v, err_msg=f"{what} {k}: not the same bits")
    assert a.n_particles == b.n_particles and a.ess == b.ess


@pytest.mark.parametrize("name,mk", RESIDENT, ids=[c[0] for c in RESIDENT])
def test_resident_path(name, mk):
    from smcnuts_amd import SMCSampler
    t, mn, new, _ = mk()
    smc = SMCSampler(K=6, N=4096, target=t, step_size=0.05, seed=5)
    with pytest.raises(RuntimeError, match="sample"):
        smc.predict(new[0], new[1], new[2])
    smc.sample(show_progress=False)
    got = smc.predict(new[0], new[1], new[2])
    _same_bits(smc.predict(new[0], new[1], new[2]), got, f"{name} repeated call")
    x, lw = smc.samples.ctx.get_state()[:2]
    _same_bits(t.predict(x, new[0], new[1], new[2], lw), got, f"{name} resident against uploaded")
    T = pr.terms(mn, x)
    ref = pr.reference(T, lw)
    pr.assert_prediction(got, ref, pr.bounds(T, lw, ref), what=f"{name} resident against the reference", close=close)
    # without y_new
    g0 = smc.predict(new[0], None, new[2])
    assert g0.lpd_i is None


def test_mergeability_and_repeatability():
    from smcnuts_amd.predict import combine_predict_partials
    for name, mk in RESIDENT:
        t, mn, new, _ = mk()
        kind, K = pr.kind_of(mn), getattr(mn, "K", 0)
        x = points(mn, 1000, 4)
        lw = 3.0 * np.random.default_rng(8).standard_normal(1000)
        lw[5:900:11] = -np.inf
        whole = t.predict_partials(x, new[0], new[1], new[2], lw)
        np.testing.assert_array_equal(whole, t.predict_partials(x, new[0], new[1], new[2], lw))
        T = pr.terms(mn, x)
        ref = pr.reference(T, lw)
        b = pr.bounds(T, lw, ref)
        for split in [(1, 999), (64, 936), (333, 333, 334)]:
            parts, m0 = [], 0
            for k in split:
                parts.append(t.predict_partials(x[m0:m0 + k], new[0], new[1], new[2], lw[m0:m0 + k]))
                m0 += k
            pr.assert_prediction(combine_predict_partials(parts, kind, K, True), ref, b, factor=2.0,
                                 what=f"{name} split {split}")


def test_resident_two_shards():
    from smcnuts_amd import SMCSampler
    from tests.test_sharding import _run_shards
    for name, mk in (RESIDENT[1], RESIDENT[3]):
        t, mn, new, _ = mk()
        kw = dict(K=4, N=2048, step_size=0.05, seed=3)
        one = SMCSampler(target=t, **kw)
        one.sample(show_progress=False)
        ref1 = one.predict(new[0], new[1], new[2])
        x, lw = one.samples.ctx.get_state()[:2]
        T = pr.terms(mn, x)
        ref = pr.reference(T, lw)
        b = pr.bounds(T, lw, ref)
        out = {}

        def drive(s):
            s.sample(show_progress=False)
            out[s.comm.rank] = s.predict(new[0], new[1], new[2])

        _run_shards(lambda c: SMCSampler(target=mk()[0], comm=c, **kw), 2, drive, device=True)
        assert sorted(out) == [0, 1]
        as_ref = {k: np.asarray(getattr(ref1, k)) for k in pr.FIELDS if getattr(ref1, k) is not None}
        for r in (0, 1):
            assert out[r].n_particles == ref1.n_particles
            pr.assert_prediction(out[r], as_ref, b, factor=2.0, what=f"{name} rank {r} of two against one shard")
        _same_bits(out[0], out[1], f"{name}: the two ranks")


def test_resident_errors():
    from smcnuts_amd import GaussianTarget, SMCSampler
    from smcnuts_amd._capi import SmcnError
    t, _, new, _ = glm_case("bernoulli_logit", 5, 100, 9, 2)
    asym = SMCSampler(K=3, N=1024, target=t, step_size=0.05, seed=1, lkernel="asymptoticLKernel", tempering=True)
    asym.sample(show_progress=False)
    with pytest.raises(NotImplementedError, match="asymptotic"):
        asym.predict(new[0], new[1])
    early = SMCSampler(K=1, N=1024, target=glm_case("bernoulli_logit", 5, 100, 9, 2)[0], step_size=0.05, seed=1,
                       lkernel="GaussianApproxLKernel", tempering=True)
    early.sample(show_progress=False)
    assert early.phi[-1] < 1.0
    with pytest.raises(RuntimeError, match="temperature"):
        early.predict(new[0], new[1])
    with pytest.raises(ValueError, match="columns"):
        early.predict(new[0][:, :2], new[1])
    g = SMCSampler(K=2, N=1024, target=GaussianTarget(3), step_size=0.3, seed=1)
    g.sample(show_progress=False)
    with pytest.raises(NotImplementedError, match="GLMTarget"):
        g.predict(np.zeros((2, 3)))
    # the C entry points of a context of another model fail with a message that names the supported ones
    ctx = g.samples.ctx
    with pytest.raises(SmcnError, match="SMCN_MODEL_HGLM"):
        ctx.predict_set_data(np.zeros(8), True)
    with pytest.raises(SmcnError, match="SMCN_MODEL_ORDINAL"):
        ctx.predict_dims()
    with pytest.raises(SmcnError, match="SMCN_MODEL_GLM"):
        ctx.call("smcn_predict_partials", None, None, 1024, None)
    with pytest.raises(SmcnError, match="SMCN_MODEL_CATEGORICAL"):
        ctx.call("smcn_predict_loglik", None, 1, None)
    # a supported context before smcn_predict_set_data, and a block the C side refuses
    done = SMCSampler(K=2, N=1024, target=t, step_size=0.05, seed=1)
    done.sample(show_progress=False)
    with pytest.raises(SmcnError, match="smcn_predict_set_data first"):
        done.samples.ctx.predict_partials()
    with pytest.raises(SmcnError, match="header"):
        done.samples.ctx.predict_set_data(np.array([1.0, 2, 4, 1, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2]), True)
    with pytest.raises(SmcnError, match="finite"):
        done.samples.ctx.predict_set_data(np.array([0.0, 1, 4, 1, 0, 1, np.nan, 1, 1]), True)
    done.samples.ctx.predict_set_data(np.array([0.0, 1, 4, 1, 0, 1, 1, 1, 1]), False)
    with pytest.raises(SmcnError, match="without y"):
        done.samples.ctx.predict_loglik(np.zeros((1, 5)))


def test_full_size():
    """N = 65 536, m = 10 000, D = 25, logistic: against the NumPy reference in chunks of 64 rows.  The inputs are chosen
    so that the reference has no -inf term and no NaN row (asserted), so no row can pass by being skipped."""
    from smcnuts_amd import GLMTarget
    N, m, D = 65536, 10000, 25
    X, y = _glm.synthetic("bernoulli_logit", 500, D - 1, 76, scale=0.5)
    Xn, yn = _glm.synthetic("bernoulli_logit", m, D - 1, 77, scale=0.5)
    sd = np.linspace(0.8, 2.5, D)
    t = GLMTarget(X, y, family="bernoulli_logit", prior_sd=sd)
    rng = np.random.default_rng(5)
    x = 0.3 * rng.standard_normal((N, D))
    lw = 3.0 * rng.standard_normal(N)
    t.predict(x[:256], Xn, yn, None, lw[:256])                   # (context, staging buffers)
    t0 = time.perf_counter()
    got = t.predict(x, Xn, yn, None, lw)
    t_dev = time.perf_counter() - t0
    assert np.all(got.n_inf_i == 0)
    for k in ("lpd_i", "mean_i", "var_i"):
        assert getattr(got, k).shape == (m,) and np.all(np.isfinite(getattr(got, k))), k
    t0 = time.perf_counter()
    used = {}
    for i0 in range(0, m, 64):
        sl = slice(i0, min(m, i0 + 64))
        mn = _glm.GLMNumpy(Xn[sl], yn[sl], "bernoulli_logit", sd)
        T = pr.terms(mn, x)
        assert np.all(np.isfinite(T["ll"])) and np.all(np.isfinite(T["mean"])) and np.all(np.isfinite(T["var"]))
        ref = pr.reference(T, lw)
        for k in ("lpd_i", "mean_i", "var_i"):
            assert np.all(np.isfinite(ref[k])), f"the reference's {k} has a non-finite entry in rows {i0}.."
        assert np.all(ref["n_inf_i"] == 0)

        class Part:
            prob = None

        part = Part()
        for k in ("lpd_i", "mean_i", "var_i", "n_inf_i"):
            setattr(part, k, getattr(got, k)[sl])
        pr.assert_prediction(part, ref, pr.bounds(T, lw, ref), what=f"full size, rows {i0}..", report=used)
    t_ref = time.perf_counter() - t0
    print(f"full size: device {t_dev * 1e3:.1f} ms (upload and download included), NumPy reference {t_ref:.1f} s; "
          f"largest share of the bound used: { {k: round(v, 4) for k, v in used.items()} }")
