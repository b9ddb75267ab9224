"""Posterior predictive draws of the five device regression targets against the NumPy restatement of
tests/_predict_draws.py, fed the device's own ancestors.  Discrete outcomes are EQUAL wherever no comparison of the
restatement is ambiguous (its module docstring derives the bounds); ambiguous draws are left out, at most
max(2, 1e-4 S m) per call (asserted).  Normal outcomes lie within their per-element bound, recorded through _tol.close.

Figures of the first run on an MI355X are in DESIGN.md 4.4 (Posterior predictive draws)."""
import math

import numpy as np
import pytest

import _glm_disp as gd
import _hglm
import _ord
import _pointwise as pw
import _predict as pr
import _predict_draws as dr
from _tol import close
from test_gpu_predict import cat_case, glm_case, hier_case, ord_case, points

pytestmark = pytest.mark.gpu
COUNT = ("poisson_log", "neg_binomial_2_log")


def spread_points(mn, M, seed):
    """tests/test_gpu_predict.py's points; for the count families every other particle is scaled up, so that mu covers
    the inversion (below 10) and the PTRS branch (far above) of the Poisson sampler."""
    x = points(mn, M, seed)
    if getattr(mn, "family", "") in COUNT:
        Dc = mn.Z.shape[1]
        x[1::2, :Dc] *= 6.0
    return x


def check_ancestors(got, lw, M, S, seed, what):
    a, amb = dr.ancestors(lw, M, S, seed)
    assert amb.sum() <= max(2, 1e-4 * S), f"{what}: {amb.sum()} ambiguous slots"
    np.testing.assert_array_equal(got[~amb], a[~amb], err_msg=f"{what}: ancestors")
    if lw is not None:
        assert np.all(np.isfinite(np.asarray(lw)[got])), f"{what}: an ancestor without a finite log-weight"
    return int(amb.sum())


def check_draws(got, mn, x, seed, what, labels=None, s_first=0, anc=None):
    """got.y against the restatement on got.ancestors -> (ambiguous draws, NaN draws)."""
    y, amb, e_y = dr.model_draws(mn, x, got.ancestors if anc is None else anc, seed, labels, s_first)
    gy = got.y
    assert gy.shape == y.shape, what
    assert amb.sum() <= max(2, 1e-4 * y.size), f"{what}: {amb.sum()} ambiguous draws of {y.size}"
    ok = ~amb
    np.testing.assert_array_equal(np.isnan(gy)[ok], np.isnan(y)[ok], err_msg=f"{what}: NaN pattern")
    fin = ok & ~np.isnan(y)
    if getattr(mn, "family", "") == "normal":
        bad = np.abs(gy - y)[fin] > e_y[fin]
        assert not bad.any(), f"{what}: {bad.sum()} normal draws beyond their bound, worst share " \
                              f"{np.max(np.abs(gy - y)[fin] / e_y[fin])}"
        close(gy[fin], y[fin], rtol=0.0, atol=float(np.max(e_y[fin], initial=1e-300)), what="normal draws (largest element bound)")
    else:
        np.testing.assert_array_equal(gy[fin], y[fin], err_msg=f"{what}: draws")
    assert got.n_bad == int(np.isnan(gy).sum()) and got.n_draws == gy.shape[0]
    return int(amb.sum()), int(np.isnan(gy).sum())


def weight_sets(M, seed):
    rng = np.random.default_rng(seed)
    lw = 3.0 * rng.standard_normal(M)
    out = [("random", lw), ("equal", None), ("spread", lw + np.where(np.arange(M) % 2 == 0, 1.0e5, -1.0e5))]
    if M > 1:
        lw3 = lw.copy()
        lw3[::3] = -np.inf
        lw3[-1] = -np.inf
        out.append(("some -inf", lw3))
    return out


def run_case(t, mn, new, S, M, seed, what, labels=None):
    x = spread_points(mn, M, seed)
    gl = new[2] if labels is None else labels
    tot = [0, 0]
    for name, lw in weight_sets(M, seed):
        got = t.predict_draws(x, new[0], S, seed=seed, groups_new=gl, logw=lw)
        check_ancestors(got.ancestors, lw, M, S, seed, f"{what} {name}")
        a, b = check_draws(got, mn, x, seed, f"{what} {name}", labels)
        tot[0] += a
        tot[1] += b
    print(f"{what}: ambiguous draws left out {tot[0]}, NaN draws {tot[1]}")


SHAPES = [(1, 1), (63, 65), (65, 700), (200, 65), (63, 700), (65, 65), (200, 700)]       # (S, M) per case below


@pytest.mark.parametrize("family", pw.FAMILIES)
@pytest.mark.parametrize("k,D,m", [(0, 2, 1), (1, 3, 65), (2, 16, 130), (3, 17, 64), (4, 32, 7), (5, 33, 65), (6, 64, 70)])
def test_glm(family, k, D, m):
    t, mn, new, _ = glm_case(family, D, 40, m, 10 * D + m)
    S, M = SHAPES[k]
    run_case(t, mn, new, S, M, 100 + D, f"{family} D={D} m={m} S={S} M={M}")


@pytest.mark.parametrize("family", _hglm.FAMILIES)
@pytest.mark.parametrize("k,Dc,J,m", [(1, 0, 3, 65), (0, 3, 4, 1), (2, 16, 10, 130), (3, 17, 33, 64), (4, 32, 5, 7),
                                      (5, 33, 28, 65), (6, 40, 22, 70)])
def test_hierarchical(family, k, Dc, J, m):
    t, mn, new, _ = hier_case(family, Dc, J, 50, m, 7 * Dc + J)
    S, M = SHAPES[k]
    run_case(t, mn, new, S, M, 200 + Dc, f"hier {family} Dc={Dc} J={J} m={m} S={S} M={M}")


@pytest.mark.parametrize("k,K,Dc,m", [(0, 2, 4, 1), (2, 16, 4, 130), (1, 13, 5, 64), (3, 8, 9, 65), (4, 3, 17, 3),
                                      (5, 2, 33, 66), (6, 2, 64, 7)])
def test_categorical(k, K, Dc, m):
    t, mn, new, _ = cat_case(K, Dc, 60, m, 3 * K + Dc)
    S, M = SHAPES[k]
    run_case(t, mn, new, S, M, 300 + K + Dc, f"cat K={K} Dc={Dc} m={m} S={S} M={M}")


@pytest.mark.parametrize("k,K,p,m", [(0, 3, 0, 1), (1, 3, 16, 65), (2, 16, 5, 130), (3, 17, 17, 64), (4, 3, 33, 7),
                                     (5, 65, 0, 65), (6, 10, 55, 70)])
def test_ordinal(k, K, p, m):
    t, mn, new, _ = ord_case(K, p, 80, m, 5 * K + p)
    S, M = SHAPES[k]
    run_case(t, mn, new, S, M, 400 + K + p, f"ord K={K} p={p} m={m} S={S} M={M}")


# ---- extreme parameters, through chosen ancestors ------------------------------------------------------------------------
def _intercept_only(family, m=70):
    """eta_i = b_0 for every row (X_new = 0): the particle's first coordinate IS eta."""
    from smcnuts_amd import GLMTarget
    import _glm
    X, y = pw.synthetic(family, 30, 1, 3)
    Xn = np.zeros((m, 1))
    if family in gd.DISP_FAMILIES:
        t = GLMTarget(X, y, family=family, prior_sd=[2.0, 2.0], intercept=True, dispersion_prior=(0.0, 1.0))
        mn = gd.GLMDispNumpy(Xn, np.zeros(m), family, np.array([2.0, 2.0]), (0.0, 1.0), intercept=True)
    else:
        t = GLMTarget(X, y, family=family, prior_sd=[2.0, 2.0], intercept=True)
        mn = _glm.GLMNumpy(Xn, np.zeros(m), family, np.array([2.0, 2.0]), intercept=True)
    return t, mn, Xn


@pytest.mark.parametrize("family", pw.FAMILIES)
def test_extreme_parameters(family):
    t, mn, Xn = _intercept_only(family)
    m = Xn.shape[0]
    etas = [800.0, -800.0, 40.0, math.log(1.0e6), math.log(1.0e9), 2.0, np.nan, 0.5]
    rows = []
    if family in gd.DISP_FAMILIES:
        taus = [0.3, math.log(1.0e-300), math.log(1.0e8), 710.0, -400.0, -709.0, -0.7]
        for e in etas:
            for ta in taus:
                rows.append([e, 0.3, ta])
    else:
        rows = [[e, 0.3] for e in etas]
    x = np.array(rows)
    S = x.shape[0]
    got = t.predict_draws(x, Xn, S, seed=9, ancestors=np.arange(S))
    np.testing.assert_array_equal(got.ancestors, np.arange(S))
    amb, nbad = check_draws(got, mn, x, 9, f"{family} extremes")
    y = got.y.reshape(len(etas), -1, m)
    assert np.all(np.isnan(y[6])), "a non-finite coordinate: every draw of that ancestor is NaN"
    if family == "bernoulli_logit":
        assert np.all(y[0] == 1.0) and np.all(y[1] == 0.0)
    elif family == "poisson_log":
        assert np.all(np.isnan(y[0])) and np.all(y[1] == 0.0) and np.all(np.isnan(y[2]))     # e^800, e^-800, mu > 2^53
        assert abs(np.mean(y[4]) / 1.0e9 - 1.0) < 6.0 / math.sqrt(1.0e9 * m)
    elif family == "neg_binomial_2_log":
        assert np.all(np.isnan(y[0])) and np.all(y[1][:3] == 0.0) and np.all(np.isnan(y[2]))
        assert np.all(np.isnan(y[:, 3])) and np.all(np.isnan(y[:, 5]))        # e^tau overflows / leaves the normal range
        assert not np.any(np.isnan(y[3, :3])) and not np.any(np.isnan(y[5, :3]))
    else:
        assert np.all(np.isnan(y[:, [1, 3, 4, 5]]))                            # e^tau or e^-2tau overflows
        assert not np.any(np.isnan(y[[0, 1, 2, 3, 4, 5, 7]][:, [0, 2]]))
    print(f"{family} extremes: ambiguous {amb}, NaN {nbad} of {got.y.size}")


def test_extreme_ordinal_and_categorical():
    t, mn, new, _ = ord_case(5, 2, 60, 66, 4)
    x = spread_points(mn, 8, 2)
    x[0, mn.p + 1:] = -800.0            # collapsed cutpoints: e^u = 0
    x[1, mn.p + 2] = 800.0              # a cutpoint overflows: NaN
    x[2, 0] = np.nan
    x[3, :mn.p] = 400.0                 # |eta| up to 800 and beyond
    x[4, :mn.p] = -400.0
    got = t.predict_draws(x, new[0], 8, seed=3, ancestors=np.arange(8))
    check_draws(got, mn, x, 3, "ordinal extremes")
    assert np.all(np.isnan(got.y[1])) and np.all(np.isnan(got.y[2])) and got.n_bad == 2 * 66
    assert set(np.unique(got.y[0])) <= {0.0, 1.0, 4.0}, "collapsed cutpoints leave the middle classes empty"
    t, mn, new, _ = cat_case(4, 3, 60, 65, 6)
    x = spread_points(mn, 6, 2)
    x[0] *= 300.0
    x[1, 1] = np.inf
    x[2, 2] = np.nan
    got = t.predict_draws(x, new[0], 6, seed=3, ancestors=np.arange(6))
    check_draws(got, mn, x, 3, "categorical extremes")
    assert np.all(np.isnan(got.y[2])) and got.n_bad >= 65


# ---- new groups ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,Dc,J", [("normal", 3, 4), ("poisson_log", 17, 33), ("neg_binomial_2_log", 2, 40)])
def test_new_groups(family, Dc, J):
    t, mn, new, _ = hier_case(family, Dc, J, 50, 66, 11)
    Xn, _, gn = new
    Xn = Xn.copy()
    Xn[1] = Xn[0]                                            # rows 0, 1: the same row in the same NEW group
    Xn[3] = Xn[2]                                            # rows 2, 3: the same row in two different new groups
    labels = gn.copy()
    labels[[0, 1]] = J + 5
    labels[2], labels[3] = J, 2 ** 32 - 1
    labels[10:20] = J + 5
    ic = bool(Dc % 2) and Dc >= 1
    g0 = np.where(labels < J, labels, 0)
    mn2 = _hglm.HGLMNumpy(Xn, np.zeros(66), g0, family, np.linspace(0.8, 2.5, Dc), 1.5, (0.0, 1.0), intercept=ic, n_groups=J)
    S, M, seed = 65, 65, 21
    x = spread_points(mn2, M, 5)
    got = t.predict_draws(x, Xn, S, seed=seed, groups_new=labels)
    check_draws(got, mn2, x, seed, f"new groups {family}", labels)
    # labels below J: exactly the fitted groups' draws, bit for bit, in the rows that keep their group
    plain = t.predict_draws(x, Xn, S, seed=seed, groups_new=g0)
    keep = labels < J
    np.testing.assert_array_equal(got.y[:, keep], plain.y[:, keep])
    np.testing.assert_array_equal(got.ancestors, plain.ancestors)
    assert not np.array_equal(got.y[:, ~keep], plain.y[:, ~keep], equal_nan=True)
    if family == "normal":
        # y - sigma z_outcome = eta: rows 0 and 1 share X and the group, so they share eta within a draw; rows 2 and 3
        # are in different new groups, and one group's intercept differs from draw to draw
        s, i = np.arange(S)[:, None], np.arange(66)[None, :]
        z, _ = dr.box_muller(dr.philox_uniform(seed, s, i, dr.ST_OUT, 0), dr.philox_uniform(seed, s, i, dr.ST_OUT, 1))
        sig = np.exp(x[got.ancestors, -1])[:, None]
        eta = got.y - sig * z
        tol = 1e-9 * (1.0 + np.abs(eta[:, 0]))
        assert np.all(np.abs(eta[:, 0] - eta[:, 1]) <= tol), "rows of one new group share its intercept"
        assert np.all(np.abs(eta[:, 2] - eta[:, 3]) > 1e-6), "different new groups have different intercepts"
        fixed = x[got.ancestors, :Dc] @ mn2.Z[0]
        alpha = eta[:, 0] - fixed
        assert np.unique(np.round(alpha, 6)).size == S, "a new group's intercept is drawn afresh in every draw"


# ---- independence of the schedule ----------------------------------------------------------------------------------------
def test_repeat_and_slot_ranges():
    for mk in (lambda: glm_case("neg_binomial_2_log", 17, 40, 70, 3), lambda: hier_case("poisson_log", 3, 4, 50, 65, 4),
               lambda: cat_case(5, 6, 60, 65, 6), lambda: ord_case(17, 3, 80, 65, 8)):
        t, mn, new, _ = mk()
        M, S, seed = 300, 200, 77
        x = spread_points(mn, M, 1)
        lw = 2.0 * np.random.default_rng(2).standard_normal(M)
        full = t.predict_draws(x, new[0], S, seed=seed, groups_new=new[2], logw=lw)
        again = t.predict_draws(x, new[0], S, seed=seed, groups_new=new[2], logw=lw)
        np.testing.assert_array_equal(full.y, again.y)
        np.testing.assert_array_equal(full.ancestors, again.ancestors)
        ctx = t._context(M)
        for s0, n in [(0, 1), (63, 65), (137, 63), (199, 1)]:
            y, anc, nbad = ctx.predict_draws(S, seed, x, lw, s_first=s0, s_count=n)
            np.testing.assert_array_equal(y, full.y[s0:s0 + n])
            np.testing.assert_array_equal(anc, full.ancestors[s0:s0 + n])
            assert nbad == int(np.isnan(y).sum())
        # S itself only moves the ancestors: with the ancestors given, the draws of slot s do not depend on S
        part = t.predict_draws(x, new[0], 70, seed=seed, groups_new=new[2], ancestors=full.ancestors[:70])
        np.testing.assert_array_equal(part.y, full.y[:70])


def test_capi_argument_checks():
    from smcnuts_amd._capi import SmcnError
    from smcnuts_amd import GaussianTarget
    t, mn, new, _ = glm_case("poisson_log", 3, 40, 5, 3)
    x = spread_points(mn, 4, 1)
    ctx = t._context(4)
    with pytest.raises(SmcnError, match="smcn_predict_set_data first"):
        ctx.predict_draws(3, 0, x)
    ctx.predict_set_data(t._predict_block(new[0])[0], False)
    for kw, msg in [(dict(s_first=2, s_count=2), "slot range"), (dict(s_first=0, s_count=0), "slot range"),
                    (dict(ancestors=np.array([0, 4, 1])), r"ancestors\[1\]"),
                    (dict(new_group=np.zeros(5, dtype=np.int64)), "SMCN_MODEL_HGLM only")]:
        with pytest.raises(SmcnError, match=msg):
            ctx.predict_draws(3, 0, x, **kw)
    with pytest.raises(SmcnError, match="number of draws"):
        ctx.predict_draws(0, 0, x, s_first=0, s_count=0)
    with pytest.raises(SmcnError, match="no particle has a finite log-weight"):
        ctx.predict_draws(3, 0, x, np.full(4, -np.inf))
    assert ctx.predict_draws_last_ms() >= 0.0
    with pytest.raises(SmcnError, match="held-out prediction covers the regression targets"):
        GaussianTarget(3)._context(4).call("smcn_predict_draws", None, None, 4, 3, 0, None, None, 0, 3, None, None, None)


# ---- through the sampler -------------------------------------------------------------------------------------------------
def _sampler_cases():
    return [("logistic", lambda: glm_case("bernoulli_logit", 5, 200, 9, 2)),
            ("hier poisson", lambda: hier_case("poisson_log", 3, 6, 150, 11, 3))]


@pytest.mark.parametrize("name,mk", _sampler_cases(), ids=[c[0] for c in _sampler_cases()])
def test_through_the_sampler(name, mk):
    from smcnuts_amd import SMCSampler
    t, mn, new, mt = mk()
    smc = SMCSampler(K=6, N=4096, target=t, step_size=0.05, seed=5)
    with pytest.raises(RuntimeError, match="sample"):
        smc.predict_draws(new[0], groups_new=new[2])
    smc.sample(show_progress=False)
    S = 4000
    d = smc.predict_draws(new[0], n_draws=S, seed=12, groups_new=new[2])
    p = smc.predict(new[0], None, new[2])
    assert d.n_bad == 0 and d.y.shape == (S, new[0].shape[0])
    dev = np.abs(d.y.mean(0) - p.mean_i) / np.sqrt(p.var_i / S)
    print(f"{name}: |mean of draws - predict().mean_i| in standard errors: {np.round(dev, 2)}")
    assert np.all(dev <= 6.0)
    # the resident path against the uploaded one, and against the restatement
    x, lw = smc.samples.ctx.get_state()[:2]
    up = t.predict_draws(x, new[0], S, seed=12, groups_new=new[2], logw=lw)
    np.testing.assert_array_equal(up.y, d.y)
    np.testing.assert_array_equal(up.ancestors, d.ancestors)
    check_ancestors(d.ancestors, lw, x.shape[0], S, 12, name)
    check_draws(d, mn, x, 12, f"{name} resident")
    # X_new = None: the training rows
    a = smc.predict_draws(n_draws=50, seed=4)
    b = smc.predict_draws(t.X, n_draws=50, seed=4, groups_new=getattr(t, "groups", None))
    np.testing.assert_array_equal(a.y, b.y)
    assert a.y.shape == (50, t.X.shape[0])
    lo, hi = d.interval(0.9)
    assert np.all(lo <= d.mean()) and np.all(d.mean() <= hi)
    assert 0.0 <= d.pvalue(np.max, new[1]) <= 1.0
    # seed=None: a fresh seed per call
    assert not np.array_equal(smc.predict_draws(new[0], 50, groups_new=new[2]).y, smc.predict_draws(new[0], 50, groups_new=new[2]).y)


def test_sampler_preconditions():
    from smcnuts_amd import SMCSampler
    t, _, new, _ = glm_case("bernoulli_logit", 5, 100, 9, 2)
    early = SMCSampler(K=1, N=1024, target=t, step_size=0.05, seed=1, lkernel="GaussianApproxLKernel", tempering=True)
    early.sample(show_progress=False)
    assert early.phi[-1] < 1.0
    with pytest.raises(RuntimeError, match="temperature"):
        early.predict_draws(new[0])
    with pytest.raises(RuntimeError, match="temperature"):
        early.predict(new[0])
    with pytest.raises(ValueError, match="columns"):
        early.predict_draws(new[0][:, :2])
    asy = SMCSampler(K=3, N=512, target=t, step_size=0.05, seed=1, lkernel="asymptoticLKernel")
    with pytest.raises(NotImplementedError, match="asymptotic"):
        asy.predict_draws(new[0])


def test_two_shards():
    """Two in-process shards draw their own slots of the one comb: the assembled y equals, bit for bit, the one-shard
    draws from the same particles wherever the ancestors agree (outside the ambiguous slots they do)."""
    from smcnuts_amd import SMCSampler
    from tests.test_sharding import _run_shards
    for mk in (lambda: glm_case("poisson_log", 5, 200, 66, 2), lambda: hier_case("normal", 3, 6, 150, 11, 3)):
        t, mn, new, _ = mk()
        kw = dict(K=4, N=2048, step_size=0.05, seed=3)
        out, S, seed = {}, 333, 19

        def drive(s):
            s.sample(show_progress=False)
            out[s.comm.rank] = (s.predict_draws(new[0], n_draws=S, seed=seed, groups_new=new[2]),) + s.samples.ctx.get_state()[:2]

        _run_shards(lambda c: SMCSampler(target=mk()[0], comm=c, **kw), 2, drive, device=True)
        assert sorted(out) == [0, 1]
        np.testing.assert_array_equal(out[0][0].y, out[1][0].y)
        np.testing.assert_array_equal(out[0][0].ancestors, out[1][0].ancestors)
        x, lw = np.concatenate([out[0][1], out[1][1]]), np.concatenate([out[0][2], out[1][2]])
        one = t.predict_draws(x, new[0], S, seed=seed, groups_new=new[2], logw=lw)
        namb = check_ancestors(out[0][0].ancestors, lw, x.shape[0], S, seed, "two shards")
        same = one.ancestors == out[0][0].ancestors
        assert (~same).sum() <= namb + max(2, 1e-4 * S)
        np.testing.assert_array_equal(out[0][0].y[same], one.y[same])
        assert out[0][0].n_bad == int(np.isnan(out[0][0].y).sum())


def test_bit_for_bit_with_the_parent_of_the_draw_plan():
    """tests/_draws_golden.py: y (NaNs by position), ancestors and n_bad of Context.predict_draws as recorded on an
    MI355X before smcn_predict_draws and smcn_forecast_draws shared their draw plan."""
    import _draws_golden as g
    g.assert_same_as_parent(g.predict_results(), "predict/")
