"""Held-out prediction, host side (no GPU): the argument checks (before any context exists), merging NumPy-built partials
in any split against the unsplit reference within the bounds of tests/_predict.py, the finishing rules for -inf terms
and non-finite weights, compare_heldout, and the row sums of `prob`."""
import numpy as np
import pytest

import _cat
import _glm
import _glm_disp as gd
import _hglm
import _ord
import _predict as pr


def _models(seed=3, m=23):
    """[(name, numpy model at the new rows, points, kind, K)] for the five targets."""
    rng = np.random.default_rng(seed)
    out = []
    for fam in ("bernoulli_logit", "poisson_log"):
        X, y = _glm.synthetic(fam, m, 3, seed)
        mm = _glm.GLMNumpy(X, y, fam, 2.0)
        out.append((fam, mm, 0.4 * rng.standard_normal((37, mm.dim)), "glm", 0))
    for fam in gd.DISP_FAMILIES:
        X, y = gd.synthetic(fam, m, 3, seed)
        mm = gd.GLMDispNumpy(X, y, fam, 2.0, (0.0, 1.0))
        out.append((fam, mm, 0.4 * rng.standard_normal((37, mm.dim)), "glm", 0))
    X, y, g = _hglm.synthetic("poisson_log", m, 2, 4, seed)[:3]
    mm = _hglm.HGLMNumpy(X, y, g, "poisson_log", n_groups=4)
    out.append(("hier", mm, 0.4 * rng.standard_normal((37, mm.dim)), "glm", 0))
    X, y = _cat.synthetic(4, m, 2, seed)
    mm = _cat.CategoricalNumpy(X, y, 4)
    out.append(("cat", mm, np.concatenate([0.5 * rng.standard_normal((29, mm.dim)), _cat.points(mm, rng)]), "cat", 4))
    for K in (5, 18):
        X, y = _ord.synthetic(K, m, 2, seed)
        mm = _ord.OrdinalNumpy(X, y, K)
        x = np.concatenate([np.array([np.concatenate([0.5 * rng.standard_normal(2), [-1.0], 0.3 * rng.standard_normal(K - 2)])
                                      for _ in range(29)]), _ord.points(mm, rng)])
        out.append((f"ord{K}", mm, x, "ord", K))
    return out


MODELS = _models()


@pytest.mark.parametrize("name,m,x,kind,K", MODELS, ids=[v[0] for v in MODELS])
@pytest.mark.parametrize("weights", ["equal", "random", "some -inf"])
def test_merge_in_any_split_equals_reference(name, m, x, kind, K, weights):
    from smcnuts_amd.predict import combine_predict_partials
    rng = np.random.default_rng(11)
    M = x.shape[0]
    lw = None if weights == "equal" else 3.0 * rng.standard_normal(M)
    if weights == "some -inf":
        lw[::4] = -np.inf
    T = pr.terms(m, x)
    ref = pr.reference(T, lw)
    b = pr.bounds(T, lw, ref)
    for cuts in ([], [1], [M // 2], [5, 6, 20], list(range(1, M))):
        edges = [0] + cuts + [M]
        parts = [pr.numpy_partials({k: v[a:z] for k, v in T.items()}, None if lw is None else lw[a:z], kind, K)
                 for a, z in zip(edges[:-1], edges[1:])]
        got = combine_predict_partials(parts, kind, K, True)
        pr.assert_prediction(got, ref, b, factor=1.0, what=f"{name} {weights} cuts={cuts[:4]}")
        assert got.n_particles == ref["n_particles"] and got.n_new == T["ll"].shape[1]
        np.testing.assert_allclose(got.ess, ref["ess"], rtol=1e-12)
        assert got.elpd == float(np.sum(got.lpd_i))
    if "prob" in ref:
        rows = np.sum(got.prob, axis=1)
        fin = np.isfinite(rows)
        assert np.all(np.abs(rows[fin] - 1.0) <= np.sum(b["prob"], axis=1)[fin] + 4 * K * _glm.U)
    else:
        assert got.prob is None or K > 16 or kind == "glm"


def test_ordinal_above_16_classes_has_no_prob():
    from smcnuts_amd.predict import combine_predict_partials, n_cols
    name, m, x, kind, K = MODELS[-1]
    assert K > 16 and n_cols("ord", K) == 5 and n_cols("ord", 16) == 21 and n_cols("cat", 16) == 20
    T = pr.terms(m, x)
    got = combine_predict_partials([pr.numpy_partials(T, None, kind, K)], kind, K, True)
    assert got.prob is None and got.mean_i is not None and got.lpd_i is not None and got.var_i is None


def test_finishing_rules():
    from smcnuts_amd.predict import combine_predict_partials
    M, m = 6, 4
    rng = np.random.default_rng(5)
    T = dict(ll=-np.abs(rng.standard_normal((M, m))), mean=rng.standard_normal((M, m)),
             var=np.abs(rng.standard_normal((M, m))))
    T["ll"][1, 0] = -np.inf                      # a contributing particle's -inf term: adds 0, is counted
    T["ll"][:, 1] = -np.inf                      # every term -inf: lpd = -inf
    T["mean"][2, 2] = np.inf                     # a non-finite mean: NaN mean and variance for that row alone
    T["var"][3, 3] = np.nan
    lw = rng.standard_normal(M)
    lw[4] = -np.inf                              # contributes to nothing, whatever it holds
    T["ll"][4, 2] = -np.inf
    T["mean"][4, 0] = np.nan
    got = combine_predict_partials([pr.numpy_partials(T, lw, "glm")], "glm", 0, True)
    ref = pr.reference(T, lw)
    np.testing.assert_array_equal(got.n_inf_i, [1, 5, 0, 0])
    assert got.lpd_i[1] == -np.inf and np.all(np.isfinite(got.lpd_i[[0, 2, 3]]))
    np.testing.assert_array_equal(np.isnan(got.mean_i), [False, False, True, True])
    np.testing.assert_array_equal(np.isnan(got.var_i), [False, False, True, True])
    assert got.n_particles == 5
    np.testing.assert_allclose(got.lpd_i[[0, 2, 3]], ref["lpd_i"][[0, 2, 3]], rtol=1e-13)
    np.testing.assert_allclose(got.mean_i[:2], ref["mean_i"][:2], rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(got.var_i[:2], ref["var_i"][:2], rtol=1e-12)
    # without y_new: no lpd, the summaries unchanged
    g2 = combine_predict_partials([pr.numpy_partials(T, lw, "glm")], "glm", 0, False)
    assert g2.lpd_i is None and g2.n_inf_i is None and g2.elpd is None and g2.se_elpd is None
    np.testing.assert_array_equal(g2.mean_i, got.mean_i)
    # no contributing particle at all
    g3 = combine_predict_partials([pr.numpy_partials(T, np.full(M, -np.inf), "glm")], "glm", 0, True)
    assert g3.n_particles == 0 and np.all(np.isnan(g3.mean_i)) and np.all(np.isnan(g3.lpd_i))


def test_between_particle_variance_is_not_the_naive_difference():
    """Means near 1e8 with a spread of 1e-4: sum w m^2 - mean^2 loses every digit, the shifted moments none."""
    from smcnuts_amd.predict import combine_predict_partials
    M = 200
    rng = np.random.default_rng(9)
    mean = 1.0e8 + 1.0e-4 * rng.standard_normal((M, 1))
    T = dict(ll=np.zeros((M, 1)), mean=mean, var=np.zeros((M, 1)))
    parts = [pr.numpy_partials({k: v[a:z] for k, v in T.items()}, None, "glm") for a, z in ((0, 70), (70, 71), (71, M))]
    got = combine_predict_partials(parts, "glm", 0, True)
    import _pointwise as pw
    exact = pw.exact_variance(mean[:, 0])
    assert abs(got.var_i[0] - exact) <= 1e-6 * exact
    assert abs(pw.naive_variance(mean[:, 0]) - exact) > 0.5 * exact


def test_compare_heldout():
    from smcnuts_amd import compare_heldout
    from smcnuts_amd.predict import Prediction
    rng = np.random.default_rng(2)
    la, lb = -np.abs(rng.standard_normal(30)), -np.abs(rng.standard_normal(30))
    a = Prediction(None, None, None, la, np.zeros(30), 10, 10.0, 30)
    b = Prediction(None, None, None, lb, np.zeros(30), 10, 10.0, 30)
    c = compare_heldout(a, b)
    d = la - lb
    np.testing.assert_allclose(c["elpd_diff"], np.sum(d), rtol=1e-14)
    np.testing.assert_allclose(c["se_elpd_diff"], np.sqrt(30 * np.var(d, ddof=1)), rtol=1e-14)
    np.testing.assert_allclose(a.se_elpd, np.sqrt(30 * np.var(la, ddof=1)), rtol=1e-14)
    assert c["n_new"] == 30 and compare_heldout(a, a)["elpd_diff"] == 0.0
    short = Prediction(None, None, None, la[:29], np.zeros(29), 10, 10.0, 29)
    with pytest.raises(ValueError, match="different numbers of rows"):
        compare_heldout(a, short)
    with pytest.raises(ValueError, match="y_new"):
        compare_heldout(a, Prediction(None, None, None, None, None, 10, 10.0, 30))


def _targets():
    from smcnuts_amd import CategoricalRegression, GLMTarget, HierarchicalGLM, OrdinalRegression
    rng = np.random.default_rng(0)
    X = rng.standard_normal((12, 3))
    return dict(
        bern=GLMTarget(X, rng.integers(0, 2, 12), family="bernoulli_logit"),
        pois=GLMTarget(X, rng.integers(0, 5, 12), family="poisson_log"),
        norm=GLMTarget(X, rng.standard_normal(12), family="normal"),
        nb=GLMTarget(X, rng.integers(0, 5, 12), family="neg_binomial_2_log"),
        hier=HierarchicalGLM(X, rng.integers(0, 2, 12), rng.integers(0, 3, 12), n_groups=3),
        cat=CategoricalRegression(X, rng.integers(0, 4, 12), n_classes=4),
        ord=OrdinalRegression(X, rng.integers(0, 4, 12), n_classes=4))


def test_argument_checks_raise_before_a_context_exists():
    T = _targets()
    Xn = np.random.default_rng(1).standard_normal((5, 3))
    g = np.array([0, 1, 2, 0, 1])
    x = {k: np.zeros((2, t.dim)) for k, t in T.items()}

    def bad(key, match, X=Xn, y=None, groups="auto", fn="predict"):
        t = T[key]
        groups = (g if key == "hier" else None) if isinstance(groups, str) else groups
        with pytest.raises(ValueError, match=match):
            if fn == "predict":
                t.predict(x[key], X, y, groups)
            else:
                t.predict_loglik(x[key], X, y, groups)
        assert t._ctx is None, f"{key}: a context was created before the check"

    for key in T:
        bad(key, "columns", X=Xn[:, :2])
        Xbad = Xn.copy()
        Xbad[3, 1] = np.nan
        bad(key, "finite", X=Xbad)
        bad(key, "y_new must be a vector", y=np.zeros(4))
        bad(key, "y_new is required", fn="loglik")
    bad("bern", r"\{0, 1\}", y=np.array([0, 1, 2, 0, 1]))
    bad("pois", "poisson_log needs", y=np.array([0, 1, -1, 0, 1]))
    bad("pois", "poisson_log needs", y=np.array([0, 1, 1.5, 0, 1]))
    bad("nb", "neg_binomial_2_log needs", y=np.array([0, 1, -2, 0, 1]))
    bad("norm", "finite y_new", y=np.array([0, 1, np.inf, 0, 1]))
    bad("hier", r"\{0, 1\}", y=np.array([0, 3, 1, 0, 1]))
    for key in ("cat", "ord"):
        bad(key, r"0\.\.3", y=np.array([0, 1, 4, 0, 1]))
        bad(key, r"0\.\.3", y=np.array([0, 1, -1, 0, 1]))
        bad(key, r"0\.\.3", y=np.array([0, 1, 0.5, 0, 1]))
    bad("hier", "groups_new is required", groups=None)
    bad("hier", "unseen groups", groups=np.array([0, 1, 3, 0, 1]))
    bad("hier", "unseen groups", groups=np.array([0, 1, -1, 0, 1]))
    bad("hier", "m = 5 integers", groups=np.array([0, 1]))
    for key in ("bern", "cat", "ord"):
        bad(key, "HierarchicalGLM only", groups=g)


def test_new_rows_block_layout():
    T = _targets()
    Xn = np.arange(6.0).reshape(2, 3)
    b, hy = T["nb"]._predict_block(Xn, [3, 0])
    np.testing.assert_array_equal(b, [3, 2, 3, 1, 3, 0, 0, 1, 2, 3, 4, 5])
    assert hy
    b, hy = T["hier"]._predict_block(Xn, None, [2, 0])
    np.testing.assert_array_equal(b, [0, 2, 3, 1, 3, 0, 0, 2, 0, 0, 1, 2, 3, 4, 5])
    assert not hy
    b, _ = T["cat"]._predict_block(Xn, [3, 1])
    np.testing.assert_array_equal(b[:6], [4, 2, 3, 1, 3, 1])
    b, _ = T["ord"]._predict_block(Xn, [3, 1])
    np.testing.assert_array_equal(b[:5], [4, 2, 3, 3, 1])


def test_sampler_predict_refuses_other_targets():
    from smcnuts_amd.predict import PredictMixin
    from smcnuts_amd import GaussianTarget, HostTarget
    assert not isinstance(GaussianTarget(3), PredictMixin)
    assert not hasattr(HostTarget, "predict_partials")
