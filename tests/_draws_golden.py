"""The cases of tests/golden/draws_parent.npz: what Context.predict_draws and Context.forecast_draws returned (y, ancestors,
n_bad) on an MI355X at the commit BEFORE smcn_predict_draws and smcn_forecast_draws came to share their draw plan
(smcnuts_amd/csrc/smcn_draw_plan.hpp).  The file holds the outputs only; the inputs are generated here from fixed NumPy
seeds, so whoever records and whoever compares computes them alike.

Every case: M = 1030 uploaded particles (two scan tiles, no multiple of 64), logw = 3 N(0, 1) with two -inf entries,
S = 130 slots, the windows (0, 130) and (37, 70).  predict_draws: m = 3 new rows of a GLMTarget (poisson_log, with an
offset), a HierarchicalGLM (one label of a NEW group), a CategoricalRegression (K = 3) and an OrdinalRegression (K = 4),
systematic ancestors.  forecast_draws: ArmaModel on a 12-point series, H = 5, systematic and caller's ancestors."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "draws_parent.npz")
M, S, SEED, H = 1030, 130, 20260, 5
WINDOWS = ((0, 130), (37, 70))


def _population(D, seed):
    rng = np.random.default_rng(seed)
    x = 0.3 * rng.standard_normal((M, D))
    lw = 3.0 * rng.standard_normal(M)
    lw[[5, M - 1]] = -np.inf
    return x, lw


def _design(seed, n=20, p=2):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, p)), rng.standard_normal((3, p)), rng


def predict_targets():
    """name -> (target, X_new, groups_new, offset_new)"""
    from smcnuts_amd.model import targets as T
    out = {}
    X, Xn, rng = _design(1)
    out["glm"] = (T.GLMTarget(X, rng.poisson(2.0, 20).astype(np.float64), family="poisson_log",
                              offset=0.2 * rng.standard_normal(20)), Xn, None, np.array([0.1, -0.2, 0.3]))
    X, Xn, rng = _design(2)
    out["hier"] = (T.HierarchicalGLM(X, rng.integers(0, 2, 20).astype(np.float64), np.arange(20) % 3), Xn,
                   np.array([0, 5, 2]), None)
    X, Xn, rng = _design(3)
    out["cat"] = (T.CategoricalRegression(X, np.arange(20) % 3, n_classes=3), Xn, None, None)
    X, Xn, rng = _design(4)
    out["ord"] = (T.OrdinalRegression(X, np.arange(20) % 4, n_classes=4), Xn, None, None)
    return out


def predict_results():
    """{key: array} of every predict_draws case, from the package that is imported."""
    out = {}
    for k, (name, (t, Xn, groups, offset)) in enumerate(predict_targets().items()):
        x, lw = _population(t.dim, 10 + k)
        block, labels, _, _ = t._draws_args(Xn, S, groups, None, None, offset)
        assert (labels is not None) == (name == "hier")
        ctx = t._context(M)
        ctx.predict_set_data(block, False)
        for s0, n in WINDOWS:
            y, anc, nbad = ctx.predict_draws(S, SEED + k, x, lw, None, labels, s_first=s0, s_count=n)
            out.update({f"predict/{name}/{s0}_{n}/y": y, f"predict/{name}/{s0}_{n}/ancestors": anc,
                        f"predict/{name}/{s0}_{n}/n_bad": np.int64(nbad)})
    return out


def forecast_results():
    """{key: array} of every forecast_draws case, from the package that is imported."""
    from smcnuts_amd import ArmaModel
    rng = np.random.default_rng(5)
    t = ArmaModel(y=np.cumsum(0.5 * rng.standard_normal(12)))
    x, lw = _population(4, 20)
    given = rng.integers(0, M, S)
    ctx = t._context(M)
    ctx.forecast_set(H)
    out = {}
    for name, anc_in in (("systematic", None), ("given", given)):
        for s0, n in WINDOWS:
            y, anc, nbad = ctx.forecast_draws(S, SEED, x, lw, anc_in, s_first=s0, s_count=n)
            out.update({f"forecast/{name}/{s0}_{n}/y": y, f"forecast/{name}/{s0}_{n}/ancestors": anc,
                        f"forecast/{name}/{s0}_{n}/n_bad": np.int64(nbad)})
    return out


def assert_same_as_parent(got, prefix):
    """Bit for bit: y with its NaNs by position, the ancestors and n_bad of every stored case under `prefix`."""
    with np.load(GOLDEN) as want:
        keys = sorted(k for k in want.files if k.startswith(prefix))
        assert keys == sorted(got) and len(keys) >= 12, (keys, sorted(got))
        for k in keys:
            a, b = np.asarray(got[k]), want[k]
            assert a.dtype == b.dtype and a.shape == b.shape, k
            assert np.array_equal(np.isnan(a), np.isnan(b)) if a.dtype.kind == "f" else True, f"{k}: NaN positions"
            assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), k
