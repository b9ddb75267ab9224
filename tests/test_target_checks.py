"""Characterisation of the regression targets' argument checks (smcnuts_amd/_checks.py and their callers): what each of
GLMTarget, WideGLMTarget, HierarchicalGLM, MultilevelGLM, CategoricalRegression, OrdinalRegression, the four factory
functions, PredictMixin._predict_block / _draws_args and the "x must be [D] or [M, D]" sites does with a table of
arguments, against tests/target_checks_expected.json, recorded from the code BEFORE the checks were folded into one
module.  The file holds, per case, the exception's class with its whole message, or for an accepted set model_id, dim,
constrained_dim, param_names(), the public attributes (values and dtypes) and SHA-256 of model_data and of every array.

The table per group of cases: the valid sets; one single-fault case per `raise` statement the group is meant to reach
(RAISES: counted in the source, two statements with the same text count twice); and, for every two checks adjacent in
the order the code makes them, the case with both faults, which records WHICH of the two is reported.

    python tests/test_target_checks.py [ROOT]     rewrites the file from the package under ROOT (default: this tree)
"""
import hashlib
import json
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EXPECTED = os.path.join(HERE, "target_checks_expected.json")

ATTRS = ("X", "y", "prior_sd", "dispersion_prior", "offset", "weights", "groups", "n_groups", "term_groups", "term_z",
         "group_sd_prior", "n_classes", "cutpoint_prior_sd", "family", "intercept")

# `raise` statements each group's single faults reach (a site "a.b/variant" counts as "a.b")
RAISES = {"GLMTarget": 22, "WideGLMTarget": 18, "HierarchicalGLM": 24, "MultilevelGLM": 31, "CategoricalRegression": 15,
          "OrdinalRegression": 15, "_predict_block": 19, "_draws_args": 4, "_exposure_offset": 4, "points": 1}
# of those, the statements whose text another statement of the group has too ("... must be integers": dtype, then value)
SAME_TEXT = {"HierarchicalGLM": 1, "MultilevelGLM": 1, "CategoricalRegression": 1, "OrdinalRegression": 1}


# ---- what is recorded ------------------------------------------------------------------------------------------------

def _fp(v):
    if isinstance(v, np.ndarray):
        h = hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest()
        return {"sha256": h, "dtype": str(v.dtype), "shape": list(v.shape)}
    if isinstance(v, (list, tuple)):
        return {type(v).__name__: [_fp(u) for u in v]}
    return {type(v).__name__: repr(v)}


def _arrays(v):
    if isinstance(v, np.ndarray):
        yield v
    elif isinstance(v, (list, tuple)):
        for u in v:
            yield from _arrays(u)


def _describe(t, kw):
    if not hasattr(t, "model_data"):           # _predict_block's and _draws_args' tuples
        return _fp(t)
    attrs = {a: getattr(t, a) for a in ATTRS if hasattr(t, a)}
    given = list(_arrays(list(kw.values())))
    kept = [(a, s) for a, v in list(attrs.items()) + [("model_data", t.model_data)] for s in _arrays(v)]
    return dict(cls=type(t).__name__, model_id=_fp(t.model_id), dim=_fp(t.dim), constrained_dim=_fp(t.constrained_dim),
                param_names=t.param_names(), model_data=_fp(t.model_data), attrs={a: _fp(v) for a, v in attrs.items()},
                shares_memory_with_arguments=sorted({a for a, s in kept for g in given if np.shares_memory(s, g)}))


def _outcome(call, kw):
    try:
        t = call(kw)
    except Exception as e:      # noqa: BLE001 -- the class is what is recorded
        return {"raises": type(e).__name__, "message": str(e)}
    return {"returns": _describe(t, kw)}


# ---- the arguments ---------------------------------------------------------------------------------------------------

def _X(n=6, p=2):
    return (np.arange(n * p, dtype=np.float64).reshape(n, p) % 7.0 - 3.0) / 4.0


def _nan(a, v=np.nan):
    a = np.array(a, dtype=np.float64)
    a.flat[0] = v
    return a


Y01 = np.array([0.0, 1.0, 1.0, 0.0, 1.0, 0.0])
YCNT = np.array([0.0, 3.0, 1.0, 7.0, 2.0, 0.0])
YREAL = np.array([0.5, -1.25, 3.0, 0.0, 2.5, -0.75])
YLAB = np.array([0, 2, 1, 0, 2, 1], dtype=np.int64)
G3 = np.array([0, 1, 2, 0, 1, 2], dtype=np.int64)
G2 = np.array([1, 0, 0, 1, 1, 0], dtype=np.int64)
Z = np.array([0.5, -1.0, 2.0, 0.25, 1.5, -0.5])
OFF = np.array([0.1, -0.2, 0.3, 0.0, 0.5, -0.4])
WTS = np.array([1.0, 2.0, 0.0, 0.5, 3.0, 1.0])


def put(**kv):
    return lambda kw: kw.update(kv)


def term(r, **kv):
    """Replace groups / z / n_groups of term r."""
    def f(kw):
        t = (list(kw["terms"][r]) + [None, None])[:3]
        for i, k in enumerate(("groups", "z", "n_groups")):
            if k in kv:
                t[i] = kv[k]
        kw["terms"] = [tuple(t) if j == r else u for j, u in enumerate(kw["terms"])]
    return f


def _family_faults():
    return [("family", put(family="logit")),
            ("dispersion.none", put(dispersion_prior=(0.0, 1.0))),
            ("dispersion.pair", put(family="normal", y=YREAL, dispersion_prior=3.0)),
            ("dispersion.pair/three", put(family="normal", y=YREAL, dispersion_prior=(0.0, 1.0, 2.0))),
            ("dispersion.m", put(family="normal", y=YREAL, dispersion_prior=(np.inf, 1.0))),
            ("dispersion.s", put(family="neg_binomial_2_log", y=YCNT, dispersion_prior=(0.0, 0.0))),
            ("dispersion.s/nan", put(family="normal", y=YREAL, dispersion_prior=(0.0, np.nan)))]


def _y_faults():
    return [("y.bernoulli", put(family="bernoulli_logit", y=_nan(Y01, 2.0))),
            ("y.poisson", put(family="poisson_log", y=_nan(YCNT, 0.5))),
            ("y.poisson/negative", put(family="poisson_log", y=_nan(YCNT, -1.0))),
            ("y.normal", put(family="normal", y=_nan(YREAL, np.inf))),
            ("y.neg_binomial", put(family="neg_binomial_2_log", y=_nan(YCNT, 2.0 ** 54))),
            ("y.neg_binomial/nan", put(family="neg_binomial_2_log", y=_nan(YCNT)))]


def _glm_faults(p, limit):
    """_glm_setup's checks in their order, for a design of p columns; `limit`: the class's own dimension faults."""
    return _family_faults() + [
        ("X.ndim", put(X=np.zeros((2, 3, 1)))),
        ("y.shape", put(y=np.zeros(5))),
        ("y.shape/2d", put(y=np.zeros((6, 1)))),
        ("n", put(X=np.zeros((0, p)), y=np.zeros(0))),
        ("Dc", put(X=np.zeros((6, 0)), intercept=False, prior_sd=1.0)),
        *limit,
        ("X.finite", put(X=_nan(_X(6, p)))),
        *_y_faults(),
        ("prior_sd.shape", put(prior_sd=np.ones(p + 3))),
        ("prior_sd.shape/dispersion", put(family="normal", y=YREAL, prior_sd=np.ones(p + 3))),
        ("prior_sd.finite", put(prior_sd=0.0)),
        ("prior_sd.finite/inf", put(prior_sd=_nan(np.ones(p + 1), np.inf)))]


OW_FAULTS = [("row_vector.numeric/offset", put(offset="abc")),
             ("row_vector.shape/offset", put(offset=np.zeros(5))),
             ("offset.finite", put(offset=_nan(OFF))),
             ("row_vector.numeric/weights", put(weights="abc")),
             ("row_vector.shape/weights", put(weights=np.zeros((6, 1)))),
             ("weights.finite", put(weights=_nan(WTS, -1.0))),
             ("weights.positive", put(weights=np.zeros(6)))]


def _group_faults(f, prefix=""):
    """The checks of one group vector; f(groups=.. / n_groups=..) makes the fault."""
    return ([(prefix + "groups.shape", f(groups=np.array([0, 1]))),
             (prefix + "groups.dtype", f(groups=np.array([True, False, True, False, True, False]))),
             (prefix + "groups.dtype/str", f(groups=list("abcabc"))),
             (prefix + "groups.whole", f(groups=np.array([0.5, 1, 2, 0, 1, 2]))),
             (prefix + "groups.whole/nan", f(groups=np.array([np.nan, 1, 2, 0, 1, 2]))),
             (prefix + "groups.negative", f(groups=np.array([-1, 1, 2, 0, 1, 2])))],
            [(prefix + "n_groups", f(n_groups=0)),
             (prefix + "n_groups/bool", f(n_groups=True)),
             (prefix + "n_groups/float", f(n_groups=3.0)),
             (prefix + "groups.range", f(n_groups=1))])


def _label_faults(n_classes_max=()):
    return [("X.ndim", put(X=np.zeros((2, 3, 1)))),
            ("n", put(X=np.zeros((0, 2)), y=np.zeros(0, dtype=np.int64))),
            ("y.shape", put(y=np.zeros(5, dtype=np.int64))),
            ("y.dtype", put(y=np.array([True, False, True, False, True, False]))),
            ("y.dtype/str", put(y=list("abcabc"))),
            ("y.whole", put(y=np.array([0.5, 2, 1, 0, 2, 1]))),
            ("y.negative", put(y=np.array([-1, 2, 1, 0, 2, 1]))),
            ("n_classes.type", put(n_classes=3.0)),
            ("n_classes.type/bool", put(n_classes=True)),
            ("n_classes.min", put(n_classes=1)),
            ("n_classes.min/labels", put(y=np.zeros(6, dtype=np.int64))),
            *n_classes_max,
            ("y.range", put(n_classes=2))]


def _constructor_groups(T):
    def glm(**kv):
        return lambda: dict(dict(X=_X(), y=Y01.copy(), family="bernoulli_logit", prior_sd=2.5, intercept=True), **kv)

    def ctor(cls):
        return lambda kw: cls(**kw)

    g = {}
    g["glm"] = ("GLMTarget", ctor(T.GLMTarget), glm(offset=OFF.copy(), weights=WTS.copy()),
                _glm_faults(2, [("limit", put(X=np.zeros((6, 64))))]) + OW_FAULTS,
                {"plain": put(offset=None, weights=None, prior_sd=np.array([1.0, 2.0, 1.5])),
                 "plain/lists": put(X=_X().tolist(), y=[0, 1, 1, 0, 1, 0], offset=None, weights=None),
                 "plain/1d": put(X=np.arange(6.0), offset=None, weights=None),
                 "plain/no_intercept": put(intercept=0, offset=None, weights=None),
                 "poisson": put(family="poisson_log", y=_nan(YCNT, 2.0 ** 60), offset=None, weights=None),
                 "normal": put(family="normal", y=YREAL.copy(), dispersion_prior=(0.2, 1.5), offset=None, weights=None),
                 "neg_binomial": put(family="neg_binomial_2_log", y=YCNT.copy(), offset=None, weights=None,
                                     prior_sd=np.array([1.0, 2.0, 1.5])),
                 "offset": put(family="poisson_log", y=YCNT.copy(), weights=None),
                 "weights": put(offset=None),
                 "offset+weights": put(family="normal", y=YREAL.copy(), dispersion_prior=[1, 2]),
                 "D64": put(X=_X(6, 63), offset=None, weights=None),
                 "refused.y.strings": put(y=list("abcdef"), offset=None, weights=None)})
    g["wglm"] = ("WideGLMTarget", ctor(T.WideGLMTarget), glm(X=_X(6, 70)),
                 _glm_faults(70, [("limit.low", put(X=np.zeros((6, 63)))), ("limit.high", put(X=np.zeros((6, 256))))]),
                 {"plain": put(), "normal": put(family="normal", y=YREAL.copy(), prior_sd=np.linspace(1.0, 2.0, 71)),
                  "D65": put(X=_X(6, 64)), "D256": put(X=_X(6, 254), family="neg_binomial_2_log", y=YCNT.copy())})

    class MyHier(T.HierarchicalGLM):
        pass

    gv, gj = _group_faults(put)
    tail = [("X.finite", put(X=_nan(_X()))), *_y_faults(),
            ("prior_sd.shape", put(prior_sd=np.ones(5))), ("prior_sd.finite", put(prior_sd=-1.0))]
    rows = [("X.ndim", put(X=np.zeros((2, 3, 1)))),
            ("n", put(X=np.zeros((0, 2)), y=np.zeros(0), groups=np.zeros(0, dtype=np.int64))),
            ("y.shape", put(y=np.zeros(5)))]
    g["hier"] = ("HierarchicalGLM", ctor(T.HierarchicalGLM), glm(groups=G3.copy(), group_sd_prior=1.3),
                 _family_faults() + [("group_sd.number", put(group_sd_prior="x")),
                                     ("group_sd.number/vector", put(group_sd_prior=[1.0, 2.0])),
                                     ("group_sd.finite", put(group_sd_prior=0.0))] + rows + gv + gj
                 + [("limit", put(n_groups=61)), ("limit/dispersion", put(family="normal", y=YREAL, n_groups=60))] + tail,
                 {"plain": put(prior_sd=np.array([1.0, 2.0, 1.5])),
                  "n_groups": put(n_groups=np.int32(5), groups=[0.0, 1.0, 2.0, 0.0, 1.0, 2.0]),
                  "normal": put(family="normal", y=YREAL.copy(), dispersion_prior=(0.3, 0.7)),
                  "Dc0": put(X=np.zeros((6, 0)), intercept=False, family="neg_binomial_2_log", y=YCNT.copy()),
                  "D64": put(n_groups=60)})
    g["hier_subclass"] = ("HierarchicalGLM", ctor(MyHier), glm(groups=G3.copy()), [("family", put(family="logit"))],
                          {"plain": put()})

    def multi(terms):
        return glm(terms=terms, group_sd_prior=np.linspace(0.5, 1.5, len(terms)))

    def multi_faults(r, R):
        pre = f"term{r + 1}." if R > 1 else ""
        gv, gj = _group_faults(lambda **kv: term(r, **kv))
        zs = [("z.numbers", term(r, z=list("abcdef"))), ("z.shape", term(r, z=np.zeros(5))),
              ("z.finite", term(r, z=_nan(Z)))]
        return (_family_faults()
                + [("terms.type", put(terms=5)), ("terms.type/item", put(terms=[5])),
                   ("terms.count", put(terms=[])), ("terms.count/five", put(terms=[(G3,)] * 5, group_sd_prior=1.0)),
                   ("terms.len", put(terms=[()] * R)), ("terms.len/four", put(terms=[(G3, None, None, 1)] * R)),
                   ("group_sd.number", put(group_sd_prior="x")), ("group_sd.shape", put(group_sd_prior=np.ones(R + 1))),
                   ("group_sd.finite", put(group_sd_prior=0.0))]
                + rows[:1] + [("n", put(X=np.zeros((0, 2)), y=np.zeros(0)))] + rows[2:]
                + [(pre + s, f) for s, f in gv + zs + gj]
                + [("limit", term(r, n_groups=61)), ("limit/dispersion", lambda kw: (put(family="normal", y=YREAL)(kw),
                                                                                    term(r, n_groups=60)(kw)))] + tail)
    g["multi1"] = ("MultilevelGLM", ctor(T.MultilevelGLM), multi([(G3.copy(),)]), multi_faults(0, 1),
                   {"plain": put(), "z": put(terms=[(G3.copy(), Z.copy())]), "scalar_sd": put(group_sd_prior=2),
                    "normal": put(family="normal", y=YREAL.copy(), terms=[[G3.tolist(), None, 7]])})
    three = [(G3.copy(),), (G3.copy(), Z.copy()), (G2.copy(), None, 3)]
    for r in (1, 2):
        faults = multi_faults(r, 3)
        g[f"multi3.{r + 1}"] = ("MultilevelGLM", ctor(T.MultilevelGLM), multi(three),
                                faults if r == 2 else [f for f in faults if f[0].startswith("term2.")],
                                {"plain": put(), "poisson": put(family="poisson_log", y=YCNT.copy(), intercept=False)})

    g["cat"] = ("CategoricalRegression", ctor(T.CategoricalRegression), lambda: dict(X=_X(), y=YLAB.copy()),
                _label_faults([("n_classes.max", put(n_classes=17))])
                + [("Dc", put(X=np.zeros((6, 0)), intercept=False)), ("limit", put(X=np.zeros((6, 32)))),
                   ("X.finite", put(X=_nan(_X()))),
                   ("prior_sd.shape", put(prior_sd=np.ones(2))), ("prior_sd.shape/2d", put(prior_sd=np.ones((3, 3)))),
                   ("prior_sd.finite", put(prior_sd=_nan(np.ones((2, 3)), 0.0)))],
                {"plain": put(), "per_column": put(prior_sd=np.array([1.0, 2.0, 3.0])),
                 "full": put(prior_sd=np.arange(1.0, 9.0).reshape(4, 2), n_classes=5, intercept=False),
                 "float_labels": put(y=[0.0, 2.0, 1.0, 0.0, 2.0, 1.0], n_classes=np.int64(4)), "D64": put(X=_X(6, 31))})
    g["ord"] = ("OrdinalRegression", ctor(T.OrdinalRegression), lambda: dict(X=_X(), y=YLAB.copy()),
                _label_faults() + [("limit", put(n_classes=64)), ("X.finite", put(X=_nan(_X()))),
                                   ("prior_sd.shape", put(prior_sd=np.ones(3))), ("prior_sd.finite", put(prior_sd=np.nan)),
                                   ("cutpoints.shape", put(cutpoint_prior_sd=np.ones(3))),
                                   ("cutpoints.finite", put(cutpoint_prior_sd=0.0))],
                {"plain": put(), "vectors": put(prior_sd=np.array([1.0, 2.0]), cutpoint_prior_sd=np.array([3.0, 4.0, 5.0]),
                                                n_classes=4),
                 "p0": put(X=np.zeros((6, 0))), "D64": put(n_classes=63)})

    def factory(f):
        return lambda kw: f(**kw)
    expo = [("both", put(offset=OFF.copy())), ("numeric", put(exposure="abc")), ("shape", put(exposure=np.ones((6, 1)))),
            ("positive", put(exposure=_nan(np.ones(6), 0.0))), ("length", put(exposure=np.ones(5)))]
    g["logistic"] = ("factory", factory(T.LogisticRegression), lambda: dict(X=_X(), y=Y01.copy()),
                     [("y", put(y=YCNT))],
                     {"plain": put(), "ow": put(offset=OFF.copy(), weights=WTS.copy(), intercept=False)})
    g["poisson"] = ("_exposure_offset", factory(T.PoissonRegression),
                    lambda: dict(X=_X(), y=YCNT.copy(), exposure=np.exp(OFF)), expo[:4],
                    {"exposure": put(), "offset": put(exposure=None, offset=OFF.copy(), prior_sd=1.0),
                     "plain": put(exposure=None)})
    g["linear"] = ("factory", factory(T.LinearRegression), lambda: dict(X=_X(), y=YREAL.copy()),
                   [("dispersion", put(dispersion_prior=None))],
                   {"plain": put(), "prior": put(dispersion_prior=(1.0, 0.5), weights=WTS.copy())})
    g["neg_binomial"] = ("factory", factory(T.NegativeBinomialRegression),
                         lambda: dict(X=_X(), y=YCNT.copy(), exposure=np.exp(OFF)), expo[4:],
                         {"exposure": put(), "plain": put(exposure=None, dispersion_prior=(0.5, 1.0))})
    return g


def _predict_groups(T):
    def block(t):
        return lambda kw: t._predict_block(**kw)

    def draws(t):
        return lambda kw: t._draws_args(kw["X_new"], kw["n_draws"], kw.get("groups_new"), kw.get("ancestors"), kw.get("M"),
                                        kw.get("offset_new"))

    class MyGLM(T.GLMTarget):
        pass

    Xn = _X(3, 2) + 0.125
    xs = [("X_new.shape", put(X_new=np.zeros((0, 2)))), ("X_new.shape/3d", put(X_new=np.zeros((1, 3, 2)))),
          ("X_new.columns", put(X_new=np.zeros((3, 3)))), ("X_new.finite", put(X_new=_nan(Xn)))]
    no_g, no_o = ("groups_new.not_hier", put(groups_new=[0, 0, 0])), ("offset_new.not_offset", put(offset_new=np.zeros(3)))
    ys = [("y_new.shape", put(y_new=np.zeros(4))), ("y_new.numeric", put(y_new=list("abc")))]
    counts = [("y_new.counts", put(y_new=[1.0, 2.0 ** 54, 0.0])), ("y_new.counts/fraction", put(y_new=[1.0, 0.5, 0.0]))]
    labels = [("y_new.labels", put(y_new=[0, 3, 1])), ("y_new.labels/fraction", put(y_new=[0, 0.5, 1]))]
    valid = {"y": put(), "no_y": put(y_new=None), "row": put(X_new=np.array([0.5, -1.0]), y_new=None),
             "lists": put(X_new=Xn.tolist())}

    def fitted(cls, **kv):
        return cls(_X(), **kv)

    g = {}
    t = MyGLM(_X(), Y01)
    g["predict.glm"] = ("_predict_block", block(t), lambda: dict(X_new=Xn.copy(), y_new=[0, 1, 1]),
                        xs + [no_g, no_o] + ys + [("y_new.bernoulli", put(y_new=[0, 2, 1]))], valid)
    g["predict.glm.p1"] = ("_predict_block", block(T.GLMTarget(np.arange(6.0), Y01)),
                           lambda: dict(X_new=np.array([0.5, -1.0, 2.0])), xs[2:3],
                           {"column": put(), "scalar_row": put(X_new=[0.5])})
    g["predict.normal"] = ("_predict_block", block(fitted(T.GLMTarget, y=YREAL, family="normal", weights=WTS)),
                           lambda: dict(X_new=Xn.copy(), y_new=[0.5, -1.0, 2.0]),
                           [no_o, ("y_new.normal", put(y_new=[0.5, np.nan, 2.0]))], {"weights": put()})
    for fam in ("poisson_log", "neg_binomial_2_log"):
        g[f"predict.{fam}"] = ("_predict_block", block(fitted(T.GLMTarget, y=YCNT, family=fam)),
                               lambda: dict(X_new=Xn.copy(), y_new=[3.0, 0.0, 2.0 ** 53]), ys + counts, {"y": put()})
    g["predict.offset"] = ("_predict_block",
                           block(fitted(T.GLMTarget, y=YCNT, family="poisson_log", offset=OFF, weights=WTS)),
                           lambda: dict(X_new=Xn.copy(), y_new=[3.0, 0.0, 1.0], offset_new=np.array([0.1, 0.2, -0.3])),
                           xs + [no_g, ("offset_new.required", put(offset_new=None)),
                                 ("offset_new.numeric", put(offset_new="abc")),
                                 ("offset_new.shape", put(offset_new=np.zeros(4))),
                                 ("offset_new.finite", put(offset_new=[0.0, np.inf, 0.0]))]
                           + ys + counts, {"y": put(), "no_y": put(y_new=None)})
    hier = fitted(T.HierarchicalGLM, y=YREAL, groups=G3, family="normal")
    gs = [("groups_new.required", put(groups_new=None)), ("groups_new.type", put(groups_new=[0, 1])),
          ("groups_new.type/bool", put(groups_new=[True, False, True])),
          ("groups_new.type/str", put(groups_new=list("abc")))]
    g["predict.hier"] = ("_predict_block", block(hier),
                         lambda: dict(X_new=Xn.copy(), y_new=[0.5, -1.0, 2.0], groups_new=[2, 0, 1]),
                         xs + gs + [("groups_new.existing", put(groups_new=[0, 3, 1])),
                                    ("groups_new.existing/fraction", put(groups_new=[0, 0.5, 1])), no_o] + ys
                         + [("y_new.normal", put(y_new=[0.5, np.inf, 2.0]))], {"y": put(), "no_y": put(y_new=None)})
    g["predict.hier.new_groups"] = ("_predict_block", block(hier),
                                    lambda: dict(X_new=Xn.copy(), groups_new=[2, 7, 1], new_groups=True),
                                    xs + gs + [("groups_new.labels", put(groups_new=[0, -1, 1])),
                                               ("groups_new.labels/large", put(groups_new=[0.0, 2.0 ** 32, 1.0])), no_o],
                                    {"new": put(), "old": put(groups_new=[0, 1, 2])})
    g["predict.glm.new_groups"] = ("_predict_block", block(t), lambda: dict(X_new=Xn.copy(), new_groups=True), [no_g],
                                   {"no_labels": put()})
    for name, cls in (("cat", T.CategoricalRegression), ("ord", T.OrdinalRegression)):
        g[f"predict.{name}"] = ("_predict_block", block(fitted(cls, y=YLAB)), lambda: dict(X_new=Xn.copy(), y_new=[0, 2, 1]),
                                xs + [no_g, no_o] + ys + labels, valid)
    anc = [("ancestors.type", put(ancestors=[0, 1, 2])), ("ancestors.type/float", put(ancestors=[0.0, 1.0, 2.0, 3.0])),
           ("ancestors.range", put(ancestors=[0, 1, 2, 8]))]
    nd = [("n_draws", put(n_draws=0)), ("n_draws/bool", put(n_draws=True)), ("n_draws/float", put(n_draws=4.0)),
          ("n_draws/large", put(n_draws=2 ** 31))]
    g["draws.glm"] = ("_draws_args", draws(t), lambda: dict(X_new=Xn.copy(), n_draws=4, ancestors=[0, 7, 3, 3], M=8),
                      nd + [("groups_new.not_hier", put(groups_new=[0, 0, 0]))] + anc,
                      {"ancestors": put(), "systematic": put(ancestors=None),
                       "no_M": put(M=None, ancestors=np.array([9, 9, 9, 9])),
                       "refused.X_new.columns": put(X_new=np.zeros((3, 3)))})
    g["draws.hier"] = ("_draws_args", draws(hier), lambda: dict(X_new=Xn.copy(), n_draws=np.int64(2), groups_new=[0, 1, 2]),
                       nd[:1] + anc[:1],
                       {"old": put(), "new": put(groups_new=[0, 5, 2]),
                        "refused.groups_new.labels": put(groups_new=[0, -1, 1])})

    def points(t, method):
        return lambda kw: getattr(t, method)(**kw)
    bad = [("points", put(x=np.zeros(5))), ("points/2d", put(x=np.zeros((4, 2)))), ("points/3d", put(x=np.zeros((1, 1, 3))))]
    for name, obj, method, extra in (("summary", t, "summary", {}), ("covariance", t, "covariance", {}),
                                     ("pointwise", t, "_points", {}), ("predict", t, "_predict_points", {}),
                                     ("predict_draws", t, "predict_draws", dict(X_new=Xn, n_draws=2)),
                                     ("wide.summary", T.WideGLMTarget(_X(6, 70), Y01), "summary", {}),
                                     ("multi.covariance", T.MultilevelGLM(_X(), Y01, [(G3,)]), "covariance", {}),
                                     ("host.summary", T.HostTarget(t), "summary", {}),
                                     ("host.covariance", T.HostTarget(t), "covariance", {})):
        g[f"points.{name}"] = ("points", points(obj, method), lambda extra=extra: dict(x=np.zeros(3), **extra), bad, {})
    g["points.pointwise"][4]["1d"], g["points.pointwise"][4]["2d"] = put(), put(x=np.ones((2, 3)))
    g["points.predict"][4]["1d"] = put()
    return g


def _site(label):
    """The `raise` statement a fault is aimed at: its label without the variant and without the term's number."""
    return re.sub(r"^term\d+\.", "", label.split("/")[0])


def build_cases(T):
    """case id -> (call, kwargs): the valid sets, the single faults, the adjacent two-fault pairs."""
    cases, sites = {}, {}
    for name, (key, call, base, faults, valid) in {**_constructor_groups(T), **_predict_groups(T)}.items():
        def add(cid, *muts):
            kw = base()
            for m in reversed(muts):        # the earlier check's fault last, so that it is the one that holds
                m(kw)
            assert cid not in cases, cid
            cases[cid] = (call, kw)
        for vname, m in valid.items():
            add(f"{name}/valid/{vname}", m)
        for site, m in faults:
            add(f"{name}/1/{site}", m)
            sites.setdefault(key, {}).setdefault(_site(site), []).append(f"{name}/1/{site}")
        for (s0, m0), (s1, m1) in zip(faults, faults[1:]):
            add(f"{name}/2/{s0}+{s1}", m0, m1)
    return cases, sites


def record(T):
    cases, _ = build_cases(T)
    return {cid: _outcome(call, kw) for cid, (call, kw) in cases.items()}


# ---- the tests -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def table():
    from smcnuts_amd.model import targets as T
    cases, sites = build_cases(T)
    with open(EXPECTED) as f:
        return cases, sites, json.load(f)


def _group_names():
    if not os.path.exists(EXPECTED):        # only while __main__ writes the first one
        return []
    with open(EXPECTED) as f:
        return sorted({cid.split("/")[0] for cid in json.load(f)})


def test_the_file_holds_exactly_the_table(table):
    cases, _, want = table
    assert sorted(cases) == sorted(want)


@pytest.mark.parametrize("group", _group_names())
def test_every_case_does_what_it_did(table, group):
    cases, _, want = table
    wrong = {}
    for cid, (call, kw) in cases.items():
        if cid.split("/")[0] == group:
            got = json.loads(json.dumps(_outcome(call, kw)))
            if got != want[cid]:
                wrong[cid] = dict(got=got, want=want[cid])
    assert not wrong, json.dumps(wrong, indent=1)[:6000]


def test_valid_sets_are_accepted_and_copied(table):
    _, _, want = table
    for cid, w in want.items():
        if "/valid/refused." in cid:
            assert "raises" in w, (cid, w)
        elif "/valid/" in cid:
            assert "returns" in w, (cid, w)
            if isinstance(w["returns"], dict) and "cls" in w["returns"]:
                assert w["returns"]["shares_memory_with_arguments"] == [], cid


@pytest.mark.parametrize("key", sorted(RAISES))
def test_every_raise_is_reached_by_a_single_fault(table, key):
    _, sites, want = table
    reached = {s for s, cids in sites[key].items() if all("raises" in want[c] for c in cids)}
    assert reached == set(sites[key]), sorted(set(sites[key]) - reached)
    assert len(reached) == RAISES[key], sorted(reached)
    # distinct messages, one case per statement: as many as statements, less those that repeat another's text
    texts = {want[cids[0]]["message"] for cids in sites[key].values()}
    assert len(texts) == RAISES[key] - SAME_TEXT.get(key, 0), sorted(texts)


if __name__ == "__main__":
    sys.path.insert(0, os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(HERE))
    from smcnuts_amd.model import targets
    out = record(targets)
    with open(EXPECTED, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(out[k], sort_keys=True)}" for k in sorted(out)) + "\n}\n")
    print(f"{len(out)} cases from {os.path.dirname(os.path.dirname(targets.__file__))} -> {EXPECTED}")
