"""The argument checks the regression targets' constructors (model/targets.py) and PredictMixin (predict.py) share.

Each function takes `who`, the prefix of its messages (the caller's name), checks ONE thing and returns the converted
value.  The callers decide the order, and with it which of several faults is reported.  A check whose CONDITION differs
from a function here stays with its caller; one that differs only in wording passes the wording in.
"""
import math

import numpy as np

GLM_FAMILIES = ("bernoulli_logit", "poisson_log", "normal", "neg_binomial_2_log")
GLM_DISPERSION = {"normal": "sigma", "neg_binomial_2_log": "phi"}    # the families with a sampled scale, and its name
GLM_MAX_DIM = 64
NO_PRIOR = object()                        # dispersion_prior's default: "not given"


def family(who, family):
    if family not in GLM_FAMILIES:
        raise ValueError(f"{who}: family must be one of {GLM_FAMILIES}, not {family!r}")
    return family


def dispersion_prior(who, family, value):
    """(m, s) of tau ~ N(m, s^2) for a family with a dispersion (NO_PRIOR: (0, 2.5)); None for one without, which
    refuses a value."""
    if family not in GLM_DISPERSION:
        if value is not NO_PRIOR:
            raise ValueError(f"{who}: {family} has no dispersion parameter; dispersion_prior is for "
                             f"{tuple(GLM_DISPERSION)}")
        return None
    return scale_prior(who, (0.0, 2.5) if value is NO_PRIOR else value)


def scale_prior(who, value):
    """(m, s) of tau ~ N(m, s^2) on a log scale or log shape that the family always has (ContinuousGLM's): a pair, m
    finite, s finite and > 0."""
    try:
        m, s = (float(v) for v in value)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: dispersion_prior must be a pair (m, s)") from None
    if not math.isfinite(m):
        raise ValueError(f"{who}: dispersion_prior's m must be finite")
    if not (math.isfinite(s) and s > 0.0):
        raise ValueError(f"{who}: dispersion_prior's s must be finite and > 0")
    return m, s


def design(who, X):
    """X as an (n, p) float matrix; a vector is one column."""
    X = np.asarray(X, dtype=np.float64)
    if X.ndim == 1:
        X = X.reshape(-1, 1)
    if X.ndim != 2:
        raise ValueError(f"{who}: X must be an (n, p) matrix")
    return X


def some_rows(who, n):
    if n < 1:
        raise ValueError(f"{who}: at least one observation")


def per_row(who, name, a, n):
    """a (an array already) holds one value per row of X."""
    if a.ndim != 1 or a.shape[0] != n:
        raise ValueError(f"{who}: {name} must be a vector of the n = {n} observations X has rows for")
    return a


def finite(who, name, a):
    if not np.all(np.isfinite(a)):
        raise ValueError(f"{who}: {name} must be finite")
    return a


def response(who, y, n):
    """y as a float vector of the n observations (what numpy cannot convert raises numpy's own error)."""
    return per_row(who, "y", np.asarray(y, dtype=np.float64), n)


def family_response(who, family, y, name="y"):
    """y within the family's support.  poisson_log has no upper bound here; neg_binomial_2_log's is 2^53."""
    if family == "bernoulli_logit":
        if not np.all((y == 0.0) | (y == 1.0)):
            raise ValueError(f"{who}: bernoulli_logit needs {name} in {{0, 1}}")
    elif family == "poisson_log":
        if not np.all(np.isfinite(y) & (y >= 0.0) & (y == np.floor(y))):
            raise ValueError(f"{who}: poisson_log needs {name} in {{0, 1, 2, ...}}")
    elif family == "normal":
        if not np.all(np.isfinite(y)):
            raise ValueError(f"{who}: normal needs finite {name}")
    elif not np.all(np.isfinite(y) & (y >= 0.0) & (y <= 2.0 ** 53) & (y == np.floor(y))):
        raise ValueError(f"{who}: neg_binomial_2_log needs {name} in {{0, 1, 2, ..., 2^53}}")
    return y


CONTINUOUS_FAMILIES = ("gamma_log", "student_t")            # ContinuousGLM's, with ids of their own (SMCN_MODEL_CGLM)
CONTINUOUS_SCALE = {"gamma_log": "shape", "student_t": "sigma"}    # what e^tau is, and its parameter name
DEFAULT_DF = 4.0


def continuous_family(who, family):
    if family not in CONTINUOUS_FAMILIES:
        raise ValueError(f"{who}: family must be one of {CONTINUOUS_FAMILIES}, not {family!r}")
    return family


def continuous_response(who, family, y, name="y"):
    """y within the family's support: finite, and > 0 for gamma_log."""
    if family == "gamma_log":
        if np.any(y == 0.0):
            raise ValueError(f"{who}: gamma_log needs {name} > 0 and {name} holds zeros (the gamma density has none: "
                             "model the zeros apart, or shift the response)")
        if not np.all(np.isfinite(y) & (y > 0.0)):
            raise ValueError(f"{who}: gamma_log needs finite {name} > 0")
    elif not np.all(np.isfinite(y)):
        raise ValueError(f"{who}: student_t needs finite {name}")
    return y


def student_df(who, family, df):
    """student_t's fixed degrees of freedom, finite and > 0; gamma_log has none and refuses a value other than the
    default.  Returns the header's slot: df, or 0 for gamma_log."""
    try:
        v = float(df)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: df must be a number") from None
    if family != "student_t":
        if v != DEFAULT_DF:
            raise ValueError(f"{who}: {family} has no degrees of freedom; df is for student_t")
        return 0.0
    if not (math.isfinite(v) and v > 0.0):
        raise ValueError(f"{who}: df must be finite and > 0")
    return v


def index_vector(who, v, n, name, what=None):
    """Labels or group indices, one per row of X: whole numbers >= 0 of an integer or float dtype (no bools, no
    strings), as float64.  `name` is the argument in the shape message, `what` (default: name) in the others."""
    v = per_row(who, name, np.asarray(v), n)
    what = what or name
    if v.dtype == bool or not (np.issubdtype(v.dtype, np.integer) or np.issubdtype(v.dtype, np.floating)):
        raise ValueError(f"{who}: {what} must be integers")
    vf = v.astype(np.float64)
    if not np.all(np.isfinite(vf) & (vf == np.floor(vf))):
        raise ValueError(f"{who}: {what} must be integers")
    if np.any(vf < 0):
        raise ValueError(f"{who}: {what} must be >= 0")
    return vf


def below(who, what, vf, count, count_name):
    """Every index of vf (index_vector's) is below count."""
    if vf.max() >= count:
        raise ValueError(f"{who}: {what} must be in 0..{count_name} - 1 = {count - 1}")


def n_groups(who, gf, value, prefix=""):
    """J: value, or the largest index of gf + 1 for None; every index is below it."""
    J = int(gf.max()) + 1 if value is None else value
    if isinstance(J, bool) or not isinstance(J, (int, np.integer)) or J < 1:
        raise ValueError(f"{who}: {prefix}n_groups must be an integer >= 1")
    below(who, f"{prefix}groups", gf, int(J), "n_groups")
    return int(J)


def n_classes(who, yf, value):
    """K >= 2: value, or the largest label of yf + 1 for None.  The caller checks the labels against it (`below`)."""
    K = int(yf.max()) + 1 if value is None else value
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)):
        raise ValueError(f"{who}: n_classes must be an integer")
    if K < 2:
        raise ValueError(f"{who}: K = n_classes must be >= 2 (one class has no likelihood)")
    return int(K)


def prior_sds(who, name, value, shape, what):
    """Standard deviations of shape `shape`, finite and > 0; a scalar is one value for all.  `what` words the shapes
    the caller accepts."""
    s = np.asarray(value, dtype=np.float64)
    if s.ndim == 0:
        s = np.full(shape, float(s))
    if s.shape != shape:
        raise ValueError(f"{who}: {name} must be {what}")
    if not np.all(np.isfinite(s) & (s > 0.0)):
        raise ValueError(f"{who}: {name} must be finite and > 0")
    return s


def row_vector(who, name, v, n, what):
    """offset / weights / exposure as a float vector of n values."""
    try:
        a = np.asarray(v, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: {name} must be numeric") from None
    if a.ndim != 1 or a.shape[0] != n:
        raise ValueError(f"{who}: {name} must be a vector of {what}")
    return a


def dim_limit(who, D, detail, limit=GLM_MAX_DIM):
    if D > limit:
        raise ValueError(f"{who}: {detail}; the device functor covers D <= {limit}. "
                         "Wrap a model object with .dim / .logpdf / .logpdfgrad in HostTarget instead.")


def points(who, x, dim):
    """x, [D] or [M, D], as [M, D]."""
    x2 = np.atleast_2d(np.asarray(x, dtype=np.float64))
    if x2.ndim != 2 or x2.shape[1] != dim:
        raise ValueError(f"{who}: x must be [{dim}] or [M, {dim}]")
    return x2
