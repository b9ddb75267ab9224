"""Held-out prediction at new rows from the device's mergeable partials (include/smcnuts_hip.h, smcn_predict_partials).

For M particles with log-weights lw_p (W_p = exp(lw_p) / sum_q exp(lw_q)) and new rows X_new (m of them), per row i:
  mean_i = sum_p W_p E[y_i | x_p]                                      (GLM families, hierarchical)
  var_i  = sum_p W_p Var(y_i | x_p) + sum_p W_p (E[y_i | x_p] - mean_i)^2   (the law of total variance)
  prob[i, k] = sum_p W_p P(y_i = k | x_p)                              (categorical; ordinal up to K = 16)
  mean_i = sum_p W_p sum_k sigma(eta_i - c_k), the expected class index   (ordinal)
and, when y_new is given,
  lpd_i = log sum_p W_p p(y_new_i | x_p),  elpd = sum_i lpd_i,  se_elpd = sqrt(m var_i(lpd_i, ddof=1)).
lpd_i is the quantity to compare ANY two of the targets on a test set or by K-fold (`compare_heldout`); the in-sample
criteria (criteria.py) exist for GLMTarget only.

Rules, continuing criteria.py: a particle with a non-finite log-weight contributes to nothing.  A contributing particle
whose term is -inf adds 0 to lpd_i and is counted in n_inf_i.  A row for which some contributing particle has a
non-finite mean, variance or probability reports NaN there.  The between-particle variance is accumulated around a shift
(the first particle's mean) and merged by re-centring, never as sum w m^2 - mean^2.

HierarchicalGLM's predict() is for EXISTING groups only (groups_new in 0..J-1): the moments of a new group's rows would
have to integrate over its unseen intercept.  predict_draws() does take new groups (labels >= J): it DRAWS the intercept
from its prior, tau_p z, per replicated data set.

Posterior predictive draws (predict_draws -> PredictiveDraws; include/smcnuts_hip.h, smcn_predict_draws): draw s of S is
one replicated data set y_rep[s, :] ~ p(. | x_{a_s}) of the m rows from ONE particle a_s, the ancestors a from systematic
resampling of the weights with S slots (or given by the caller).  Every uniform is keyed by (seed, s, row), so a draw
does not depend on how the work was tiled, sliced or sharded.  A draw whose law is undefined (non-finite eta, mean or
cutpoint, mu > 2^53, an attempt cap of a rejection sampler reached) is NaN and counted in n_bad.
"""
import numpy as np

from . import _capi
from . import _checks
from .criteria import _merge_lse, _se

# columns of a partials block (row 0: header [mw, sw, sw2, cnt, 0 ..]; row 1 + i: new row i)
MA, SA, NINF, NBAD = range(4)
C0, SW, S1, S2, VAR = range(4, 9)       # GLM families and hierarchical: Q = 9
CAT_P0 = 4                              # categorical: Q = 4 + K
ORD_EM, ORD_P0 = 4, 5                   # ordinal: Q = 5 + K (K <= MAX_PROB_CLASSES), 5 above
MAX_PROB_CLASSES = 16


def n_cols(kind, K=0):
    """Columns of a partials block: kind 'glm' (GLM families, hierarchical), 'cat' or 'ord'."""
    if kind == "glm":
        return 9
    if kind == "cat":
        return CAT_P0 + K
    if kind == "ord":
        return ORD_P0 + (K if K <= MAX_PROB_CLASSES else 0)
    raise ValueError(f"unknown kind {kind!r}")


def merge_predict_partials(a, b, kind):
    """The partials of the union of two disjoint particle sets (a's particles first)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or a.ndim != 2 or a.shape[1] < 5:
        raise ValueError("partials blocks of one model and one set of new rows have the same shape [1 + m][Q]")
    if b[0, 3] == 0.0:
        return a.copy()
    if a[0, 3] == 0.0:
        return b.copy()
    out = np.zeros_like(a)
    mw = max(a[0, 0], b[0, 0])
    da, db = a[0, 0] - mw, b[0, 0] - mw                 # (<= 0, one of them 0)
    fa, fb = np.exp(da), np.exp(db)
    out[0, 0] = mw
    out[0, 1] = a[0, 1] * fa + b[0, 1] * fb
    out[0, 2] = a[0, 2] * fa * fa + b[0, 2] * fb * fb
    out[0, 3] = a[0, 3] + b[0, 3]
    A, B, O = a[1:], b[1:], out[1:]
    O[:, MA], O[:, SA] = _merge_lse(A[:, MA] + da, A[:, SA], B[:, MA] + db, B[:, SA])
    O[:, NINF] = A[:, NINF] + B[:, NINF]
    O[:, NBAD] = A[:, NBAD] + B[:, NBAD]
    if kind == "glm":
        # moments: both to the common weight scale, b's re-centred on a's shift
        ha, hb = ~np.isnan(A[:, C0]), ~np.isnan(B[:, C0])
        c = np.where(ha, A[:, C0], B[:, C0])
        with np.errstate(invalid="ignore"):
            d = np.where(ha & hb, B[:, C0] - A[:, C0], 0.0)
        swb, s1b, s2b = B[:, SW] * fb, B[:, S1] * fb, B[:, S2] * fb
        O[:, C0] = c
        O[:, SW] = A[:, SW] * fa + swb
        O[:, S1] = A[:, S1] * fa + (s1b + d * swb)
        O[:, S2] = A[:, S2] * fa + (s2b + d * (2.0 * s1b + d * swb))
        O[:, VAR] = A[:, VAR] * fa + B[:, VAR] * fb
    else:
        with np.errstate(invalid="ignore"):
            O[:, 4:] = A[:, 4:] * fa + B[:, 4:] * fb
    return out


class Prediction:
    """Posterior predictive summaries at m new rows (arrays of length m; `prob` is [m][K]).  Fields a model does not
    have are None: mean_i / var_i for categorical, var_i for ordinal, prob for the GLM families, hierarchical and an
    ordinal model with more than 16 classes; lpd_i, n_inf_i, elpd, se_elpd without y_new."""

    def __init__(self, mean_i, var_i, prob, lpd_i, n_inf_i, n_particles, ess, n_new):
        self.mean_i, self.var_i, self.prob, self.lpd_i, self.n_inf_i = mean_i, var_i, prob, lpd_i, n_inf_i
        self.n_particles = int(n_particles)       # contributing particles (finite log-weight)
        self.ess = float(ess)                     # effective sample size of the weights
        self.n_new = int(n_new)

    @property
    def elpd(self):
        return None if self.lpd_i is None else float(np.sum(self.lpd_i))

    @property
    def se_elpd(self):
        return None if self.lpd_i is None else _se(self.lpd_i)

    def summary(self):
        return dict(n_new=self.n_new, n_particles=self.n_particles, ess=self.ess, elpd=self.elpd, se_elpd=self.se_elpd,
                    n_inf=None if self.n_inf_i is None else int(np.sum(self.n_inf_i)))


def combine_predict_partials(partials, kind, K=0, has_y=True):
    """Merges partials blocks of disjoint particle sets in list order and finishes them -> Prediction."""
    partials = list(partials)
    if not partials:
        raise ValueError("combine_predict_partials: no partials")
    Q = n_cols(kind, K)
    acc = np.array(partials[0], dtype=np.float64, copy=True)
    if acc.ndim != 2 or acc.shape[1] != Q:
        raise ValueError(f"a partials block of this model is [1 + m][{Q}]")
    for p in partials[1:]:
        acc = merge_predict_partials(acc, p, kind)
    sw, sw2, cnt = acc[0, 1], acc[0, 2], acc[0, 3]
    P = acc[1:]
    m = P.shape[0]
    with_prob = kind == "cat" or (kind == "ord" and K <= MAX_PROB_CLASSES)
    if cnt == 0.0:
        nan = np.full(m, np.nan)
        return Prediction(None if kind == "cat" else nan, nan.copy() if kind == "glm" else None,
                          np.full((m, K), np.nan) if with_prob else None, nan.copy() if has_y else None,
                          np.zeros(m) if has_y else None, 0, 0.0, m)
    bad = P[:, NBAD] > 0.0
    mean = var = prob = lpd = ninf = None
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if has_y:
            lpd = np.where(P[:, SA] > 0.0, P[:, MA] + np.log(P[:, SA]) - np.log(sw), -np.inf)
            ninf = P[:, NINF].copy()
        if kind == "glm":
            m1 = P[:, S1] / P[:, SW]
            mean = np.where(bad, np.nan, P[:, C0] + m1)
            between = np.maximum(P[:, S2] / P[:, SW] - m1 * m1, 0.0)
            var = np.where(bad, np.nan, P[:, VAR] / P[:, SW] + between)
        else:
            p0 = CAT_P0 if kind == "cat" else ORD_P0
            if kind == "ord":
                mean = np.where(bad, np.nan, P[:, ORD_EM] / sw)
            if with_prob:
                prob = np.where(bad[:, None], np.nan, P[:, p0:p0 + K] / sw)
    return Prediction(mean, var, prob, lpd, ninf, cnt, sw * sw / sw2, m)


def compare_heldout(a, b):
    """a against b on the same held-out rows: the difference of the lpd totals (a - b) with its paired standard error
    sqrt(m var_i(diff_i, ddof=1))."""
    if a.n_new != b.n_new:
        raise ValueError(f"compare_heldout: the two were computed on different numbers of rows ({a.n_new} and {b.n_new})")
    if a.lpd_i is None or b.lpd_i is None:
        raise ValueError("compare_heldout: both predictions need y_new (lpd_i)")
    with np.errstate(invalid="ignore"):
        d = a.lpd_i - b.lpd_i
    return dict(elpd_diff=float(np.sum(d)), se_elpd_diff=_se(d), n_new=a.n_new)


def _philox_uniform(seed, it, particle, stream, q):
    """The library's philox_uniform (Philox4x32-10, 53-bit uniforms) for ONE key, on the host: the ancestor offset u0
    that several shards must agree on."""
    c = [q >> 1, particle, it, stream]
    k0, k1, M = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & M, (p0 >> 32) ^ c[3] ^ k1, p0 & M]
        k0, k1 = (k0 + 0x9E3779B9) & M, (k1 + 0xBB67AE85) & M
    a, b = (c[2], c[3]) if q & 1 else (c[0], c[1])
    return ((a >> 5) * 67108864.0 + (b >> 6)) / 9007199254740992.0


ANCESTOR_STREAM = 16


def shard_slots(lw, S, seed, comm, stream=ANCESTOR_STREAM):
    """Several shards, one systematic comb (its offset u0 on Philox stream `stream`): (s_first, s_count, local ancestors
    [S] (0 outside the range), rank offsets).
    Every rank all-gathers (largest finite log-weight, sum of exp(lw - that)); A, the ranks' cumulative weight bounds, is
    summed on the host in rank order with the last bound +inf; rank r owns the slots whose position (s + u0) / S falls in
    [A_r, A_r+1) and searches its own cumulative sum, offset by A_r, for them."""
    lw = np.asarray(lw, dtype=np.float64)
    fin = np.isfinite(lw)
    mw = float(np.max(lw[fin])) if fin.any() else -np.inf
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        w = np.where(fin, np.exp(np.where(fin, lw - mw, 0.0)), 0.0)
    allp = np.asarray(comm.allgather(np.array([mw, float(np.sum(w)), float(lw.shape[0])]))).reshape(-1, 3)
    gm = float(np.max(allp[:, 0]))
    if not np.isfinite(gm):
        raise RuntimeError("predict_draws: no particle has a finite log-weight")
    with np.errstate(under="ignore"):
        tot = np.where(np.isfinite(allp[:, 0]), allp[:, 1] * np.exp(allp[:, 0] - gm), 0.0)
    A = np.concatenate([[0.0], np.cumsum(tot)])
    total = A[-1]
    r = comm.rank
    pos = (np.arange(S) + _philox_uniform(int(seed), 0, 0, stream, 0)) / S
    bounds = A / total
    bounds[-1] = np.inf
    own = np.nonzero((pos >= bounds[r]) & (pos < bounds[r + 1]))[0]
    anc = np.zeros(S, dtype=np.int64)
    if own.size:
        with np.errstate(under="ignore"):
            cl = (A[r] + np.cumsum(w * np.exp(mw - gm))) / total
        a = np.searchsorted(cl, pos[own], side="right")
        last = int(np.nonzero(fin)[0][-1])
        anc[own] = np.minimum(a, last)
    offs = np.concatenate([[0], np.cumsum(allp[:, 2])]).astype(np.int64)
    return (int(own[0]) if own.size else 0), int(own.size), anc, offs


class PredictiveDraws:
    """Posterior predictive draws at m rows: y [S][m] (row s: one replicated data set, from particle ancestors[s]),
    n_bad the number of NaN draws (the law was undefined or a sampler gave up)."""

    def __init__(self, y, ancestors, n_bad):
        self.y = np.asarray(y, dtype=np.float64)
        self.ancestors = np.asarray(ancestors, dtype=np.int64)
        self.n_bad = int(n_bad)
        self.n_draws = int(self.y.shape[0])

    def mean(self):
        """Row-wise mean over the draws (NaN draws left out; NaN for a row without any other)."""
        with np.errstate(invalid="ignore", divide="ignore"):
            ok = ~np.isnan(self.y)
            return np.where(ok, self.y, 0.0).sum(0) / ok.sum(0)

    def interval(self, level=0.9):
        """(lo, hi): the row-wise equal-tailed `level` interval over the draws (NaN draws left out)."""
        if not 0.0 < level < 1.0:
            raise ValueError("PredictiveDraws.interval: level must lie in (0, 1)")
        a = 0.5 * (1.0 - level)
        out = np.full((2, self.y.shape[1]), np.nan)
        for i in range(self.y.shape[1]):
            col = self.y[:, i]
            col = col[~np.isnan(col)]
            if col.size:
                out[:, i] = np.quantile(col, [a, 1.0 - a])
        return out[0], out[1]

    def pvalue(self, stat, y_obs):
        """The share of the draws with stat(y_rep) >= stat(y_obs) (draws whose statistic is NaN left out)."""
        t = np.array([float(stat(r)) for r in self.y])
        t0 = float(stat(np.asarray(y_obs, dtype=np.float64)))
        ok = ~np.isnan(t)
        return float(np.mean(t[ok] >= t0)) if ok.any() else float("nan")


class PredictMixin:
    """predict / predict_loglik / predict_partials of GLMTarget, HierarchicalGLM, CategoricalRegression and
    OrdinalRegression.  Every argument check runs on the host, before a context exists."""

    def _predict_kind(self):
        if self.model_id == _capi.MODEL_CATEGORICAL:
            return "cat", self.n_classes
        if self.model_id == _capi.MODEL_ORDINAL:
            return "ord", self.n_classes
        return "glm", 0

    def _predict_block(self, X_new, y_new=None, groups_new=None, new_groups=False, offset_new=None):
        """(block, has_y): the new rows as the model's data block without the priors, checked.  new_groups (predict_draws):
        labels >= J name new groups; such rows carry group 0 in the block and (block, has_y, labels) is returned.
        A GLMTarget with offsets takes offset_new, one per new row; after a fit with weights the new rows carry weight 1."""
        name = type(self).__name__
        who = f"{name}.predict"
        hier = self.model_id == _capi.MODEL_HGLM
        oglm = self.model_id == _capi.MODEL_OGLM
        # not _checks.design: a vector is ONE ROW of a design with p > 1 columns, and m >= 1 belongs to the shape check
        X = np.asarray(X_new, dtype=np.float64)
        p = self.X.shape[1]
        if X.ndim == 1:
            X = X.reshape(-1, 1) if p == 1 else X.reshape(1, -1)
        if X.ndim != 2 or X.shape[0] < 1:
            raise ValueError(f"{who}: X_new must be an (m, p) matrix with m >= 1")
        m = X.shape[0]
        if X.shape[1] != p:
            raise ValueError(f"{who}: X_new has {X.shape[1]} columns, the training design has {p}")
        _checks.finite(who, "X_new", X)
        if hier:
            if groups_new is None:
                raise ValueError(f"{who}: groups_new is required (each new row's group, an existing group "
                                 f"0..{self.n_groups - 1}; predictions for new, unseen groups are not implemented)")
            # not _checks.index_vector: shape and dtype are ONE check with one text here, and so are the value checks
            g = np.asarray(groups_new)
            if g.ndim != 1 or g.shape[0] != m or g.dtype == bool or \
                    not (np.issubdtype(g.dtype, np.integer) or np.issubdtype(g.dtype, np.floating)):
                raise ValueError(f"{who}: groups_new must be a vector of m = {m} integers")
            gf = g.astype(np.float64)
            if new_groups:
                if not np.all(np.isfinite(gf) & (gf == np.floor(gf)) & (gf >= 0) & (gf < 2.0 ** 32)):
                    raise ValueError(f"{name}.predict_draws: groups_new must be labels in 0..2^32-1 (below "
                                     f"{self.n_groups}: a fitted group; from {self.n_groups}: a new group)")
                labels = gf.astype(np.int64)
                gf = np.where(gf < self.n_groups, gf, 0.0)
            elif not np.all(np.isfinite(gf) & (gf == np.floor(gf)) & (gf >= 0) & (gf < self.n_groups)):
                raise ValueError(f"{who}: groups_new must be existing groups 0..{self.n_groups - 1} "
                                 "(predictions for new, unseen groups are not implemented)")
        elif groups_new is not None:
            raise ValueError(f"{who}: groups_new is for HierarchicalGLM only")
        ow = []
        if oglm and self.offset is not None:
            if offset_new is None:
                raise ValueError(f"{who}: offset_new is required (each new row's offset: the model was fitted "
                                 "with offsets)")
            o = _checks.row_vector(who, "offset_new", offset_new, m, f"the m = {m} rows X_new has")
            ow.append(_checks.finite(who, "offset_new", o))
        elif offset_new is not None:
            raise ValueError(f"{who}: offset_new is for a GLMTarget fitted with offsets only")
        if oglm and self.weights is not None:
            ow.append(np.ones(m))
        has_y = y_new is not None
        if has_y:
            # not _checks.row_vector: the shape is checked before the conversion to numbers
            y = np.asarray(y_new)
            if y.ndim != 1 or y.shape[0] != m:
                raise ValueError(f"{who}: y_new must be a vector of the m = {m} rows X_new has")
            try:
                y = y.astype(np.float64)
            except (TypeError, ValueError):
                raise ValueError(f"{who}: y_new must be numeric") from None
            kind, K = self._predict_kind()
            if kind != "glm":           # whole, >= 0 and < K in ONE check with one text, unlike the constructors' labels
                if not np.all(np.isfinite(y) & (y == np.floor(y)) & (y >= 0) & (y < K)):
                    raise ValueError(f"{who}: the labels y_new must be integers in 0..{K - 1}")
            elif self.family in ("bernoulli_logit", "normal"):
                _checks.family_response(who, self.family, y, "y_new")
            # the count families: unlike the constructors', poisson_log's y_new is bounded by 2^53 too, under one text
            elif not np.all(np.isfinite(y) & (y >= 0.0) & (y <= 2.0 ** 53) & (y == np.floor(y))):
                raise ValueError(f"{who}: {self.family} needs y_new in {{0, 1, 2, ...}}")
        else:
            y = np.zeros(m)
        nh = 3 if self.model_id == _capi.MODEL_ORDINAL else (5 if hier or oglm else 4)
        head = np.array(self.model_data[:nh], dtype=np.float64)
        head[1] = float(m)
        block = np.concatenate([head, y, gf if hier else [], *ow, X.reshape(-1)])
        if new_groups:
            return block, has_y, (labels if hier else None)
        return block, has_y

    def _predict_points(self, x):
        return _checks.points(type(self).__name__, x, self.dim)

    _PR_CHUNK = 1 << 25          # doubles of the matrix the device holds at once (256 MB)

    def predict_loglik(self, x, X_new, y_new, groups_new=None, offset_new=None):
        """log p(y_new_i | x_p): [m] for a 1-D x, [M, m] for 2-D.  The matrix is formed on the device in slabs of
        particles; it has to fit on the host.  At the training rows its row sums are logpdf_parts(x)[1]."""
        if y_new is None:
            raise ValueError(f"{type(self).__name__}.predict_loglik: y_new is required")
        block, _ = self._predict_block(X_new, y_new, groups_new, offset_new=offset_new)
        x2 = self._predict_points(x)
        M, m = x2.shape[0], int(block[1])
        step = max(1, min(M, self._PR_CHUNK // m))
        ctx = self._context(step)
        ctx.predict_set_data(block, True)
        out = np.empty((M, m))
        for m0 in range(0, M, step):
            out[m0:m0 + step] = ctx.predict_loglik(x2[m0:m0 + step])
        return out[0] if np.ndim(x) == 1 else out

    def predict_partials(self, x, X_new, y_new=None, groups_new=None, logw=None, offset_new=None):
        """The mergeable partials of x's rows at the new rows ([1 + m][Q], include/smcnuts_hip.h)."""
        block, has_y = self._predict_block(X_new, y_new, groups_new, offset_new=offset_new)
        x2 = self._predict_points(x)
        ctx = self._context(x2.shape[0])
        ctx.predict_set_data(block, has_y)
        return ctx.predict_partials(x2, logw)

    def predict(self, x, X_new, y_new=None, groups_new=None, logw=None, offset_new=None):
        """Posterior predictive summaries of the weighted points (x [M, D], logw unnormalised or None for equal weights)
        at the new rows -> Prediction; with y_new, the log predictive density of each held-out row as well."""
        part = self.predict_partials(x, X_new, y_new, groups_new, logw, offset_new)
        kind, K = self._predict_kind()
        return combine_predict_partials([part], kind, K, y_new is not None)

    def _draws_args(self, X_new, n_draws, groups_new, ancestors, M, offset_new=None):
        """predict_draws' host checks -> (block, labels, S, ancestors)."""
        name = type(self).__name__
        if isinstance(n_draws, bool) or not isinstance(n_draws, (int, np.integer)) or not 1 <= n_draws < 2 ** 31:
            raise ValueError(f"{name}.predict_draws: n_draws must be an integer in 1..2^31-1")
        S = int(n_draws)
        if groups_new is not None and self.model_id != _capi.MODEL_HGLM:
            raise ValueError(f"{name}.predict_draws: groups_new is for HierarchicalGLM only")
        block, _, labels = self._predict_block(X_new, None, groups_new, new_groups=True, offset_new=offset_new)
        if labels is not None and not np.any(labels >= self.n_groups):
            labels = None
        if ancestors is not None:
            a = np.asarray(ancestors)
            if a.ndim != 1 or a.shape[0] != S or a.dtype == bool or not np.issubdtype(a.dtype, np.integer):
                raise ValueError(f"{name}.predict_draws: ancestors must be a vector of n_draws = {S} integers")
            if M is not None and not np.all((a >= 0) & (a < M)):
                raise ValueError(f"{name}.predict_draws: ancestors must be particles 0..{M - 1}")
            ancestors = a.astype(np.int64)
        return block, labels, S, ancestors

    def predict_draws(self, x, X_new, n_draws, seed=0, groups_new=None, logw=None, ancestors=None, offset_new=None):
        """n_draws replicated data sets at the new rows from the weighted points (x [M, D], logw unnormalised or None
        for equal weights; ancestors: the particle of each draw instead of the systematic resampling) ->
        PredictiveDraws.  HierarchicalGLM: groups_new labels >= J are NEW groups, their intercept drawn per data set."""
        x2 = self._predict_points(x)
        M = x2.shape[0]
        block, labels, S, ancestors = self._draws_args(X_new, n_draws, groups_new, ancestors, M, offset_new)
        if logw is not None and np.shape(logw) != (M,):
            raise ValueError(f"{type(self).__name__}.predict_draws: logw must hold one log-weight per row of x")
        ctx = self._context(M)
        ctx.predict_set_data(block, False)
        return PredictiveDraws(*ctx.predict_draws(S, seed, x2, logw, ancestors, labels))
