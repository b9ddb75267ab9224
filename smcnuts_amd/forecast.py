"""Forecasts of the arma target from the device's mergeable partials (include/smcnuts_hip.h, smcn_forecast_partials).

Per particle x = (mu, beta, theta, log sigma) the h-step law given the series is y_{T+h} | y_{1:T}, x ~ N(m_h, v_h):
  m_1 = mu + beta y_T + theta err_T,  m_h = mu + beta m_{h-1};   v_h = sigma^2 sum_{j<h} psi_j^2,
  psi_0 = 1, psi_1 = beta + theta, psi_j = beta psi_{j-1}        (iterative: |beta| >= 1 gives growing, finite variances).
The posterior predictive of y_{T+h} is the mixture of these laws over the particles with weights W_p:
  mean_h = sum_p W_p m_h,   var_h = sum_p W_p v_h + sum_p W_p (m_h - mean_h)^2,
  cdf[h, k] = sum_p W_p Phi((at[h, k] - m_h) / sqrt(v_h)),
and, when a held-out continuation y_future is given,
  lpd_marginal_h = log sum_p W_p N(yf_h | m_h, v_h)              each horizon on its own, from the END of the series
  lpd_joint_h    = log sum_p W_p p(yf_1..yf_h | y_{1:T}, x_p)    cumulative: the one-step densities chained through yf.

Rules, continuing predict.py: a particle with a non-finite log-weight contributes to nothing.  A contributing particle
whose sigma, m_h or v_h is non-finite (or v_h <= 0) is counted in n_bad[h] and adds nothing to that horizon; a horizon
with n_bad > 0 reports NaN moments and cdf, and its lpd over the other particles.  The between-particle variance is
accumulated around a shift (a wavefront's own weighted mean of m_h) and merged by re-centring, never as sum w m^2 - mean^2.

Paths (forecast_draws -> predict.PredictiveDraws; smcn_forecast_draws): path s of S is simulated from ONE particle a_s,
the ancestors from systematic resampling of the weights with S slots (or given by the caller); every normal is keyed by
(seed, s, h), so a path does not depend on how the work was tiled or sharded.  From its first non-finite value on a
path is NaN, counted in n_bad.
"""
import numpy as np

from .criteria import _merge_lse

MAX_HORIZON = 512
MAX_THRESHOLDS = 16
ANCESTOR_STREAM = 20
# columns of a partials block (row 0: header [mw, sw, sw2, cnt, 0 ..]; row h: horizon h)
MA, SA, MJ, SJ, NBAD, C0, SW, S1, S2, VAR = range(10)
P0 = 10                                 # 10 + k: sum w Phi((at[h][k] - m_h) / sqrt(v_h)); Q = 10 + Tn


def check_horizon(who, horizon):
    if isinstance(horizon, bool) or not isinstance(horizon, (int, np.integer)) or not 1 <= horizon <= MAX_HORIZON:
        raise ValueError(f"{who}: horizon must be an integer in 1..{MAX_HORIZON}")
    return int(horizon)


def check_y_future(who, y_future, H):
    if y_future is None:
        return None
    try:
        y = np.asarray(y_future, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: y_future must be numeric") from None
    if y.shape != (H,):
        raise ValueError(f"{who}: y_future must hold one value per horizon ({H})")
    if not np.all(np.isfinite(y)):
        raise ValueError(f"{who}: y_future must be finite")
    return np.ascontiguousarray(y)


def check_at(who, at, H):
    """None, or the thresholds as [H][Tn]: a scalar and [Tn] are repeated for every horizon."""
    if at is None:
        return None
    try:
        a = np.asarray(at, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: at must be numeric") from None
    if a.ndim == 0:
        a = np.full((H, 1), float(a))
    elif a.ndim == 1:
        a = np.tile(a, (H, 1))
    if a.ndim != 2 or a.shape[0] != H or not 1 <= a.shape[1] <= MAX_THRESHOLDS:
        raise ValueError(f"{who}: at must be a scalar, [Tn] or [{H}][Tn] with 1 <= Tn <= {MAX_THRESHOLDS}")
    if not np.all(np.isfinite(a)):
        raise ValueError(f"{who}: at must be finite")
    return np.ascontiguousarray(a)


def check_draws(who, n_draws, ancestors, M):
    if isinstance(n_draws, bool) or not isinstance(n_draws, (int, np.integer)) or not 1 <= n_draws < 2 ** 31:
        raise ValueError(f"{who}: n_draws must be an integer in 1..2^31-1")
    S = int(n_draws)
    if ancestors is not None:
        a = np.asarray(ancestors)
        if a.ndim != 1 or a.shape[0] != S or a.dtype == bool or not np.issubdtype(a.dtype, np.integer):
            raise ValueError(f"{who}: ancestors must be a vector of n_draws = {S} integers")
        if M is not None and not np.all((a >= 0) & (a < M)):
            raise ValueError(f"{who}: ancestors must be particles 0..{M - 1}")
        ancestors = a.astype(np.int64)
    return S, ancestors


def merge_forecast_partials(a, b):
    """The partials of the union of two disjoint particle sets (a's particles first)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or a.ndim != 2 or a.shape[1] < P0 or a.shape[0] < 2:
        raise ValueError("partials blocks of one horizon and one set of thresholds have the same shape [1 + H][10 + Tn]")
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
    O[:, MJ], O[:, SJ] = _merge_lse(A[:, MJ] + da, A[:, SJ], B[:, MJ] + db, B[:, SJ])
    O[:, NBAD] = A[:, NBAD] + B[:, NBAD]
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
    O[:, VAR:] = A[:, VAR:] * fa + B[:, VAR:] * fb
    return out


class Forecast:
    """Posterior predictive summaries of y_{T+1..T+H} (arrays of length H; `at` and `cdf` are [H][Tn], None without
    thresholds; lpd_marginal and lpd_joint are None without y_future)."""

    def __init__(self, mean, var, at, cdf, lpd_marginal, lpd_joint, n_bad, n_particles, ess):
        self.mean, self.var, self.at, self.cdf = mean, var, at, cdf
        self.lpd_marginal, self.lpd_joint, self.n_bad = lpd_marginal, lpd_joint, n_bad
        self.horizon = int(np.shape(mean)[0])
        self.n_particles = int(n_particles)       # contributing particles (finite log-weight)
        self.ess = float(ess)                     # effective sample size of the weights

    @property
    def sd(self):
        with np.errstate(invalid="ignore"):
            return np.sqrt(self.var)

    def summary(self):
        """One row per horizon: dict(h, mean, sd, n_bad [, lpd_marginal, lpd_joint] [, cdf])."""
        rows = []
        for i in range(self.horizon):
            r = dict(h=i + 1, mean=float(self.mean[i]), sd=float(self.sd[i]), n_bad=int(self.n_bad[i]))
            if self.lpd_marginal is not None:
                r.update(lpd_marginal=float(self.lpd_marginal[i]), lpd_joint=float(self.lpd_joint[i]))
            if self.cdf is not None:
                r["cdf"] = [float(v) for v in self.cdf[i]]
            rows.append(r)
        return rows


def combine_forecast_partials(partials, Tn=0, has_y=True, at=None):
    """Merges partials blocks of disjoint particle sets in list order and finishes them -> Forecast."""
    partials = list(partials)
    if not partials:
        raise ValueError("combine_forecast_partials: no partials")
    Q = P0 + int(Tn)
    acc = np.array(partials[0], dtype=np.float64, copy=True)
    if acc.ndim != 2 or acc.shape[1] != Q or acc.shape[0] < 2:
        raise ValueError(f"a partials block with {int(Tn)} thresholds is [1 + H][{Q}]")
    for p in partials[1:]:
        acc = merge_forecast_partials(acc, p)
    sw, sw2, cnt = acc[0, 1], acc[0, 2], acc[0, 3]
    P = acc[1:]
    H = P.shape[0]
    at = None if at is None or not Tn else np.asarray(at, dtype=np.float64)
    if cnt == 0.0:
        nan = np.full(H, np.nan)
        return Forecast(nan, nan.copy(), at, np.full((H, Tn), np.nan) if Tn else None, nan.copy() if has_y else None,
                        nan.copy() if has_y else None, np.zeros(H), 0, 0.0)
    bad = P[:, NBAD] > 0.0
    lpd_m = lpd_j = cdf = None
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if has_y:
            lpd_m = np.where(P[:, SA] > 0.0, P[:, MA] + np.log(P[:, SA]) - np.log(sw), -np.inf)
            lpd_j = np.where(P[:, SJ] > 0.0, P[:, MJ] + np.log(P[:, SJ]) - np.log(sw), -np.inf)
        m1 = P[:, S1] / P[:, SW]
        mean = np.where(bad, np.nan, P[:, C0] + m1)
        between = np.maximum(P[:, S2] / P[:, SW] - m1 * m1, 0.0)
        var = np.where(bad, np.nan, P[:, VAR] / P[:, SW] + between)
        if Tn:
            cdf = np.where(bad[:, None], np.nan, P[:, P0:P0 + Tn] / P[:, SW][:, None])
    return Forecast(mean, var, at, cdf, lpd_m, lpd_j, P[:, NBAD].copy(), cnt, sw * sw / sw2)
