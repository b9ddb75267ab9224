"""One-step residual checks of an arma fit from the device's mergeable partials (include/smcnuts_hip.h,
smcn_residuals_partials): does ARMA(1,1) describe the series at all?

Per particle x = (mu, beta, theta, log sigma) and the series y_1..y_T the density's own chain gives the innovations
err_t, the one-step means nu_t = y_t - err_t, the standardised residuals r_t = err_t / sigma, the one-step log densities
l_t = log N(y_t | nu_t, sigma) (their sum is the arma log-likelihood) and the PIT values Phi(r_t).  Over the particles
with weights W_p:
  mean_t = sum_p W_p nu_t,  var_t = sum_p W_p sigma^2 + sum_p W_p (nu_t - mean_t)^2      the one-step predictive law of y_t
  lpd_t  = log sum_p W_p N(y_t | nu_t, sigma),  lppd = sum_t lpd_t                      (in-sample, one step ahead)
  z_t, z_sd_t    the posterior mean and sd of r_t;   pit_t = sum_p W_p Phi(r_t)
With L lags, per particle (uncentred: the innovations have mean 0 under the model; a mean residual shows in z)
  rho_k = sum_{t>k} r_t r_{t-k} / sum_t r_t^2,     Q = T (T + 2) sum_{k<=L} rho_k^2 / (T - k)          (Ljung-Box)
and acf, acf_sd, ljung_box, ljung_box_sd are their posterior means and sds.  Q is a REALISED discrepancy: evaluated at a
draw from the posterior the r_t are iid N(0, 1) if the model holds, so Q is compared with chi-square on L degrees of
freedom, with NO correction for the p + q fitted parameters (that correction belongs to residuals at a point estimate).
exceed[j] is the posterior probability that Q exceeds the chi-square 1 - levels[j] quantile, critical[j]: near levels[j]
when the model holds, near 1 when the residuals are autocorrelated.

Rules, continuing forecast.py: a particle with a non-finite log-weight contributes to nothing.  A contributing particle
whose sigma is not finite and positive, or whose err_t or r_t is not finite, is counted in n_bad[t] and adds nothing to
row t; a row with n_bad > 0 reports NaN moments, z and pit, and its lpd over the other particles.  A particle that is bad
at any t, or whose sum of squares or Q is not finite and positive, is counted in n_bad_acf and adds nothing to the lag
rows, which then report NaN.  Every second moment is accumulated around a shift and merged by re-centring.
A chain on its way to overflowing passes through steps where err_t and r_t are still finite but their squares are not
(beyond about 1e154): there the particle is not yet bad, n_bad[t] may be 0, and var[t] and z_sd[t] are inf or NaN.
"""
import math

import numpy as np

from .criteria import _merge_lse

MAX_LAGS = 32
MAX_LEVELS = 8
QC = 20                                 # columns of a partials block
# columns (row 0: header [mw, sw, sw2, cnt, 0 ..]; rows 1..T: the time rows; then L lag rows and the Q row)
ML, SL, NBAD, C0, SW, S1, S2, VAR, CZ, Z1, Z2, PIT = range(12)
P0 = 12                                 # 12 + j: sum w [Q > q_at[j]] (the Q row)


def default_lags(T):
    return min(10, int(T) // 5)


def check_lags(who, lags, T):
    """The number of lags L in 0..32 with L <= T - 1; None: min(10, T // 5)."""
    if lags is None:
        return default_lags(T)
    if isinstance(lags, bool) or not isinstance(lags, (int, np.integer)) or not 0 <= lags <= MAX_LAGS:
        raise ValueError(f"{who}: lags must be an integer in 0..{MAX_LAGS}")
    if lags > T - 1:
        raise ValueError(f"{who}: lags = {int(lags)} needs a series of at least {int(lags) + 1} values (T = {int(T)})")
    return int(lags)


def check_levels(who, levels):
    """The test levels, each in (0, 1), at most 8 -> a tuple of floats."""
    try:
        lv = np.atleast_1d(np.asarray(levels, dtype=np.float64))
    except (TypeError, ValueError):
        raise ValueError(f"{who}: levels must be numeric") from None
    if lv.ndim != 1 or lv.size > MAX_LEVELS:
        raise ValueError(f"{who}: levels must be a scalar or a vector of at most {MAX_LEVELS} values")
    if not np.all((lv > 0.0) & (lv < 1.0)):
        raise ValueError(f"{who}: every level must lie in (0, 1)")
    return tuple(float(v) for v in lv)


# ---- chi-square tails: the regularised incomplete gamma functions, series below x = a + 1 and continued fraction above ----
def _gamma_pq(a, x):
    """(P(a, x), Q(a, x)), each to a few ulp of itself where it is the smaller of the two."""
    if x <= 0.0:
        return 0.0, 1.0
    if math.isinf(x):
        return 1.0, 0.0
    pre = math.exp(a * math.log(x) - x - math.lgamma(a))
    if x < a + 1.0:
        ap, term = a, 1.0 / a
        tot = term
        for _ in range(100000):
            ap += 1.0
            term *= x / ap
            tot += term
            if abs(term) < abs(tot) * 1e-17:
                break
        p = min(tot * pre, 1.0)
        return p, 1.0 - p
    tiny = 1e-300
    b = x + 1.0 - a
    c, d = 1.0 / tiny, 1.0 / b
    h = d
    for i in range(1, 100000):
        an = -i * (i - a)
        b += 2.0
        d = an * d + b
        d = tiny if abs(d) < tiny else d
        c = b + an / c
        c = tiny if abs(c) < tiny else c
        d = 1.0 / d
        de = d * c
        h *= de
        if abs(de - 1.0) < 1e-16:
            break
    q = min(h * pre, 1.0)
    return 1.0 - q, q


def _check_df(df):
    if not df > 0:
        raise ValueError("chi-square: df must be positive")
    return 0.5 * float(df)


def chi2_sf(x, df):
    """P(X > x) of a chi-square variable on df degrees of freedom."""
    return _gamma_pq(_check_df(df), 0.5 * float(x))[1]


def chi2_isf(p, df):
    """The x with chi2_sf(x, df) = p, by bisection (on the upper tail for p <= 1/2, on the lower one above)."""
    a, p = _check_df(df), float(p)
    if not 0.0 <= p <= 1.0:
        raise ValueError("chi2_isf: p must lie in [0, 1]")
    if p == 0.0:
        return math.inf
    if p == 1.0:
        return 0.0
    upper = p <= 0.5
    over = (lambda x: _gamma_pq(a, 0.5 * x)[1] > p) if upper else (lambda x: _gamma_pq(a, 0.5 * x)[0] < 1.0 - p)
    lo, hi = 0.0, max(2.0 * a, 1.0)          # over(lo), not over(hi): the root lies between
    while over(hi):
        lo, hi = hi, 2.0 * hi
    for _ in range(2000):
        mid = 0.5 * (lo + hi)
        if mid <= lo or mid >= hi:
            break
        if over(mid):
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


# ---- partials --------------------------------------------------------------------------------------------------------------
def block_rows(T, lags):
    return 1 + int(T) + (int(lags) + 1 if lags else 0)


def merge_residual_partials(a, b):
    """The partials of the union of two disjoint particle sets (a's particles first)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or a.ndim != 2 or a.shape[1] != QC or a.shape[0] < 2:
        raise ValueError(f"partials blocks of one series and one number of lags have the same shape [1 + T (+ L + 1)][{QC}]")
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
    O[:, ML], O[:, SL] = _merge_lse(A[:, ML] + da, A[:, SL], B[:, ML] + db, B[:, SL])
    O[:, NBAD] = A[:, NBAD] + B[:, NBAD]
    # the two moment groups: both to the common weight scale, b's re-centred on a's shift
    swb = B[:, SW] * fb
    for c0, c1, c2 in ((C0, S1, S2), (CZ, Z1, Z2)):
        ha, hb = ~np.isnan(A[:, c0]), ~np.isnan(B[:, c0])
        with np.errstate(invalid="ignore"):
            d = np.where(ha & hb, B[:, c0] - A[:, c0], 0.0)
        s1b, s2b = B[:, c1] * fb, B[:, c2] * fb
        O[:, c0] = np.where(ha, A[:, c0], B[:, c0])
        O[:, c1] = A[:, c1] * fa + (s1b + d * swb)
        O[:, c2] = A[:, c2] * fa + (s2b + d * (2.0 * s1b + d * swb))
    O[:, SW] = A[:, SW] * fa + swb
    for col in [VAR] + list(range(PIT, QC)):
        O[:, col] = A[:, col] * fa + B[:, col] * fb
    return out


class OneStepResiduals:
    """In-sample one-step checks of an arma fit.  Arrays of length T: mean, var, sd (the one-step predictive law of y_t),
    lpd (lppd: their sum), z, z_sd (posterior mean and sd of the standardised residual), pit, n_bad.  With lags > 0,
    arrays of length `lags`: acf, acf_sd; acf_band = 1.96 / sqrt(T); ljung_box, ljung_box_sd; levels, critical and
    exceed (one per level); n_bad_acf.  With lags = 0 these are None."""

    def __init__(self, mean, var, lpd, z, z_sd, pit, n_bad, acf, acf_sd, ljung_box, ljung_box_sd, levels, critical, exceed,
                 n_bad_acf, n_particles, ess):
        self.mean, self.var, self.lpd, self.z, self.z_sd, self.pit, self.n_bad = mean, var, lpd, z, z_sd, pit, n_bad
        self.T = int(np.shape(mean)[0])
        self.lags = 0 if acf is None else int(np.shape(acf)[0])
        self.acf, self.acf_sd = acf, acf_sd
        self.acf_band = 1.96 / math.sqrt(self.T) if self.lags else None
        self.ljung_box, self.ljung_box_sd = ljung_box, ljung_box_sd
        self.levels, self.critical, self.exceed, self.n_bad_acf = levels, critical, exceed, n_bad_acf
        self.n_particles = int(n_particles)       # contributing particles (finite log-weight)
        self.ess = float(ess)                     # effective sample size of the weights

    @property
    def sd(self):
        with np.errstate(invalid="ignore"):
            return np.sqrt(self.var)

    @property
    def lppd(self):
        return float(np.sum(self.lpd))

    def summary(self):
        """dict(lppd, n_particles, ess [, ljung_box, ljung_box_sd, critical, exceed, acf, acf_band, n_bad_acf], rows): one
        row per t, dict(t, mean, sd, lpd, z, pit, n_bad)."""
        out = dict(lppd=self.lppd, n_particles=self.n_particles, ess=self.ess)
        if self.lags:
            out.update(lags=self.lags, ljung_box=float(self.ljung_box), ljung_box_sd=float(self.ljung_box_sd),
                       levels=list(self.levels), critical=[float(v) for v in self.critical],
                       exceed=[float(v) for v in self.exceed], acf=[float(v) for v in self.acf], acf_band=self.acf_band,
                       n_bad_acf=int(self.n_bad_acf))
        sd = self.sd
        out["rows"] = [dict(t=i + 1, mean=float(self.mean[i]), sd=float(sd[i]), lpd=float(self.lpd[i]), z=float(self.z[i]),
                            pit=float(self.pit[i]), n_bad=int(self.n_bad[i])) for i in range(self.T)]
        return out


def _shifted(P, c0, c1, c2, bad):
    """(mean, variance) of a shifted moment group, NaN on the rows `bad`."""
    m1 = P[:, c1] / P[:, SW]
    return np.where(bad, np.nan, P[:, c0] + m1), np.where(bad, np.nan, np.maximum(P[:, c2] / P[:, SW] - m1 * m1, 0.0))


def combine_residual_partials(partials, lags, levels=()):
    """Merges partials blocks of disjoint particle sets in list order and finishes them -> OneStepResiduals.  `levels`:
    the test levels whose chi-square quantiles (chi2_isf(level, lags)) the blocks' thresholds of Q were."""
    partials = list(partials)
    if not partials:
        raise ValueError("combine_residual_partials: no partials")
    L, levels = int(lags), tuple(levels) if lags else ()
    acc = np.array(partials[0], dtype=np.float64, copy=True)
    T = acc.shape[0] - 1 - (L + 1 if L else 0) if acc.ndim == 2 else 0
    if acc.ndim != 2 or acc.shape[1] != QC or T < 1:
        raise ValueError(f"a partials block with {L} lags is [1 + T{' + ' + str(L + 1) if L else ''}][{QC}]")
    for p in partials[1:]:
        acc = merge_residual_partials(acc, p)
    sw, sw2, cnt = acc[0, 1], acc[0, 2], acc[0, 3]
    critical = tuple(chi2_isf(v, L) for v in levels)
    nanv = lambda n: np.full(n, np.nan)                 # noqa: E731
    if cnt == 0.0:
        lag = (nanv(L), nanv(L), np.nan, np.nan, levels, critical, nanv(len(levels)), 0) if L else (None,) * 7 + (None,)
        return OneStepResiduals(nanv(T), nanv(T), nanv(T), nanv(T), nanv(T), nanv(T), np.zeros(T), *lag, 0, 0.0)
    P, G = acc[1:1 + T], acc[1 + T:]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        bad = P[:, NBAD] > 0.0
        lpd = np.where(P[:, SL] > 0.0, P[:, ML] + np.log(P[:, SL]) - np.log(sw), -np.inf)
        mean, between = _shifted(P, C0, S1, S2, bad)
        var = P[:, VAR] / P[:, SW] + between
        z, zv = _shifted(P, CZ, Z1, Z2, bad)
        pit = np.where(bad, np.nan, P[:, PIT] / P[:, SW])
        lag = (None,) * 8
        if L:
            gm, gv = _shifted(G, C0, S1, S2, G[:, NBAD] > 0.0)
            exceed = np.where(G[L, NBAD] > 0.0, np.nan, G[L, P0:P0 + len(levels)] / G[L, SW])
            lag = (gm[:L], np.sqrt(gv[:L]), float(gm[L]), float(np.sqrt(gv[L])), levels, critical, exceed, int(G[L, NBAD]))
        return OneStepResiduals(mean, var, lpd, z, np.sqrt(zv), pit, P[:, NBAD].copy(), *lag, cnt, sw * sw / sw2)
