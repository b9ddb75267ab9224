"""Pointwise predictive criteria from the device's mergeable partials (include/smcnuts_hip.h, smcn_pointwise_partials).

For M particles with log-weights lw_p (W_p = exp(lw_p) / sum_q exp(lw_q)) and ll[p, i] = log p(y_i | x_p), per
observation i:
  lppd_i        = log sum_p W_p exp(ll[p, i])
  mean_loglik_i = sum_p W_p ll[p, i]
  p_waic_i      = sum_p W_p (ll[p, i] - mean_loglik_i)^2
  elpd_waic_i   = lppd_i - p_waic_i
  elpd_loo_i    = -log sum_p W_p exp(-ll[p, i])               (plain importance-sampling LOO)
  loo_ess_i     = (sum_p r_p)^2 / sum_p r_p^2, r_p = W_p exp(-ll[p, i])
  fitted_i      = sum_p W_p E[y_i | x_p]
Plain IS-LOO has heavy-tailed ratios: `loo_ess_i` is the effective number of particles behind `elpd_loo_i`, and a value
of a few says that observation's estimate is not to be trusted: `GLMTarget.loo` / `SMCSampler.loo` (psis.py) smooth the
tail of the ratios on the device and report the Pareto shape k beside the smoothed elpd_loo_i.

Rules: a particle with a non-finite log-weight contributes to nothing.  An observation for which some contributing
particle has ll = -inf keeps lppd_i as defined (that particle adds 0), has mean_loglik_i = elpd_loo_i = -inf,
loo_ess_i = 0, and NaN for p_waic_i, elpd_waic_i and fitted_i; the other observations are unaffected.
"""
import numpy as np

# columns of a partials block (row 0: header [mw, sw, sw2, cnt, 0 ..]; row 1 + i: observation i)
MA, SA, MB, SB, SB2, C0, SW, S1, S2, FIT, NINF = range(11)
N_COLS = 11


def _merge_lse(m1, s1, m2, s2, *more):
    """Max-shifted sums (m, s [, squares]) of two sets -> of their union; `more` = (q1, q2): sums of squared terms."""
    with np.errstate(invalid="ignore", over="ignore"):
        m = np.maximum(m1, m2)
        e1 = np.where(s1 > 0.0, np.exp(np.where(s1 > 0.0, m1 - m, 0.0)), 0.0)
        e2 = np.where(s2 > 0.0, np.exp(np.where(s2 > 0.0, m2 - m, 0.0)), 0.0)
        m = np.where(s1 > 0.0, np.where(s2 > 0.0, m, m1), m2)
        out = [m, s1 * e1 + s2 * e2]
        if more:
            out.append(more[0] * e1 * e1 + more[1] * e2 * e2)
    return out


def merge_pointwise_partials(a, b):
    """The partials of the union of two disjoint particle sets (a's particles first)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or a.ndim != 2 or a.shape[1] != N_COLS:
        raise ValueError("partials blocks of one model have the same shape [1 + n][%d]" % N_COLS)
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
    O[:, MB], O[:, SB], O[:, SB2] = _merge_lse(A[:, MB] + da, A[:, SB], B[:, MB] + db, B[:, SB], A[:, SB2], B[:, SB2])
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
    O[:, FIT] = A[:, FIT] * fa + B[:, FIT] * fb
    O[:, NINF] = A[:, NINF] + B[:, NINF]
    return out


def _se(v):
    n = v.shape[0]
    with np.errstate(invalid="ignore"):
        return float(np.sqrt(n * np.var(v, ddof=1))) if n > 1 else float("nan")


class Pointwise:
    """Per-observation criteria of one fitted model (arrays of length n) and their totals."""

    def __init__(self, lppd_i, mean_loglik_i, p_waic_i, elpd_waic_i, elpd_loo_i, loo_ess_i, fitted_i, n_particles, ess):
        self.lppd_i, self.mean_loglik_i, self.p_waic_i = lppd_i, mean_loglik_i, p_waic_i
        self.elpd_waic_i, self.elpd_loo_i, self.loo_ess_i, self.fitted_i = elpd_waic_i, elpd_loo_i, loo_ess_i, fitted_i
        self.n_particles = int(n_particles)       # contributing particles (finite log-weight)
        self.ess = float(ess)                     # effective sample size of the weights
        self.n_obs = int(lppd_i.shape[0])

    lppd = property(lambda self: float(np.sum(self.lppd_i)))
    p_waic = property(lambda self: float(np.sum(self.p_waic_i)))
    elpd_waic = property(lambda self: float(np.sum(self.elpd_waic_i)))
    elpd_loo = property(lambda self: float(np.sum(self.elpd_loo_i)))
    se_elpd_waic = property(lambda self: _se(self.elpd_waic_i))
    se_elpd_loo = property(lambda self: _se(self.elpd_loo_i))

    def summary(self):
        return dict(n_obs=self.n_obs, n_particles=self.n_particles, ess=self.ess, lppd=self.lppd, p_waic=self.p_waic,
                    elpd_waic=self.elpd_waic, se_elpd_waic=self.se_elpd_waic, elpd_loo=self.elpd_loo,
                    se_elpd_loo=self.se_elpd_loo, min_loo_ess=float(np.min(self.loo_ess_i)),
                    n_nonfinite=int(np.sum(~np.isfinite(self.elpd_waic_i))))


def combine_pointwise_partials(partials):
    """Merges partials blocks of disjoint particle sets in list order and finishes them -> Pointwise."""
    partials = list(partials)
    if not partials:
        raise ValueError("combine_pointwise_partials: no partials")
    acc = np.array(partials[0], dtype=np.float64, copy=True)
    if acc.ndim != 2 or acc.shape[1] != N_COLS:
        raise ValueError("a partials block is [1 + n][%d]" % N_COLS)
    for p in partials[1:]:
        acc = merge_pointwise_partials(acc, p)
    sw, sw2, cnt = acc[0, 1], acc[0, 2], acc[0, 3]
    P = acc[1:]
    n = P.shape[0]
    if cnt == 0.0:
        nan = np.full(n, np.nan)
        return Pointwise(nan, nan.copy(), nan.copy(), nan.copy(), nan.copy(), nan.copy(), nan.copy(), 0, 0.0)
    bad = P[:, NINF] > 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        lsw = np.log(sw)
        lppd = np.where(P[:, SA] > 0.0, P[:, MA] + np.log(P[:, SA]) - lsw, -np.inf)
        m1 = P[:, S1] / P[:, SW]
        mean = P[:, C0] + m1
        var = np.maximum(P[:, S2] / P[:, SW] - m1 * m1, 0.0)
        loo = -(P[:, MB] + np.log(P[:, SB]) - lsw)
        less = P[:, SB] * P[:, SB] / P[:, SB2]
        fit = P[:, FIT] / P[:, SW]
    mean = np.where(bad, -np.inf, mean)
    loo = np.where(bad, -np.inf, loo)
    less = np.where(bad, 0.0, less)
    var = np.where(bad, np.nan, var)
    fit = np.where(bad, np.nan, fit)
    with np.errstate(invalid="ignore"):
        waic = np.where(bad, np.nan, lppd - var)
    return Pointwise(lppd, mean, var, waic, loo, less, fit, cnt, sw * sw / sw2)


def compare(a, b):
    """a against b on the same observations: the differences of the elpd totals (a - b) with their paired standard errors
    sqrt(n var_i(diff_i, ddof=1))."""
    if a.n_obs != b.n_obs:
        raise ValueError(f"compare: the two were computed on different numbers of observations ({a.n_obs} and {b.n_obs})")
    with np.errstate(invalid="ignore"):
        dw, dl = a.elpd_waic_i - b.elpd_waic_i, a.elpd_loo_i - b.elpd_loo_i
    return dict(elpd_waic_diff=float(np.sum(dw)), se_elpd_waic_diff=_se(dw), elpd_loo_diff=float(np.sum(dl)),
                se_elpd_loo_diff=_se(dl), n_obs=a.n_obs)
