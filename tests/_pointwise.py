"""References, error bounds and helpers for the pointwise criteria (smcnuts_amd.criteria; smcn_pointwise_*).

`terms(model, x2)` is the term matrix ll[p, i] of the existing NumPy models (`_glm.GLMNumpy.terms`,
`_glm_disp.GLMDispNumpy.obs`; a dispersion coordinate out of range makes every term of the particle -inf), with the
per-element bound e_term of `device_bounds` (|device - numpy| <= e_term[p, i]), E[y_i | x_p] and its bound.
`criteria_reference(ll, logw)` is the definition in NumPy (max-shifted log-sum-exps, two-pass variance);
`exact_variance` the rational value for the ill-conditioned case; `numpy_partials` builds a partials block from a term
matrix by the documented column layout of include/smcnuts_hip.h, independently of the kernel.

Bounds (`criteria_bounds`), u = 2^-53, M contributing particles, E_i = max_p e_term[p, i], W the normalised weights:
  lppd_i, elpd_loo_i   E_i + (M + 16) u + 4 u |value|: an error e in every term moves a log-sum-exp by at most e; a sum of
                       M non-negative numbers is within M u relative in any order, M u absolute on its log.
  mean_loglik_i        sum_p W_p e_term + (M + 2) u sum_p W_p |ll - c_i| + 4 u |value|, c_i the first contributing term
                       (the device sums ll - c_i).
  p_waic_i             The device forms v = S2 / SW - (S1 / SW)^2 with S1, S2 the weighted first and second moments of
                       a_p = ll_p - c_i.  (1) The variance is shift-invariant, so the terms' errors eps_p (|eps_p| <= E_i)
                       act as a perturbation of the sample: |sd' - sd| <= sd(eps) <= E_i, hence |v' - v| <= 2 sqrt(v) E_i +
                       E_i^2.  (2) Rounding: S2 / SW and (S1 / SW)^2 are each sums of M products with relative error
                       (M + 16) u on sums of non-negative terms bounded by m2 = sum_p W_p a_p^2 (and (S1 / SW)^2 <= m2),
                       so the difference is within 3 (M + 16) u m2.  m2 = v + (mean - c_i)^2 <= v + range^2 scales with the
                       spread of the column, never with ll^2.  Bound: 2 sqrt(v) E_i + E_i^2 + 3 (M + 16) u m2 + 4 u v.
  loo_ess_i            r_p = W_p exp(-ll_p) moves by a factor within exp(+-E_i); (sum r)^2 / sum r^2 then by at most
                       exp(4 E_i); the two sums are within (M + 16) u relative each, the ratio within 4 (M + 16) u:
                       value (expm1(4 E_i) + 4 (M + 16) u).
  fitted_i             sum_p W_p e_mean + (M + 16) u sum_p W_p |mean_p|, e_mean = 8 u |mean| + |d mean / d eta| e_eta.
"""
import math
from fractions import Fraction

import numpy as np

import _glm
import _glm_disp as gd
from _glm import U

FAMILIES = ("bernoulli_logit", "poisson_log", "normal", "neg_binomial_2_log")
N_COLS = 11
MA, SA, MB, SB, SB2, C0, SW, S1, S2, FIT, NINF = range(11)


def synthetic(family, n, p, seed, scale=0.5):
    if family in gd.DISP_FAMILIES:
        return gd.synthetic(family, n, p, seed, scale=scale)
    return _glm.synthetic(family, n, p, seed, scale=scale)


def make(family, n, D, seed, scale=0.5):
    """(GLMTarget, numpy model) with D coordinates, intercept as D % 2."""
    from smcnuts_amd import GLMTarget
    ic = bool(D % 2)
    disp = family in gd.DISP_FAMILIES
    Dc = D - (1 if disp else 0)
    p = Dc - ic
    assert Dc >= 1 and p >= 0, "the dispersion families need D >= 2"
    X, y = synthetic(family, n, p, seed, scale=scale)
    sd = np.linspace(0.8, 2.5, Dc)
    if disp:
        t = GLMTarget(X, y, family=family, prior_sd=sd, intercept=ic, dispersion_prior=(0.0, 1.0))
        m = gd.GLMDispNumpy(X, y, family, sd, (0.0, 1.0), intercept=ic)
    else:
        t = GLMTarget(X, y, family=family, prior_sd=sd, intercept=ic)
        m = _glm.GLMNumpy(X, y, family, sd, intercept=ic)
    return t, m


def points(m, M, seed, scale=0.3):
    rng = np.random.default_rng(seed)
    x = scale * rng.standard_normal((M, m.dim))
    return x


def terms(m, x2):
    """ll [M, n], e_term [M, n], mean = E[y | x] [M, n], e_mean [M, n]."""
    x2 = np.atleast_2d(np.asarray(x2, dtype=np.float64))
    with np.errstate(all="ignore"):
        if m.family in gd.DISP_FAMILIES:
            eta, (term, d, gt, m_term, *_r) = m.obs(x2)
            bad = m.bad(x2[:, -1])
            term = np.where(bad[:, None], -np.inf, term)
            Dc = m.Dc
            A = np.abs(x2[:, :Dc]) @ np.abs(m.Z).T
            e_eta = (2 * Dc + 4) * U * A + 4 * U * np.abs(eta)
            if m.family == "normal":
                # normal_obs counts c0 = -tau - log(2 pi) / 2 at |c0|, but its two addends round at their own size (the
                # device's constant and math.log's differ in the last place): where tau is near -0.919 and the residual
                # small, |c0| + q undercounts.  The magnitudes of the addends, as for the other terms:
                tau = np.where(bad, 0.0, x2[:, -1])[:, None]
                m_term = m_term - np.abs(-tau - gd.HALF_LOG_2PI) + (np.abs(tau) + gd.HALF_LOG_2PI)
            e_term = 64 * U * m_term + np.abs(d) * e_eta
            if m.family == "normal":
                mean, e_mean = eta, e_eta + 8 * U * np.abs(eta)
            else:
                mean = np.exp(eta)
                e_mean = mean * (8 * U + e_eta)
        else:
            eta, term, d = m.terms(x2)
            D = m.dim
            A = np.abs(x2) @ np.abs(m.Z).T
            e_eta = (2 * D + 4) * U * A + 4 * U * np.abs(eta)
            if m.family == "bernoulli_logit":
                t = np.exp(-np.abs(eta))
                sig = np.where(eta >= 0.0, 1.0 / (1.0 + t), t / (1.0 + t))
                mag = np.abs(eta) + np.log1p(t)
                mean, e_mean = sig, 8 * U * sig + sig * (1.0 - sig) * e_eta
            else:
                mu = np.exp(eta)
                mag = np.abs(m.y * eta) + mu + m.lgy
                mean, e_mean = mu, mu * (8 * U + e_eta)
            e_term = 8 * U * mag + np.abs(d) * e_eta
        fin = np.isfinite(term)
        e_term = np.where(fin, e_term, 0.0)
        e_mean = np.where(fin, e_mean, 0.0)
    return term, e_term, mean, e_mean


def _lse0(a):
    """log sum exp over axis 0 around the maximum; -inf where every entry is -inf."""
    with np.errstate(all="ignore"):
        mx = np.max(a, axis=0)
        safe = np.where(np.isfinite(mx), mx, 0.0)
        s = np.sum(np.exp(a - safe), axis=0)
        return np.where(np.isfinite(mx), safe + np.log(s), mx)


def _norm_weights(logw, M):
    lw = np.zeros(M) if logw is None else np.asarray(logw, dtype=np.float64)
    keep = np.isfinite(lw)
    l = lw[keep] - np.max(lw[keep])
    lW = l - np.log(np.sum(np.exp(l)))
    return keep, lW


def criteria_reference(ll, logw=None, mean=None):
    """Section-1 definitions from a term matrix ll [M, n] -> dict of the seven per-observation arrays (+ ess, n_particles)."""
    ll = np.asarray(ll, dtype=np.float64)
    keep, lW = _norm_weights(logw, ll.shape[0])
    ll = ll[keep]
    W = np.exp(lW)[:, None]
    bad = np.any(np.isneginf(ll), axis=0)
    with np.errstate(all="ignore"):
        lppd = _lse0(lW[:, None] + ll)
        llz = np.where(np.isfinite(ll), ll, 0.0)
        mu = np.sum(W * llz, axis=0)
        mu = mu + np.sum(W * (llz - mu), axis=0)             # (second pass)
        var = np.sum(W * (llz - mu) ** 2, axis=0)
        a = lW[:, None] - llz
        loo = -_lse0(a)
        ess = np.exp(2.0 * _lse0(a) - _lse0(2.0 * a))
        fit = np.full(ll.shape[1], np.nan) if mean is None else np.sum(W * np.where(np.isfinite(ll), mean[keep], 0.0), axis=0)
        out = dict(lppd_i=lppd, mean_loglik_i=np.where(bad, -np.inf, mu), p_waic_i=np.where(bad, np.nan, var),
                   elpd_waic_i=np.where(bad, np.nan, lppd - var), elpd_loo_i=np.where(bad, -np.inf, loo),
                   loo_ess_i=np.where(bad, 0.0, ess), fitted_i=np.where(bad, np.nan, fit))
    out["ess"] = float(1.0 / np.sum(np.exp(2.0 * lW)))
    out["n_particles"] = int(np.sum(keep))
    return out


def criteria_bounds(ll, logw, e_term, mean, e_mean):
    """Per-observation |device - reference| bounds (module docstring); NaN / inf entries of the reference are compared
    by pattern, their bounds are irrelevant."""
    ll = np.asarray(ll, dtype=np.float64)
    keep, lW = _norm_weights(logw, ll.shape[0])
    ll, e_term, mean, e_mean = ll[keep], e_term[keep], mean[keep], e_mean[keep]
    M = ll.shape[0]
    W = np.exp(lW)[:, None]
    ref = criteria_reference(ll, lW, mean)
    fin = np.isfinite(ll)
    with np.errstate(all="ignore"):
        E = np.max(np.where(fin, e_term, 0.0), axis=0)
        first = np.argmax(fin, axis=0)
        c = ll[first, np.arange(ll.shape[1])]
        a = np.where(fin, ll - c, 0.0)
        m2 = np.sum(W * a * a, axis=0)
        v = np.nan_to_num(ref["p_waic_i"], nan=0.0, posinf=0.0)
        b = dict(
            lppd_i=E + (M + 16) * U + 4 * U * np.abs(ref["lppd_i"]),
            elpd_loo_i=E + (M + 16) * U + 4 * U * np.abs(ref["elpd_loo_i"]),
            mean_loglik_i=np.sum(W * e_term, axis=0) + (M + 2) * U * np.sum(W * np.abs(a), axis=0)
            + 4 * U * np.abs(ref["mean_loglik_i"]),
            p_waic_i=2.0 * np.sqrt(v) * E + E * E + 3 * (M + 16) * U * m2 + 4 * U * v,
            loo_ess_i=ref["loo_ess_i"] * (np.expm1(4.0 * E) + 4 * (M + 16) * U),
            fitted_i=np.sum(W * np.where(fin, e_mean, 0.0), axis=0) + (M + 16) * U * np.sum(W * np.where(fin, np.abs(mean), 0.0), axis=0),
        )
        b["elpd_waic_i"] = b["lppd_i"] + b["p_waic_i"]
    return ref, {k: np.where(np.isfinite(val), val, 0.0) for k, val in b.items()}


def weight_shift_bounds(ll, logw, mean, delta):
    """How far the criteria move when every log-weight moves by at most delta (the rounding of lw + 1e5: delta =
    u max |lw + 1e5|).  The normalised weights then move by factors within exp(+-2 delta), r = expm1(2 delta):
      lppd_i, elpd_loo_i  logs of ratios of two sums that each move by a factor within exp(+-delta): 2 delta
      mean_loglik_i       |sum (W' - W)(ll - mean)| <= r sum W |ll - mean| =: r A1
      p_waic_i            with a = ll - mean: |sum W' a^2 - (sum W' a)^2 - v| <= r sum W a^2 + (r A1)^2
      loo_ess_i           r_p moves within exp(+-2 delta), (sum r)^2 / sum r^2 within exp(+-8 delta): value expm1(8 delta)
      fitted_i            r sum W |mean_p - fitted|."""
    ll = np.asarray(ll, dtype=np.float64)
    keep, lW = _norm_weights(logw, ll.shape[0])
    ref = criteria_reference(ll, logw, mean)
    ll, mean = ll[keep], mean[keep]
    W = np.exp(lW)[:, None]
    r = math.expm1(2.0 * delta)
    with np.errstate(all="ignore"):
        fin = np.isfinite(ll)
        a = np.where(fin, ll - ref["mean_loglik_i"], 0.0)
        a = np.where(np.isfinite(a), a, 0.0)
        A1 = np.sum(W * np.abs(a), axis=0)
        dm = np.where(fin, np.abs(mean - ref["fitted_i"]), 0.0)
        b = dict(lppd_i=np.full(ll.shape[1], 2.0 * delta), elpd_loo_i=np.full(ll.shape[1], 2.0 * delta),
                 mean_loglik_i=r * A1, p_waic_i=r * np.sum(W * a * a, axis=0) + (r * A1) ** 2,
                 loo_ess_i=ref["loo_ess_i"] * math.expm1(8.0 * delta),
                 fitted_i=r * np.sum(W * np.where(np.isfinite(dm), dm, 0.0), axis=0))
        b["elpd_waic_i"] = b["lppd_i"] + b["p_waic_i"]
    return {k: np.where(np.isfinite(v), v, 0.0) for k, v in b.items()}


def as_ref(pointwise):
    """A Pointwise's per-observation arrays in the form assert_pointwise takes as its reference."""
    return {k: np.asarray(getattr(pointwise, k)) for k in FIELDS}


FIELDS = ("lppd_i", "mean_loglik_i", "p_waic_i", "elpd_waic_i", "elpd_loo_i", "loo_ess_i", "fitted_i")


def assert_pointwise(got, ref, bounds, factor=1.0, what="", close=None, report=None):
    """Element by element: the same non-finite pattern, |got - ref| <= factor * bound elsewhere."""
    for k in FIELDS:
        g, r, b = np.asarray(getattr(got, k)), np.asarray(ref[k]), factor * bounds[k]
        fin = np.isfinite(r)
        np.testing.assert_array_equal(np.isnan(g), np.isnan(r), err_msg=f"{what} {k}: NaN pattern")
        np.testing.assert_array_equal(g[~fin & ~np.isnan(r)], r[~fin & ~np.isnan(r)], err_msg=f"{what} {k}: infinities")
        err = np.abs(g[fin] - r[fin])
        if report is not None:
            with np.errstate(all="ignore"):
                report[k] = max(report.get(k, 0.0), float(np.max(err / np.maximum(b[fin], 1e-300), initial=0.0)))
        worst = int(np.argmax(err - b[fin])) if err.size else 0
        assert np.all(err <= b[fin]), (f"{what} {k}: |got - ref| = {err[worst]:.3e} > bound {b[fin][worst]:.3e} "
                                       f"(got {g[fin][worst]!r}, ref {r[fin][worst]!r})")
        if close is not None and err.size:
            close(g[fin], r[fin], rtol=0.0, atol=float(np.max(b[fin])), what=f"pointwise {k}")


def exact_variance(col):
    """Equal-weight variance (divisor M) of the float64 numbers `col`, in rational arithmetic."""
    fr = [Fraction(float(v)) for v in col]
    M = len(fr)
    mean = sum(fr) / M
    return float(sum((v - mean) ** 2 for v in fr) / M)


def naive_variance(col):
    """sum W ll^2 - mean^2 in float64 (what the kernels must NOT do)."""
    col = np.asarray(col, dtype=np.float64)
    W = 1.0 / col.shape[0]
    return float(np.sum(W * col * col) - np.sum(W * col) ** 2)


def numpy_partials(ll, logw=None, mean=None):
    """A partials block [1 + n][11] from a term matrix, by the documented layout (include/smcnuts_hip.h)."""
    ll = np.asarray(ll, dtype=np.float64)
    M, n = ll.shape
    lw = np.zeros(M) if logw is None else np.asarray(logw, dtype=np.float64)
    mean = np.zeros_like(ll) if mean is None else mean
    out = np.zeros((1 + n, N_COLS))
    keep = np.isfinite(lw)
    if not np.any(keep):
        out[0, 0] = -np.inf
        out[1:, MA] = out[1:, MB] = -np.inf
        out[1:, C0] = np.nan
        return out
    mw = np.max(lw[keep])
    l = lw[keep] - mw
    w = np.exp(l)
    out[0, :4] = mw, np.sum(w), np.sum(w * w), np.sum(keep)
    llk, mk = ll[keep], mean[keep]
    for i in range(n):
        col = llk[:, i]
        fin = np.isfinite(col)
        r = out[1 + i]
        r[NINF] = np.sum(~fin)
        if not np.any(fin):
            r[MA] = r[MB] = -np.inf
            r[C0] = np.nan
            continue
        cf, lf, wf = col[fin], l[fin], w[fin]
        a, b = lf + cf, lf - cf
        r[MA], r[MB] = np.max(a), np.max(b)
        r[SA] = np.sum(np.exp(a - r[MA]))
        e = np.exp(b - r[MB])
        r[SB], r[SB2] = np.sum(e), np.sum(e * e)
        r[C0] = cf[0]
        d = cf - cf[0]
        r[SW], r[S1], r[S2] = np.sum(wf), np.sum(wf * d), np.sum(wf * d * d)
        r[FIT] = np.sum(wf * mk[fin, i])
    return out
