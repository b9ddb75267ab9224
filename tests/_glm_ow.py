"""Reference densities for the GLM target with per-observation offsets and weights (GLMTarget(offset=, weights=);
SMCN_MODEL_OGLM), over tests/_glm.py's and tests/_glm_disp.py's models:

  eta_i = [b_0 +] X_i b + o_i,   llik = sum_i w_i l(y_i | eta_i [, tau]),   grad = sum_i w_i d_i X_i  (tau: sum_i w_i gt_i),

a row with w_i = 0 contributing exactly 0 whatever its term is, and the families' -inf rules looking at the rows with
w_i != 0 only.  `GLMOWNumpy` has the reference's StanModel surface (.dim, .logpdf(x, phi), .logpdfgrad(x, phi),
.constrain(x)): it runs through HostTarget and oracle/pynuts.PyNUTS.

The per-observation terms ARE the parent helpers': they are called on a model whose design carries o as one more column,
at points that carry a 1 in that column's place, so eta = Z b + o comes out of their own matrix product.

`exact_parts` takes every sum with math.fsum over the float64 addends w_i term_i (one rounding of the exact sum of the
rounded products).  `device_bounds` is the parent helpers' bound with the two roundings the device adds, derived:
  eta_i:       the device adds o_i to its D fused multiply-adds in one rounding, u (|eta_i - o_i| + |o_i|); the
               reference's product has one more addend, covered by taking A_i = sum_j |b_j Z_ij| + |o_i| in the parent's
               (2 D + 4) u A_i;
  w_i term_i:  one rounding of the product on the device and one in the reference, u |w_i term_i| each, on top of w_i
               times the term's own error; the sums over n are then within (n + 2) u of sum_i |w_i term_i| -- and the
               same for w_i d_i and w_i gt_i.
`mp_llik` is the 40-digit mpmath value.
"""
import math

import numpy as np

import _glm
import _glm_disp
from _glm import HALF_LOG_2PI, U

CANONICAL = ("bernoulli_logit", "poisson_log")
FAMILIES = CANONICAL + _glm_disp.DISP_FAMILIES


class GLMOWNumpy:
    def __init__(self, X, y, family="bernoulli_logit", prior_sd=2.5, intercept=True, dispersion_prior=(0.0, 2.5),
                 offset=None, weights=None):
        X = np.asarray(X, dtype=np.float64)
        if X.ndim == 1:
            X = X.reshape(-1, 1)
        n = X.shape[0]
        self.family, self.intercept = family, bool(intercept)
        self.disp = family in _glm_disp.DISP_FAMILIES
        self.o = np.zeros(n) if offset is None else np.asarray(offset, dtype=np.float64).copy()
        self.w = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64).copy()
        self.has_offset, self.has_weights = offset is not None, weights is not None
        # the model without offsets and weights (priors, names, Z), and the one whose design carries o as its last column
        Xo = np.hstack([X, self.o[:, None]])
        if self.disp:
            self.base = _glm_disp.GLMDispNumpy(X, y, family, prior_sd, dispersion_prior, intercept)
            sd = np.concatenate([self.base.s[:-1], [1.0]])
            self.aug = _glm_disp.GLMDispNumpy(Xo, y, family, sd, dispersion_prior, intercept)
            self.Dc = self.base.Dc
        else:
            self.base = _glm.GLMNumpy(X, y, family, prior_sd, intercept)
            self.aug = _glm.GLMNumpy(Xo, y, family, np.concatenate([self.base.s, [1.0]]), intercept)
            self.Dc = self.base.dim
        self.Z, self.y = self.base.Z, self.base.y
        self.dim = self.constrained_dim = self.base.dim
        self.live = self.w != 0.0
        self.calls = 0

    def param_names(self):
        return self.base.param_names()

    def at(self, X_new, y_new=None, offset_new=None):
        """The model at new rows (priors kept, weights 1: weights belong to the training likelihood); y_new = None: zeros,
        as the device's block carries them."""
        X_new = np.asarray(X_new, dtype=np.float64).reshape(-1, self.Z.shape[1] - self.intercept)
        y = np.zeros(X_new.shape[0]) if y_new is None else y_new
        sd = self.base.s[:self.Dc]
        dp = (self.base.m[-1], self.base.s[-1]) if self.disp else (0.0, 2.5)
        return GLMOWNumpy(X_new, y, self.family, sd, self.intercept, dp, offset_new, None)

    def pair(self, x2):
        """(the parent helper's model whose design carries o as its last column, x2 with a 1 in that column's place):
        what tests/_pointwise.py, _predict.py and _predict_draws.py take as (model, points) for terms that include o."""
        return self.aug, self._aug_points(np.atleast_2d(np.asarray(x2, dtype=np.float64)))

    def constrain(self, x):
        return self.base.constrain(x) if self.disp else np.array(x, dtype=np.float64, copy=True)

    def _aug_points(self, x2):
        return np.concatenate([x2[:, :self.Dc], np.ones((x2.shape[0], 1)), x2[:, self.Dc:]], axis=1)

    def obs(self, x2):
        """eta [M, n], then (term, d, gt or None) per observation, unweighted, and the parent's magnitudes (dispersion
        families: m_term, m_d, m_gt, w_d, w_gt; else None)."""
        x2 = np.atleast_2d(np.asarray(x2, dtype=np.float64))
        xa = self._aug_points(x2)
        if self.disp:
            eta, (term, d, gt, *mags) = self.aug.obs(xa)
            return eta, term, d, gt, mags
        eta, term, d = self.aug.terms(xa)
        return eta, term, d, None, None

    def bad(self, x2):
        """particles whose dispersion coordinate is out of range (llik = -inf whatever the rows are)"""
        return self.base.bad(x2[:, -1]) if self.disp else np.zeros(x2.shape[0], dtype=bool)

    def lpri_terms(self, x2):
        if self.disp:
            v = x2 - self.base.m
            return -0.5 * (v / self.base.s) ** 2 - np.log(self.base.s) - HALF_LOG_2PI, -v / self.base.s ** 2
        return -0.5 * (x2 / self.base.s) ** 2 - np.log(self.base.s) - HALF_LOG_2PI, -x2 / self.base.s ** 2

    def weighted(self, x2):
        """(w term, w d, w gt) [M, n] with exact zeros in the columns of the rows with w = 0"""
        _, term, d, gt, _ = self.obs(x2)
        L = self.live
        with np.errstate(invalid="ignore", over="ignore"):
            wt = np.where(L, self.w * np.where(L, term, 0.0), 0.0)
            wd = np.where(L, self.w * np.where(L, d, 0.0), 0.0)
            wg = None if gt is None else np.where(L, self.w * np.where(L, gt, 0.0), 0.0)
        return wt, wd, wg

    def parts(self, x):
        x2 = np.atleast_2d(np.asarray(x, dtype=np.float64))
        wt, wd, wg = self.weighted(x2)
        pri, gpri = self.lpri_terms(x2)
        lpri = np.sum(pri, axis=1)
        with np.errstate(invalid="ignore"):
            llik = np.sum(wt, axis=1)
            llik = np.where(self.bad(x2) | ~np.isfinite(llik), -np.inf, llik)
            glik = wd @ self.Z
            if wg is not None:
                glik = np.concatenate([glik, np.sum(wg, axis=1, keepdims=True)], axis=1)
        return lpri, llik, gpri, glik

    def logpdf(self, x, phi=1.0):
        self.calls += 1
        lpri, llik, _, _ = self.parts(x)
        with np.errstate(invalid="ignore"):
            lp = lpri + phi * llik
        lp = np.where(np.isfinite(lp), lp, -np.inf)
        return float(lp[0]) if np.ndim(x) == 1 else lp

    def logpdfgrad(self, x, phi=1.0):
        lpri, llik, gpri, glik = self.parts(x)
        with np.errstate(invalid="ignore"):
            g = gpri + phi * glik
            bad = ~np.isfinite(lpri + phi * llik)
        g = np.where(bad[:, None], -np.inf, g)
        return g[0] if np.ndim(x) == 1 else g


def _fsum_rows(a):
    return np.array([math.fsum(r.tolist()) if np.all(np.isfinite(r)) else np.nan for r in a])


def exact_parts(model, x2):
    """(lpri, llik, gpri, glik) with every sum over observations / coordinates taken by math.fsum; llik = -inf where a
    row with w != 0 has a -inf term or the dispersion coordinate is out of range."""
    x2 = np.atleast_2d(np.asarray(x2, dtype=np.float64))
    wt, wd, wg = model.weighted(x2)
    pri, gpri = model.lpri_terms(x2)
    lpri = _fsum_rows(pri)
    llik = _fsum_rows(wt)
    llik = np.where(model.bad(x2) | np.isnan(llik), -np.inf, llik)
    glik = np.empty_like(x2)
    for k in range(x2.shape[0]):
        prod = wd[k][:, None] * model.Z
        glik[k, :model.Dc] = _fsum_rows(prod.T)
        if wg is not None:
            glik[k, -1] = _fsum_rows(wg[k][None, :])[0]
    return lpri, llik, gpri, glik


def device_bounds(model, x2, c_obs=64):
    """Worst-case |device - exact| of lpri, llik (per particle) and glik (per particle and coordinate): the parent
    helpers' bounds (tests/_glm.py, tests/_glm_disp.py device_bounds, restated per observation) with the offset's and
    the weights' roundings (module docstring)."""
    x2 = np.atleast_2d(np.asarray(x2, dtype=np.float64))
    eta, term, d, gt, mags = model.obs(x2)
    n, Dc = model.Z.shape
    w, o = model.w[None, :], model.o[None, :]
    live = model.live[None, :]
    A = np.abs(x2[:, :Dc]) @ np.abs(model.Z).T + np.abs(o)
    with np.errstate(over="ignore", invalid="ignore"):
        e_eta = (2 * Dc + 4) * U * A + 4 * U * np.abs(eta) + U * (np.abs(eta - o) + np.abs(o))
        if model.disp:
            m_term, m_d, m_gt, w_d, w_gt = mags
            e_term = c_obs * U * m_term + np.abs(d) * e_eta
            e_d = c_obs * U * m_d + w_d * e_eta
            e_gt = c_obs * U * m_gt + w_gt * e_eta
        else:
            if model.family == "bernoulli_logit":
                t = np.exp(-np.abs(eta))
                sig = np.where(eta >= 0.0, 1.0 / (1.0 + t), t / (1.0 + t))
                dw, mag, v = sig * (1.0 - sig), np.abs(eta) + np.log1p(t), sig
            else:
                mu = np.exp(eta)
                dw, mag, v = mu, np.abs(model.y * eta) + mu + model.aug.lgy, mu
            e_term = 8 * U * mag + np.abs(d) * e_eta
            e_d = 8 * U * v + dw * e_eta
            e_gt = None

        def summed(val, err):
            # w_i err_i + 2 u |w_i val_i| (the two products) + (n + 2) u |w_i val_i| (the sum), over the rows that count
            wv = np.where(live, np.abs(w * np.where(live, val, 0.0)), 0.0)
            return np.where(live, w * np.where(live, err, 0.0), 0.0) + (n + 4) * U * wv

        b_llik = np.sum(summed(term, e_term), axis=1)
        b_glik = summed(d, e_d) @ np.abs(model.Z)
        if e_gt is not None:
            b_glik = np.concatenate([b_glik, np.sum(summed(gt, e_gt), axis=1, keepdims=True)], axis=1)
    if model.disp:
        b_lpri = _glm_disp.device_bounds(model.base, x2)[0]
    else:
        b_lpri = _glm.device_bounds(model.base, x2)[0]
    return b_lpri, b_llik, b_glik


def mp_llik(model, x, dps=40):
    """log likelihood at one point with mpmath at `dps` digits (each term from the float64 data exactly); -inf by the
    contract where e^eta overflows fp64 in a row with w != 0 (poisson_log, neg_binomial_2_log)."""
    import mpmath as mp
    x = np.asarray(x, dtype=np.float64)
    with mp.workdps(dps):
        total = mp.mpf(0)
        dmax = mp.mpf(float(np.finfo(np.float64).max))
        tau = mp.mpf(float(x[-1])) if model.disp else None
        for i in range(model.Z.shape[0]):
            if model.w[i] == 0.0:
                continue
            eta = mp.fsum(mp.mpf(float(b)) * mp.mpf(float(z)) for b, z in zip(x[:model.Dc], model.Z[i])) \
                + mp.mpf(float(model.o[i]))
            y = mp.mpf(float(model.y[i]))
            if model.family == "bernoulli_logit":
                t = y * eta - (mp.log1p(mp.exp(eta)) if eta < 0 else eta + mp.log1p(mp.exp(-eta)))
            elif model.family == "poisson_log":
                mu = mp.exp(eta)
                if mu > dmax:
                    return -np.inf
                t = (0 if y == 0 else y * eta) - mu - mp.loggamma(y + 1)
            elif model.family == "normal":
                r = y - eta
                t = -tau - mp.log(2 * mp.pi) / 2 - r * r * mp.exp(-2 * tau) / 2
            else:
                if eta > mp.mpf(_glm_disp.LOG_DBL_MAX):
                    return -np.inf
                mu, phi = mp.exp(eta), mp.exp(tau)
                L = mp.log(mu + phi)
                t = mp.loggamma(y + phi) - mp.loggamma(phi) - mp.loggamma(y + 1) + phi * (tau - L) + y * (eta - L)
            total += mp.mpf(float(model.w[i])) * t
        return float(total)


def synthetic(family, n, p, seed, scale=None, flags=3):
    """A fixed-seed regression with offsets (flags & 1: log exposures in [0.25, 4]) and weights (flags & 2: 0 .. 3 in
    quarter steps, one row in six dropped): (X, y, offset or None, weights or None)."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, p)) / math.sqrt(max(p, 1))
    beta = rng.standard_normal(p + 1) * (1.0 if scale is None else scale)
    o = np.log(rng.uniform(0.25, 4.0, n)) if flags & 1 else None
    w = None
    if flags & 2:
        w = rng.integers(0, 13, n) / 4.0
        w[rng.random(n) < 1.0 / 6.0] = 0.0
        if not np.any(w > 0.0):
            w[0] = 1.0
    eta = beta[0] + X @ beta[1:] + (o if o is not None else 0.0)
    if family == "bernoulli_logit":
        y = (rng.random(n) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
    elif family == "poisson_log":
        y = rng.poisson(np.exp(np.clip(eta, -20, 5))).astype(np.float64)
    elif family == "normal":
        y = eta + 0.7 * rng.standard_normal(n)
    else:
        mu = np.exp(np.clip(eta, -20, 5))
        y = rng.poisson(rng.gamma(3.0, mu / 3.0)).astype(np.float64)
    return X, y, o, w


def block(X, y, family, prior_sd, intercept, dispersion_prior, offset, weights):
    """SMCN_MODEL_OGLM's data block, restated from include/smcnuts_hip.h."""
    X = np.asarray(X, dtype=np.float64).reshape(len(y), -1)
    n, p = X.shape
    Dc = p + (1 if intercept else 0)
    s = np.asarray(prior_sd, dtype=np.float64)
    s = np.full(Dc, float(s)) if s.ndim == 0 else s
    flags = (1 if offset is not None else 0) | (2 if weights is not None else 0)
    disp = family in _glm_disp.DISP_FAMILIES
    return np.concatenate([[float(FAMILIES.index(family)), n, p, 1.0 if intercept else 0.0, float(flags)], s,
                           list(dispersion_prior) if disp else [], np.asarray(y, dtype=np.float64),
                           offset if offset is not None else [], weights if weights is not None else [], X.reshape(-1)])
