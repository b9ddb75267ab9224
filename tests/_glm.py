"""Reference densities for the canonical-link GLM target (smcnuts_amd.GLMTarget; SMCN_MODEL_GLM).

`GLMNumpy` is the same model as a plain Python object with the reference's StanModel surface (.dim, .logpdf(x, phi),
.logpdfgrad(x, phi)): it runs through HostTarget and through oracle/pynuts.PyNUTS.  `exact_parts` takes every sum of
one evaluation with math.fsum over the float64 terms (one rounding of the exact sum) and returns, beside each value,
the worst-case bound of the error the device's evaluation may have against it (`device_bounds`).  `mp_llik` is the
40-digit mpmath value the CPU tests check the terms against.

The density (include/smcnuts_hip.h, SMCN_MODEL_GLM): eta_i = [b_0 +] sum_j X_ij b_j,
  lpri = sum_c [-(b_c / s_c)^2 / 2 - log s_c - log(2 pi) / 2],
  bernoulli_logit: llik = sum_i [y_i eta_i - softplus(eta_i)],   gradient X^T (y - sigmoid(eta)),
  poisson_log:     llik = sum_i [y_i eta_i - exp(eta_i) - lgamma(y_i + 1)] (y_i eta_i = 0 for y_i = 0; -inf once exp
                   overflows),                                   gradient X^T (y - exp(eta)).
"""
import math

import numpy as np

EPS = float(np.finfo(np.float64).eps)
U = EPS / 2                                   # unit roundoff
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


class GLMNumpy:
    def __init__(self, X, y, family="bernoulli_logit", prior_sd=2.5, intercept=True):
        X = np.asarray(X, dtype=np.float64)
        if X.ndim == 1:
            X = X.reshape(-1, 1)
        self.family, self.intercept = family, bool(intercept)
        self.y = np.asarray(y, dtype=np.float64)
        self.Z = np.hstack([np.ones((X.shape[0], 1)), X]) if intercept else X.copy()     # design incl. the intercept column
        self.dim = self.Z.shape[1]
        self.constrained_dim = self.dim
        s = np.asarray(prior_sd, dtype=np.float64)
        self.s = np.full(self.dim, float(s)) if s.ndim == 0 else s.copy()
        self.lgy = np.array([math.lgamma(v + 1.0) for v in self.y]) if family == "poisson_log" else np.zeros_like(self.y)
        self.calls = 0

    def param_names(self):
        return (["Intercept"] if self.intercept else []) + [f"beta.{j + 1}" for j in range(self.dim - self.intercept)]

    # ---- per-observation terms and residuals, [M, n] ----
    def terms(self, x2):
        eta = x2 @ self.Z.T
        y = self.y
        with np.errstate(over="ignore", invalid="ignore"):
            if self.family == "bernoulli_logit":
                t = np.exp(-np.abs(eta))
                l1 = np.log1p(t)
                term = np.where(y != 0.0, np.minimum(eta, 0.0), -np.maximum(eta, 0.0)) - l1
                sig = np.where(eta >= 0.0, 1.0 / (1.0 + t), t / (1.0 + t))
                d = y - sig
            else:
                mu = np.exp(eta)
                term = (np.where(y == 0.0, 0.0, y * eta) - mu) - self.lgy
                term = np.where(np.isfinite(mu), term, -np.inf)
                d = y - mu
        return eta, term, d

    def parts(self, x):
        x2 = np.atleast_2d(np.asarray(x, dtype=np.float64))
        _, term, d = self.terms(x2)
        lpri = np.sum(-0.5 * (x2 / self.s) ** 2 - np.log(self.s) - HALF_LOG_2PI, axis=1)
        llik = np.sum(term, axis=1)
        with np.errstate(invalid="ignore"):
            glik = d @ self.Z
        gpri = -x2 / self.s ** 2
        return lpri, llik, gpri, glik

    def logpdf(self, x, phi=1.0):
        self.calls += 1
        lpri, llik, _, _ = self.parts(x)
        with np.errstate(invalid="ignore"):
            lp = lpri + phi * llik                      # (0 * -inf: -inf, as the device's convention for any non-finite value)
        lp = np.where(np.isfinite(lp), lp, -np.inf)
        return float(lp[0]) if np.ndim(x) == 1 else lp

    def logpdfgrad(self, x, phi=1.0):
        lpri, llik, gpri, glik = self.parts(x)
        with np.errstate(invalid="ignore"):
            g = gpri + phi * glik
            bad = ~np.isfinite(lpri + phi * llik)
        g = np.where(bad[:, None], -np.inf, g)
        return g[0] if np.ndim(x) == 1 else g


def exact_parts(model, x2):
    """(lpri, llik, gpri, glik) with every sum over observations / coefficients taken by math.fsum."""
    x2 = np.atleast_2d(np.asarray(x2, dtype=np.float64))
    eta, term, d = model.terms(x2)
    M = x2.shape[0]
    lpri = np.array([math.fsum((-0.5 * (x2[m] / model.s) ** 2 - np.log(model.s) - HALF_LOG_2PI).tolist()) for m in range(M)])
    llik = np.array([math.fsum(term[m].tolist()) if np.all(np.isfinite(term[m])) else -np.inf for m in range(M)])
    glik = np.empty_like(x2)
    for m in range(M):
        prod = d[m][:, None] * model.Z                  # [n, D]
        for c in range(model.dim):
            glik[m, c] = math.fsum(prod[:, c].tolist()) if np.all(np.isfinite(prod[:, c])) else np.nan
    gpri = -x2 / model.s ** 2
    return lpri, llik, gpri, glik


def device_bounds(model, x2):
    """Worst-case |device - exact| of lpri, llik (per particle) and glik (per particle and coordinate).

    The device forms eta_i by D fused multiply-adds (error <= D u sum_j |b_j Z_ij| =: D u A_i), evaluates each term with
    exp_fast / log1p_pos (a few ulp: 8 u of the magnitudes involved is a safe cover), and sums n terms in per-lane
    sequences followed by a butterfly -- within the sequential bound (n + 2) u sum |term_i|.  An error e in eta_i moves
    the term by <= |d_i| e and the residual d_i by <= w_i e (w_i = sigmoid'(eta_i) <= 1/4, or mu_i)."""
    x2 = np.atleast_2d(np.asarray(x2, dtype=np.float64))
    eta, term, d = model.terms(x2)
    n, D = model.Z.shape
    A = np.abs(x2) @ np.abs(model.Z).T                   # [M, n]
    e_eta = (2 * D + 4) * U * A + 4 * U * np.abs(eta)       # (the device's eta and the reference's, each within D u A_i)
    with np.errstate(over="ignore", invalid="ignore"):
        if model.family == "bernoulli_logit":
            t = np.exp(-np.abs(eta))
            sig = np.where(eta >= 0.0, 1.0 / (1.0 + t), t / (1.0 + t))
            w = sig * (1.0 - sig)
            mag = np.abs(eta) + np.log1p(t)                  # |y eta| + softplus
            v = sig
        else:
            mu = np.exp(eta)
            w = mu
            mag = np.abs(model.y * eta) + mu + model.lgy
            v = mu
        e_term = 8 * U * mag + np.abs(d) * e_eta
        e_d = 8 * U * v + w * e_eta
        b_llik = np.sum(e_term, axis=1) + (n + 2) * U * np.sum(np.abs(term), axis=1)
        b_glik = (e_d + (n + 2) * U * np.abs(d)) @ np.abs(model.Z)
    pri = -0.5 * (x2 / model.s) ** 2 - np.log(model.s) - HALF_LOG_2PI
    b_lpri = (D + 6) * U * np.sum(np.abs(pri) + 0.5 * (x2 / model.s) ** 2 + np.abs(np.log(model.s)) + HALF_LOG_2PI, axis=1)
    return b_lpri, b_llik, b_glik


def mp_llik(model, x, dps=40):
    """log likelihood at one point with mpmath at `dps` digits (each term from the float64 data exactly)."""
    import mpmath as mp
    with mp.workdps(dps):
        total = mp.mpf(0)
        for i in range(model.Z.shape[0]):
            eta = mp.fsum(mp.mpf(float(b)) * mp.mpf(float(z)) for b, z in zip(x, model.Z[i]))
            y = mp.mpf(float(model.y[i]))
            if model.family == "bernoulli_logit":
                total += y * eta - (mp.log1p(mp.exp(eta)) if eta < 0 else eta + mp.log1p(mp.exp(-eta)))
            else:
                mu = mp.exp(eta)
                if mu > mp.mpf(np.finfo(np.float64).max):
                    return -np.inf                        # exp(eta) overflows in fp64: -inf by the contract
                total += (0 if y == 0 else y * eta) - mu - mp.loggamma(y + 1)
        return float(total)


def mp_grad(model, x, dps=40):
    import mpmath as mp
    with mp.workdps(dps):
        g = [mp.mpf(0)] * model.dim
        for i in range(model.Z.shape[0]):
            eta = mp.fsum(mp.mpf(float(b)) * mp.mpf(float(z)) for b, z in zip(x, model.Z[i]))
            y = mp.mpf(float(model.y[i]))
            r = y - (1 / (1 + mp.exp(-eta)) if model.family == "bernoulli_logit" else mp.exp(eta))
            g = [g[c] + r * mp.mpf(float(model.Z[i, c])) for c in range(model.dim)]
        return np.array([float(v) for v in g])


def synthetic(family, n, p, seed, scale=None):
    """A fixed-seed synthetic regression: X ~ N(0, 1) / sqrt(p), coefficients ~ N(0, 1)."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, p)) / math.sqrt(max(p, 1))
    beta = rng.standard_normal(p + 1) * (1.0 if scale is None else scale)
    eta = beta[0] + X @ beta[1:]
    if family == "bernoulli_logit":
        y = (rng.random(n) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
    else:
        y = rng.poisson(np.exp(np.clip(eta, -20, 5))).astype(np.float64)
    return X, y
