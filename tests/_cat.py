"""Reference density for the categorical (multinomial logistic) regression target (smcnuts_amd.CategoricalRegression;
SMCN_MODEL_CATEGORICAL).

Stan's categorical_logit with class 0 the reference: K classes, Dc = p + intercept columns, Z_i = ([1,] X_i),
  eta_i0 = 0,  eta_ik = Z_i b_k (k = 1..K-1),  log p(y_i) = eta_{i,y_i} - logsumexp(0, eta_i1, .., eta_i,K-1),
  b_kj ~ N(0, s_kj^2);  x = (b_1,1..b_1,Dc, .., b_K-1,Dc) class-major, D = (K - 1) Dc.
The log-sum-exp as the device forms it: m = max(0, eta_ik), S = the sum of e^(eta_ik - m) over every class but the
(first) one that attains m, lse = m + log1p(S); the residuals d_ik = [y_i = k] - e^(eta_ik - m) / (1 + S).  Non-finite:
-inf once a logit is not finite.

`CategoricalNumpy` has the reference's StanModel surface (.dim, .logpdf(x, phi), .logpdfgrad(x, phi), .constrain(x),
.param_names()): it runs through HostTarget and oracle/pynuts.PyNUTS.  `exact_parts` / `device_bounds` are the fsum
reference and the worst-case bound of the device's evaluation, as tests/_glm.py has them; `mp_parts` is the 40-digit
mpmath value.
"""
import math

import numpy as np

from _glm import HALF_LOG_2PI, U


class CategoricalNumpy:
    def __init__(self, X, y, n_classes=None, prior_sd=2.5, intercept=True):
        X = np.asarray(X, dtype=np.float64)
        if X.ndim == 1:
            X = X.reshape(-1, 1)
        self.intercept = bool(intercept)
        self.y = np.asarray(y).astype(np.int64)
        self.K = int(self.y.max()) + 1 if n_classes is None else int(n_classes)
        self.Z = np.hstack([np.ones((X.shape[0], 1)), X]) if intercept else X.copy()
        self.Dc = self.Z.shape[1]
        self.dim = (self.K - 1) * self.Dc
        self.constrained_dim = self.dim
        s = np.asarray(prior_sd, dtype=np.float64)
        if s.ndim == 0:
            s = np.full((self.K - 1, self.Dc), float(s))
        elif s.shape == (self.Dc,):
            s = np.tile(s, (self.K - 1, 1))
        self.s = s.reshape(-1).copy()
        self.calls = 0

    def param_names(self):
        p = self.Dc - self.intercept
        return [nm for k in range(1, self.K)
                for nm in (([f"Intercept.{k}"] if self.intercept else []) + [f"beta.{k}.{j + 1}" for j in range(p)])]

    def constrain(self, x):
        return np.array(x, dtype=np.float64, copy=True)

    # ---- per observation, [M, n] and [M, n, K] ----
    def terms(self, x2):
        """(logits incl. class 0, term, residuals of classes 1..K-1, m, S, probabilities of classes 0..K-1)"""
        x2 = np.atleast_2d(np.asarray(x2, dtype=np.float64))
        M, n = x2.shape[0], self.Z.shape[0]
        B = x2.reshape(M, self.K - 1, self.Dc)
        with np.errstate(over="ignore", invalid="ignore"):
            eta = np.einsum("mkj,ij->mik", B, self.Z)
            full = np.concatenate([np.zeros((M, n, 1)), eta], axis=2)            # [M, n, K]
            m = np.max(full, axis=2)
            ks = np.argmax(full, axis=2)                                        # (the first class that attains m)
            ex = np.exp(full - m[..., None])
            top = np.arange(self.K)[None, None, :] == ks[..., None]
            S = np.sum(np.where(top, 0.0, ex), axis=2)
            ey = np.take_along_axis(full, np.broadcast_to(self.y[None, :, None], (M, n, 1)), axis=2)[..., 0]
            term = (ey - m) - np.log1p(S)
            term = np.where(np.isfinite(term), term, -np.inf)
            prob = np.where(top, 1.0, ex) / (1.0 + S)[..., None]
            onehot = (self.y[:, None] == np.arange(self.K)[None, :]).astype(np.float64)
            d = onehot[None, :, 1:] - prob[..., 1:]
        return full, term, d, m, S, prob

    def parts(self, x):
        x2 = np.atleast_2d(np.asarray(x, dtype=np.float64))
        _, term, d, _, _, _ = self.terms(x2)
        lpri = np.sum(-0.5 * (x2 / self.s) ** 2 - np.log(self.s) - HALF_LOG_2PI, axis=1)
        llik = np.sum(term, axis=1)
        with np.errstate(invalid="ignore"):
            glik = np.einsum("mik,ij->mkj", d, self.Z).reshape(x2.shape[0], -1)
        gpri = -x2 / self.s ** 2
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


def exact_parts(model, x2):
    """(lpri, llik, gpri, glik) with every sum over observations / coefficients taken by math.fsum."""
    x2 = np.atleast_2d(np.asarray(x2, dtype=np.float64))
    _, term, d, _, _, _ = model.terms(x2)
    M = x2.shape[0]
    lpri = np.array([math.fsum((-0.5 * (x2[m] / model.s) ** 2 - np.log(model.s) - HALF_LOG_2PI).tolist())
                     for m in range(M)])
    llik = np.array([math.fsum(term[m].tolist()) if np.all(np.isfinite(term[m])) else -np.inf for m in range(M)])
    glik = np.empty_like(x2)
    with np.errstate(invalid="ignore"):
        for m in range(M):
            for k in range(model.K - 1):
                prod = d[m, :, k][:, None] * model.Z                             # [n, Dc]
                for j in range(model.Dc):
                    col = prod[:, j]
                    glik[m, k * model.Dc + j] = math.fsum(col.tolist()) if np.all(np.isfinite(col)) else np.nan
    gpri = -x2 / model.s ** 2
    return lpri, llik, gpri, glik


def device_bounds(model, x2):
    """Worst-case |device - exact| of lpri, llik (per particle) and glik (per particle and coordinate).

    The device forms each eta_ik by Dc fused multiply-adds (error <= Dc u A_ik, A_ik = sum_j |b_kj Z_ij|; the
    reference's einsum is within the same), exp_fast / log1p_pos are within a few ulp, and exp(eta_ik - m) carries the
    rounding of its argument, u |eta_ik - m| relative, at most 0.37 u absolute (x e^-x <= 1/e).  So the term is within
    8 u (|eta_y| + m + log K + K) plus sum_k |d_ik| e_ik, the residual d_ik within (4 K + 8) u plus the effect of the
    logits' errors, p_ik (e_ik + sum_l p_il e_il).  The n terms are summed in per-lane sequences and a butterfly: within
    (n + 2) u sum |term_i|."""
    x2 = np.atleast_2d(np.asarray(x2, dtype=np.float64))
    full, term, d, m, S, prob = model.terms(x2)
    M, n = x2.shape[0], model.Z.shape[0]
    K, Dc, D = model.K, model.Dc, model.dim
    B = np.abs(x2.reshape(M, K - 1, Dc))
    A = np.einsum("mkj,ij->mik", B, np.abs(model.Z))                           # [M, n, K-1]
    eta = full[..., 1:]
    with np.errstate(over="ignore", invalid="ignore"):
        e_eta = (2 * Dc + 4) * U * A + 4 * U * np.abs(eta)
        ey = np.take_along_axis(full, np.broadcast_to(model.y[None, :, None], (M, n, 1)), axis=2)[..., 0]
        e_term = 8 * U * (np.abs(ey) + np.abs(m) + math.log(K) + K) + np.sum(np.abs(d) * e_eta, axis=2)
        p = prob[..., 1:]
        e_d = (4 * K + 8) * U + p * (e_eta + np.sum(p * e_eta, axis=2)[..., None])
        b_llik = np.sum(e_term, axis=1) + (n + 2) * U * np.sum(np.abs(term), axis=1)
        b_glik = np.einsum("mik,ij->mkj", e_d + (n + 2) * U * np.abs(d), np.abs(model.Z)).reshape(M, -1)
    pri = -0.5 * (x2 / model.s) ** 2 - np.log(model.s) - HALF_LOG_2PI
    b_lpri = (D + 6) * U * np.sum(np.abs(pri) + 0.5 * (x2 / model.s) ** 2 + np.abs(np.log(model.s)) + HALF_LOG_2PI,
                                  axis=1)
    return b_lpri, b_llik, b_glik


def mp_parts(model, x, dps=40):
    """(lpri, llik, glik) at one point with mpmath at `dps` digits (each logit from the float64 data exactly)."""
    import mpmath as mp
    x = np.asarray(x, dtype=np.float64)
    K, Dc = model.K, model.Dc
    with mp.workdps(dps):
        lpri = mp.fsum(-(mp.mpf(float(v)) / mp.mpf(float(s))) ** 2 / 2 - mp.log(mp.mpf(float(s))) - mp.log(2 * mp.pi) / 2
                       for v, s in zip(x, model.s))
        llik = mp.mpf(0)
        g = [mp.mpf(0)] * model.dim
        for i in range(model.Z.shape[0]):
            eta = [mp.mpf(0)] + [mp.fsum(mp.mpf(float(x[k * Dc + j])) * mp.mpf(float(model.Z[i, j])) for j in range(Dc))
                                 for k in range(K - 1)]
            top = max(eta)
            lse = top + mp.log(mp.fsum(mp.exp(e - top) for e in eta))
            llik += eta[model.y[i]] - lse
            for k in range(1, K):
                r = (1 if model.y[i] == k else 0) - mp.exp(eta[k] - lse)
                for j in range(Dc):
                    g[(k - 1) * Dc + j] += r * mp.mpf(float(model.Z[i, j]))
        return float(lpri), float(llik), np.array([float(v) for v in g])


def points(m, rng):
    """Benign points, the intercepts at +-800 (the logits at +-800 where the other coefficients are 0), ties between
    classes, one class dominating the others (intercept models)."""
    D, Dc, K = m.dim, m.Dc, m.K
    x = [rng.standard_normal(D) * 0.5 for _ in range(3)]
    big = np.zeros(D)
    big[0::Dc] = 800.0 * np.where(np.arange(K - 1) % 2 == 0, 1.0, -1.0)      # the intercepts at +-800
    x.append(big)
    x.append(-np.abs(big))                                                      # every class below the reference
    tie = np.zeros(D)
    tie[0::Dc] = 3.0                                                            # classes 1..K-1 tied (intercepts)
    x.append(tie)
    x.append(np.zeros(D))                                                       # all K classes tied
    dom = rng.standard_normal(D) * 0.1
    dom[(K - 2) * Dc] = 60.0                                                    # the last class dominates
    x.append(dom)
    return np.array(x)


def synthetic(K, n, p, seed, scale=1.0):
    """A fixed-seed synthetic K-class problem: X ~ N(0, 1) / sqrt(p), coefficients ~ N(0, scale^2), y drawn from the
    softmax of the logits (class 0 the reference)."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, p)) / math.sqrt(max(p, 1))
    B = rng.standard_normal((K - 1, p + 1)) * scale
    eta = np.concatenate([np.zeros((n, 1)), B[:, 0][None, :] + X @ B[:, 1:].T], axis=1)
    pr = np.exp(eta - eta.max(axis=1, keepdims=True))
    pr /= pr.sum(axis=1, keepdims=True)
    u = rng.random(n)
    y = np.minimum((np.cumsum(pr, axis=1) < u[:, None]).sum(axis=1), K - 1)
    return X, y.astype(np.int64)
