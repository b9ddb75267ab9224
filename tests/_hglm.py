"""Reference density for the varying-intercept (hierarchical) GLM target (smcnuts_amd.HierarchicalGLM; SMCN_MODEL_HGLM).

Non-centred, all constants kept: Dc = p + intercept fixed coefficients b, J groups, group index g_i per observation,
  eta_i = [b_0 +] X_i b + e^lt z_{g_i},   y_i ~ family(eta_i [, e^ld])
  b_c ~ N(0, s_c^2), z_j ~ N(0, 1), e^lt ~ half-normal(s_tau) on lt with its Jacobian:
      log 2 - log s_tau - log(2 pi) / 2 - e^(2 lt) / (2 s_tau^2) + lt,
  ld ~ N(m_d, s_d^2) (families normal / neg_binomial_2_log).
x = (b_1..b_Dc, z_1..z_J, lt [, ld]).  The per-observation terms are GLMTarget's: tests/_glm.py's canonical families
(restated on eta), tests/_glm_disp.py's normal_obs / nb_obs.  Non-finite (-inf in lpri and llik): e^(2 lt) overflows;
then the GLM rules.

`HGLMNumpy` has the reference's StanModel surface (.dim, .logpdf(x, phi), .logpdfgrad(x, phi), .constrain(x),
.param_names()): it runs through HostTarget and oracle/pynuts.PyNUTS.  `exact_parts` / `device_bounds` are the fsum
reference and the worst-case bound of the device's evaluation, as tests/_glm.py and tests/_glm_disp.py have them;
`mp_parts` is the 40-digit mpmath value.
"""
import math

import numpy as np

import _glm_disp as gd
from _glm import HALF_LOG_2PI, U

FAMILIES = ("bernoulli_logit", "poisson_log", "normal", "neg_binomial_2_log")
LOG2 = math.log(2.0)


def canon_obs(family, y, eta, lgy):
    """bernoulli_logit / poisson_log per observation, in the tuple layout of _glm_disp.normal_obs / nb_obs."""
    with np.errstate(over="ignore", invalid="ignore"):
        if family == "bernoulli_logit":
            t = np.exp(-np.abs(eta))
            l1 = np.log1p(t)
            term = np.where(y != 0.0, np.minimum(eta, 0.0), -np.maximum(eta, 0.0)) - l1
            sig = np.where(eta >= 0.0, 1.0 / (1.0 + t), t / (1.0 + t))
            d = y - sig
            m_term, m_d, w_d = np.abs(eta) + l1, np.abs(y) + sig, sig * (1.0 - sig)
        else:
            mu = np.exp(eta)
            term = (np.where(y == 0.0, 0.0, y * eta) - mu) - lgy
            term = np.where(np.isfinite(mu), term, -np.inf)
            d = y - mu
            m_term, m_d, w_d = np.abs(y * eta) + mu + lgy, y + mu, mu
    z = np.zeros_like(term)
    return term, d, z, m_term, m_d, z, w_d, z


class HGLMNumpy:
    def __init__(self, X, y, groups, family="bernoulli_logit", prior_sd=2.5, group_sd_prior=1.0,
                 dispersion_prior=(0.0, 2.5), intercept=True, n_groups=None):
        X = np.asarray(X, dtype=np.float64)
        if X.ndim == 1:
            X = X.reshape(-1, 1)
        self.family, self.intercept = family, bool(intercept)
        self.disp = family in ("normal", "neg_binomial_2_log")
        self.y = np.asarray(y, dtype=np.float64)
        self.g = np.asarray(groups).astype(np.int64)
        self.J = int(self.g.max()) + 1 if n_groups is None else int(n_groups)
        self.Z = np.hstack([np.ones((X.shape[0], 1)), X]) if intercept else X.copy()
        self.Dc = self.Z.shape[1]
        self.lt = self.Dc + self.J                              # index of lt
        self.dim = self.lt + 1 + (1 if self.disp else 0)
        self.constrained_dim = self.dim
        s = np.asarray(prior_sd, dtype=np.float64)
        self.s = np.full(self.Dc, float(s)) if s.ndim == 0 else s.copy()
        self.s_tau = float(group_sd_prior)
        self.md, self.sd = (float(dispersion_prior[0]), float(dispersion_prior[1])) if self.disp else (0.0, 1.0)
        self.lgy = gd.lgamma1p(self.y) if family in ("poisson_log", "neg_binomial_2_log") else np.zeros_like(self.y)
        self.onehot = np.zeros((len(self.y), self.J))
        self.onehot[np.arange(len(self.y)), self.g] = 1.0
        self.calls = 0

    def param_names(self):
        return (["Intercept"] if self.intercept else []) + [f"beta.{j + 1}" for j in range(self.Dc - self.intercept)] \
            + [f"alpha.{j + 1}" for j in range(self.J)] + ["tau"] \
            + (["sigma" if self.family == "normal" else "phi"] if self.disp else [])

    def constrain(self, x):
        x = np.array(x, dtype=np.float64, copy=True)
        tau = np.exp(x[..., self.lt])
        x[..., self.Dc:self.lt] *= tau[..., None]
        x[..., self.lt:] = np.exp(x[..., self.lt:])
        return x

    def split(self, x2):
        """tau, e^(2 lt), and whether e^(2 lt) overflows, per particle."""
        with np.errstate(over="ignore"):
            tau = np.exp(x2[:, self.lt])
            e2 = tau * tau
        return tau, e2, ~np.isfinite(e2)

    def obs(self, x2):
        """eta [M, n], alpha_{g_i} [M, n] and the per-observation tuple (term, d, gt, magnitudes..); rows whose lt or
        ld is out of range are evaluated at 0 there (their llik is -inf regardless)."""
        x2 = np.atleast_2d(np.asarray(x2, dtype=np.float64))
        tau, _, bad = self.split(x2)
        tau = np.where(bad, 1.0, tau)
        a = tau[:, None] * x2[:, self.Dc:self.lt][:, self.g]
        eta = x2[:, :self.Dc] @ self.Z.T + a
        y = self.y[None, :]
        if self.family == "normal":
            ld = x2[:, -1:]
            return eta, a, gd.normal_obs(y, eta, np.where(self.bad_d(ld), 0.0, ld))
        if self.family == "neg_binomial_2_log":
            ld = x2[:, -1:]
            return eta, a, gd.nb_obs(y, eta, np.where(self.bad_d(ld), 0.0, ld), self.lgy[None, :])
        return eta, a, canon_obs(self.family, y, eta, self.lgy[None, :])

    def bad_d(self, ld):
        if self.family == "normal":
            return -2.0 * ld > gd.LOG_DBL_MAX
        if self.family == "neg_binomial_2_log":
            return ~((ld <= gd.LOG_DBL_MAX) & (ld >= gd.LOG_DBL_MIN))
        return np.zeros(np.shape(ld), dtype=bool)

    def bad(self, x2):
        _, _, b = self.split(x2)
        return b | (self.bad_d(x2[:, -1]) if self.disp else False)

    def prior_terms(self, x2):
        """per-coordinate prior terms and gradients [M, D]"""
        _, e2, _ = self.split(x2)
        Dc, lt = self.Dc, self.lt
        t = np.empty_like(x2)
        g = np.empty_like(x2)
        b = x2[:, :Dc]
        t[:, :Dc] = -0.5 * (b / self.s) ** 2 - np.log(self.s) - HALF_LOG_2PI
        g[:, :Dc] = -b / self.s ** 2
        z = x2[:, Dc:lt]
        t[:, Dc:lt] = -0.5 * z * z - HALF_LOG_2PI
        g[:, Dc:lt] = -z
        with np.errstate(over="ignore", invalid="ignore"):
            t[:, lt] = ((LOG2 - math.log(self.s_tau)) - HALF_LOG_2PI + x2[:, lt]) - 0.5 * e2 / self.s_tau ** 2
            g[:, lt] = 1.0 - e2 / self.s_tau ** 2
        if self.disp:
            v = x2[:, -1] - self.md
            t[:, -1] = -0.5 * (v / self.sd) ** 2 - math.log(self.sd) - HALF_LOG_2PI
            g[:, -1] = -v / self.sd ** 2
        return t, g

    def grad_lik(self, x2, d, gt, a, tau):
        with np.errstate(invalid="ignore", over="ignore"):
            cols = [d @ self.Z, tau[:, None] * (d @ self.onehot), np.sum(d * a, axis=1, keepdims=True)]
            if self.disp:
                cols.append(np.sum(gt, axis=1, keepdims=True))
        return np.concatenate(cols, axis=1)

    def parts(self, x):
        x2 = np.atleast_2d(np.asarray(x, dtype=np.float64))
        _, a, (term, d, gt, *_r) = self.obs(x2)
        tp, gpri = self.prior_terms(x2)
        tau, _, badt = self.split(x2)
        lpri = np.where(badt, -np.inf, np.sum(tp, axis=1))
        llik = np.where(self.bad(x2), -np.inf, np.sum(term, axis=1))
        return lpri, llik, gpri, self.grad_lik(x2, d, gt, a, tau)

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


def _fsum(v):
    return math.fsum(v.tolist()) if np.all(np.isfinite(v)) else np.nan


def exact_parts(model, x2):
    """(lpri, llik, gpri, glik) with every sum over observations / coordinates taken by math.fsum."""
    x2 = np.atleast_2d(np.asarray(x2, dtype=np.float64))
    _, a, (term, d, gt, *_r) = model.obs(x2)
    tp, gpri = model.prior_terms(x2)
    tau, _, badt = model.split(x2)
    bad = model.bad(x2)
    M = x2.shape[0]
    lpri = np.array([-np.inf if badt[k] else _fsum(tp[k]) for k in range(M)])
    llik = np.array([-np.inf if (bad[k] or not np.all(np.isfinite(term[k]))) else _fsum(term[k]) for k in range(M)])
    glik = np.empty_like(x2)
    Dc, lt = model.Dc, model.lt
    for k in range(M):
        for c in range(Dc):
            glik[k, c] = _fsum(d[k] * model.Z[:, c])
        for j in range(model.J):
            glik[k, Dc + j] = tau[k] * _fsum(d[k][model.g == j])
        glik[k, lt] = _fsum(d[k] * a[k])
        if model.disp:
            glik[k, -1] = _fsum(gt[k])
    return lpri, llik, gpri, glik


def device_bounds(model, x2, c_obs=64):
    """Worst-case |device - exact| of lpri, llik (per particle) and glik (per particle and coordinate).

    tau = e^lt within 4 u (exp_fast), alpha_{g_i} = tau z within 6 u; eta = fixed part (Dc fused multiply-adds in two
    chains) + alpha, within (2 Dc + 8) u of sum |b_j Z_ij| + |alpha| (the reference's the same again); each
    per-observation quantity within c_obs u of the magnitudes of its addends plus the eta error times its derivative
    (tests/_glm_disp.py); the sums over n within (n + 2) u of the sum of magnitudes; the group sums once more by tau's
    error; the lt sum by alpha's."""
    x2 = np.atleast_2d(np.asarray(x2, dtype=np.float64))
    eta, a, (term, d, gt, m_term, m_d, m_gt, w_d, w_gt) = model.obs(x2)
    n, Dc = model.Z.shape
    tau, e2, _ = model.split(x2)
    A = np.abs(x2[:, :Dc]) @ np.abs(model.Z).T + np.abs(a)
    e_eta = (2 * Dc + 8) * U * A + 4 * U * np.abs(eta)
    with np.errstate(over="ignore", invalid="ignore"):
        e_term = c_obs * U * m_term + np.abs(d) * e_eta
        e_d = c_obs * U * m_d + w_d * e_eta
        e_gt = c_obs * U * m_gt + w_gt * e_eta
        b_llik = np.sum(e_term, axis=1) + (n + 2) * U * np.sum(np.abs(term), axis=1)
        ed = e_d + (n + 2) * U * np.abs(d)
        cols = [ed @ np.abs(model.Z),
                tau[:, None] * (ed @ model.onehot) + 8 * U * tau[:, None] * (np.abs(d) @ model.onehot),
                (np.sum(ed * np.abs(a) + 8 * U * np.abs(d * a), axis=1) + (n + 2) * U * np.sum(np.abs(d * a), axis=1))[:, None]]
        if model.disp:
            cols.append((np.sum(e_gt, axis=1) + (n + 2) * U * np.sum(np.abs(gt), axis=1))[:, None])
        b_glik = np.concatenate(cols, axis=1)
    tp, _ = model.prior_terms(x2)
    D = model.dim
    mag = np.sum(np.abs(tp), axis=1) + 0.5 * np.sum(x2[:, :Dc] ** 2 / model.s ** 2, axis=1) \
        + 0.5 * np.sum(x2[:, Dc:model.lt] ** 2, axis=1) + np.abs(x2[:, model.lt]) + 2.0 + 4.0 * e2 / model.s_tau ** 2
    if model.disp:
        v = x2[:, -1] - model.md
        mag = mag + 0.5 * (v / model.sd) ** 2 + np.abs(x2[:, -1] * v) / model.sd ** 2
    b_lpri = (D + 16) * U * mag
    return b_lpri, b_llik, b_glik


def mp_parts(model, x, dps=40):
    """(log prior, log likelihood, gradient of each) at one point with mpmath at `dps` digits, from the float64 data."""
    import mpmath as mp
    x = [float(v) for v in x]
    Dc, lt, J = model.Dc, model.lt, model.J
    with mp.workdps(dps):
        X = [mp.mpf(v) for v in x]
        tau = mp.exp(X[lt])
        hl = mp.log(2 * mp.pi) / 2
        lp = mp.mpf(0)
        gp = [mp.mpf(0)] * model.dim
        for c in range(Dc):
            s = mp.mpf(float(model.s[c]))
            lp += -(X[c] / s) ** 2 / 2 - mp.log(s) - hl
            gp[c] = -X[c] / s ** 2
        for j in range(J):
            lp += -X[Dc + j] ** 2 / 2 - hl
            gp[Dc + j] = -X[Dc + j]
        st = mp.mpf(model.s_tau)
        lp += mp.log(2) - mp.log(st) - hl - tau ** 2 / (2 * st ** 2) + X[lt]
        gp[lt] = 1 - tau ** 2 / st ** 2
        if model.disp:
            v, sd = X[-1] - mp.mpf(model.md), mp.mpf(model.sd)
            lp += -(v / sd) ** 2 / 2 - mp.log(sd) - hl
            gp[-1] = -v / sd ** 2
        ll = mp.mpf(0)
        gl = [mp.mpf(0)] * model.dim
        for i in range(len(model.y)):
            gi = int(model.g[i])
            alpha = tau * X[Dc + gi]
            eta = mp.fsum(X[c] * mp.mpf(float(model.Z[i, c])) for c in range(Dc)) + alpha
            y = mp.mpf(float(model.y[i]))
            gt = mp.mpf(0)
            if model.family == "bernoulli_logit":
                term = y * eta - (mp.log1p(mp.exp(eta)) if eta < 0 else eta + mp.log1p(mp.exp(-eta)))
                d = y - 1 / (1 + mp.exp(-eta))
            elif model.family == "poisson_log":
                mu = mp.exp(eta)
                term = (0 if y == 0 else y * eta) - mu - mp.loggamma(y + 1)
                d = y - mu
            elif model.family == "normal":
                w = mp.exp(-2 * X[-1])
                r = y - eta
                term, d, gt = -X[-1] - hl - r * r * w / 2, r * w, r * r * w - 1
            else:
                mu, phi = mp.exp(eta), mp.exp(X[-1])
                L = mp.log(mu + phi)
                term = mp.loggamma(y + phi) - mp.loggamma(phi) - mp.loggamma(y + 1) + phi * (X[-1] - L) + y * (eta - L)
                d = y - (y + phi) * mu / (mu + phi)
                gt = phi * (mp.digamma(y + phi) - mp.digamma(phi) - mp.log1p(mu / phi) + (mu - y) / (mu + phi))
            ll += term
            for c in range(Dc):
                gl[c] += d * mp.mpf(float(model.Z[i, c]))
            gl[Dc + gi] += d * tau
            gl[lt] += d * alpha
            if model.disp:
                gl[-1] += gt
        return float(lp), float(ll), np.array([float(v) for v in gp]), np.array([float(v) for v in gl])


def synthetic(family, n, p, J, seed, tau=0.8, scale=0.5, empty=()):
    """A fixed-seed synthetic varying-intercept regression: X ~ N(0, 1) / sqrt(p), coefficients ~ N(0, scale^2), group
    intercepts ~ N(0, tau^2), groups drawn uniformly from 0..J-1 leaving out `empty`; sigma = 0.7 (normal), phi = 3
    (NB)."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, p)) / math.sqrt(max(p, 1))
    beta = rng.standard_normal(p + 1) * scale
    alpha = rng.standard_normal(J) * tau
    live = np.array([j for j in range(J) if j not in set(empty)])
    g = live[rng.integers(0, len(live), n)]
    eta = beta[0] + X @ beta[1:] + alpha[g]
    if family == "bernoulli_logit":
        y = (rng.random(n) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
    elif family == "poisson_log":
        y = rng.poisson(np.exp(np.clip(eta, -20, 5))).astype(np.float64)
    elif family == "normal":
        y = eta + 0.7 * rng.standard_normal(n)
    else:
        mu = np.exp(np.clip(eta, -20, 5))
        y = rng.poisson(rng.gamma(3.0, mu / 3.0)).astype(np.float64)
    return X, y, g
