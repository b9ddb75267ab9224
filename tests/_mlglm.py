"""Reference density for the multilevel GLM target (smcnuts_amd.MultilevelGLM; SMCN_MODEL_MLGLM).

Non-centred, all constants kept: Dc = p + intercept fixed coefficients b and R independent varying terms; term r has J_r
levels, a level g_ir and a multiplier z_ir per observation,
  eta_i = [b_0 +] X_i b + sum_r z_ir e^lt_r u_{r,g_ir},   y_i ~ family(eta_i [, e^ld])
  b_c ~ N(0, s_c^2), u_rj ~ N(0, 1), e^lt_r ~ half-normal(s_tau_r) on lt_r with its Jacobian:
      log 2 - log s_tau_r - log(2 pi) / 2 - e^(2 lt_r) / (2 s_tau_r^2) + lt_r,
  ld ~ N(m_d, s_d^2) (families normal / neg_binomial_2_log).
x = (b_1..b_Dc, u_1,1..u_1,J1, .., u_R,1..u_R,JR, lt_1..lt_R [, ld]).  The per-observation terms are tests/_hglm.py's
(canon_obs, _glm_disp.normal_obs / nb_obs).  Non-finite (-inf in lpri and llik): any e^(2 lt_r) overflows; then the GLM
rules.  With R = 1 and z = 1 every operation is _hglm.HGLMNumpy's, in its order.

`MLGLMNumpy` has the reference's StanModel surface (.dim, .logpdf(x, phi), .logpdfgrad(x, phi), .constrain(x),
.param_names()): it runs through HostTarget and oracle/pynuts.PyNUTS.  `exact_parts` / `device_bounds` are the fsum
reference and the worst-case bound of the device's evaluation (_hglm.device_bounds restated with R group addends);
`mp_parts` is the 40-digit mpmath value.
"""
import math

import numpy as np

import _glm_disp as gd
from _glm import HALF_LOG_2PI, U
from _hglm import FAMILIES, LOG2, canon_obs, _fsum  # noqa: F401


class MLGLMNumpy:
    def __init__(self, X, y, terms, family="bernoulli_logit", prior_sd=2.5, group_sd_prior=1.0,
                 dispersion_prior=(0.0, 2.5), intercept=True):
        """terms: [(groups, z or None, n_groups or None)]"""
        X = np.asarray(X, dtype=np.float64)
        if X.ndim == 1:
            X = X.reshape(-1, 1)
        n = X.shape[0]
        self.family, self.intercept = family, bool(intercept)
        self.disp = family in ("normal", "neg_binomial_2_log")
        self.y = np.asarray(y, dtype=np.float64)
        self.R = len(terms)
        self.g, self.z, self.J = [], [], []
        for t in terms:
            t = tuple(t) + (None, None)
            g = np.asarray(t[0]).astype(np.int64)
            self.g.append(g)
            self.z.append(np.ones(n) if t[1] is None else np.asarray(t[1], dtype=np.float64))
            self.J.append(int(g.max()) + 1 if t[2] is None else int(t[2]))
        self.Z = np.hstack([np.ones((n, 1)), X]) if intercept else X.copy()
        self.Dc = self.Z.shape[1]
        self.off = [self.Dc + sum(self.J[:r]) for r in range(self.R)]     # first u of term r
        self.lt0 = self.Dc + sum(self.J)                                  # index of lt_1
        self.dim = self.lt0 + self.R + (1 if self.disp else 0)
        self.constrained_dim = self.dim
        s = np.asarray(prior_sd, dtype=np.float64)
        self.s = np.full(self.Dc, float(s)) if s.ndim == 0 else s.copy()
        st = np.asarray(group_sd_prior, dtype=np.float64)
        self.s_tau = np.full(self.R, float(st)) if st.ndim == 0 else st.copy()
        self.md, self.sd = (float(dispersion_prior[0]), float(dispersion_prior[1])) if self.disp else (0.0, 1.0)
        self.lgy = gd.lgamma1p(self.y) if family in ("poisson_log", "neg_binomial_2_log") else np.zeros_like(self.y)
        self.onehot = []
        for r in range(self.R):
            oh = np.zeros((n, self.J[r]))
            oh[np.arange(n), self.g[r]] = 1.0
            self.onehot.append(oh)
        self.calls = 0

    def u_slice(self, r):
        return slice(self.off[r], self.off[r] + self.J[r])

    def param_names(self):
        return (["Intercept"] if self.intercept else []) + [f"beta.{j + 1}" for j in range(self.Dc - self.intercept)] \
            + [f"alpha.{r + 1}.{j + 1}" for r in range(self.R) for j in range(self.J[r])] \
            + [f"tau.{r + 1}" for r in range(self.R)] \
            + (["sigma" if self.family == "normal" else "phi"] if self.disp else [])

    def constrain(self, x):
        x = np.array(x, dtype=np.float64, copy=True)
        for r in range(self.R):
            x[..., self.u_slice(r)] *= np.exp(x[..., self.lt0 + r])[..., None]
        x[..., self.lt0:] = np.exp(x[..., self.lt0:])
        return x

    def split(self, x2):
        """tau [M, R], e^(2 lt) [M, R], and whether any e^(2 lt_r) overflows, per particle."""
        with np.errstate(over="ignore"):
            tau = np.exp(x2[:, self.lt0:self.lt0 + self.R])
            e2 = tau * tau
        return tau, e2, ~np.all(np.isfinite(e2), axis=1)

    def obs(self, x2):
        """eta [M, n], the R addends a_r = z_r e^lt_r u_{r,g_r} [M, n] each and the per-observation tuple (term, d, gt,
        magnitudes..); rows whose lt or ld is out of range are evaluated at tau = 1 / ld = 0 (their llik is -inf
        regardless)."""
        x2 = np.atleast_2d(np.asarray(x2, dtype=np.float64))
        tau, _, bad = self.split(x2)
        tau = np.where(bad[:, None], 1.0, tau)
        a = [(tau[:, r:r + 1] * x2[:, self.u_slice(r)][:, self.g[r]]) * self.z[r][None, :] for r in range(self.R)]
        s = a[0]
        for r in range(1, self.R):
            s = s + a[r]
        eta = x2[:, :self.Dc] @ self.Z.T + s
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
        Dc, lt0 = self.Dc, self.lt0
        t = np.empty_like(x2)
        g = np.empty_like(x2)
        b = x2[:, :Dc]
        t[:, :Dc] = -0.5 * (b / self.s) ** 2 - np.log(self.s) - HALF_LOG_2PI
        g[:, :Dc] = -b / self.s ** 2
        u = x2[:, Dc:lt0]
        t[:, Dc:lt0] = -0.5 * u * u - HALF_LOG_2PI
        g[:, Dc:lt0] = -u
        with np.errstate(over="ignore", invalid="ignore"):
            for r in range(self.R):
                st = float(self.s_tau[r])
                t[:, lt0 + r] = ((LOG2 - math.log(st)) - HALF_LOG_2PI + x2[:, lt0 + r]) - 0.5 * e2[:, r] / st ** 2
                g[:, lt0 + r] = 1.0 - e2[:, r] / st ** 2
        if self.disp:
            v = x2[:, -1] - self.md
            t[:, -1] = -0.5 * (v / self.sd) ** 2 - math.log(self.sd) - HALF_LOG_2PI
            g[:, -1] = -v / self.sd ** 2
        return t, g

    def grad_lik(self, x2, d, gt, a, tau):
        with np.errstate(invalid="ignore", over="ignore"):
            cols = [d @ self.Z]
            cols += [tau[:, r:r + 1] * ((d * self.z[r][None, :]) @ self.onehot[r]) for r in range(self.R)]
            cols += [np.sum(d * a[r], axis=1, keepdims=True) for r in range(self.R)]
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
    for k in range(M):
        for c in range(model.Dc):
            glik[k, c] = _fsum(d[k] * model.Z[:, c])
        for r in range(model.R):
            dz = d[k] * model.z[r]
            for j in range(model.J[r]):
                glik[k, model.off[r] + j] = tau[k, r] * _fsum(dz[model.g[r] == j])
            glik[k, model.lt0 + r] = _fsum(d[k] * a[r][k])
        if model.disp:
            glik[k, -1] = _fsum(gt[k])
    return lpri, llik, gpri, glik


def device_bounds(model, x2, c_obs=64):
    """Worst-case |device - exact| of lpri, llik (per particle) and glik (per particle and coordinate):
    _hglm.device_bounds with R group addends.

    tau_r = e^lt_r within 4 u (exp_fast), a_r = (tau_r u) z within 7 u (one product more than the hierarchical model's
    alpha); eta = fixed part (Dc fused multiply-adds in two chains) + the R addends added one by one, within
    (2 Dc + 8 + 4 R) u of sum |b_j Z_ij| + sum_r |a_r| for the device and the reference together (per term: the product
    with z on either side, and an addition on either side); each per-observation quantity within c_obs u of the
    magnitudes of its addends plus the eta error times its derivative (tests/_glm_disp.py); the sums over n within
    (n + 2) u of the sum of magnitudes; a level's sum of d z once more by tau_r's error and the rounding of d z
    (10 u); the lt_r sum by a_r's (10 u)."""
    x2 = np.atleast_2d(np.asarray(x2, dtype=np.float64))
    eta, a, (term, d, gt, m_term, m_d, m_gt, w_d, w_gt) = model.obs(x2)
    n, Dc = model.Z.shape
    R = model.R
    tau, e2, _ = model.split(x2)
    A = np.abs(x2[:, :Dc]) @ np.abs(model.Z).T + sum(np.abs(a[r]) for r in range(R))
    e_eta = (2 * Dc + 8 + 4 * R) * U * A + 4 * U * np.abs(eta)
    with np.errstate(over="ignore", invalid="ignore"):
        e_term = c_obs * U * m_term + np.abs(d) * e_eta
        e_d = c_obs * U * m_d + w_d * e_eta
        e_gt = c_obs * U * m_gt + w_gt * e_eta
        b_llik = np.sum(e_term, axis=1) + (n + 2) * U * np.sum(np.abs(term), axis=1)
        ed = e_d + (n + 2) * U * np.abs(d)
        cols = [ed @ np.abs(model.Z)]
        for r in range(R):
            az = np.abs(model.z[r])[None, :]
            cols.append(tau[:, r:r + 1] * ((ed * az) @ model.onehot[r])
                        + 10 * U * tau[:, r:r + 1] * ((np.abs(d) * az) @ model.onehot[r]))
        for r in range(R):
            da = np.abs(d * a[r])
            cols.append((np.sum(ed * np.abs(a[r]) + 10 * U * da, axis=1) + (n + 2) * U * np.sum(da, axis=1))[:, None])
        if model.disp:
            cols.append((np.sum(e_gt, axis=1) + (n + 2) * U * np.sum(np.abs(gt), axis=1))[:, None])
        b_glik = np.concatenate(cols, axis=1)
    tp, _ = model.prior_terms(x2)
    D = model.dim
    lts = x2[:, model.lt0:model.lt0 + R]
    with np.errstate(over="ignore", invalid="ignore"):
        mag = np.sum(np.abs(tp), axis=1) + 0.5 * np.sum(x2[:, :Dc] ** 2 / model.s ** 2, axis=1) \
            + 0.5 * np.sum(x2[:, Dc:model.lt0] ** 2, axis=1) \
            + np.sum(np.abs(lts) + 2.0 + 4.0 * e2 / model.s_tau ** 2, axis=1)
    if model.disp:
        v = x2[:, -1] - model.md
        mag = mag + 0.5 * (v / model.sd) ** 2 + np.abs(x2[:, -1] * v) / model.sd ** 2
    b_lpri = (D + 16) * U * mag
    return b_lpri, b_llik, b_glik


def mp_parts(model, x, dps=40):
    """(log prior, log likelihood, gradient of each) at one point with mpmath at `dps` digits, from the float64 data."""
    import mpmath as mp
    x = [float(v) for v in x]
    Dc, lt0, R = model.Dc, model.lt0, model.R
    with mp.workdps(dps):
        X = [mp.mpf(v) for v in x]
        tau = [mp.exp(X[lt0 + r]) for r in range(R)]
        hl = mp.log(2 * mp.pi) / 2
        lp = mp.mpf(0)
        gp = [mp.mpf(0)] * model.dim
        for c in range(Dc):
            s = mp.mpf(float(model.s[c]))
            lp += -(X[c] / s) ** 2 / 2 - mp.log(s) - hl
            gp[c] = -X[c] / s ** 2
        for c in range(Dc, lt0):
            lp += -X[c] ** 2 / 2 - hl
            gp[c] = -X[c]
        for r in range(R):
            st = mp.mpf(float(model.s_tau[r]))
            lp += mp.log(2) - mp.log(st) - hl - tau[r] ** 2 / (2 * st ** 2) + X[lt0 + r]
            gp[lt0 + r] = 1 - tau[r] ** 2 / st ** 2
        if model.disp:
            v, sd = X[-1] - mp.mpf(model.md), mp.mpf(model.sd)
            lp += -(v / sd) ** 2 / 2 - mp.log(sd) - hl
            gp[-1] = -v / sd ** 2
        ll = mp.mpf(0)
        gl = [mp.mpf(0)] * model.dim
        for i in range(len(model.y)):
            own = [model.off[r] + int(model.g[r][i]) for r in range(R)]
            zi = [mp.mpf(float(model.z[r][i])) for r in range(R)]
            a = [zi[r] * tau[r] * X[own[r]] for r in range(R)]
            eta = mp.fsum(X[c] * mp.mpf(float(model.Z[i, c])) for c in range(Dc)) + mp.fsum(a)
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
                rr = y - eta
                term, d, gt = -X[-1] - hl - rr * rr * w / 2, rr * w, rr * rr * w - 1
            else:
                mu, phi = mp.exp(eta), mp.exp(X[-1])
                L = mp.log(mu + phi)
                term = mp.loggamma(y + phi) - mp.loggamma(phi) - mp.loggamma(y + 1) + phi * (X[-1] - L) + y * (eta - L)
                d = y - (y + phi) * mu / (mu + phi)
                gt = phi * (mp.digamma(y + phi) - mp.digamma(phi) - mp.log1p(mu / phi) + (mu - y) / (mu + phi))
            ll += term
            for c in range(Dc):
                gl[c] += d * mp.mpf(float(model.Z[i, c]))
            for r in range(R):
                gl[own[r]] += d * zi[r] * tau[r]
                gl[lt0 + r] += d * a[r]
            if model.disp:
                gl[-1] += gt
        return float(lp), float(ll), np.array([float(v) for v in gp]), np.array([float(v) for v in gl])


def synthetic(family, n, p, terms, seed, intercept=True, tau=0.8, scale=0.5, empty=None, zero=None):
    """A fixed-seed synthetic multilevel regression.  `terms` is [(J, factor)]: terms with the same `factor` share one
    draw of levels (their J must agree); the first term on a factor is a varying intercept (z = 1), every further one a
    varying slope on its own N(0, 1) covariate.  X ~ N(0, 1) / sqrt(p), coefficients ~ N(0, scale^2), effects ~ N(0,
    tau^2); empty = (r, j) leaves level j of term r's factor without observations, zero = r sets z_r = 0 throughout;
    sigma = 0.7 (normal), phi = 3 (NB).  Returns X, y and [(g_r, z_r, J_r)]."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, p)) / math.sqrt(max(p, 1))
    beta = rng.standard_normal(p + 1) * scale
    levels, out = {}, []
    eta = (beta[0] if intercept else 0.0) + X @ beta[1:]
    for r, (J, f) in enumerate(terms):
        first = f not in levels
        if first:
            skip = {empty[1]} if empty is not None and terms[empty[0]][1] == f else set()
            live = np.array([j for j in range(J) if j not in skip])
            levels[f] = live[rng.integers(0, len(live), n)]
        g = levels[f]
        z = np.ones(n) if first else rng.standard_normal(n)
        if zero == r:
            z = np.zeros(n)
        eta = eta + z * (rng.standard_normal(J) * tau)[g]
        out.append((g, z, J))
    if family == "bernoulli_logit":
        y = (rng.random(n) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
    elif family == "poisson_log":
        y = rng.poisson(np.exp(np.clip(eta, -20, 5))).astype(np.float64)
    elif family == "normal":
        y = eta + 0.7 * rng.standard_normal(n)
    else:
        mu = np.exp(np.clip(eta, -20, 5))
        y = rng.poisson(rng.gamma(3.0, mu / 3.0)).astype(np.float64)
    return X, y, out
