"""Reference densities for the GLM target's dispersion families (GLMTarget family "normal" / "neg_binomial_2_log";
SMCN_MODEL_GLM families 2 and 3).

x = (b_1..b_Dc, tau), D = Dc + 1; eta = [b_0 +] X b; prior N(0, s_c^2) on b_c and N(m, s^2) on tau.
  normal (sigma = e^tau):   term_i = -tau - log(2 pi) / 2 - (y_i - eta_i)^2 e^-2tau / 2
  NB2 (mu = e^eta, phi = e^tau, L = log(mu + phi)):
                            term_i = lgamma(y + phi) - lgamma(phi) - lgamma(y + 1) + phi (tau - L) + y (eta - L)
Non-finite (-inf): e^-2tau overflows (normal); e^eta or e^tau overflows, or e^tau is below the normal range (NB).

`GLMDispNumpy` is the model as a plain Python object with the reference's StanModel surface (.dim, .logpdf(x, phi),
.logpdfgrad(x, phi), .constrain(x)): it runs through HostTarget and oracle/pynuts.PyNUTS.  Its NB terms take the
device's algorithm (smcn_glm_family.hpp glm_disp_obs): for phi >= 10 lgamma(y + phi) - lgamma(phi) - y tau and
psi(y + phi) - psi(phi) from Stirling's series and log1p(y / phi), below from a shift up to >= 10 and the same series.
`mp_obs` is the 40-digit mpmath value of one observation's term and derivatives; `exact_parts` / `device_bounds`
are the fsum reference and the worst-case error bound of the device's evaluation, as tests/_glm.py has them.
"""
import math

import numpy as np

from _glm import HALF_LOG_2PI, U

LOG_DBL_MAX = 709.782712893384           # exp(v) is finite for v <= this
LOG_DBL_MIN = -708.3964185322641         # exp(v) is a normal double for v >= this
ASYM = 10.0
ST = (1 / 12, -1 / 360, 1 / 1260, -1 / 1680, 1 / 1188, -691 / 360360, 1 / 156, -3617 / 122400)
DT = (1 / 12, -1 / 120, 1 / 252, -1 / 240, 1 / 132, -691 / 32760, 1 / 12, -3617 / 8160)
DISP_FAMILIES = ("normal", "neg_binomial_2_log")


def _poly(c, t):
    p = c[-1]
    for v in reversed(c[:-1]):
        p = p * t + v
    return p


def stirling_tail(ix):
    return _poly(ST, ix * ix) * ix


def digamma_tail(ix):
    t = ix * ix
    return _poly(DT, t) * t


def gamma_shift(x):
    """x shifted up to >= 10 (x > 0), the product P of the values passed and the sum S of their reciprocals."""
    x = np.array(x, dtype=np.float64, copy=True)
    P, S = np.ones_like(x), np.zeros_like(x)
    for _ in range(11):
        m = x < ASYM
        if not np.any(m):
            break
        xm = np.where(m, x, 1.0)
        P = np.where(m, P * xm, P)
        S = np.where(m, S + 1.0 / xm, S)
        x = np.where(m, x + 1.0, x)
    return x, P, S


def digamma(x):
    """The device's digamma_pos (smcn_device.hpp), restated: shift, then log x - 1 / (2x) - the series."""
    xs, _, S = gamma_shift(x)
    ix = 1.0 / xs
    return ((np.log(xs) - 0.5 * ix) - digamma_tail(ix)) - S


def lgamma_digamma(x):
    xs, P, S = gamma_shift(x)
    ix = 1.0 / xs
    lx = np.log(xs)
    lg = (((xs - 0.5) * lx - xs) + (HALF_LOG_2PI + stirling_tail(ix))) - np.log(P)
    psi = ((lx - 0.5 * ix) - digamma_tail(ix)) - S
    return lg, psi, xs, P, S


def lgamma1p(y):
    return np.array([math.lgamma(v + 1.0) for v in np.ravel(y)]).reshape(np.shape(y))


def nb_obs(y, eta, tau, lgy=None):
    """NB2 per observation (broadcast): term, d term / d eta, d term / d tau, and the magnitudes of the addends each
    is formed from (the scale of its rounding error).  tau must be in range (phi finite and normal)."""
    y, eta, tau = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (y, eta, tau)))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        phi = np.exp(tau)
        iphi = 1.0 / phi
        big = phi >= ASYM
        x = y + phi
        lgy = lgamma1p(y) if lgy is None else np.broadcast_to(lgy, y.shape)
        # phi >= 10
        l1 = np.log1p(y * iphi)
        ixb = 1.0 / x
        Ab = ((x - 0.5) * l1 - y) + (stirling_tail(ixb) - stirling_tail(iphi))
        Bb = (0.5 * y * (ixb * iphi) + l1) - (digamma_tail(ixb) - digamma_tail(iphi))
        mAb = (x + 0.5) * np.abs(l1) + y
        mBb = np.abs(l1) + y * ixb * iphi
        # phi < 10
        lgx, psx, xs, P, S = lgamma_digamma(np.where(y == 0.0, ASYM, x))
        lgp, psp, ps, Pp, Sp = lgamma_digamma(phi)
        As, Bs = lgx - lgp, psx - psp
        mAs = (xs + 0.5) * np.abs(np.log(xs)) + xs + np.abs(np.log(P)) + (ps + 0.5) * np.abs(np.log(ps)) + ps \
            + np.abs(np.log(Pp)) + 2.0
        mBs = np.abs(np.log(xs)) + S + np.abs(np.log(ps)) + Sp + 1.0
        A = np.where(y == 0.0, 0.0, np.where(big, Ab, As))
        B = np.where(y == 0.0, 0.0, np.where(big, Bb, Bs))
        mA = np.where(y == 0.0, 0.0, np.where(big, mAb, mAs))
        mB = np.where(y == 0.0, 0.0, np.where(big, mBb, mBs))
        ts = np.where(big, 0.0, tau)
        z = eta - tau
        t = np.exp(-np.abs(z))
        inv = 1.0 / (1.0 + t)
        sp = np.maximum(z, 0.0) + np.log1p(t)
        ti = t * inv
        sg = np.where(z >= 0.0, inv, ti)
        sc = np.where(z >= 0.0, ti, inv)
        term = ((A - lgy) - x * sp) + y * (eta - ts)
        term = np.where(eta <= LOG_DBL_MAX, term, -np.inf)
        d = y - x * sg
        gt = phi * ((B - sp) + sg) - y * sc
        m_term = mA + lgy + x * sp + np.abs(y * eta) + np.abs(y * ts)
        m_d = y + x * sg
        m_gt = phi * (mB + sp + sg) + y * sc
        w_d = x * sg * sc                                   # |d d / d eta|
        w_gt = phi * sg * sg + y * sg * sc                  # |d gt / d eta| <= this
    return term, d, gt, m_term, m_d, m_gt, w_d, w_gt


def normal_obs(y, eta, tau):
    y, eta, tau = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (y, eta, tau)))
    with np.errstate(over="ignore", invalid="ignore"):
        w = np.exp(-2.0 * tau)
        c0 = -tau - HALF_LOG_2PI
        r = y - eta
        rw = r * w
        q = r * rw
        term = c0 - 0.5 * q
        gt = q - 1.0
        m_term = np.abs(c0) + q
        m_d = np.abs(rw)
        m_gt = q + 1.0
        w_d = w
        w_gt = 2.0 * np.abs(rw)
    return term, rw, gt, m_term, m_d, m_gt, w_d, w_gt


class GLMDispNumpy:
    def __init__(self, X, y, family="normal", prior_sd=2.5, dispersion_prior=(0.0, 2.5), intercept=True):
        X = np.asarray(X, dtype=np.float64)
        if X.ndim == 1:
            X = X.reshape(-1, 1)
        self.family, self.intercept = family, bool(intercept)
        self.y = np.asarray(y, dtype=np.float64)
        self.Z = np.hstack([np.ones((X.shape[0], 1)), X]) if intercept else X.copy()
        self.Dc = self.Z.shape[1]
        self.dim = self.Dc + 1
        self.constrained_dim = self.dim
        s = np.asarray(prior_sd, dtype=np.float64)
        sc = np.full(self.Dc, float(s)) if s.ndim == 0 else s.copy()
        self.m = np.concatenate([np.zeros(self.Dc), [float(dispersion_prior[0])]])
        self.s = np.concatenate([sc, [float(dispersion_prior[1])]])
        self.lgy = lgamma1p(self.y) if family == "neg_binomial_2_log" else np.zeros_like(self.y)
        self.calls = 0

    def param_names(self):
        return (["Intercept"] if self.intercept else []) + [f"beta.{j + 1}" for j in range(self.Dc - self.intercept)] \
            + ["sigma" if self.family == "normal" else "phi"]

    def constrain(self, x):
        x = np.array(x, dtype=np.float64, copy=True)
        x[..., -1] = np.exp(x[..., -1])
        return x

    def bad(self, tau):
        if self.family == "normal":
            return -2.0 * tau > LOG_DBL_MAX
        return ~((tau <= LOG_DBL_MAX) & (tau >= LOG_DBL_MIN))

    def obs(self, x2):
        """eta [M, n] and the per-observation tuple of *_obs; rows whose tau is out of range get tau = 0 (their llik
        is -inf regardless)."""
        x2 = np.atleast_2d(np.asarray(x2, dtype=np.float64))
        eta = x2[:, :self.Dc] @ self.Z.T
        tau = x2[:, -1:]
        tau = np.where(self.bad(tau), 0.0, tau)
        if self.family == "normal":
            return eta, normal_obs(self.y[None, :], eta, tau)
        return eta, nb_obs(self.y[None, :], eta, tau, self.lgy[None, :])

    def parts(self, x):
        x2 = np.atleast_2d(np.asarray(x, dtype=np.float64))
        _, (term, d, gt, *_r) = self.obs(x2)
        v = x2 - self.m
        lpri = np.sum(-0.5 * (v / self.s) ** 2 - np.log(self.s) - HALF_LOG_2PI, axis=1)
        llik = np.where(self.bad(x2[:, -1]), -np.inf, np.sum(term, axis=1))
        with np.errstate(invalid="ignore"):
            glik = np.concatenate([d @ self.Z, np.sum(gt, axis=1, keepdims=True)], axis=1)
        gpri = -v / self.s ** 2
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
    """(lpri, llik, gpri, glik) with every sum over observations / coordinates taken by math.fsum."""
    x2 = np.atleast_2d(np.asarray(x2, dtype=np.float64))
    _, (term, d, gt, *_r) = model.obs(x2)
    M = x2.shape[0]
    v = x2 - model.m
    lpri = np.array([math.fsum((-0.5 * (v[k] / model.s) ** 2 - np.log(model.s) - HALF_LOG_2PI).tolist()) for k in range(M)])
    bad = model.bad(x2[:, -1])
    llik = np.array([math.fsum(term[k].tolist()) if (np.all(np.isfinite(term[k])) and not bad[k]) else -np.inf
                     for k in range(M)])
    glik = np.empty_like(x2)
    for k in range(M):
        prod = d[k][:, None] * model.Z
        for c in range(model.Dc):
            glik[k, c] = math.fsum(prod[:, c].tolist()) if np.all(np.isfinite(prod[:, c])) else np.nan
        glik[k, -1] = math.fsum(gt[k].tolist()) if np.all(np.isfinite(gt[k])) else np.nan
    return lpri, llik, -v / model.s ** 2, glik


def device_bounds(model, x2, c_obs=64):
    """Worst-case |device - exact| of lpri, llik (per particle) and glik (per particle and coordinate).

    eta as in tests/_glm.py (D fused multiply-adds, error <= D u A_i, the reference's the same); each per-observation
    quantity within c_obs u of the magnitudes of the addends it is formed from (exp_fast, log1p_pos, log_ge1 and the
    series: a few ulp each, the reference's float64 the same again), plus the eta error times its derivative in eta;
    the sums over n within (n + 2) u of the sum of magnitudes."""
    x2 = np.atleast_2d(np.asarray(x2, dtype=np.float64))
    eta, (term, d, gt, m_term, m_d, m_gt, w_d, w_gt) = model.obs(x2)
    n, Dc = model.Z.shape
    A = np.abs(x2[:, :Dc]) @ np.abs(model.Z).T
    e_eta = (2 * Dc + 4) * U * A + 4 * U * np.abs(eta)
    with np.errstate(over="ignore", invalid="ignore"):
        e_term = c_obs * U * m_term + np.abs(d) * e_eta
        e_d = c_obs * U * m_d + w_d * e_eta
        e_gt = c_obs * U * m_gt + w_gt * e_eta
        b_llik = np.sum(e_term, axis=1) + (n + 2) * U * np.sum(np.abs(term), axis=1)
        b_glik = np.concatenate([(e_d + (n + 2) * U * np.abs(d)) @ np.abs(model.Z),
                                 (np.sum(e_gt, axis=1) + (n + 2) * U * np.sum(np.abs(gt), axis=1))[:, None]], axis=1)
    v = x2 - model.m
    pri = -0.5 * (v / model.s) ** 2 - np.log(model.s) - HALF_LOG_2PI
    b_lpri = (Dc + 8) * U * np.sum(np.abs(pri) + 0.5 * (v / model.s) ** 2 + np.abs(np.log(model.s)) + HALF_LOG_2PI
                                   + np.abs(x2) * np.abs(v) / model.s ** 2, axis=1)
    return b_lpri, b_llik, b_glik


def mp_obs(family, y, eta, tau, dps=40):
    """(term, d term / d eta, d term / d tau) of one observation with mpmath at `dps` digits."""
    import mpmath as mp
    with mp.workdps(dps):
        y, eta, tau = mp.mpf(float(y)), mp.mpf(float(eta)), mp.mpf(float(tau))
        if family == "normal":
            w = mp.exp(-2 * tau)
            r = y - eta
            return (float(-tau - mp.log(2 * mp.pi) / 2 - r * r * w / 2), float(r * w), float(r * r * w - 1))
        mu, phi = mp.exp(eta), mp.exp(tau)
        L = mp.log(mu + phi)
        term = mp.loggamma(y + phi) - mp.loggamma(phi) - mp.loggamma(y + 1) + phi * (tau - L) + y * (eta - L)
        d = y - (y + phi) * mu / (mu + phi)
        g = phi * (mp.digamma(y + phi) - mp.digamma(phi) - mp.log1p(mu / phi) + (mu - y) / (mu + phi))
        return float(term), float(d), float(g)


def synthetic(family, n, p, seed, scale=None, tau=None):
    """A fixed-seed synthetic regression: X ~ N(0, 1) / sqrt(p), coefficients ~ N(0, 1); sigma = 0.7 (normal) or
    phi = 3 (NB) unless tau is given."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, p)) / math.sqrt(max(p, 1))
    beta = rng.standard_normal(p + 1) * (1.0 if scale is None else scale)
    eta = beta[0] + X @ beta[1:]
    if family == "normal":
        sigma = 0.7 if tau is None else math.exp(tau)
        y = eta + sigma * rng.standard_normal(n)
    else:
        phi = 3.0 if tau is None else math.exp(tau)
        mu = np.exp(np.clip(eta, -20, 5))
        y = rng.poisson(rng.gamma(phi, mu / phi)).astype(np.float64)
    return X, y
