"""Reference densities for the continuous-response GLM target (ContinuousGLM family "gamma_log" / "student_t";
SMCN_MODEL_CGLM families 0 and 1), modelled on tests/_glm_disp.py.

x = (b_1..b_Dc, tau), D = Dc + 1; eta = [b_0 +] X b; prior N(0, s_c^2) on b_c and N(m, s^2) on tau.
  gamma_log (a = e^tau, c = log y, u = c - eta, r = e^u):
      term = a (tau + u - r) - lgamma(a) - c,   d / d eta = a (r - 1),   d / d tau = a (tau + 1 - psi(a) + u - r)
  student_t (z = (y - eta) e^-tau):
      term = C(df) - tau - (df + 1) / 2 log1p(z^2 / df),   d / d eta = (df + 1) z e^-tau / (df + z^2),
      d / d tau = (df + 1) z^2 / (df + z^2) - 1
Non-finite (-inf): e^tau (gamma) or e^-tau (student_t) leaves the normal range -- the evaluation then runs with tau = 0,
so the gradients stay numbers --, e^-eta overflows (gamma), z overflows (student_t).

`ContGLMNumpy` is the model as a plain Python object with the reference's StanModel surface (.dim, .logpdf(x, phi),
.logpdfgrad(x, phi), .constrain(x)): it runs through HostTarget and oracle/pynuts.PyNUTS.  Its terms take the device's
algorithm (smcn_glm_cont.hpp): a tau - lgamma(a) and tau + 1 - psi(a) from Stirling's series for a >= 10 and from a shift
up to >= 10 below; C(df) from the series' difference for df >= 20; log1p(z^2 / df) as log(1 + w) with the rounding of
1 + w put back, and beyond |z| > T = 1e150 min(1, sqrt(df)) the limits 2 log|z| - log df, (df + 1) / z e^-tau and df.
`mp_obs` is the mpmath value (>= 40 digits) of one observation's term and derivatives, `mp_parts` the whole density's;
`exact_parts` is math.fsum over the float64 terms.

device_bounds: the worst-case |device - exact|.  Every per-observation quantity is within c_obs u (u = 2^-53) of the sum
of the magnitudes of the addends of the formula AS EVALUATED -- for the gamma term |k0's addends| + a |u| + a r + |c|, for
student_t |C's addends| + |tau| + hp (|l| [+ |log df| + |log|z||]) + (df + 1) w / (1 + w), the last for the relative
rounding of z, which the logarithm sees through d l / d log z <= 2 w / (1 + w) -- plus |d term / d eta| e_eta for the
linear predictor, e_eta as in _glm_disp (gamma: + 2 u (|c| + |eta|) for log y and the subtraction c - eta).  c_obs = 64
is the constant _glm_disp.device_bounds uses for the flat dispersion families: the operations behind one quantity here
are an exp_fast or a log_ge1 with an rcp_nr (a few ulp each), at most three fused multiply-adds and the per-evaluation
constants (lgamma_digamma_pos or the two series: under 20 roundings of their own addends), the reference's float64 the
same again -- well under 64, so the constant stands as it is.  The sums over n are within (n + 2) u of the sum of
magnitudes.
"""
import math

import numpy as np

import _glm_disp as gd
from _glm import HALF_LOG_2PI, U

LOG_DBL_MAX, LOG_DBL_MIN, ASYM = gd.LOG_DBL_MAX, gd.LOG_DBL_MIN, gd.ASYM
FAMILIES = ("gamma_log", "student_t")
LOG_PI = math.log(math.pi)


def _m_lgamma(x):
    """lgamma_digamma(x) with the magnitudes of the addends lgamma and psi are formed from."""
    lg, ps, xs, P, S = gd.lgamma_digamma(x)
    lx = np.abs(np.log(xs))
    return lg, ps, (xs + 0.5) * lx + xs + np.abs(np.log(P)) + 1.0, lx + S + 1.0


def df_const(df):
    """What the device derives from df alone (glm_cont_df): dict, with mc the magnitude of C's addends."""
    df = float(df)
    x = 0.5 * df
    f = dict(df=df, idf=1.0 / df, dfp1=df + 1.0, hp=0.5 * (df + 1.0), ldf=math.log(df), T=1e150 * min(1.0, math.sqrt(df)))
    f["q"] = f["dfp1"] * f["idf"]
    if x >= ASYM:
        l1 = math.log1p(0.5 / x)
        f["c"] = ((x * l1 - 0.5) - HALF_LOG_2PI) + float(gd.stirling_tail(1.0 / (x + 0.5)) - gd.stirling_tail(1.0 / x))
        f["mc"] = x * l1 + 0.5 + HALF_LOG_2PI + 1.0
    else:
        la, _, ma, _ = _m_lgamma(np.array(x + 0.5))
        lb, _, mb, _ = _m_lgamma(np.array(x))
        f["c"] = float(la - lb) - 0.5 * (f["ldf"] + LOG_PI)
        f["mc"] = float(ma + mb) + 0.5 * (abs(f["ldf"]) + LOG_PI)
    return f


def gamma_obs(y, c, eta, tau):
    """gamma_log per observation (broadcast): term, d / d eta, d / d tau, the magnitudes of the addends each is formed
    from, |d d / d eta| and |d gt / d eta|.  tau must be in range."""
    y, c, eta, tau = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (y, c, eta, tau)))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        a = np.exp(tau)
        big = a >= ASYM
        ia = 1.0 / a
        k0b = ((0.5 * tau + a) - HALF_LOG_2PI) - gd.stirling_tail(ia)
        k1b = 1.0 + (0.5 * ia + gd.digamma_tail(ia))
        lg, ps, mlg, mps = _m_lgamma(np.where(big, ASYM, a))
        k0s = a * tau - lg
        k1s = (tau + 1.0) - ps
        k0, k1 = np.where(big, k0b, k0s), np.where(big, k1b, k1s)
        mk0 = np.where(big, np.abs(0.5 * tau) + a + HALF_LOG_2PI + 1.0, np.abs(a * tau) + mlg)
        mk1 = np.where(big, 2.0, np.abs(tau) + 1.0 + mps)
        u = c - eta
        r = np.exp(np.clip(u, -800.0, 800.0))
        term = (k0 + a * (u - r)) - c
        term = np.where(-eta <= LOG_DBL_MAX, term, -np.inf)
        d = a * (r - 1.0)
        gt = a * ((k1 + u) - r)
        m_term = mk0 + a * (np.abs(u) + r) + np.abs(c)
        m_d = a * (r + 1.0)
        m_gt = a * (mk1 + np.abs(u) + r)
        w_d = a * r
        w_gt = a * (r + 1.0)
        e_u = 2.0 * U * (np.abs(c) + np.abs(eta))
    return term, d, gt, m_term, m_d, m_gt, w_d, w_gt, e_u


def student_obs(y, eta, tau, f):
    y, eta, tau = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (y, eta, tau)))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        eit = np.exp(-tau)
        z = (y - eta) * eit
        za = np.abs(z)
        far = za > f["T"]
        w = (z * z) * f["idf"]
        u1 = np.where(far, za, 1.0 + w)
        inv = 1.0 / u1
        lg = np.log(u1)
        l = np.where(far, 2.0 * lg - f["ldf"], (w - (u1 - 1.0)) * inv + lg)
        term = (f["c"] - tau) - f["hp"] * l
        term = np.where(za < np.inf, term, -np.inf)
        d = np.where(far, (f["dfp1"] * eit) * np.copysign(inv, z), (f["q"] * inv) * (z * eit))
        wi = np.where(far, 1.0, w * inv)
        gt = np.where(far, f["df"], f["dfp1"] * wi - 1.0)
        m_term = f["mc"] + np.abs(tau) + f["hp"] * (np.abs(l) + np.where(far, abs(f["ldf"]) + np.abs(lg), 0.0)) + f["dfp1"] * wi
        m_d = np.abs(d)
        m_gt = f["dfp1"] * wi + 1.0
        w_d = np.where(far, f["dfp1"] * (eit * inv) ** 2, f["q"] * inv * eit * eit)
        w_gt = 2.0 * np.abs(d)
    return term, d, gt, m_term, m_d, m_gt, w_d, w_gt, np.zeros_like(term)


class ContGLMNumpy:
    def __init__(self, X, y, family="gamma_log", prior_sd=2.5, dispersion_prior=(0.0, 2.5), intercept=True, df=4.0):
        X = np.asarray(X, dtype=np.float64)
        if X.ndim == 1:
            X = X.reshape(-1, 1)
        assert family in FAMILIES
        self.family, self.intercept = family, bool(intercept)
        self.student = family == "student_t"
        self.df = float(df) if self.student else None
        self.f = df_const(df) if self.student else None
        self.y = np.asarray(y, dtype=np.float64)
        self.c = np.zeros_like(self.y) if self.student else np.array([math.log(v) for v in self.y])
        self.Z = np.hstack([np.ones((X.shape[0], 1)), X]) if intercept else X.copy()
        self.Dc = self.Z.shape[1]
        self.dim = self.Dc + 1
        self.constrained_dim = self.dim
        s = np.asarray(prior_sd, dtype=np.float64)
        sc = np.full(self.Dc, float(s)) if s.ndim == 0 else s.copy()
        self.m = np.concatenate([np.zeros(self.Dc), [float(dispersion_prior[0])]])
        self.s = np.concatenate([sc, [float(dispersion_prior[1])]])
        self.calls = 0

    def param_names(self):
        return (["Intercept"] if self.intercept else []) + [f"beta.{j + 1}" for j in range(self.Dc - self.intercept)] \
            + ["sigma" if self.student else "shape"]

    def constrain(self, x):
        x = np.array(x, dtype=np.float64, copy=True)
        x[..., -1] = np.exp(x[..., -1])
        return x

    def bad(self, tau):
        s = -tau if self.student else tau
        return ~((s <= LOG_DBL_MAX) & (s >= LOG_DBL_MIN))

    def obs(self, x2):
        """eta [M, n] and the per-observation tuple of *_obs; rows whose tau is out of range are evaluated at tau = 0
        (their llik is -inf regardless)."""
        x2 = np.atleast_2d(np.asarray(x2, dtype=np.float64))
        eta = x2[:, :self.Dc] @ self.Z.T
        tau = x2[:, -1:]
        tau = np.where(self.bad(tau), 0.0, tau)
        if self.student:
            return eta, student_obs(self.y[None, :], eta, tau, self.f)
        return eta, gamma_obs(self.y[None, :], self.c[None, :], eta, tau)

    def parts(self, x):
        x2 = np.atleast_2d(np.asarray(x, dtype=np.float64))
        _, (term, d, gt, *_r) = self.obs(x2)
        v = x2 - self.m
        lpri = np.sum(-0.5 * (v / self.s) ** 2 - np.log(self.s) - HALF_LOG_2PI, axis=1)
        with np.errstate(invalid="ignore"):
            llik = np.where(self.bad(x2[:, -1]), -np.inf, np.sum(term, axis=1))
            llik = np.where(np.isnan(llik), -np.inf, llik)
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


def _fsum(v):
    return math.fsum(v.tolist()) if np.all(np.isfinite(v)) else np.nan


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
            glik[k, c] = _fsum(prod[:, c])
        glik[k, -1] = _fsum(gt[k])
    return lpri, llik, -v / model.s ** 2, glik


def device_bounds(model, x2, c_obs=64):
    """Worst-case |device - exact| of lpri, llik (per particle) and glik (per particle and coordinate); the module's
    docstring has the derivation."""
    x2 = np.atleast_2d(np.asarray(x2, dtype=np.float64))
    eta, (term, d, gt, m_term, m_d, m_gt, w_d, w_gt, e_u) = model.obs(x2)
    n, Dc = model.Z.shape
    A = np.abs(x2[:, :Dc]) @ np.abs(model.Z).T
    e_eta = (2 * Dc + 4) * U * A + 4 * U * np.abs(eta) + e_u
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


def mp_obs(family, y, eta, tau, df=4.0, dps=40):
    """(term, d term / d eta, d term / d tau) of one observation with mpmath at `dps` digits, from the densities'
    textbook forms; a value beyond the doubles comes back as +-inf."""
    import mpmath as mp
    with mp.workdps(dps):
        y, eta, tau = mp.mpf(float(y)), mp.mpf(float(eta)), mp.mpf(float(tau))
        if family == "gamma_log":
            a = mp.exp(tau)
            r = y * mp.exp(-eta)
            term = a * (tau - eta) + (a - 1) * mp.log(y) - a * r - mp.loggamma(a)
            out = (term, a * (r - 1), a * (tau + 1 - mp.digamma(a) + mp.log(y) - eta - r))
        else:
            df = mp.mpf(float(df))
            s = mp.exp(tau)
            z = (y - eta) / s
            C = mp.loggamma((df + 1) / 2) - mp.loggamma(df / 2) - mp.log(df * mp.pi) / 2
            out = (C - tau - (df + 1) / 2 * mp.log1p(z * z / df), (df + 1) * z / s / (df + z * z),
                   (df + 1) * z * z / (df + z * z) - 1)
        return tuple(float(v) for v in out)


def mp_parts(model, x, dps=40):
    """(llik, glik [D]) of one point x [D] with mpmath: the sums over the observations at `dps` digits."""
    import mpmath as mp
    x = np.asarray(x, dtype=np.float64)
    with mp.workdps(dps):
        b = [mp.mpf(float(v)) for v in x[:model.Dc]]
        tau = float(x[-1])
        ll, g, gtau = mp.mpf(0), [mp.mpf(0)] * model.Dc, mp.mpf(0)
        for i in range(model.y.shape[0]):
            zi = [mp.mpf(float(v)) for v in model.Z[i]]
            eta = mp.fsum(p * q for p, q in zip(b, zi))
            yv = mp.mpf(float(model.y[i]))
            if model.student:
                df, s = mp.mpf(model.df), mp.exp(mp.mpf(tau))
                z = (yv - eta) / s
                C = mp.loggamma((df + 1) / 2) - mp.loggamma(df / 2) - mp.log(df * mp.pi) / 2
                t, d, gt = (C - tau - (df + 1) / 2 * mp.log1p(z * z / df), (df + 1) * z / s / (df + z * z),
                            (df + 1) * z * z / (df + z * z) - 1)
            else:
                a = mp.exp(mp.mpf(tau))
                r = yv * mp.exp(-eta)
                t = a * (tau - eta) + (a - 1) * mp.log(yv) - a * r - mp.loggamma(a)
                d, gt = a * (r - 1), a * (tau + 1 - mp.digamma(a) + mp.log(yv) - eta - r)
            ll += t
            g = [gc + d * zc for gc, zc in zip(g, zi)]
            gtau += gt
        return float(ll), np.array([float(v) for v in g] + [float(gtau)])


def synthetic(family, n, p, seed, scale=None, tau=None, df=4.0):
    """A fixed-seed synthetic regression: X ~ N(0, 1) / sqrt(p), coefficients ~ N(0, 1); shape = 3 (gamma_log) or
    sigma = 0.7 (student_t, with t_df noise) unless tau is given."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, p)) / math.sqrt(max(p, 1))
    beta = rng.standard_normal(p + 1) * (1.0 if scale is None else scale)
    eta = beta[0] + X @ beta[1:]
    if family == "gamma_log":
        a = 3.0 if tau is None else math.exp(tau)
        y = np.maximum(rng.gamma(a, np.exp(np.clip(eta, -20, 5)) / a), 1e-300)
    else:
        sigma = 0.7 if tau is None else math.exp(tau)
        y = eta + sigma * rng.standard_normal(n) * np.sqrt(df / rng.chisquare(df, n))
    return X, y


def outlier_data(seed=8):
    """n = 200, y = 1 + 2 x + N(0, 1), and the 10 rows with the largest x moved up by 50 sd: leverage and a common
    direction, so that a normal likelihood's slope is dragged (tests/test_cglm_robust_host.py has by how much)."""
    rng = np.random.default_rng(seed)
    n = 200
    x = rng.standard_normal(n)
    y = 1.0 + 2.0 * x + rng.standard_normal(n)
    y[np.argsort(x)[-10:]] += 50.0
    return x, y
