"""Reference of the arma forecasts (smcnuts_amd/forecast.py; include/smcnuts_hip.h, smcn_forecast_*): an fp64 NumPy
restatement of every definition, the same in mpmath at 50 digits, err_T with every fma rounded once (exact), the paths
and the systematic ancestors.

Per point x = (mu, beta, theta, s), sigma = exp(s), series y_1..y_T (y_0 := mu, err_0 := 0):
  err_1 = y_1 - mu - beta mu,  err_t = y_t - mu - beta y_{t-1} - theta err_{t-1}
  m_1 = mu + beta y_T + theta err_T,  m_h = mu + beta m_{h-1}
  psi_0 = 1, psi_1 = beta + theta, psi_j = beta psi_{j-1};  v_h = sigma^2 sum_{j<h} psi_j^2
  bad at h: sigma, m_h or v_h non-finite, or v_h <= 0
  a_h = log N(yf_h | m_h, v_h);  J_h = sum_{j<=h} normal_lpdf(yf_j | nu_{T+j}, sigma), the recurrence continued through yf
Mixture over the particles with a finite lw that are not bad at h, w = exp(lw - mw):
  mean_h = sum w m_h / sum w,  var_h = sum w v_h / sum w + sum w (m_h - mean_h)^2 / sum w,
  cdf_hk = sum w Phi((at_hk - m_h) / sqrt(v_h)) / sum w,
  lpd_marginal_h = log sum w exp(a_h) - log sw,  lpd_joint_h = log sum w exp(J_h) - log sw   (sw: over every finite lw)
Paths: e_h = sigma z_{s,h}, z the Box-Muller cosine of philox_uniform(seed, s, h, stream 21, q = 0, 1), h = 1..H;
  y_{T+1} = m_1 + e_1,  y_{T+h} = (mu + beta y_{T+h-1} + theta e_{h-1}) + e_h;  NaN from the first non-finite value on.
"""
import math

import mpmath as mp
import numpy as np

import _arma_recur
from _predict_draws import box_muller, philox_uniform

U = 2.0 ** -53
ST_ANC, ST_NOISE = 20, 21
LOG2PI = math.log(2.0 * math.pi)
MA, SA, MJ, SJ, NBAD, C0, SW, S1, S2, VAR, P0 = range(11)


# ---- fp64 ---------------------------------------------------------------------------------------------------------------
def err_chain(series, X, yf=None):
    """(err_T [M], e [M, H]: the recurrence continued through yf)."""
    y = np.asarray(series, dtype=np.float64)
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    mu, beta, theta = X[:, 0], X[:, 1], X[:, 2]
    with np.errstate(all="ignore"):
        err = y[0] - mu - beta * mu
        for t in range(1, len(y)):
            err = y[t] - mu - beta * y[t - 1] - theta * err
        out = []
        e, yp = err, y[-1]
        for v in ([] if yf is None else np.asarray(yf, dtype=np.float64)):
            e = v - mu - beta * yp - theta * e
            yp = v
            out.append(e)
    return err, (np.stack(out, axis=1) if out else None)


def laws(series, X, H):
    """(err_T [M], m [M, H], v [M, H], bad [M, H])."""
    y = np.asarray(series, dtype=np.float64)
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    mu, beta, theta, s = X.T
    err, _ = err_chain(y, X)
    with np.errstate(all="ignore"):
        sigma = np.exp(s)
        m = np.empty((X.shape[0], H))
        v = np.empty((X.shape[0], H))
        mh = mu + beta * y[-1] + theta * err
        psi, cum = np.ones_like(mu), np.ones_like(mu)
        for h in range(H):
            if h > 0:
                mh = mu + beta * mh
                psi = beta + theta if h == 1 else beta * psi
                cum = cum + psi * psi
            m[:, h], v[:, h] = mh, sigma * sigma * cum
        bad = ~(np.isfinite(sigma)[:, None] & np.isfinite(m) & np.isfinite(v) & (v > 0.0))
    return err, m, v, bad


def terms(series, X, yf):
    """(a [M, H] marginal terms (NaN when bad), J [M, H] cumulative joint terms)."""
    yf = np.asarray(yf, dtype=np.float64)
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    _, m, v, bad = laws(series, X, len(yf))
    _, e = err_chain(series, X, yf)
    with np.errstate(all="ignore"):
        a = np.where(bad, np.nan, -0.5 * (LOG2PI + np.log(v)) - 0.5 * (yf - m) ** 2 / v)
        sigma = np.exp(X[:, 3])[:, None]
        lj = (-0.5 * LOG2PI - X[:, 3])[:, None] - 0.5 * (e / sigma) ** 2
        J = np.cumsum(lj, axis=1)
    return a, J


def arma_llik(series, X):
    """The arma density's log-likelihood of the whole series, per point."""
    y = np.asarray(series, dtype=np.float64)
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    mu, beta, theta, s = X.T
    err = y[0] - mu - beta * mu
    ss = err * err
    for t in range(1, len(y)):
        err = y[t] - mu - beta * y[t - 1] - theta * err
        ss = ss + err * err
    return -0.5 * len(y) * LOG2PI - len(y) * s - 0.5 * ss / np.exp(2.0 * s)


def _phi(z):
    try:
        from scipy.special import erfc
    except ImportError:
        erfc = np.vectorize(math.erfc, otypes=[np.float64])
    return 0.5 * erfc(-np.asarray(z, dtype=np.float64) / math.sqrt(2.0))


def partials(series, X, lw, H, yf=None, at=None):
    """The mergeable partials [1 + H][10 + Tn] of the whole set as ONE block (include/smcnuts_hip.h)."""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    M = X.shape[0]
    lw = np.zeros(M) if lw is None else np.asarray(lw, dtype=np.float64)
    Tn = 0 if at is None else np.shape(at)[1]
    out = np.zeros((1 + H, P0 + Tn))
    fin = np.isfinite(lw)
    out[1:, MA], out[1:, MJ], out[1:, C0] = -np.inf, -np.inf, np.nan
    if not fin.any():
        out[0, 0] = -np.inf
        return out
    mw = np.max(lw[fin])
    w = np.where(fin, np.exp(np.where(fin, lw - mw, 0.0)), 0.0)
    out[0, :4] = mw, w.sum(), (w * w).sum(), fin.sum()
    _, m, v, bad = laws(series, X, H)
    if yf is not None:
        a, J = terms(series, X, yf)
    for h in range(H):
        ok = fin & ~bad[:, h]
        r = out[1 + h]
        r[NBAD] = np.sum(fin & bad[:, h])
        if not ok.any():
            continue
        if yf is not None:
            for col, t in ((MA, a[:, h]), (MJ, J[:, h])):
                use = ok & np.isfinite(t)
                if use.any():
                    tt = (lw - mw)[use] + t[use]
                    r[col] = tt.max()
                    r[col + 1] = np.exp(tt - tt.max()).sum()
        if not (ok & (w > 0.0)).any():
            continue
        c = m[ok & (w > 0.0), h][0]
        r[C0], r[SW] = c, w[ok].sum()
        r[S1], r[S2] = (w[ok] * (m[ok, h] - c)).sum(), (w[ok] * (m[ok, h] - c) ** 2).sum()
        r[VAR] = (w[ok] * v[ok, h]).sum()
        for k in range(Tn):
            r[P0 + k] = (w[ok] * _phi((at[h][k] - m[ok, h]) / np.sqrt(v[ok, h]))).sum()
    return out


def mixture(series, X, lw, H, yf=None, at=None):
    """dict(mean, var, cdf, lpd_marginal, lpd_joint, n_bad, n_particles, ess) straight from the definitions."""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    M = X.shape[0]
    lw = np.zeros(M) if lw is None else np.asarray(lw, dtype=np.float64)
    fin = np.isfinite(lw)
    mw = np.max(lw[fin])
    w = np.where(fin, np.exp(np.where(fin, lw - mw, 0.0)), 0.0)
    _, m, v, bad = laws(series, X, H)
    Tn = 0 if at is None else np.shape(at)[1]
    out = dict(mean=np.full(H, np.nan), var=np.full(H, np.nan), cdf=np.full((H, Tn), np.nan), n_bad=np.zeros(H),
               lpd_marginal=np.full(H, -np.inf), lpd_joint=np.full(H, -np.inf), n_particles=int(fin.sum()),
               ess=w.sum() ** 2 / (w * w).sum())
    if yf is not None:
        a, J = terms(series, X, yf)
    for h in range(H):
        ok = fin & ~bad[:, h]
        out["n_bad"][h] = np.sum(fin & bad[:, h])
        if yf is not None:
            for key, t in (("lpd_marginal", a[:, h]), ("lpd_joint", J[:, h])):
                use = ok & np.isfinite(t)
                if use.any():
                    tt = (lw - mw)[use] + t[use]
                    out[key][h] = tt.max() + math.log(np.exp(tt - tt.max()).sum()) - math.log(w.sum())
        if out["n_bad"][h] > 0 or not ok.any():
            continue
        W = w[ok].sum()
        mean = (w[ok] * m[ok, h]).sum() / W
        out["mean"][h] = mean
        out["var"][h] = (w[ok] * v[ok, h]).sum() / W + (w[ok] * (m[ok, h] - mean) ** 2).sum() / W
        for k in range(Tn):
            out["cdf"][h, k] = (w[ok] * _phi((at[h][k] - m[ok, h]) / np.sqrt(v[ok, h]))).sum() / W
    return out


# ---- 50 digits ------------------------------------------------------------------------------------------------------------
def _mpf_rows(X):
    return [[mp.mpf(float(v)) for v in row] for row in np.atleast_2d(np.asarray(X, dtype=np.float64))]


def laws_mp(series, X, H, yf=None):
    """Per point (finite coordinates, sigma representable): dict(err, m [H], v [H], a [H], J [H]) of mpf values."""
    out = []
    with mp.workdps(50):
        y = [mp.mpf(float(t)) for t in series]
        f = None if yf is None else [mp.mpf(float(t)) for t in yf]
        for mu, beta, theta, s in _mpf_rows(X):
            err = y[0] - mu - beta * mu
            for t in range(1, len(y)):
                err = y[t] - mu - beta * y[t - 1] - theta * err
            sigma = mp.exp(s)
            m, v, a, J = [], [], [], []
            mh, psi, cum = mu + beta * y[-1] + theta * err, mp.mpf(1), mp.mpf(1)
            e, yp, jc = err, y[-1], mp.mpf(0)
            for h in range(H):
                if h > 0:
                    mh = mu + beta * mh
                    psi = beta + theta if h == 1 else beta * psi
                    cum += psi * psi
                vh = sigma * sigma * cum
                m.append(mh)
                v.append(vh)
                if f is not None:
                    a.append(-(mp.log(2 * mp.pi) + mp.log(vh)) / 2 - (f[h] - mh) ** 2 / vh / 2)
                    e = f[h] - mu - beta * yp - theta * e
                    yp = f[h]
                    jc += -mp.log(2 * mp.pi) / 2 - s - (e / sigma) ** 2 / 2
                    J.append(jc)
            out.append(dict(err=err, m=m, v=v, a=a, J=J))
    return out


def points_mp(series, X, H, yf=None):
    """laws_mp rounded to fp64: (err_T [M], m, v [M, H], a, J [M, H] or None)."""
    L = laws_mp(series, X, H, yf)
    f = lambda key: np.array([[float(t) for t in r[key]] for r in L], dtype=np.float64).reshape(len(L), -1)
    err = np.array([float(r["err"]) for r in L])
    return err, f("m"), f("v"), (f("a") if yf is not None else None), (f("J") if yf is not None else None)


def mixture_mp(series, X, lw, H, yf=None, at=None):
    """mixture() at 50 digits, over the particles with a finite lw (none of them bad)."""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    lw = np.zeros(X.shape[0]) if lw is None else np.asarray(lw, dtype=np.float64)
    keep = np.nonzero(np.isfinite(lw))[0]
    L = laws_mp(series, X[keep], H, yf)
    Tn = 0 if at is None else np.shape(at)[1]
    out = dict(mean=np.empty(H), var=np.empty(H), cdf=np.empty((H, Tn)), lpd_marginal=np.empty(H), lpd_joint=np.empty(H))
    with mp.workdps(50):
        lwm = [mp.mpf(float(lw[i])) for i in keep]
        mw = max(lwm)
        w = [mp.exp(t - mw) for t in lwm]
        W = mp.fsum(w)
        for h in range(H):
            mean = mp.fsum(wi * r["m"][h] for wi, r in zip(w, L)) / W
            var = mp.fsum(wi * (r["v"][h] + (r["m"][h] - mean) ** 2) for wi, r in zip(w, L)) / W
            out["mean"][h], out["var"][h] = float(mean), float(var)
            for k in range(Tn):
                t = mp.mpf(float(at[h][k]))
                out["cdf"][h, k] = float(mp.fsum(wi * mp.ncdf((t - r["m"][h]) / mp.sqrt(r["v"][h])) for wi, r in zip(w, L)) / W)
            if yf is not None:
                out["lpd_marginal"][h] = float(mp.log(mp.fsum(wi * mp.exp(r["a"][h]) for wi, r in zip(w, L)) / W))
                out["lpd_joint"][h] = float(mp.log(mp.fsum(wi * mp.exp(r["J"][h]) for wi, r in zip(w, L)) / W))
    return out


# ---- err_T, every fma rounded once ----------------------------------------------------------------------------------------
def err_T_exact(series, X):
    fma = _arma_recur.fma
    y = [float(t) for t in series]
    out = []
    for mu, beta, theta, _ in np.atleast_2d(np.asarray(X, dtype=np.float64)):
        mu, beta, theta = float(mu), float(beta), float(theta)
        with np.errstate(all="ignore"):
            err = fma(-beta, mu, float(np.float64(y[0]) - np.float64(mu)))
            for t in range(1, len(y)):
                err = fma(-theta, err, fma(-beta, y[t - 1], float(np.float64(y[t]) - np.float64(mu))))
        out.append(err)
    return np.array(out, dtype=np.float64)


# ---- paths ----------------------------------------------------------------------------------------------------------------
def ancestors(logw, M, S, seed):
    """Systematic ancestors of S slots, the offset on stream 20 -> (a [S], amb [S]: the comparison is within rounding)."""
    lw = np.zeros(M) if logw is None else np.asarray(logw, dtype=np.float64)
    fin = np.isfinite(lw)
    with np.errstate(all="ignore"):
        w = np.where(fin, np.exp(np.where(fin, lw - np.max(lw[fin]), 0.0)), 0.0)
    C = np.cumsum(w / np.sum(w))
    pos = (np.arange(S) + float(philox_uniform(seed, 0, 0, ST_ANC, 0))) / S
    a = np.searchsorted(C, pos, side="right")
    last = int(np.nonzero(fin)[0][-1])
    near = np.minimum(np.abs(C[np.minimum(a, M - 1)] - pos), np.abs(C[np.maximum(a - 1, 0)] - pos))
    return np.minimum(a, last).astype(np.int64), near <= (M + 20) * U


def paths(series, X, anc, seed, H, s_first=0):
    """(y [n, H], bound [n, H]) for the slots s_first .. from the particles anc [n].  bound: on |device - this| from
    operation counts, u = 2^-53: sigma = e^s (|s| + 4) u relative; z to 128 u rad (tests/_predict_draws.py); m_1 to
    8 u (|mu| + |beta y_T| + |theta| (|err_T| + amplified chain rounding)); each step adds its terms' magnitudes times
    8 u and carries |beta| times the bound so far."""
    y = np.asarray(series, dtype=np.float64)
    xa = np.atleast_2d(np.asarray(X, dtype=np.float64))[np.asarray(anc)]
    n = xa.shape[0]
    mu, beta, theta, s = xa.T
    err, _ = err_chain(y, xa)
    s_idx = (s_first + np.arange(n))[:, None]
    h_idx = np.arange(1, H + 1)[None, :]
    z, rad = box_muller(philox_uniform(seed, s_idx, h_idx, ST_NOISE, 0), philox_uniform(seed, s_idx, h_idx, ST_NOISE, 1))
    with np.errstate(all="ignore"):
        sigma = np.exp(s)
        e = sigma[:, None] * z
        be = sigma[:, None] * (128 * U * rad + np.abs(z) * (np.abs(s)[:, None] + 8) * U)
        # the chain's rounding: each step adds ~4 u of its terms and carries |theta| times what it had
        amp = 1.0 / np.maximum(1.0 - np.abs(theta), 1e-3)
        berr = 8 * U * amp * (np.abs(y).max() * (1 + np.abs(beta)) + np.abs(mu) + np.abs(err))
        out = np.empty((n, H))
        bound = np.empty((n, H))
        yv = mu + beta * y[-1] + theta * err
        b = 8 * U * (np.abs(mu) + np.abs(beta * y[-1]) + np.abs(theta * err)) + np.abs(theta) * berr
        for h in range(H):
            if h > 0:
                base = mu + beta * yv + theta * e[:, h - 1]
                b = np.abs(beta) * b + np.abs(theta) * be[:, h - 1] + \
                    8 * U * (np.abs(mu) + np.abs(beta * yv) + np.abs(theta * e[:, h - 1]))
                yv = base
            yv = yv + e[:, h]
            b = b + be[:, h] + 4 * U * np.abs(yv)
            out[:, h], bound[:, h] = yv, b
        dead = np.cumsum(~np.isfinite(out), axis=1) > 0
        out[dead] = np.nan
    return out, bound


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def shipped_series():
    from smcnuts_amd import ArmaModel
    return np.array(ArmaModel().model_data[1:], dtype=np.float64)


def synthetic_series(T, seed=0):
    """A short ARMA(1,1) series (mu 0.4, beta 0.5, theta -0.3, sigma 0.7)."""
    rng = np.random.default_rng(1000 + seed)
    e = 0.7 * rng.standard_normal(T)
    y = np.empty(T)
    y[0] = 0.4 + 0.5 * 0.4 + e[0]
    for t in range(1, T):
        y[t] = 0.4 + 0.5 * y[t - 1] - 0.3 * e[t - 1] + e[t]
    return y


def value_particles(M, seed=0):
    """Particles for value comparisons: |theta| <= 0.95, beta in [-1.3, 1.3] (|beta| > 1 included), s ~ N(-0.5, 0.4),
    mu ~ N(0.3, 0.3)."""
    rng = np.random.default_rng(seed)
    X = np.stack([0.3 + 0.3 * rng.standard_normal(M), rng.uniform(-1.3, 1.3, M), rng.uniform(-0.95, 0.95, M),
                  -0.5 + 0.4 * rng.standard_normal(M)], axis=1)
    if M >= 4:
        X[1, 1], X[2, 1], X[3, 2] = 1.3, -1.25, 0.95
    return X


def odd_particles():
    """Particles for classification and the bit-for-bit err_T only: |theta| > 1, s = 400 (sigma^2 overflows), s = -400
    (sigma^2 underflows to 0), NaN and inf coordinates."""
    return np.array([[0.2, 0.5, 1.3, -0.4], [0.1, -0.7, -1.6, 0.1], [0.3, 0.4, 0.2, 400.0], [0.3, 0.4, 0.2, -400.0],
                     [np.nan, 0.4, 0.2, -0.5], [0.3, np.inf, 0.2, -0.5], [0.3, 0.4, -np.inf, -0.5], [0.3, 0.4, 0.2, np.nan]])


# ---- magnitudes the tolerances are relative to (each >= |value| elementwise) and the rule --------------------------------
def scales(series, X, H, yf=None):
    """dict(err, m, v, a, J): the sums of the magnitudes of the addends each value is made of."""
    y = np.asarray(series, dtype=np.float64)
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    mu, beta, theta, s = X.T
    err, m, v, _ = laws(y, X, H)
    with np.errstate(all="ignore"):
        amp = 1.0 / np.maximum(1.0 - np.abs(theta), 0.05)
        s_err = amp * (np.abs(y).max() * (1.0 + np.abs(beta)) + np.abs(mu)) + np.abs(err)
        m1 = np.abs(mu) + np.abs(beta * y[-1]) + np.abs(theta) * s_err
        s_m = np.maximum(np.maximum.accumulate(np.abs(m), axis=1), m1[:, None])
        for h in range(1, H):       # m_h inherits |beta| times the magnitude behind m_{h-1}
            s_m[:, h] = np.maximum(s_m[:, h], np.abs(mu) + np.abs(beta) * s_m[:, h - 1])
        out = dict(err=s_err, m=s_m, v=np.abs(v))
        if yf is not None:
            yf = np.asarray(yf, dtype=np.float64)
            _, e = err_chain(y, X, yf)
            d = (np.abs(yf) + s_m) ** 2 / v
            out["a"] = 0.5 * LOG2PI + 0.5 * np.abs(np.log(v)) + 0.5 * d
            s_e = amp[:, None] * (np.abs(np.concatenate([[y[-1]], yf])).max() * (1.0 + np.abs(beta)) + np.abs(mu))[:, None] \
                + np.abs(theta)[:, None] * s_err[:, None] + np.abs(e)
            out["J"] = np.cumsum(np.abs(-0.5 * LOG2PI - s)[:, None] + 0.5 * (s_e / np.exp(s)[:, None]) ** 2, axis=1)
    return out


FLOOR = 1e-14


def share(a, b, scale):
    """max |a - b| / scale over the elements where both are finite."""
    a, b, scale = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), scale)
    ok = np.isfinite(a) & np.isfinite(b)
    return float(np.max(np.abs(a - b)[ok] / scale[ok], initial=0.0))


def tolerance(ref64, refmp, scale):
    """The project's rule: 10 x the error of the fp64 restatement against 50 digits on the test's
    own inputs, as a share of the magnitude `scale`, with a floor of 1e-14."""
    return max(10.0 * share(ref64, refmp, scale), FLOOR)


def mixture_scales(series, X, lw, H, yf=None, at=None):
    """dict(mean, var, cdf, lpd_marginal, lpd_joint): the magnitudes behind the mixture's values, over the particles with
    a finite lw (none bad).  mean: the weighted mean of m's magnitude.  var: itself plus what m's own error moves the
    between-particle part by, 2 sd_between times m's magnitude.  cdf: 1 plus pdf(z) <= 0.4 times the magnitude of z's
    numerator over sqrt(v).  lpd: 1 plus the terms' magnitudes weighted by the particles' shares of the sum."""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    lw = np.zeros(X.shape[0]) if lw is None else np.asarray(lw, dtype=np.float64)
    fin = np.isfinite(lw)
    X, lw = X[fin], lw[fin]
    w = np.exp(lw - lw.max())[:, None]
    W = w.sum()
    sc = scales(series, X, H, yf)
    _, m, v, _ = laws(series, X, H)
    mean = (w * m).sum(0) / W
    between = (w * (m - mean) ** 2).sum(0) / W
    s_mean = (w * sc["m"]).sum(0) / W
    out = dict(mean=s_mean, var=(w * v).sum(0) / W + between + 2.0 * np.sqrt(between) * s_mean)
    Tn = 0 if at is None else np.shape(at)[1]
    at = np.zeros((H, 0)) if at is None else np.asarray(at, dtype=np.float64)
    out["cdf"] = np.stack([1.0 + 0.4 * (w * (np.abs(at[:, k]) + sc["m"]) / np.sqrt(v)).sum(0) / W for k in range(Tn)],
                          axis=1) if Tn else np.zeros((H, 0))
    if yf is not None:
        a, J = terms(series, X, yf)
        for key, t, s in (("lpd_marginal", a, sc["a"]), ("lpd_joint", J, sc["J"])):
            r = np.log(w) + t
            r = np.exp(r - r.max(0))
            out[key] = 1.0 + (r * s).sum(0) / r.sum(0)
    return out
