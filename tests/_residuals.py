"""Reference of the arma one-step residual checks (smcnuts_amd/residuals.py; include/smcnuts_hip.h, smcn_residuals_*): an
fp64 NumPy restatement of every definition, the same in mpmath at 50 digits, nu_t with every fma rounded once (exact),
the magnitudes the tolerances are relative to.

Per point x = (mu, beta, theta, s), sigma = exp(s), series y_1..y_T (y_0 := mu, err_0 := 0):
  err_1 = y_1 - mu - beta mu,  err_t = y_t - mu - beta y_{t-1} - theta err_{t-1}
  nu_t = y_t - err_t,  r_t = err_t / sigma,  l_t = -0.5 log 2 pi - s - 0.5 r_t^2,  PIT_t = Phi(r_t)
  bad at t: sigma not finite or not > 0, err_t or r_t not finite
  rho_k = sum_{t>k} r_t r_{t-k} / sum_t r_t^2,  Q = T (T + 2) sum_{k<=L} rho_k^2 / (T - k)
  bad for the lag rows: bad at any t, sum_t r_t^2 not finite or not > 0, Q not finite
Mixture over the particles with a finite lw that are not bad (at t; for the lag rows), w = exp(lw - mw): weighted means
and variances of nu_t (plus sum w sigma^2 / sum w), r_t, rho_k, Q; pit_t = sum w Phi(r_t) / sum w;
lpd_t = log sum w exp(l_t) - log sw (sw: over every finite lw); exceed_j = sum w [Q > q_at_j] / sum w.
"""
import math

import mpmath as mp
import numpy as np

import _arma_recur
from _forecast import FLOOR, LOG2PI, U, _phi, share, tolerance  # noqa: F401

QC = 20
ML, SL, NBAD, C0, SW, S1, S2, VAR, CZ, Z1, Z2, PIT, P0 = range(13)


def rows(T, L):
    return 1 + T + (L + 1 if L else 0)


# ---- fp64 ---------------------------------------------------------------------------------------------------------------
def chain(series, X):
    """err [M, T]."""
    y = np.asarray(series, dtype=np.float64)
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    mu, beta, theta = X[:, 0], X[:, 1], X[:, 2]
    out = np.empty((X.shape[0], len(y)))
    with np.errstate(all="ignore"):
        err = y[0] - mu - beta * mu
        out[:, 0] = err
        for t in range(1, len(y)):
            err = y[t] - mu - beta * y[t - 1] - theta * err
            out[:, t] = err
    return out


def points(series, X, L):
    """dict(nu [M, T], r [M, T], l [M, T], bad [M, T], rho [M, L], Q [M], A0 [M], pbad [M])."""
    y = np.asarray(series, dtype=np.float64)
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    T = len(y)
    err = chain(y, X)
    with np.errstate(all="ignore"):
        sigma = np.exp(X[:, 3])[:, None]
        r = err / sigma
        nu = y[None, :] - err
        l = (-0.5 * LOG2PI - X[:, 3])[:, None] - 0.5 * r * r
        bad = ~(np.isfinite(sigma) & (sigma > 0.0) & np.isfinite(err) & np.isfinite(r))
        A0 = (r * r).sum(1)
        rho = np.stack([(r[:, k:] * r[:, :T - k]).sum(1) / A0 for k in range(1, L + 1)], axis=1) if L else np.zeros((len(X), 0))
        Q = T * (T + 2.0) * (rho * rho / (T - np.arange(1, L + 1))[None, :]).sum(1)
        pbad = bad.any(1) | ~(np.isfinite(A0) & (A0 > 0.0)) | ~np.isfinite(Q)
    return dict(nu=nu, r=r, l=l, bad=bad, rho=rho, Q=Q, A0=A0, pbad=pbad, sigma=sigma[:, 0])


def nu_exact(series, X):
    """nu_t = y_t - err_t [M, T] of the device's chain, every fma rounded once."""
    fma = _arma_recur.fma
    y = [float(t) for t in series]
    out = []
    for mu, beta, theta, _ in np.atleast_2d(np.asarray(X, dtype=np.float64)):
        mu, beta, theta = float(mu), float(beta), float(theta)
        row = []
        with np.errstate(all="ignore"):
            err = fma(-beta, mu, float(np.float64(y[0]) - np.float64(mu)))
            row.append(float(np.float64(y[0]) - np.float64(err)))
            for t in range(1, len(y)):
                err = fma(-theta, err, fma(-beta, y[t - 1], float(np.float64(y[t]) - np.float64(mu))))
                row.append(float(np.float64(y[t]) - np.float64(err)))
        out.append(row)
    return np.array(out, dtype=np.float64)


def _weights(lw, M):
    lw = np.zeros(M) if lw is None else np.asarray(lw, dtype=np.float64)
    fin = np.isfinite(lw)
    if not fin.any():
        return lw, fin, -np.inf, np.zeros(M)
    mw = np.max(lw[fin])
    with np.errstate(all="ignore"):
        return lw, fin, mw, np.where(fin, np.exp(np.where(fin, lw - mw, 0.0)), 0.0)


def _moments_row(r, w, ok, v, c0, c1, c2):
    use = ok & (w > 0.0)
    if not use.any():
        return
    c = v[use][0]
    r[c0] = c
    with np.errstate(all="ignore"):
        r[c1], r[c2] = (w[ok] * (v[ok] - c)).sum(), (w[ok] * (v[ok] - c) ** 2).sum()


def partials(series, X, lw, L, q_at=None):
    """The mergeable partials [1 + T (+ L + 1)][20] of the whole set as ONE block (include/smcnuts_hip.h)."""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    M, T = X.shape[0], len(series)
    lw, fin, mw, w = _weights(lw, M)
    out = np.zeros((rows(T, L), QC))
    out[1:, ML], out[1:, C0], out[1:, CZ] = -np.inf, np.nan, np.nan
    if not fin.any():
        out[0, 0] = -np.inf
        return out
    out[0, :4] = mw, w.sum(), (w * w).sum(), fin.sum()
    p = points(series, X, L)
    with np.errstate(all="ignore"):
        for t in range(T):
            ok = fin & ~p["bad"][:, t]
            r = out[1 + t]
            r[NBAD] = np.sum(fin & p["bad"][:, t])
            tt = (lw - mw) + p["l"][:, t]
            use = ok & np.isfinite(tt)
            if use.any():
                r[ML] = tt[use].max()
                r[SL] = np.exp(tt[use] - r[ML]).sum()
            r[SW] = w[ok].sum()
            _moments_row(r, w, ok, p["nu"][:, t], C0, S1, S2)
            _moments_row(r, w, ok, p["r"][:, t], CZ, Z1, Z2)
            r[VAR] = (w[ok] * p["sigma"][ok] ** 2).sum()
            r[PIT] = (w[ok] * _phi(p["r"][ok, t])).sum()
        ok = fin & ~p["pbad"]
        for k in range(L + 1 if L else 0):
            r = out[1 + T + k]
            r[NBAD], r[SW] = np.sum(fin & p["pbad"]), w[ok].sum()
            _moments_row(r, w, ok, p["rho"][:, k] if k < L else p["Q"], C0, S1, S2)
        if L and q_at is not None:
            for j, q in enumerate(q_at):
                out[T + L + 1, P0 + j] = w[ok & (p["Q"] > q)].sum()
    return out


KEYS_T = ("mean", "var", "lpd", "z", "z_var", "pit")
KEYS_L = ("acf", "acf_var")


def _wstats(w, v):
    W = w.sum()
    m = (w * v).sum() / W
    return m, (w * (v - m) ** 2).sum() / W


def mixture(series, X, lw, L, q_at=None):
    """dict(mean, var, lpd, z, z_var, pit, n_bad [T]; acf, acf_var [L]; ljung_box, ljung_box_var; exceed [Tn], exceed_amb
    [Tn]: the weight share of particles whose Q lies within rounding of the threshold; n_bad_acf, n_particles, ess)
    straight from the definitions."""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    M, T = X.shape[0], len(series)
    lw, fin, mw, w = _weights(lw, M)
    p = points(series, X, L)
    Tn = 0 if q_at is None or not L else len(q_at)
    out = {k: np.full(T, np.nan) for k in KEYS_T}
    out.update({k: np.full(L, np.nan) for k in KEYS_L})
    out.update(lpd=np.full(T, -np.inf), n_bad=np.zeros(T), ljung_box=np.nan, ljung_box_var=np.nan, exceed=np.full(Tn, np.nan),
               exceed_amb=np.zeros(Tn), n_bad_acf=int(np.sum(fin & p["pbad"])), n_particles=int(fin.sum()),
               ess=w.sum() ** 2 / (w * w).sum() if fin.any() else 0.0)
    with np.errstate(all="ignore"):
        for t in range(T):
            ok = fin & ~p["bad"][:, t]
            out["n_bad"][t] = np.sum(fin & p["bad"][:, t])
            tt = (lw - mw) + p["l"][:, t]
            use = ok & np.isfinite(tt)
            if use.any():
                out["lpd"][t] = tt[use].max() + math.log(np.exp(tt[use] - tt[use].max()).sum()) - math.log(w.sum())
            if out["n_bad"][t] > 0 or not ok.any():
                continue
            out["mean"][t], between = _wstats(w[ok], p["nu"][ok, t])
            out["var"][t] = (w[ok] * p["sigma"][ok] ** 2).sum() / w[ok].sum() + between
            out["z"][t], out["z_var"][t] = _wstats(w[ok], p["r"][ok, t])
            out["pit"][t] = (w[ok] * _phi(p["r"][ok, t])).sum() / w[ok].sum()
        ok = fin & ~p["pbad"]
        if L and out["n_bad_acf"] == 0 and ok.any():
            for k in range(L):
                out["acf"][k], out["acf_var"][k] = _wstats(w[ok], p["rho"][ok, k])
            out["ljung_box"], out["ljung_box_var"] = _wstats(w[ok], p["Q"][ok])
            sq = scales(series, X, L)["Q"]
            for j in range(Tn):
                out["exceed"][j] = w[ok & (p["Q"] > q_at[j])].sum() / w[ok].sum()
                out["exceed_amb"][j] = w[ok & (np.abs(p["Q"] - q_at[j]) <= 1e-9 * sq)].sum() / w[ok].sum()
    return out


# ---- 50 digits ------------------------------------------------------------------------------------------------------------
def points_mp_raw(series, X, L):
    """Per point (finite coordinates): dict(nu [T], r [T], l [T], rho [L], Q, sigma) of mpf values."""
    out = []
    with mp.workdps(50):
        y = [mp.mpf(float(t)) for t in series]
        T = len(y)
        half_l2pi = mp.log(2 * mp.pi) / 2
        for row in np.atleast_2d(np.asarray(X, dtype=np.float64)):
            mu, beta, theta, s = (mp.mpf(float(v)) for v in row)
            sigma = mp.exp(s)
            err, es = None, []
            for t in range(T):
                err = y[0] - mu - beta * mu if t == 0 else y[t] - mu - beta * y[t - 1] - theta * err
                es.append(err)
            r = [e / sigma for e in es]
            A0 = mp.fsum(v * v for v in r)
            rho = [mp.fsum(r[t] * r[t - k] for t in range(k, T)) / A0 for k in range(1, L + 1)]
            Q = T * (T + 2) * mp.fsum(rho[k - 1] ** 2 / (T - k) for k in range(1, L + 1))
            out.append(dict(nu=[y[t] - es[t] for t in range(T)], r=r, l=[-half_l2pi - s - v * v / 2 for v in r], rho=rho, Q=Q,
                            sigma=sigma))
    return out


def _f(v):
    """An mpf as the nearest double (inf beyond the range)."""
    try:
        return float(v)
    except OverflowError:
        return math.copysign(math.inf, float(mp.sign(v)))


def _ncdf(v):
    """Phi at 50 digits; beyond |v| = 10^4 the tail is below e^(-5 10^7), 0 to any precision used here."""
    return mp.ncdf(v) if abs(v) < 10000 else mp.mpf(0 if v < 0 else 1)


def points_mp(series, X, L):
    """points_mp_raw rounded to fp64: dict(nu, r [M, T], rho [M, L], Q [M])."""
    P = points_mp_raw(series, X, L)
    g = lambda key: np.array([[_f(t) for t in r[key]] for r in P], dtype=np.float64).reshape(len(P), -1)    # noqa: E731
    with mp.workdps(50):
        llik = np.array([_f(mp.fsum(r["l"])) for r in P])
    return dict(nu=g("nu"), r=g("r"), l=g("l"), rho=g("rho"), Q=np.array([_f(r["Q"]) for r in P]), llik=llik)


def mixture_mp(series, X, lw, L, q_at=None):
    """mixture() at 50 digits, over the particles with a finite lw (every one of them taken as not bad)."""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    lw = np.zeros(X.shape[0]) if lw is None else np.asarray(lw, dtype=np.float64)
    keep = np.nonzero(np.isfinite(lw))[0]
    P = points_mp_raw(series, X[keep], L)
    T = len(series)
    Tn = 0 if q_at is None or not L else len(q_at)
    out = {k: np.empty(T) for k in KEYS_T}
    out.update({k: np.empty(L) for k in KEYS_L})
    out["exceed"] = np.empty(Tn)
    with mp.workdps(50):
        lwm = [mp.mpf(float(lw[i])) for i in keep]
        mw = max(lwm)
        w = [mp.exp(t - mw) for t in lwm]
        W = mp.fsum(w)

        def stats(vals):
            m = mp.fsum(wi * v for wi, v in zip(w, vals)) / W
            return m, mp.fsum(wi * (v - m) ** 2 for wi, v in zip(w, vals)) / W

        for t in range(T):
            m, b = stats([r["nu"][t] for r in P])
            out["mean"][t], out["var"][t] = _f(m), _f(mp.fsum(wi * r["sigma"] ** 2 for wi, r in zip(w, P)) / W + b)
            m, b = stats([r["r"][t] for r in P])
            out["z"][t], out["z_var"][t] = _f(m), _f(b)
            out["pit"][t] = _f(mp.fsum(wi * _ncdf(r["r"][t]) for wi, r in zip(w, P)) / W)
            tot = mp.fsum(wi * mp.exp(r["l"][t]) for wi, r in zip(w, P))
            out["lpd"][t] = _f(mp.log(tot / W)) if tot > 0 else -math.inf
        for k in range(L):
            m, b = stats([r["rho"][k] for r in P])
            out["acf"][k], out["acf_var"][k] = _f(m), _f(b)
        if L:
            m, b = stats([r["Q"] for r in P])
            out["ljung_box"], out["ljung_box_var"] = _f(m), _f(b)
            for j in range(Tn):
                out["exceed"][j] = _f(mp.fsum(wi for wi, r in zip(w, P) if r["Q"] > mp.mpf(float(q_at[j]))) / W)
    return out


# ---- magnitudes the tolerances are relative to (each >= |value| elementwise) ----------------------------------------------
def scales(series, X, L):
    """dict(nu, r, l [M, T], rho [M, L], Q [M]): the sums of the magnitudes of the addends each value is made of.  err_t:
    tests/_forecast.py's s_err with |err_t|.  rho_k = A_k / A_0 moves by dA_k / A_0 - rho_k dA_0 / A_0: (N_k + |rho_k| D) /
    A_0 with N_k, D the lag sums of r's magnitudes.  Q moves by T (T + 2) sum 2 |rho_k| d rho_k / (T - k), plus itself."""
    y = np.asarray(series, dtype=np.float64)
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    T = len(y)
    mu, beta, theta, s = X.T
    p = points(y, X, L)
    err = y[None, :] - p["nu"]
    with np.errstate(all="ignore"):
        amp = 1.0 / np.maximum(1.0 - np.abs(theta), 0.05)
        s_err = (amp * (np.abs(y).max() * (1.0 + np.abs(beta)) + np.abs(mu)))[:, None] + np.abs(err)
        s_r = s_err / p["sigma"][:, None]
        out = dict(nu=np.abs(y)[None, :] + s_err, r=s_r, l=np.abs(-0.5 * LOG2PI - s)[:, None] + 0.5 * s_r * s_r)
        D = (s_r * s_r).sum(1)
        N = np.stack([(s_r[:, k:] * s_r[:, :T - k]).sum(1) for k in range(1, L + 1)], axis=1) if L else np.zeros((len(X), 0))
        out["rho"] = (N + np.abs(p["rho"]) * D[:, None]) / p["A0"][:, None]
        out["Q"] = np.abs(p["Q"]) + T * (T + 2.0) * (2.0 * np.abs(p["rho"]) * out["rho"] / (T - np.arange(1, L + 1))[None, :]).sum(1)
    return out


def mixture_scales(series, X, lw, L, q_at=None):
    """The magnitudes behind mixture()'s values, over the particles with a finite lw (none bad).  Means: the weighted mean
    of the values' magnitudes.  Variances: themselves plus what the values' own errors move them by, 2 sd times the mean's
    magnitude.  pit: 1 plus pdf <= 0.4 times r's magnitude.  lpd: 1 plus the terms' magnitudes weighted by the particles'
    shares of the sum.  exceed: 1."""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    lw = np.zeros(X.shape[0]) if lw is None else np.asarray(lw, dtype=np.float64)
    fin = np.isfinite(lw)
    X, lw = X[fin], lw[fin]
    w = np.exp(lw - lw.max())[:, None]
    W = w.sum()
    sc, p = scales(series, X, L), points(series, X, L)
    wm = lambda a: (w * a).sum(0) / W                                           # noqa: E731
    with np.errstate(all="ignore"):
        var = lambda v, s: wm((v - wm(v)) ** 2) + 2.0 * np.sqrt(wm((v - wm(v)) ** 2)) * wm(s)     # noqa: E731
        out = dict(mean=wm(sc["nu"]), var=wm(p["sigma"][:, None] ** 2 * np.ones_like(p["nu"])) + var(p["nu"], sc["nu"]),
                   z=wm(sc["r"]), z_var=var(p["r"], sc["r"]), pit=1.0 + 0.4 * wm(sc["r"]))
        rr = np.log(w) + p["l"]
        rr = np.exp(rr - rr.max(0))
        out["lpd"] = 1.0 + np.where(rr > 0.0, rr * sc["l"], 0.0).sum(0) / rr.sum(0)
        if L:
            out.update(acf=wm(sc["rho"]), acf_var=var(p["rho"], sc["rho"]), ljung_box=float(wm(sc["Q"][:, None])[0]),
                       ljung_box_var=float(var(p["Q"][:, None], sc["Q"][:, None])[0]))
        out["exceed"] = 1.0
    return out


def mixture_stream(series, X, lw, L, q_at=None, at_rows=None):
    """(mixture(), mixture_scales()) of a set without bad particles in O(M L) memory, for series too long to hold [M, T]
    arrays of: one pass over t.  at_rows: the time rows (0-based) to evaluate, the others stay NaN (None: all)."""
    y = np.asarray(series, dtype=np.float64)
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    lw = np.zeros(X.shape[0]) if lw is None else np.asarray(lw, dtype=np.float64)
    fin = np.isfinite(lw)
    X, lwf = X[fin], lw[fin]
    T = len(y)
    mu, beta, theta, s = X.T
    w = np.exp(lwf - lwf.max())
    W = w.sum()
    sigma = np.exp(s)
    amp = 1.0 / np.maximum(1.0 - np.abs(theta), 0.05)
    base = amp * (np.abs(y).max() * (1.0 + np.abs(beta)) + np.abs(mu))
    lc, s_lc = -0.5 * LOG2PI - s, np.abs(-0.5 * LOG2PI - s)
    want = np.zeros(T, dtype=bool)
    want[np.arange(T) if at_rows is None else np.asarray(at_rows)] = True
    val = {k: np.full(T, np.nan) for k in KEYS_T}
    sc = {k: np.full(T, np.nan) for k in KEYS_T}
    wm = lambda a: float((w * a).sum() / W)                                     # noqa: E731

    def var(v, sv):
        m = wm(v)
        b = wm((v - m) ** 2)
        return m, b, b + 2.0 * math.sqrt(b) * wm(sv)

    A, N = np.zeros((L + 1, len(w))), np.zeros((L + 1, len(w)))
    past, s_past = [], []
    err = None
    for t in range(T):
        err = y[0] - mu - beta * mu if t == 0 else y[t] - mu - beta * y[t - 1] - theta * err
        r = err / sigma
        s_r = (base + np.abs(err)) / sigma
        assert np.all(np.isfinite(r))
        A[0] += r * r
        N[0] += s_r * s_r
        for k in range(1, min(L, t) + 1):
            A[k] += r * past[-k]
            N[k] += s_r * s_past[-k]
        past, s_past = (past + [r])[-L:] if L else [], (s_past + [s_r])[-L:] if L else []
        if not want[t]:
            continue
        nu, s_nu = y[t] - err, abs(y[t]) + base + np.abs(err)
        val["mean"][t], b, sb = var(nu, s_nu)
        val["var"][t], sc["mean"][t], sc["var"][t] = wm(sigma * sigma) + b, wm(s_nu), wm(sigma * sigma) + sb
        val["z"][t], val["z_var"][t], sc["z_var"][t] = var(r, s_r)
        sc["z"][t], sc["pit"][t] = wm(s_r), 1.0 + 0.4 * wm(s_r)
        val["pit"][t] = wm(_phi(r))
        tt = (lwf - lwf.max()) + (lc - 0.5 * r * r)
        e = np.exp(tt - tt.max())
        val["lpd"][t] = tt.max() + math.log(e.sum()) - math.log(W)
        sc["lpd"][t] = 1.0 + float((e * (s_lc + 0.5 * s_r * s_r)).sum() / e.sum())
    val.update(n_bad=np.zeros(T), n_bad_acf=0, n_particles=int(fin.sum()), ess=W * W / float((w * w).sum()))
    if L:
        rho = A[1:] / A[0]
        s_rho = (N[1:] + np.abs(rho) * N[0]) / A[0]
        den = (T - np.arange(1, L + 1))[:, None]
        Q = T * (T + 2.0) * (rho * rho / den).sum(0)
        s_Q = np.abs(Q) + T * (T + 2.0) * (2.0 * np.abs(rho) * s_rho / den).sum(0)
        st = [var(rho[k], s_rho[k]) for k in range(L)]
        val.update(acf=np.array([v[0] for v in st]), acf_var=np.array([v[1] for v in st]))
        sc.update(acf=np.array([wm(s_rho[k]) for k in range(L)]), acf_var=np.array([v[2] for v in st]))
        val["ljung_box"], val["ljung_box_var"], sc["ljung_box_var"] = var(Q, s_Q)
        sc["ljung_box"] = wm(s_Q)
        q_at = [] if q_at is None else q_at
        val["Q"] = Q
        val["exceed"] = np.array([wm(Q > q) for q in q_at])
        val["exceed_amb"] = np.array([wm(np.abs(Q - q) <= 1e-9 * s_Q) for q in q_at])
    return val, sc


def of(res):
    """A smcnuts_amd.residuals.OneStepResiduals as mixture()'s dictionary."""
    out = dict(mean=res.mean, var=res.var, lpd=res.lpd, z=res.z, z_var=res.z_sd ** 2, pit=res.pit, n_bad=res.n_bad,
               n_particles=res.n_particles, ess=res.ess)
    if res.lags:
        out.update(acf=res.acf, acf_var=res.acf_sd ** 2, ljung_box=res.ljung_box, ljung_box_var=res.ljung_box_sd ** 2,
                   exceed=np.asarray(res.exceed), n_bad_acf=res.n_bad_acf)
    return out


def seasonal_series(T=200, seed=0):
    """y_t = 0.8 y_{t-4} + e_t: a lag-4 seasonal series ARMA(1,1) cannot describe."""
    rng = np.random.default_rng(2000 + seed)
    e = rng.standard_normal(T + 4)
    y = np.zeros(T + 4)
    for t in range(4, T + 4):
        y[t] = 0.8 * y[t - 4] + e[t]
    return y[4:]
