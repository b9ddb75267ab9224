"""References for the calibration checks (smcn_calibration_*, smcnuts_amd/calibration.py).

* `tails64`: an fp64 NumPy restatement of the device's tail algorithms (smcn_glm_family.hpp: glm_tails), the iteration
  bound and the unconverged flag included.  The prefactor is exp(term) with the term restated as the density forms it
  (the dispersion family's Stirling branch for phi >= 10, lgamma differences below).
* `tails_mp`: the same tails at 50 digits with mpmath from eta formed there: gammainc regularised, ncdf, and the
  regularised incomplete beta function from a continued fraction at 60 digits (mpmath's betainc gives up at b = 2e5).
* `mixture`: the finished values of calibration.Calibration from a matrix of tails and of terms, in fp64 or (exact=True)
  summed with mpmath.
* `case`: the inputs of the GPU tests.  Particle p carries the intercept log mu_g of a grid of means, row i is designed
  for one mean of the grid and one kind (y = 0, y = 1, the mode, 3 sd below, 3 sd above, 10 mu + 3), so every family meets
  every kind at every mean on the pairs whose grid index agrees, and far tails of every size on the others.
* `tolerance`, `share`: the project's rule: 10 x the restatement's error against 50 digits on the
  same inputs, floor 1e-14.  A tail is compared as a relative error of itself (both are sums of non-negative terms).
  Below TINY = 1e-290 a double has lost relative accuracy (denormals), so there the comparison is "both below TINY".
"""
import functools
import math

import numpy as np

FAMILIES = ("bernoulli_logit", "poisson_log", "normal", "neg_binomial_2_log")
MAXIT = 2048
FLOOR = 1e-14
TINY = 1e-290
KINDS = 6
MEANS = np.array([1e-3, 0.3, 1.0, 7.5, 100.0, 2500.0, 2e4])
PHIS = np.array([0.05, 0.5, 1.0, 8.0, 30.0, 1e3, 1e6])
MEANS_MOD = np.array([0.05, 0.3, 1.0, 3.0, 7.5, 30.0, 100.0])      # (moderate=True: the mixtures' cases, 5 kinds)
PHIS_MOD = np.array([0.3, 0.5, 1.0, 3.0, 8.0, 30.0, 300.0])
_lgamma = np.vectorize(math.lgamma, otypes=[np.float64])
_erfc = np.vectorize(math.erfc, otypes=[np.float64])


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def _design_y(fam, kind, mu, phi):
    """The response of `kind` for a count family with mean mu (and dispersion phi)."""
    var = mu if fam == 1 else mu + mu * mu / phi
    mode = math.floor(mu) if fam == 1 else max(0.0, math.floor(mu * (1.0 - 1.0 / phi) if phi > 1.0 else 0.0))
    sd = math.sqrt(var)
    return [0.0, 1.0, float(mode), float(max(0.0, math.floor(mu - 3.0 * sd))), float(math.ceil(mu + 3.0 * sd)),
            float(math.floor(10.0 * mu + 3.0))][kind]


@functools.lru_cache(maxsize=None)
def case(family, n, M, Dc, offset=False, seed=0, bad_particle=True, moderate=False):
    """dict(X [n][Dc - 1], y [n], offset [n] or None, x [M'][D], finite [M'] (rows of x without a non-finite coordinate),
    family): intercept + Dc - 1 columns.  Row i belongs to mean g = i % G and kind i % KINDS, particle p to mean
    p % G and dispersion (p // G) % G.  With bad_particle, a particle with a NaN coordinate sits in the middle of x."""
    fam = FAMILIES.index(family)
    rng = np.random.default_rng(1000 * seed + 7 * n + 13 * M + Dc + fam)
    G = len(MEANS)
    means, phis, kinds = (MEANS_MOD, PHIS_MOD, KINDS - 1) if moderate else (MEANS, PHIS, KINDS)
    p = Dc - 1
    X = rng.uniform(-1.0, 1.0, size=(n, p))
    off = rng.uniform(-0.2, 0.2, size=n) if offset else None
    D = Dc + (1 if fam >= 2 else 0)
    x = np.zeros((M, D))
    x[:, 1:Dc] = rng.normal(0.0, 0.02 / max(1, p) ** 0.5, size=(M, p))
    gp, gd = np.arange(M) % G, (np.arange(M) // G) % G
    y = np.zeros(n)
    gi, ki = np.arange(n) % G, np.arange(n) % kinds          # (G and kinds are coprime: G x kinds rows meet every combination)
    if fam == 0:
        x[:, 0] = np.array([-40.0, -3.0, -0.5, 0.0, 0.7, 5.0, 38.0])[gp]
        y = (ki % 2).astype(np.float64)
    elif fam == 2:
        x[:, 0] = np.array([-3.0, -1.0, -0.2, 0.0, 0.1, 1.5, 4.0])[gp]
        x[:, Dc] = np.log(np.array([0.15, 0.5, 1.0, 2.0, 5.0, 0.3, 1.0]))[gd]
        y = np.array([-1.5, -0.5, 0.0, 0.2, 0.5, 1.0])[ki] + 0.1 * gi      # |z| up to (4.4 + 1.6) / 0.15 = 30 and a little more
    else:
        x[:, 0] = np.log(means)[gp]
        phi_row = phis[(gi + ki) % G]
        if fam == 3:
            x[:, Dc] = np.log(phis)[gd]
        y = np.array([_design_y(fam, int(k), float(means[g]), float(ph)) for g, k, ph in zip(gi, ki, phi_row)])
    fin = np.ones(M, dtype=bool)
    if bad_particle and M >= 3:
        x[M // 2, 0] = np.nan
        fin[M // 2] = False
    return dict(family=family, fam=fam, X=X, y=y, offset=off, x=x, finite=fin, Dc=Dc)


def target(c, **kw):
    from smcnuts_amd import GLMTarget
    disp = dict(dispersion_prior=(0.0, 2.0)) if c["fam"] >= 2 else {}
    return GLMTarget(c["X"], c["y"], family=c["family"], prior_sd=2.5, intercept=True, offset=c["offset"], **disp, **kw)


# ---- the fp64 restatement ----------------------------------------------------------------------------------------------------
def eta64(c, x=None):
    x = c["x"] if x is None else np.atleast_2d(x)
    Dc = c["Dc"]
    eta = x[:, :1] + x[:, 1:Dc] @ c["X"].T
    return eta + c["offset"][None, :] if c["offset"] is not None else eta


def _stirling_tail(ix):
    t = ix * ix
    p = -3617.0 / 122400.0
    for k in (1.0 / 156.0, -691.0 / 360360.0, 1.0 / 1188.0, -1.0 / 1680.0, 1.0 / 1260.0, -1.0 / 360.0, 1.0 / 12.0):
        p = p * t + k
    return p * ix


def term64(fam, eta, y, tau=None):
    """log p(y | eta [, tau]) elementwise as the density forms it (broadcasting)."""
    eta, y = np.broadcast_arrays(np.asarray(eta, dtype=np.float64), np.asarray(y, dtype=np.float64))
    with np.errstate(all="ignore"):
        if fam == 0:
            return np.where(y != 0.0, np.minimum(eta, 0.0), -np.maximum(eta, 0.0)) - np.log1p(np.exp(-np.abs(eta)))
        if fam == 1:
            return (np.where(y == 0.0, 0.0, y * eta) - np.exp(eta)) - _lgamma(y + 1.0)
        tau = np.broadcast_to(np.asarray(tau, dtype=np.float64), eta.shape)
        if fam == 2:
            r = y - eta
            return -0.5 * (r * (r * np.exp(-2.0 * tau))) + (-tau - 0.5 * math.log(2.0 * math.pi))
        phi = np.exp(tau)
        x = y + phi
        z = eta - tau
        sp = np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z)))
        big = phi >= 10.0
        A_big = (x - 0.5) * np.log1p(y / phi) - y + (_stirling_tail(1.0 / x) - _stirling_tail(1.0 / phi))
        A_small = _lgamma(x) - _lgamma(phi)
        A = np.where(y == 0.0, 0.0, np.where(big, A_big, A_small))
        term = ((A - _lgamma(y + 1.0)) - x * sp) + y * (eta - np.where(big, 0.0, tau))
        return np.where(eta <= 709.782712893384, term, -np.inf)          # e^eta overflows


def _poisson_tails(y, mu, pmf):
    upper = y + 1.0 > mu
    with np.errstate(all="ignore"):
        imu = 1.0 / mu
    t, s = np.ones_like(y), np.zeros_like(y)
    live = np.ones(y.shape, dtype=bool)
    for k in range(1, MAXIT + 1):
        with np.errstate(all="ignore"):
            r = np.where(upper, mu / (y + k), (y - (k - 1.0)) * imu)
        t = np.where(live, t * r, t)
        s = np.where(live, s + t, s)
        live &= ~(t <= 1e-17 * s)
        if not live.any():
            break
    tail = pmf * s
    rest = np.maximum((1.0 - pmf) - tail, 0.0)
    return np.where(y == 0.0, 0.0, np.where(upper, rest, tail)), np.where(upper, tail, rest), ~live


def _beta_cf(a, b, x):
    tiny = 1e-300
    fix = lambda v: np.where(np.abs(v) < tiny, tiny, v)      # noqa: E731
    qab, qap, qam = a + b, a + 1.0, a - 1.0
    c = np.ones_like(a)
    d = 1.0 / fix(1.0 - qab * x / qap)
    h = d.copy()
    live = np.ones(a.shape, dtype=bool)
    for m in range(1, MAXIT + 1):
        m2 = 2.0 * m
        aa = m * (b - m) * x / ((qam + m2) * (a + m2))
        d1 = 1.0 / fix(1.0 + aa * d)
        c1 = fix(1.0 + aa / c)
        h1 = h * d1 * c1
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2))
        d2 = 1.0 / fix(1.0 + aa * d1)
        c2 = fix(1.0 + aa / c1)
        de = d2 * c2
        d, c, h = np.where(live, d2, d), np.where(live, c2, c), np.where(live, h1 * de, h)
        live &= ~(np.abs(de - 1.0) <= 4.5e-16)
        if not live.any():
            break
    return h, ~live


def _nb_tails(y, phi, z, pmf):
    t = np.exp(-np.abs(z))
    inv = 1.0 / (1.0 + t)
    q, pr = np.where(z >= 0.0, inv, t * inv), np.where(z >= 0.0, t * inv, inv)
    upper = q * (y + phi + 3.0) < y + 2.0
    h, conv = _beta_cf(np.where(upper, y + 1.0, phi), np.where(upper, phi, y), np.where(upper, q, pr))
    pre = np.where(upper, q * (y + phi) / (y + 1.0), y / phi)
    tail = pmf * pre * h
    rest = np.maximum((1.0 - pmf) - tail, 0.0)
    return np.where(y == 0.0, 0.0, np.where(upper, rest, tail)), np.where(upper, tail, rest), conv


def tails64(c, x=None):
    """(lo, up, term, converged), each [M][n]: the device's algorithm in NumPy.  lo, up NaN where the term is not finite or
    the pair is unconverged."""
    x = c["x"] if x is None else np.atleast_2d(np.asarray(x, dtype=np.float64))
    fam, Dc = c["fam"], c["Dc"]
    eta = eta64(c, x)
    y = np.broadcast_to(c["y"][None, :], eta.shape).copy()
    tau = x[:, Dc:Dc + 1] if fam >= 2 else None
    term = term64(fam, eta, y, tau)
    ok = np.isfinite(term)
    e = np.where(ok, eta, 0.0)
    with np.errstate(all="ignore"):
        conv = np.ones(eta.shape, dtype=bool)
        if fam == 0:
            t = np.exp(-np.abs(e))
            inv = 1.0 / (1.0 + t)
            lo = np.where(y != 0.0, np.where(e >= 0.0, t * inv, inv), 0.0)
            up = np.where(y != 0.0, 0.0, np.where(e >= 0.0, inv, t * inv))
        elif fam == 2:
            z = (y - e) * np.exp(-np.broadcast_to(tau, eta.shape)) * 0.70710678118654752440
            z = np.where(ok, z, 0.0)
            lo, up = 0.5 * _erfc(-z), 0.5 * _erfc(z)
        else:
            pmf = np.exp(np.where(ok, np.maximum(term, -800.0), 0.0))
            if fam == 1:
                lo, up, conv = _poisson_tails(y, np.exp(e), pmf)
            else:
                ta = np.where(ok, np.broadcast_to(tau, eta.shape), 0.0)
                lo, up, conv = _nb_tails(y, np.exp(ta), e - ta, pmf)
    good = ok & conv
    return np.where(good, lo, np.nan), np.where(good, up, np.nan), term, conv | ~ok


# ---- 50 digits -------------------------------------------------------------------------------------------------------------
def _mp():
    import mpmath
    mpmath.mp.dps = 60          # (50 digits asked of the results; ten to spare for the recurrences)
    return mpmath


def pair_mp(c, xrow, i):
    """(lo, up, pmf, log pmf -- `normal`: 0 and the log density) of particle `xrow` and row i as mpmath numbers."""
    mp = _mp()
    fam, Dc = c["fam"], c["Dc"]
    eta = mp.mpf(float(xrow[0]))
    for j in range(1, Dc):
        eta += mp.mpf(float(xrow[j])) * mp.mpf(float(c["X"][i, j - 1]))
    if c["offset"] is not None:
        eta += mp.mpf(float(c["offset"][i]))
    y = int(c["y"][i]) if fam != 2 else mp.mpf(float(c["y"][i]))
    if fam == 0:
        s1, s0 = 1 / (1 + mp.exp(-eta)), 1 / (1 + mp.exp(eta))
        return (s0, mp.mpf(0), s1, mp.log(s1)) if y else (mp.mpf(0), s1, s0, mp.log(s0))
    if fam == 2:
        tau = mp.mpf(float(xrow[Dc]))
        z = (y - eta) / mp.exp(tau)
        return mp.ncdf(z), mp.ncdf(-z), mp.mpf(0), -z * z / 2 - tau - mp.log(2 * mp.pi) / 2
    mu = mp.exp(eta)
    if fam == 1:
        lp = y * eta - mu - mp.loggamma(y + 1)
        lo = mp.gammainc(y, mu, mp.inf, regularized=True) if y >= 1 else mp.mpf(0)
        return lo, mp.gammainc(y + 1, 0, mu, regularized=True), mp.exp(lp), lp
    phi = mp.exp(mp.mpf(float(xrow[Dc])))
    pr, q = phi / (mu + phi), mu / (mu + phi)
    lp = mp.loggamma(y + phi) - mp.loggamma(phi) - mp.loggamma(y + 1) + phi * mp.log(pr) + y * mp.log(q)
    pmf = mp.exp(lp)
    # the tail on the convergent side of its continued fraction, the other as the complement at 60 digits: a tail too
    # small for that (< 1e-45) lies far from the mean on its own side, where its own fraction is the convergent one
    if q * (y + phi + 3) < y + 2:
        up = _betainc_mp(mp.mpf(y + 1), phi, q, pr)
        lo = 1 - pmf - up if y >= 1 else mp.mpf(0)
    else:
        lo = _betainc_mp(phi, mp.mpf(y), pr, q) if y >= 1 else mp.mpf(0)
        up = 1 - pmf - lo
    return lo, up, pmf, lp


def _betainc_mp(a, b, x, x1, maxit=6000):
    """I_x(a, b) at the working precision, x1 = 1 - x given: the continued fraction DLMF 8.17.22 by the modified Lentz
    recurrence run to 1e-58, for x < (a + 1) / (a + b + 2) where it converges in O(sqrt(max(a, b))) iterations (mpmath's own
    betainc gives up on a = 2e5, b = 0.05; tests/test_calibration.py compares the two where it does not)."""
    mp = _mp()
    tiny, eps = mp.mpf(10) ** -2000, mp.mpf(10) ** -58
    qab, qap, qam = a + b, a + 1, a - 1
    c, d = mp.mpf(1), 1 - qab * x / qap
    d = 1 / (d if d != 0 else tiny)
    h = d
    for m in range(1, maxit + 1):
        m2 = 2 * m
        for aa in (m * (b - m) * x / ((qam + m2) * (a + m2)), -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2))):
            d = 1 + aa * d
            d = 1 / (d if d != 0 else tiny)
            c = 1 + aa / c
            c = c if c != 0 else tiny
            de = d * c
            h *= de
        if abs(de - 1) < eps:
            pre = mp.exp(a * mp.log(x) + b * mp.log(x1) + mp.loggamma(a + b) - mp.loggamma(a + 1) - mp.loggamma(b))
            return pre * h
    raise ArithmeticError("_betainc_mp: no convergence")


def _f(v):
    """An mpmath number as the nearest double; below the doubles' range: 0."""
    return float(v) if abs(v) > 1e-320 else 0.0


@functools.lru_cache(maxsize=None)
def _tails_mp(key, pairs):
    c = case(*key)
    out = np.empty((len(pairs), 4))
    worst = 0.0
    for r, (p, i) in enumerate(pairs):
        lo, up, pmf, lp = pair_mp(c, c["x"][p], i)
        worst = max(worst, abs(float(lo + up + pmf - 1)))
        out[r] = _f(lo), _f(up), _f(pmf), float(lp)
    assert worst < 1e-40, f"the 50-digit tails do not add to 1: {worst}"
    return out


def tails_mp(key, pairs):
    """[(lo, up, pmf, log pmf)] at 50 digits, rounded to doubles, of the (particle, row) pairs of case(*key); cached.  Asserts that
    the three add to 1 within 1e-40, which checks the reference against itself."""
    return _tails_mp(tuple(key), tuple((int(p), int(i)) for p, i in pairs))


def sample_pairs(c, cap=400):
    """Pairs (particle, row) to compare at 50 digits: every pair if there are at most `cap`, else every designed pair
    (the particle's mean is the row's) up to half the cap and an even stride through the others.  Finite particles only."""
    M, n = c["x"].shape[0], c["y"].shape[0]
    G = len(MEANS)
    allp = [(p, i) for p in range(M) if c["finite"][p] for i in range(n)]
    if len(allp) <= cap:
        return allp
    des = [pi for pi in allp if pi[0] % G == pi[1] % G]
    des = des[::max(1, len(des) // (cap // 2))][:cap // 2]
    rest = [pi for pi in allp if pi[0] % G != pi[1] % G]
    rest = rest[::max(1, len(rest) // (cap - len(des)))][:cap - len(des)]
    return des + rest


# ---- comparison ------------------------------------------------------------------------------------------------------------
def share(got, want):
    """max |got - want| / want over the elements with want >= TINY (both finite); asserts got < 2 TINY where want < TINY."""
    got, want = np.broadcast_arrays(np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64))
    small = want < TINY
    assert np.all(got[small] < 2.0 * TINY), "a tail below the doubles' normal range is not small on the other side"
    ok = ~small & np.isfinite(got)
    return float(np.max(np.abs(got - want)[ok] / want[ok], initial=0.0))


def tolerance(ref64, refmp):
    return max(10.0 * share(ref64, refmp), FLOOR)


# ---- mixtures ----------------------------------------------------------------------------------------------------------------
def mixture(lo, up, term, lw, exact=False):
    """The finished values from tails and terms [M][n] and log-weights lw [M] (NaN-free rows only): dict(pit_lo, sf,
    pit_lo_loo, sf_loo); exact: sums in mpmath."""
    lw = np.asarray(lw, dtype=np.float64)
    fin = np.isfinite(lw)
    lo, up, term, lw = lo[fin], up[fin], term[fin], lw[fin]
    if exact:
        mp = _mp()
        out = {k: np.empty(lo.shape[1]) for k in ("pit_lo", "sf", "pit_lo_loo", "sf_loo")}
        w = [mp.exp(mp.mpf(float(v)) - mp.mpf(float(lw.max()))) for v in lw]
        for i in range(lo.shape[1]):
            r = [w[p] * mp.exp(-mp.mpf(float(term[p, i]))) for p in range(len(w))]
            L, U = [mp.mpf(float(v)) for v in lo[:, i]], [mp.mpf(float(v)) for v in up[:, i]]
            out["pit_lo"][i] = _f(mp.fsum(a * b for a, b in zip(w, L)) / mp.fsum(w))
            out["sf"][i] = _f(mp.fsum(a * b for a, b in zip(w, U)) / mp.fsum(w))
            out["pit_lo_loo"][i] = _f(mp.fsum(a * b for a, b in zip(r, L)) / mp.fsum(r))
            out["sf_loo"][i] = _f(mp.fsum(a * b for a, b in zip(r, U)) / mp.fsum(r))
        return out
    w = np.exp(lw - lw.max())[:, None]
    v = lw[:, None] - term
    r = np.exp(v - v.max(0))
    return dict(pit_lo=(w * lo).sum(0) / w.sum(), sf=(w * up).sum(0) / w.sum(),
                pit_lo_loo=(r * lo).sum(0) / r.sum(0), sf_loo=(r * up).sum(0) / r.sum(0))
