"""NumPy restatement of the posterior predictive draws (smcnuts_amd.predict.predict_draws; smcn_predict_draws) and the
rounding bounds that say where the restatement's own comparisons are AMBIGUOUS.

Everything is keyed as include/smcnuts_hip.h says: philox_uniform(seed, iter = s, particle = i, stream, q) with streams
16 (ancestor offset), 17 (outcome), 18 (gamma), 19 (new-group intercept, particle = label).  `philox_uniform` is a
vectorised Philox4x32-10 (tests/test_predict_draws_host.py pins it to oracle.philox_uniforms).

Every sampler returns the outcome and a mask `amb`: True where some comparison the sampler made -- u against a CDF step,
a floor argument against an integer, an accept test against its threshold, a branch on mu -- has its two sides closer
than the bound on |device - numpy| of their difference.  There the device may legitimately take the other branch and
the draw is left out of an equality check.  Bounds, u = 2^-53, from operation counts (library functions: 4 u relative):
  inputs     e_mean, e_eta, e_prob, e_c: tests/_predict.py's pair bounds.  phi, sigma = e^tau: (|tau| + 4) u relative.
  Bernoulli  |u - p| <= e_p.
  categor.   F_k = P_0 + .. + P_k: sum_{l<=k} e_P_l + (k + 2) u F_k.
  ordinal    lat = eta + (log u - log1p(-u)): e_eta + 4 u (|log u| + |log1p(-u)|) + 2 u |lat|, against c_k with e_c_k.
  normal     z = rad cos(2 pi u2), rad = sqrt(-2 log1p(-u1)): |dz| <= 128 u rad (8 u relative on rad, the reduced angle to
             2 pi u 2^-53 absolute, and slack); y = eta + sigma z: e_eta + sigma (e_z + |z| (e_sigma + 4 u)) + 2 u |y|.
  Poisson    inversion, step k: F_k carries (2 k + 10) u F_k + e_mu (|dF/dmu| = pmf <= 1).  The branch at mu = 10 and the
             limit 2^53: |mu - 10|, |mu - 2^53| <= e_mu (an exact mu, e_mu = 0, takes the same branch on both sides).  PTRS: b, a, vr, log ialpha are smooth in sqrt(mu): r = 8 u +
             e_mu / mu relative.  Floor argument A = (2a / w + b) U + mu + 0.43 (U, w exact): 16 u (|(2a / w + b) U| + mu
             + 1) + 2 e_mu + 4 r |(2a / w + b) U|, against the nearest integer.  V <= vr: 16 u + 4 r.  The last test,
             log V + log ialpha - log(a / w^2 + b) <= -mu + k log mu - lgamma(k + 1): 16 u times the sum of the addends'
             magnitudes, + e_mu (|k / mu - 1|) + 8 r.
  gamma      d = a' - 1/3 (a' >= 1: relative e_d = 1.5 e_phi + 2 u), c = 1 / sqrt(9 d) (e_d / 2 + 4 u); v1 = 1 + c z:
             e_v1 = c e_z + |c z| e_c + 4 u (1 + |c z|); v = v1^3: relative 3 e_v1 / |v1| + 4 u.  v <= 0: |v1| <= e_v1.
             Accept: log1p(-u3) < z^2 / 2 + d - d v + d log v: 16 u (the addends' magnitudes) + |z| e_z + d e_v +
             d e_v / v + e_d d |1 - v + log v| + 4 u |log1p(-u3)|.  G = d v; boost exp(log(u) / phi): relative
             |log u / phi| (4 u + e_phi) + 8 u.
  NB2        NaN once mu itself is above 2^53.  lam = mu (G / phi): relative e_mu / mu + e_G + e_phi + 4 u, then Poisson's bounds with e_mu = e_lam.
  ancestors  C_p, the normalised inclusive cumulative sum over M particles: (M + 16) u (C <= 1; exp 4 u, the sum M u,
             the division 2 u), the position (s + u0) / S: 4 u.
"""
import math

import numpy as np

import _glm_disp as gd
import _hglm
import _ord
import _predict as pr
from _glm import U

ST_ANC, ST_OUT, ST_GAMMA, ST_GROUP = 16, 17, 18, 19
ATTEMPTS, INV_STEPS, BOOST_Q, MAX_MU = 64, 1000, 192, 2.0 ** 53
LOG_DBL_MAX, LOG_DBL_MIN_NORMAL = 709.782712893384, -708.3964185322641
_lgamma = np.vectorize(math.lgamma, otypes=[np.float64])
_M32 = np.uint64(0xFFFFFFFF)


def philox_uniform(seed, it, particle, stream, q):
    """philox_uniform of smcn_device.hpp for arrays of (iter, particle, q) (broadcast): draw q is half q & 1 of block q >> 1."""
    it, particle, q = np.broadcast_arrays(np.asarray(it, dtype=np.uint64), np.asarray(particle, dtype=np.uint64),
                                          np.asarray(q, dtype=np.uint64))
    c = [q >> np.uint64(1), particle & _M32, it & _M32, np.full(q.shape, stream, dtype=np.uint64)]
    k0, k1 = np.uint64(int(seed) & 0xFFFFFFFF), np.uint64((int(seed) >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & _M32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    odd = (q & np.uint64(1)) == 1
    a, b = np.where(odd, c[2], c[0]), np.where(odd, c[3], c[1])
    return ((a >> np.uint64(5)).astype(np.float64) * 67108864.0 + (b >> np.uint64(6)).astype(np.float64)) / 9007199254740992.0


def ancestors(logw, M, S, seed):
    """Systematic ancestors of S slots -> (a [S], amb [S])."""
    lw = np.zeros(M) if logw is None else np.asarray(logw, dtype=np.float64)
    fin = np.isfinite(lw)
    with np.errstate(all="ignore"):
        w = np.where(fin, np.exp(np.where(fin, lw - np.max(lw[fin]), 0.0)), 0.0)
    C = np.cumsum(w / np.sum(w))
    pos = (np.arange(S) + float(philox_uniform(seed, 0, 0, ST_ANC, 0))) / S
    a = np.searchsorted(C, pos, side="right")
    last = int(np.nonzero(fin)[0][-1])
    e = (M + 20) * U
    near = np.minimum(np.abs(C[np.minimum(a, M - 1)] - pos), np.abs(C[np.maximum(a - 1, 0)] - pos))
    return np.minimum(a, last).astype(np.int64), near <= e


def box_muller(u1, u2):
    """(z, rad): the cosine branch and its radius."""
    rad = np.sqrt(-2.0 * np.log1p(-u1))
    return rad * np.cos(2.0 * np.pi * u2), rad


def bernoulli(p, e_p, seed, s, i):
    u = philox_uniform(seed, s, i, ST_OUT, 0)
    bad = ~np.isfinite(p)
    return np.where(bad, np.nan, (u < p).astype(np.float64)), ~bad & (np.abs(u - p) <= e_p)


def poisson(mu, e_mu, seed, s, i):
    """(y, amb, attempts) for flat arrays; NaN outside [0, 2^53] and at a cap."""
    mu, e_mu, s, i = (np.asarray(v).reshape(-1) for v in np.broadcast_arrays(mu, e_mu, s, i))
    n = mu.shape[0]
    y, amb, att = np.full(n, np.nan), np.zeros(n, dtype=bool), np.zeros(n)
    with np.errstate(all="ignore"):
        ok = (mu >= 0.0) & (mu <= MAX_MU)
        amb |= np.isfinite(mu) & (e_mu > 0.0) & ((np.abs(mu - 10.0) <= e_mu) | (np.abs(mu - MAX_MU) <= e_mu))
        lo = np.nonzero(ok & (mu < 10.0))[0]
        if lo.size:
            m_, e_, u = mu[lo], e_mu[lo], philox_uniform(seed, s[lo], i[lo], ST_OUT, 0)
            p = np.exp(-m_)
            F, k, a_ = p.copy(), np.zeros(lo.size), np.zeros(lo.size, dtype=bool)
            a_ |= np.abs(u - F) <= 10 * U * F + e_
            for step in range(1, INV_STEPS + 1):
                act = (u > F) & (k == step - 1)
                if not act.any():
                    break
                p = np.where(act, p * (m_ / step), p)
                F = np.where(act, F + p, F)
                k = np.where(act, float(step), k)
                a_ |= act & (np.abs(u - F) <= (2 * step + 10) * U * F + e_)
            y[lo] = np.where(u > F, np.nan, k)
            amb[lo] |= a_
            att[lo] = 1.0
        hi = np.nonzero(ok & (mu >= 10.0))[0]
        if hi.size:
            m_, e_ = mu[hi], e_mu[hi]
            r = 8 * U + e_ / m_
            b = 0.931 + 2.53 * np.sqrt(m_)
            a = -0.059 + 0.02483 * b
            lial, vr, lmu = np.log(1.1239 + 1.1328 / (b - 3.4)), 0.9277 - 3.6224 / (b - 2.0), np.log(m_)
            yy, aa, live, na = np.full(hi.size, np.nan), np.zeros(hi.size, dtype=bool), np.ones(hi.size, dtype=bool), np.zeros(hi.size)
            for t in range(ATTEMPTS):
                if not live.any():
                    break
                Uc = philox_uniform(seed, s[hi], i[hi], ST_OUT, 2 * t) - 0.5
                V = philox_uniform(seed, s[hi], i[hi], ST_OUT, 2 * t + 1)
                na += live
                w = 0.5 - np.abs(Uc)
                lin = (2.0 * a / w + b) * Uc
                A = lin + m_ + 0.43
                k = np.floor(A)
                e_k = 16 * U * (np.abs(lin) + m_ + 1.0) + 2 * e_ + 4 * r * np.abs(lin)
                aa |= live & np.isfinite(A) & (np.abs(A - np.rint(A)) <= e_k)
                fast = (w >= 0.07) & (V <= vr)
                aa |= live & (w >= 0.07) & (np.abs(V - vr) <= 16 * U + 4 * r)
                retry = ~fast & ((k < 0.0) | ((w < 0.013) & (V > w)))
                third = live & ~fast & ~retry
                kk = np.where(third, k, 1.0)
                lg = _lgamma(kk + 1.0)
                t1, t2, t3 = np.log(V), np.log(a / (w * w) + b), kk * lmu
                lhs, rhs = t1 + lial - t2, -m_ + t3 - lg
                e3 = 16 * U * (np.abs(t1) + np.abs(lial) + np.abs(t2) + m_ + np.abs(t3) + np.abs(lg)) \
                    + e_ * np.abs(kk / m_ - 1.0) + 8 * r
                aa |= third & (np.abs(lhs - rhs) <= e3)
                acc = live & (fast | (third & (lhs <= rhs)))
                yy = np.where(acc, k, yy)
                live &= ~acc
            y[hi], att[hi] = yy, na
            amb[hi] |= aa
    return y, amb, att


def gamma(phi, e_phi, seed, s, i):
    """Marsaglia-Tsang -> (G, relative bound on G, amb, attempts) for flat arrays (phi > 0 finite)."""
    phi, e_phi, s, i = (np.asarray(v).reshape(-1) for v in np.broadcast_arrays(phi, e_phi, s, i))
    n = phi.shape[0]
    with np.errstate(all="ignore"):
        small = phi < 1.0
        ap = np.where(small, phi + 1.0, phi)
        d = ap - 1.0 / 3.0
        c = 1.0 / np.sqrt(9.0 * d)
        e_d = 1.5 * e_phi + 2 * U
        e_c = 0.5 * e_d + 4 * U
        G, eG, amb, live, na = np.full(n, np.nan), np.zeros(n), np.abs(phi - 1.0) <= e_phi * phi, np.ones(n, dtype=bool), np.zeros(n)
        for t in range(ATTEMPTS):
            if not live.any():
                break
            na += live
            z, rad = box_muller(philox_uniform(seed, s, i, ST_GAMMA, 3 * t), philox_uniform(seed, s, i, ST_GAMMA, 3 * t + 1))
            e_z = 128 * U * rad
            cz = c * z
            v1 = 1.0 + cz
            e_v1 = c * e_z + np.abs(cz) * e_c + 4 * U * (1.0 + np.abs(cz))
            v = v1 * v1 * v1
            amb |= live & (np.abs(v1) <= e_v1)
            pos = live & (v > 0.0)
            vs = np.where(pos, v, 1.0)
            e_v = vs * (3.0 * e_v1 / np.abs(np.where(pos, v1, 1.0)) + 4 * U)
            lhs = np.log1p(-philox_uniform(seed, s, i, ST_GAMMA, 3 * t + 2))
            lv = np.log(vs)
            rhs = 0.5 * z * z + d - d * vs + d * lv
            e = 16 * U * (0.5 * z * z + d + d * vs + d * np.abs(lv)) + np.abs(z) * e_z + d * e_v + d * e_v / vs \
                + e_d * d * np.abs(1.0 - vs + lv) + 4 * U * np.abs(lhs)
            amb |= pos & (np.abs(lhs - rhs) <= e)
            acc = pos & (lhs < rhs)
            G = np.where(acc, d * vs, G)
            eG = np.where(acc, e_v / vs + e_d + 4 * U, eG)
            live &= ~acc
        lu = np.log(philox_uniform(seed, s, i, ST_GAMMA, BOOST_Q))
        G = np.where(small, G * np.exp(lu / phi), G)
        eG = np.where(small, eG + np.abs(lu / phi) * (4 * U + e_phi) + 8 * U, eG)
    return G, eG, amb, na


def nb2(mu, e_mu, phi, e_phi, seed, s, i):
    """(y, amb, (gamma attempts, Poisson attempts))."""
    mu, e_mu, phi, e_phi, s, i = (np.asarray(v).reshape(-1) for v in np.broadcast_arrays(mu, e_mu, phi, e_phi, s, i))
    G, eG, ag, na = gamma(phi, e_phi, seed, s, i)
    with np.errstate(all="ignore"):
        lam = mu * (G / phi)
        e_lam = np.where(lam > 0.0, lam * (e_mu / mu + eG + e_phi + 4 * U), 0.0) + 16 * 2.0 ** -1074
    y, ap, npo = poisson(lam, e_lam, seed, s, i)
    return y, ag | ap, (na, npo)


def normal(eta, e_eta, sigma, e_sigma, seed, s, i):
    """(y, bound on |device - numpy|)."""
    z, rad = box_muller(philox_uniform(seed, s, i, ST_OUT, 0), philox_uniform(seed, s, i, ST_OUT, 1))
    y = eta + sigma * z
    return y, e_eta + sigma * (128 * U * rad + np.abs(z) * (e_sigma + 4 * U)) + 2 * U * np.abs(y)


def ordinal(eta, e_eta, c, e_c, seed, s, i):
    """eta [..], c, e_c [.., K-1] -> (y, amb); NaN for a non-finite eta or cutpoint."""
    u = philox_uniform(seed, s, i, ST_OUT, 0)
    with np.errstate(all="ignore"):
        l1, l2 = np.log(u), np.log1p(-u)
        lat = eta + (l1 - l2)
        e_lat = e_eta + 4 * U * (np.abs(l1) + np.abs(l2)) + 2 * U * np.abs(lat)
        bad = ~np.isfinite(eta) | ~np.all(np.isfinite(c), axis=-1)
        y = np.sum(c < lat[..., None], axis=-1).astype(np.float64)
        amb = np.any(np.abs(c - lat[..., None]) <= e_c + e_lat[..., None], axis=-1) & (u > 0.0)
    return np.where(bad, np.nan, y), amb & ~bad


def categorical(P, e_P, seed, s, i):
    """P, e_P [.., K] -> (y, amb); NaN where a probability is not finite."""
    u = philox_uniform(seed, s, i, ST_OUT, 0)
    K = P.shape[-1]
    with np.errstate(all="ignore"):
        bad = ~np.all(np.isfinite(P), axis=-1)
        F = np.cumsum(P, axis=-1)
        e_F = np.cumsum(e_P, axis=-1) + (np.arange(K) + 2) * U * F
        gt = F[..., :K - 1] > u[..., None]
        y = np.where(np.any(gt, axis=-1), np.argmax(gt, axis=-1), K - 1).astype(np.float64)
        amb = np.any(np.abs(F[..., :K - 1] - u[..., None]) <= e_F[..., :K - 1], axis=-1)
    return np.where(bad, np.nan, y), amb & ~bad


def family_draws(family, mean, e_mean, tau, seed, s, i):
    """One outcome per element of `mean` (the law's p / mu / eta / mu as tests/_predict.py's `mean`), tau the dispersion
    coordinate broadcast to it -> (y, amb, e_y): e_y is the bound of a normal outcome (0 elsewhere)."""
    shape = mean.shape
    s, i = np.broadcast_arrays(s, i)
    s, i = np.broadcast_to(s, shape), np.broadcast_to(i, shape)
    e_y = np.zeros(shape)
    with np.errstate(all="ignore"):
        if family == "bernoulli_logit":
            y, amb = bernoulli(mean, e_mean, seed, s, i)
        elif family == "poisson_log":
            y, amb, _ = poisson(mean, np.where(np.isfinite(e_mean), e_mean, 0.0), seed, s, i)
        elif family == "normal":
            tau = np.broadcast_to(tau, shape)
            sig = np.exp(tau)
            y, e_y = normal(mean, e_mean, sig, (np.abs(tau) + 4) * U, seed, s, i)
            bad = ~np.isfinite(mean) | ~((-2.0 * tau <= LOG_DBL_MAX) & (tau <= LOG_DBL_MAX))
            y, amb = np.where(bad, np.nan, y), np.zeros(shape, dtype=bool)
        else:
            tau = np.broadcast_to(tau, shape)
            okd = (tau <= LOG_DBL_MAX) & (tau >= LOG_DBL_MIN_NORMAL)
            ok = okd & np.isfinite(mean) & (mean <= MAX_MU)
            phi = np.exp(np.where(okd, tau, 0.0))
            y, amb, _ = nb2(np.where(ok, mean, np.nan), np.where(ok, e_mean, 0.0), phi, (np.abs(tau) + 4) * U, seed, s, i)
            amb = (amb & ok.reshape(-1)) | (okd & np.isfinite(mean) & (np.abs(mean - MAX_MU) <= e_mean)).reshape(-1)
    return np.reshape(y, shape), np.reshape(amb, shape), e_y


def model_draws(mn, x, anc, seed, labels=None, s_first=0):
    """The restatement of one call: mn the NumPy model AT THE NEW ROWS (tests/_predict.py), x [M, D] the particles, anc the
    ancestors of the slots s_first .. -> (y [n, m], amb [n, m], e_y [n, m])."""
    xa = np.atleast_2d(np.asarray(x, dtype=np.float64))[np.asarray(anc)]
    n = xa.shape[0]
    s = (s_first + np.arange(n))[:, None]
    kind = pr.kind_of(mn)
    with np.errstate(all="ignore"):
        if kind == "cat":
            T = pr.terms(mn, xa)
            i = np.arange(T["prob"].shape[1])[None, :]
            fin = np.all(np.isfinite(mn.terms(xa)[0]), axis=2)          # a non-finite logit, -inf included: no draw
            y, amb = categorical(np.where(fin[..., None], T["prob"], np.nan), T["e_prob"], seed, *np.broadcast_arrays(s, i))
            return y, amb, np.zeros(y.shape)
        if kind == "ord":
            p, K = mn.p, mn.K
            eta, c = mn.terms(xa)[:2]
            inc = mn.increments(xa)
            e_c = (np.arange(1, K) + 6)[None, :] * U * np.cumsum(np.abs(inc), axis=1)
            e_eta = (2 * p + 4) * U * (np.abs(xa[:, :p]) @ np.abs(mn.X).T) + 4 * U * np.abs(eta)
            i = np.arange(eta.shape[1])[None, :]
            cb = np.broadcast_to(c[:, None, :], eta.shape + (K - 1,))
            y, amb = ordinal(eta, e_eta, cb, e_c[:, None, :], seed, *np.broadcast_arrays(s, i))
            return y, amb, np.zeros(y.shape)
        Dc = mn.Z.shape[1]
        m = mn.Z.shape[0]
        i = np.arange(m)[None, :]
        if isinstance(mn, _hglm.HGLMNumpy):
            tau_g = np.exp(xa[:, mn.lt])
            zsel = xa[:, Dc:mn.lt][:, mn.g]
            e_z = np.zeros((n, m))
            if labels is not None:
                lab = np.asarray(labels)[None, :]
                new = np.broadcast_to(lab >= mn.J, (n, m))
                zn, rad = box_muller(philox_uniform(seed, s, lab, ST_GROUP, 0), philox_uniform(seed, s, lab, ST_GROUP, 1))
                zsel, e_z = np.where(new, zn, zsel), np.where(new, 128 * U * rad, 0.0)
            a = tau_g[:, None] * zsel
            eta = xa[:, :Dc] @ mn.Z.T + a
            A = np.abs(xa[:, :Dc]) @ np.abs(mn.Z).T + np.abs(a)
            e_eta = (2 * Dc + 8) * U * A + 4 * U * np.abs(eta) + tau_g[:, None] * e_z
            tau = xa[:, -1:] if mn.disp else None
            bad = ~(tau_g * tau_g < np.inf)
        else:
            eta = xa[:, :Dc] @ mn.Z.T
            e_eta = (2 * Dc + 4) * U * (np.abs(xa[:, :Dc]) @ np.abs(mn.Z).T) + 4 * U * np.abs(eta)
            tau = xa[:, -1:] if mn.family in gd.DISP_FAMILIES else None
            bad = np.zeros(n, dtype=bool)
        mean, e_mean, _, _ = pr._mean_var(mn.family, eta, e_eta, tau)
        if mn.family == "neg_binomial_2_log":
            mean = np.where(eta > LOG_DBL_MAX, np.inf, mean)
        mean = np.where(bad[:, None] | ~np.isfinite(eta), np.nan, mean)
        return family_draws(mn.family, mean, e_mean + pr.SUB, tau, seed, s, i)
