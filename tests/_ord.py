"""Reference density for the ordinal (ordered-logistic) regression target (smcnuts_amd.OrdinalRegression;
SMCN_MODEL_ORDINAL).

Stan's ordered_logistic with y shifted to 0..K-1: p columns, no intercept, eta_i = X_i b, cutpoints from Stan's `ordered`
transform of u, c_1 = u_1, c_k = c_{k-1} + e^u_k (the running sum, in this order, as the device forms it),
  P(y_i = k) = logit^-1(eta_i - c_k) - logit^-1(eta_i - c_{k+1}),   b_j ~ N(0, s_j^2),  c_k ~ N(0, t_k^2),
with the log-Jacobian sum_{k>=2} u_k in the prior;  x = (b_1..b_p, u_1..u_{K-1}), D = p + K - 1.
The stable form the device evaluates, delta_k = e^u_{k+1}:
  log P(y_i = k) = -softplus(c_k - eta_i) [k >= 1] - softplus(eta_i - c_{k+1}) [k <= K-2] + log(1 - e^-delta_k) [middle],
the last term summed as n_k log(1 - e^-delta_k) over the class counts (= u_{k+1} for u_{k+1} < -36).  Non-finite:
lpri = llik = -inf once a cutpoint is not finite, llik = -inf once an eta_i is not finite.

`OrdinalNumpy` has the reference's StanModel surface (.dim, .logpdf(x, phi), .logpdfgrad(x, phi), .constrain(x),
.constrained_dim, .param_names()): it runs through HostTarget and oracle/pynuts.PyNUTS and reports the same constrained
moments as the device target.  `exact_parts` / `device_bounds` are the fsum reference and the worst-case bound of the
device's evaluation, as tests/_glm.py has them; `mp_parts` is the mpmath value (log domain: 1 - sigma(t) is never formed
at working precision), `mp_logpdf` the density it differentiates for the central-difference check.
"""
import math

import numpy as np

from _glm import HALF_LOG_2PI, U

TINY_U = -36.0          # below it e^u is under the rounding of 1: log(1 - e^-e^u) = u, e^u / expm1(e^u) = 1


def log1mexp_e(u):
    """log(1 - e^-e^u) and e^u / expm1(e^u), elementwise, as the device forms them."""
    u = np.asarray(u, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        ev = np.exp(u)
        tiny = u < TINY_U
        L = np.where(tiny, u, np.log(-np.expm1(-ev)))
        R = np.where(tiny, 1.0, ev / np.expm1(ev))
    return L, R


class OrdinalNumpy:
    def __init__(self, X, y, n_classes=None, prior_sd=2.5, cutpoint_prior_sd=5.0):
        X = np.asarray(X, dtype=np.float64)
        if X.ndim == 1:
            X = X.reshape(-1, 1)
        self.X = X.copy()
        self.y = np.asarray(y).astype(np.int64)
        self.K = int(self.y.max()) + 1 if n_classes is None else int(n_classes)
        self.p = X.shape[1]
        self.dim = self.p + self.K - 1
        self.constrained_dim = self.dim
        s = np.asarray(prior_sd, dtype=np.float64)
        t = np.asarray(cutpoint_prior_sd, dtype=np.float64)
        self.s = np.full(self.p, float(s)) if s.ndim == 0 else s.copy()
        self.t = np.full(self.K - 1, float(t)) if t.ndim == 0 else t.copy()
        self.sd = np.concatenate([self.s, self.t])
        self.counts = np.bincount(self.y, minlength=self.K).astype(np.float64)
        self.calls = 0

    def param_names(self):
        return [f"beta.{j + 1}" for j in range(self.p)] + [f"cutpoint.{k}" for k in range(1, self.K)]

    def increments(self, x2):
        """(c_1, c_2 - c_1, .., c_{K-1} - c_{K-2}) = (u_1, e^u_2, ..), [M, K-1]"""
        u = x2[:, self.p:]
        with np.errstate(over="ignore"):
            return np.concatenate([u[:, :1], np.exp(u[:, 1:])], axis=1)

    def cutpoints(self, x2):
        with np.errstate(over="ignore", invalid="ignore"):
            return np.cumsum(self.increments(x2), axis=1)      # (sequential: the device's order)

    def constrain(self, x):
        x = np.array(x, dtype=np.float64, copy=True)
        x2 = np.atleast_2d(x)
        with np.errstate(invalid="ignore"):
            x2[:, self.p:] = self.cutpoints(x2)
        return x2[0] if x.ndim == 1 else x2

    # ---- per observation, [M, n] ----
    def terms(self, x2):
        """(eta, cutpoints, term, d/d eta, lower and upper cutpoint partials, a1, a2, sigma(a1), sigma(a2), hl, hh)"""
        x2 = np.atleast_2d(np.asarray(x2, dtype=np.float64))
        p, K, y = self.p, self.K, self.y
        c = self.cutpoints(x2)
        with np.errstate(over="ignore", invalid="ignore"):
            eta = x2[:, :p] @ self.X.T
            hl, hh = y >= 1, y <= K - 2
            lo = c[:, np.maximum(y - 1, 0)]
            hi = c[:, np.minimum(y, K - 2)]
            a1, a2 = lo - eta, eta - hi

            def sp_sig(a):
                t = np.exp(-np.abs(a))
                return np.maximum(a, 0.0) + np.log1p(t), np.where(a >= 0.0, 1.0 / (1.0 + t), t / (1.0 + t))

            sp1, s1 = sp_sig(a1)
            sp2, s2 = sp_sig(a2)
            term = -(np.where(hl, sp1, 0.0) + np.where(hh, sp2, 0.0))
            term = np.where(np.isfinite(eta), term, -np.inf)
            glo = np.where(hl, -s1, 0.0)
            ghi = np.where(hh, s2, 0.0)
            de = -(glo + ghi)
        return eta, c, term, de, glo, ghi, a1, a2, s1, s2, hl, hh

    def count_terms(self, x2):
        """n_k log(1 - e^-delta_k) and n_k delta_k / expm1(delta_k) on u_2..u_{K-1}, [M, K-2]"""
        L, R = log1mexp_e(x2[:, self.p + 1:])
        n = self.counts[1:self.K - 1]
        return np.where(n > 0, n * L, 0.0), np.where(n > 0, n * R, 0.0)

    def cut_partials(self, glo, ghi):
        """d llik / d c_m (m = 1..K-1) from the per-observation partials, [M, K-1]"""
        M, K = glo.shape[0], self.K
        g = np.zeros((M, K - 1))
        for m in range(1, K):
            g[:, m - 1] = glo[:, self.y == m].sum(axis=1) + ghi[:, self.y == m - 1].sum(axis=1)
        return g

    def chain(self, x2, gc):
        """d / d u from d / d c: suffix sums times dc/du_m (1 for m = 1, e^u_m above), [M, K-1]"""
        suf = np.cumsum(gc[:, ::-1], axis=1)[:, ::-1]
        dm = self.increments(x2).copy()
        dm[:, 0] = 1.0
        return dm * suf

    def parts(self, x):
        x2 = np.atleast_2d(np.asarray(x, dtype=np.float64))
        p = self.p
        eta, c, term, de, glo, ghi, *_ = self.terms(x2)
        cl, cg = self.count_terms(x2)
        with np.errstate(over="ignore", invalid="ignore"):
            v = np.concatenate([x2[:, :p], c], axis=1)
            lpri = np.sum(-0.5 * (v / self.sd) ** 2 - np.log(self.sd) - HALF_LOG_2PI, axis=1) \
                + np.sum(x2[:, p + 1:], axis=1)
            llik = np.sum(term, axis=1) + np.sum(cl, axis=1)
            gpri = np.concatenate([-x2[:, :p] / self.s ** 2, self.chain(x2, -c / self.t ** 2)], axis=1)
            gpri[:, p + 1:] += 1.0
            gu = self.chain(x2, self.cut_partials(glo, ghi))
            gu[:, 1:] += cg
            glik = np.concatenate([de @ self.X, gu], axis=1)
        bad = ~np.all(np.isfinite(c), axis=1)
        lpri = np.where(bad, -np.inf, lpri)
        llik = np.where(bad | ~np.isfinite(llik), -np.inf, llik)
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
    """(lpri, llik, gpri, glik) with every sum over observations, classes and coordinates taken by math.fsum over the
    float64 terms (the cutpoints and the chain's suffix sums as the model forms them)."""
    x2 = np.atleast_2d(np.asarray(x2, dtype=np.float64))
    p, K, M = model.p, model.K, x2.shape[0]
    eta, c, term, de, glo, ghi, *_ = model.terms(x2)
    cl, cg = model.count_terms(x2)
    lpri0, _, gpri, _ = model.parts(x2)
    lpri, llik = np.empty(M), np.empty(M)
    glik = np.empty_like(x2)
    with np.errstate(over="ignore", invalid="ignore"):
        v = np.concatenate([x2[:, :p], c], axis=1)
        pri = -0.5 * (v / model.sd) ** 2 - np.log(model.sd) - HALF_LOG_2PI
        dm = model.increments(x2)
        dm[:, 0] = 1.0
        for m in range(M):
            bad = not np.all(np.isfinite(c[m]))
            lpri[m] = -np.inf if bad else math.fsum(pri[m].tolist() + x2[m, p + 1:].tolist())
            tl = term[m].tolist() + cl[m].tolist()
            llik[m] = -np.inf if bad or not np.all(np.isfinite(tl)) else math.fsum(tl)
            for j in range(p):
                col = de[m] * model.X[:, j]
                glik[m, j] = math.fsum(col.tolist()) if np.all(np.isfinite(col)) else np.nan
            gc = [math.fsum(glo[m, model.y == k].tolist() + ghi[m, model.y == k - 1].tolist()) for k in range(1, K)]
            for k in range(1, K):
                glik[m, p + k - 1] = dm[m, k - 1] * math.fsum(gc[k - 1:]) + (cg[m, k - 2] if k >= 2 else 0.0)
    return lpri, llik, gpri, glik


def device_bounds(model, x2):
    """Worst-case |device - exact| of lpri, llik (per particle), gpri and glik (per particle and coordinate).

    The cutpoint c_m is a running sum of m values, within (m + 6) u sum_{j<=m} |c_j - c_{j-1}| of the reference's (the
    increments' exp within an ulp on either side).  eta_i comes from p fused multiply-adds, within (2 p + 4) u
    sum_j |b_j X_ij| + 4 u |eta_i|; a = c - eta carries both plus its own rounding.  A softplus term moves by
    sigma(a) e_a and is within 8 u (|a| + 1) of its own rounding (exp_fast, log1p_pos); a sigmoid by
    sigma (1 - sigma) e_a, and 8 u sigma.  The count terms are within 8 u (|L| + 1) per count.  The n + K terms are summed
    in per-lane sequences and a butterfly: (n + K + 4) u sum |term|.  The gradient's sums over observations are within
    (n + 2) u of the sums of magnitudes, the suffix sums within (K + 8) u, the chain's product and the count gradient
    add 4 u of their magnitudes."""
    x2 = np.atleast_2d(np.asarray(x2, dtype=np.float64))
    p, K, n, M, y = model.p, model.K, model.X.shape[0], x2.shape[0], model.y
    eta, c, term, de, glo, ghi, a1, a2, s1, s2, hl, hh = model.terms(x2)
    cl, cg = model.count_terms(x2)
    inc = model.increments(x2)
    dm = inc.copy()
    dm[:, 0] = 1.0
    with np.errstate(over="ignore", invalid="ignore"):
        e_c = (np.arange(1, K) + 6)[None, :] * U * np.cumsum(np.abs(inc), axis=1)      # [M, K-1]
        A = np.abs(x2[:, :p]) @ np.abs(model.X).T
        e_eta = (2 * p + 4) * U * A + 4 * U * np.abs(eta)
        e_lo = e_c[:, np.maximum(y - 1, 0)]
        e_hi = e_c[:, np.minimum(y, K - 2)]
        e_a1 = e_lo + e_eta + 2 * U * np.abs(a1)
        e_a2 = e_hi + e_eta + 2 * U * np.abs(a2)
        e_t = np.where(hl, s1 * e_a1 + 8 * U * (np.abs(a1) + 1.0), 0.0) \
            + np.where(hh, s2 * e_a2 + 8 * U * (np.abs(a2) + 1.0), 0.0)
        e_s1 = np.where(hl, s1 * (1.0 - s1) * e_a1 + 8 * U * s1, 0.0)
        e_s2 = np.where(hh, s2 * (1.0 - s2) * e_a2 + 8 * U * s2, 0.0)
        e_de = e_s1 + e_s2 + U * np.abs(de)
        L, R = log1mexp_e(x2[:, p + 1:])
        nk = model.counts[1:K - 1][None, :]
        b_llik = np.sum(e_t, axis=1) + np.sum(nk * 8 * U * (np.abs(L) + 1.0), axis=1) \
            + (n + K + 4) * U * (np.sum(np.abs(term), axis=1) + np.sum(np.abs(cl), axis=1))
        # gradient: the columns, then the cutpoint partials, their suffix sums and the chain
        b_gb = (e_de + (n + 2) * U * np.abs(de)) @ np.abs(model.X)
        e_gc = np.zeros((M, K - 1))
        mag = np.zeros((M, K - 1))
        for m in range(1, K):
            lo_m, hi_m = y == m, y == m - 1
            e_gc[:, m - 1] = np.sum(e_s1[:, lo_m] + (n + 2) * U * s1[:, lo_m] * hl[lo_m], axis=1) \
                + np.sum(e_s2[:, hi_m] + (n + 2) * U * s2[:, hi_m] * hh[hi_m], axis=1)
            mag[:, m - 1] = np.sum(np.abs(glo[:, lo_m]), axis=1) + np.sum(np.abs(ghi[:, hi_m]), axis=1)

        def suffix(v):
            return np.cumsum(v[:, ::-1], axis=1)[:, ::-1]

        gc = model.cut_partials(glo, ghi)
        e_S = suffix(e_gc) + (K + 8) * U * suffix(mag)
        S = suffix(gc)
        b_gu = dm * e_S + 4 * U * dm * np.abs(S)
        b_gu[:, 1:] += 8 * U * np.abs(cg) + 4 * U * np.abs(cg + dm[:, 1:] * S[:, 1:])
        b_glik = np.concatenate([b_gb, b_gu], axis=1)
        # prior
        v = np.concatenate([x2[:, :p], c], axis=1)
        pri = -0.5 * (v / model.sd) ** 2 - np.log(model.sd) - HALF_LOG_2PI
        b_lpri = (model.dim + 6) * U * (np.sum(np.abs(pri) + 0.5 * (v / model.sd) ** 2 + np.abs(np.log(model.sd))
                                               + HALF_LOG_2PI, axis=1) + np.sum(np.abs(x2[:, p + 1:]), axis=1)) \
            + np.sum(np.abs(c) / model.t ** 2 * e_c, axis=1)
        pc = -c / model.t ** 2
        e_Sp = suffix(e_c / model.t ** 2 + 4 * U * np.abs(pc)) + (K + 8) * U * suffix(np.abs(pc))
        Sp = suffix(pc)
        b_gp_u = dm * e_Sp + 4 * U * dm * np.abs(Sp) + 4 * U * (np.abs(dm * Sp) + 1.0)
        b_gpri = np.concatenate([8 * U * np.abs(x2[:, :p] / model.s ** 2), b_gp_u], axis=1)
    return b_lpri, b_llik, b_gpri, b_glik


def _mp_setup(model, x, mp):
    p, K = model.p, model.K
    b = [mp.mpf(float(v)) for v in x[:p]]
    u = [mp.mpf(float(v)) for v in x[p:]]
    c = [u[0]]
    for k in range(1, K - 1):
        c.append(c[-1] + mp.exp(u[k]))
    eta = [mp.fsum(b[j] * mp.mpf(float(model.X[i, j])) for j in range(p)) for i in range(model.X.shape[0])]
    return b, u, c, eta


def _mp_logp(y, K, eta, c, u, mp):
    """log P(y | eta) in the log domain: no 1 - sigma(t) at working precision"""
    v = mp.mpf(0)
    if y >= 1:
        v -= mp.log1p(mp.exp(c[y - 1] - eta))
    if y <= K - 2:
        v -= mp.log1p(mp.exp(eta - c[y]))
    if 1 <= y <= K - 2:
        v += mp.log(-mp.expm1(-mp.exp(u[y])))                    # delta_y = c_{y+1} - c_y = e^u_{y+1}
    return v


def mp_logpdf(model, x, phi=1.0, dps=60):
    """log pi_phi at one point with mpmath (x given as mpf or float)."""
    import mpmath as mp
    p, K = model.p, model.K
    with mp.workdps(dps):
        b = [mp.mpf(v) for v in x[:p]]
        u = [mp.mpf(v) for v in x[p:]]
        c = [u[0]]
        for k in range(1, K - 1):
            c.append(c[-1] + mp.exp(u[k]))
        v = b + c
        sd = [mp.mpf(float(s)) for s in model.sd]
        lpri = mp.fsum(-(a / s) ** 2 / 2 - mp.log(s) - mp.log(2 * mp.pi) / 2 for a, s in zip(v, sd)) + mp.fsum(u[1:])
        llik = mp.mpf(0)
        for i in range(model.X.shape[0]):
            e = mp.fsum(b[j] * mp.mpf(float(model.X[i, j])) for j in range(p))
            llik += _mp_logp(int(model.y[i]), K, e, c, u, mp)
        return lpri + phi * llik


def mp_parts(model, x, dps=50):
    """(lpri, llik, gpri, glik) at one point with mpmath at `dps` digits: the cutpoints from u, each eta from the
    float64 data exactly, the log-domain density and the analytic gradient (suffix-sum chain)."""
    import mpmath as mp
    x = np.asarray(x, dtype=np.float64)
    p, K = model.p, model.K
    with mp.workdps(dps):
        b, u, c, eta = _mp_setup(model, x, mp)
        sd = [mp.mpf(float(s)) for s in model.sd]
        v = b + c
        lpri = mp.fsum(-(a / s) ** 2 / 2 - mp.log(s) - mp.log(2 * mp.pi) / 2 for a, s in zip(v, sd)) + mp.fsum(u[1:])
        llik = mp.mpf(0)
        gb = [mp.mpf(0)] * p
        gcut = [mp.mpf(0)] * (K - 1)
        sig = lambda a: 1 / (1 + mp.exp(-a))
        for i in range(model.X.shape[0]):
            y, e = int(model.y[i]), eta[i]
            llik += _mp_logp(y, K, e, c, u, mp)
            de = mp.mpf(0)
            if y >= 1:
                s1 = sig(c[y - 1] - e)
                de += s1
                gcut[y - 1] -= s1
            if y <= K - 2:
                s2 = sig(e - c[y])
                de -= s2
                gcut[y] += s2
            for j in range(p):
                gb[j] += de * mp.mpf(float(model.X[i, j]))
        gp_c = [-c[k] / sd[p + k] ** 2 for k in range(K - 1)]
        glik, gpri = list(gb), [-b[j] / sd[j] ** 2 for j in range(p)]
        for m in range(K - 1):
            dmul = mp.mpf(1) if m == 0 else mp.exp(u[m])
            gl = dmul * mp.fsum(gcut[m:])
            gq = dmul * mp.fsum(gp_c[m:])
            if m >= 1:
                d = mp.exp(u[m])
                gl += model.counts[m] * d / mp.expm1(d)        # the middle class m (0-based) below c_{m+1}
                gq += 1
            glik.append(gl)
            gpri.append(gq)
        return (float(lpri), float(llik), np.array([float(g) for g in gpri]), np.array([float(g) for g in glik]))


def points(m, rng):
    """Benign points; |eta| near 800 with the cutpoints near 0; the cutpoints at +-800 (everything in an end class); gaps
    of e^-700 between cutpoints (collapsed middle classes, finite); widely spread cutpoints."""
    p, K, D = m.p, m.K, m.dim
    x = [np.concatenate([rng.standard_normal(p) * 0.5, [rng.standard_normal() - 1.0],
                         rng.standard_normal(K - 2) * 0.3]) for _ in range(3)]
    if p:
        big = np.zeros(D)
        big[:p] = 800.0 / max(np.abs(m.X).sum(axis=1).max(), 1e-300) * np.where(np.arange(p) % 2 == 0, 1.0, -1.0)
        x.append(big)
    for c1 in (800.0, -800.0):
        v = np.zeros(D)
        v[p] = c1
        x.append(v)
    gap = np.zeros(D)
    gap[p] = -0.3
    gap[p + 1:] = -700.0
    x.append(gap)
    wide = np.zeros(D)
    wide[p] = -3.0
    wide[p + 1:] = 2.0
    x.append(wide)
    return np.array(x)


def synthetic(K, n, p, seed, scale=1.0):
    """A fixed-seed synthetic K-class ordinal problem: X ~ N(0, 1) / sqrt(p), b ~ N(0, scale^2), evenly spread
    cutpoints, y drawn from the ordered-logistic probabilities (every class likely to occur)."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, p)) / math.sqrt(max(p, 1))
    b = rng.standard_normal(p) * scale
    c = np.linspace(-1.5, 1.5, K - 1) if K > 2 else np.zeros(1)
    eta = X @ b
    cdf = 1.0 / (1.0 + np.exp(-(c[None, :] - eta[:, None])))                   # P(y <= k), k = 0..K-2
    u = rng.random(n)
    y = (u[:, None] > cdf).sum(axis=1)
    return X, y.astype(np.int64)
