"""References, error bounds and helpers for held-out prediction (smcnuts_amd.predict; smcn_predict_*).

`terms(model, x2)` evaluates an existing NumPy model BUILT AT THE NEW ROWS (`_glm.GLMNumpy`, `_glm_disp.GLMDispNumpy`,
`_hglm.HGLMNumpy`, `_cat.CategoricalNumpy`, `_ord.OrdinalNumpy` with X_new, y_new [, groups_new] and the training priors)
at the points x2 and returns, per (particle, row): the term ll = log p(y_new_i | x_p), E[y_i | x_p] and Var(y_i | x_p)
(GLM families, hierarchical), the class probabilities (categorical, ordinal) and sum_k sigma(eta_i - c_k) (ordinal), each
with a bound on |device - numpy|.  `reference(T, logw)` applies the definitions of smcnuts_amd/predict.py with
max-shifted sums and a two-pass variance; `bounds(T, logw, ref)` the per-element bounds below; `numpy_partials` builds a
partials block by the documented column layout of include/smcnuts_hip.h, independently of the kernel.

Per-pair bounds, u = 2^-53, from the models' own magnitude counts (their `device_bounds`):
  e_eta   (2 D + 4) u sum_j |b_j Z_ij| + 4 u |eta|  (hierarchical: (2 Dc + 8) u (.. + |alpha|), _hglm.device_bounds)
  e_ll    GLM: 8 u mag + |d| e_eta;  dispersion families and hierarchical: 64 u m_term + |d| e_eta (normal with the
          addends' own magnitudes, tests/_pointwise.py);  categorical: _cat.device_bounds' e_term;  ordinal:
          _ord.device_bounds' e_t plus 8 u (|L| + 1) for the middle class's log(1 - e^-delta) and 4 u |ll| for the sum.
  e_mean  sigmoid: 8 u s + s (1 - s) e_eta;  e^eta: mu (8 u + e_eta);  eta: e_eta + 8 u |eta|   (as fitted_i)
  e_var   p (1 - p): |1 - 2 s| e_mean + e_mean^2 + 2 u (the rounding of 1 - s is absolute);  mu: e_mean;
          sigma^2 = e^2tau: 8 u sigma^2;  mu + mu^2 / phi: e_mean (1 + 2 mu / phi) + 16 u var.
  e_prob  categorical: (4 K + 8) u + p_k (e_eta_k + sum_l p_l e_eta_l)  (_cat.device_bounds' e_d; e_eta_0 = 0);
          ordinal, P_k = sigma(a_k) sigma(-a_{k+1}) (1 - e^-delta_k): a relative error of
          (1 - sigma(a_k)) e_a_k + sigma(a_{k+1}) e_a_{k+1} + 32 u, e_a = e_c + e_eta + 2 u |a| (_ord.device_bounds);
  e_em    sum_k (s_k (1 - s_k) e_a_k + 8 u s_k) + (K + 4) u em.
Per-row bounds, M contributing particles, W the normalised weights, E = max_p of the pair bound:
  lpd_i   follows lppd_i:  E_ll + (M + 16) u + 4 u |lpd_i|.
  mean_i  follows fitted_i, with the shifts (each particle slice sums mean_p - c_s, c_s the slice's first mean, and the
          merge re-centres; |c_s| <= cmax = max_p |mean_p|):
          sum_p W_p e_mean + (M + 16) u sum_p W_p (|mean_p| + cmax) + 4 u |mean_i|;  ordinal: the same without a shift.
  prob    follows fitted_i:  sum_p W_p e_prob + (M + 16) u prob.
  var_i   the sum of the fitted_i argument for sum_p W_p Var(y | x_p) and the p_waic_i argument for the weighted
          variance of the means (E -> E_mean, m2 = sum_p W_p (mean_p - c)^2 = v + (mean_i - c)^2 <= v + range^2, the
          range of the means, for whichever particle's mean a slice is centred on):
          sum_p W_p e_var + (M + 16) u sum_p W_p Var_p + 2 sqrt(v) E_mean + E_mean^2 + 3 (M + 16) u m2 + 4 u var_i.
Every pair bound of a sigmoid, a probability or a mean also carries SUB = 16 x 2^-1074: a value that lands in the
subnormal range is rounded to a multiple of 2^-1074, whatever its relative bound says (e^-|a| for |a| in 708..745).
Non-finite reference entries are compared by pattern (`assert_prediction`).
"""
import math

import numpy as np

import _cat
import _glm
import _glm_disp as gd
import _hglm
import _ord
from _glm import U
from _pointwise import _lse0, _norm_weights

MA, SA, NINF, NBAD, C0, SW, S1, S2, VAR = range(9)
FIELDS = ("lpd_i", "mean_i", "var_i", "prob")
SUB = 16 * 2.0 ** -1074


def kind_of(m):
    if isinstance(m, _cat.CategoricalNumpy):
        return "cat"
    if isinstance(m, _ord.OrdinalNumpy):
        return "ord"
    return "glm"


def _mean_var(family, eta, e_eta, tau):
    """E[y | eta], Var(y | eta, tau) and their bounds; tau [M, 1] (dispersion families) or None."""
    with np.errstate(all="ignore"):
        if family == "bernoulli_logit":
            t = np.exp(-np.abs(eta))
            s = np.where(eta >= 0.0, 1.0 / (1.0 + t), t / (1.0 + t))
            e_mean = 8 * U * s + s * (1.0 - s) * e_eta
            return s, e_mean, s * (1.0 - s), np.abs(1.0 - 2.0 * s) * e_mean + e_mean ** 2 + 2 * U
        if family == "normal":
            var = np.broadcast_to(np.exp(2.0 * tau), eta.shape)
            return eta, e_eta + 8 * U * np.abs(eta), var, 8 * U * var
        mu = np.exp(eta)
        e_mean = mu * (8 * U + e_eta)
        if family == "poisson_log":
            return mu, e_mean, mu, e_mean
        iphi = np.exp(-tau)
        var = mu + mu * mu * iphi
        return mu, e_mean, var, e_mean * (1.0 + 2.0 * mu * iphi) + 16 * U * var


def terms(m, x2):
    """dict(ll, e_ll [M, m]; glm: mean, e_mean, var, e_var; cat / ord: prob, e_prob [M, m, K]; ord: em, e_em)."""
    x2 = np.atleast_2d(np.asarray(x2, dtype=np.float64))
    T = {}
    with np.errstate(all="ignore"):
        if isinstance(m, _hglm.HGLMNumpy):
            _, _, (term, d, gt, m_term, *_r) = m.obs(x2)
            Dc = m.Dc
            tau = np.exp(x2[:, m.lt])
            a = tau[:, None] * x2[:, Dc:m.lt][:, m.g]
            eta = x2[:, :Dc] @ m.Z.T + a                         # (the real tau: obs() evaluates bad particles at 1)
            A = np.abs(x2[:, :Dc]) @ np.abs(m.Z).T + np.abs(a)
            e_eta = (2 * Dc + 8) * U * A + 4 * U * np.abs(eta)
            ld = x2[:, -1:] if m.disp else None
            if m.family == "normal":
                lz = np.where(m.bad_d(ld), 0.0, ld)
                m_term = m_term - np.abs(-lz - gd.HALF_LOG_2PI) + (np.abs(lz) + gd.HALF_LOG_2PI)
            T["ll"] = np.where(m.bad(x2)[:, None], -np.inf, term)
            T["e_ll"] = 64 * U * m_term + np.abs(d) * e_eta
            T["mean"], T["e_mean"], T["var"], T["e_var"] = _mean_var(m.family, eta, e_eta, ld)
        elif isinstance(m, gd.GLMDispNumpy):
            eta, (term, d, gt, m_term, *_r) = m.obs(x2)
            bad = m.bad(x2[:, -1])
            Dc = m.Dc
            A = np.abs(x2[:, :Dc]) @ np.abs(m.Z).T
            e_eta = (2 * Dc + 4) * U * A + 4 * U * np.abs(eta)
            if m.family == "normal":
                tz = np.where(bad, 0.0, x2[:, -1])[:, None]
                m_term = m_term - np.abs(-tz - gd.HALF_LOG_2PI) + (np.abs(tz) + gd.HALF_LOG_2PI)
            T["ll"] = np.where(bad[:, None], -np.inf, term)
            T["e_ll"] = 64 * U * m_term + np.abs(d) * e_eta
            T["mean"], T["e_mean"], T["var"], T["e_var"] = _mean_var(m.family, eta, e_eta, x2[:, -1:])
        elif isinstance(m, _glm.GLMNumpy):
            eta, term, d = m.terms(x2)
            A = np.abs(x2) @ np.abs(m.Z).T
            e_eta = (2 * m.dim + 4) * U * A + 4 * U * np.abs(eta)
            if m.family == "bernoulli_logit":
                mag = np.abs(eta) + np.log1p(np.exp(-np.abs(eta)))
            else:
                mag = np.abs(m.y * eta) + np.exp(eta) + m.lgy
            T["ll"], T["e_ll"] = term, 8 * U * mag + np.abs(d) * e_eta
            T["mean"], T["e_mean"], T["var"], T["e_var"] = _mean_var(m.family, eta, e_eta, None)
        elif isinstance(m, _cat.CategoricalNumpy):
            full, term, d, mx, S, prob = m.terms(x2)
            M, n, K, Dc = x2.shape[0], m.Z.shape[0], m.K, m.Dc
            A = np.einsum("mkj,ij->mik", np.abs(x2.reshape(M, K - 1, Dc)), np.abs(m.Z))
            e_eta = (2 * Dc + 4) * U * A + 4 * U * np.abs(full[..., 1:])
            ey = np.take_along_axis(full, np.broadcast_to(m.y[None, :, None], (M, n, 1)), axis=2)[..., 0]
            T["ll"] = term
            T["e_ll"] = 8 * U * (np.abs(ey) + np.abs(mx) + math.log(K) + K) + np.sum(np.abs(d) * e_eta, axis=2)
            e0 = np.concatenate([np.zeros((M, n, 1)), e_eta], axis=2)
            T["prob"] = prob
            T["e_prob"] = (4 * K + 8) * U + prob * (e0 + np.sum(prob * e0, axis=2)[..., None])
        else:
            p, K, y = m.p, m.K, m.y
            eta, c, term, de, glo, ghi, a1, a2, s1, s2, hl, hh = m.terms(x2)
            inc = m.increments(x2)
            e_c = (np.arange(1, K) + 6)[None, :] * U * np.cumsum(np.abs(inc), axis=1)          # [M, K-1]
            A = np.abs(x2[:, :p]) @ np.abs(m.X).T
            e_eta = (2 * p + 4) * U * A + 4 * U * np.abs(eta)
            e_a1 = e_c[:, np.maximum(y - 1, 0)] + e_eta + 2 * U * np.abs(a1)
            e_a2 = e_c[:, np.minimum(y, K - 2)] + e_eta + 2 * U * np.abs(a2)
            L, _ = _ord.log1mexp_e(x2[:, p:])                    # [M, K-1]; column j: log(1 - e^-delta_j), j >= 1
            mid = (y >= 1) & (y <= K - 2)
            Ly = np.where(mid[None, :], L[:, np.clip(y, 1, max(K - 2, 1)) if K > 2 else np.zeros_like(y)], 0.0)
            ll = term + Ly
            bad = ~np.all(np.isfinite(c), axis=1)
            T["ll"] = np.where(bad[:, None], -np.inf, ll)
            T["e_ll"] = np.where(hl, s1 * e_a1 + 8 * U * (np.abs(a1) + 1.0), 0.0) \
                + np.where(hh, s2 * e_a2 + 8 * U * (np.abs(a2) + 1.0), 0.0) \
                + np.where(mid[None, :], 8 * U * (np.abs(Ly) + 1.0), 0.0) + 4 * U * np.abs(ll)
            # every cutpoint: s[.., k] = sigma(eta - c_{k+1}), sc its complement, from one exponential
            a = eta[..., None] - c[:, None, :]                   # [M, m, K-1]
            t = np.exp(-np.abs(a))
            s = np.where(a >= 0.0, 1.0 / (1.0 + t), t / (1.0 + t))
            sc = np.where(a >= 0.0, t / (1.0 + t), 1.0 / (1.0 + t))
            e_a = e_c[:, None, :] + e_eta[..., None] + 2 * U * np.abs(a)
            T["em"] = np.sum(s, axis=2)
            T["e_em"] = np.sum(s * (1.0 - s) * e_a + 8 * U * s, axis=2) + (K + 4) * U * T["em"]
            if K <= 16:
                om = -np.expm1(-inc)                             # column j >= 1: 1 - e^-delta_j
                one = np.ones(eta.shape + (1,))
                zero = np.zeros(eta.shape + (1,))
                lo = np.concatenate([one, s], axis=2)            # sigma(eta - c_k), k = 0..K-1 (c_0 = -inf)
                hi = np.concatenate([sc, one], axis=2)           # sigma(c_{k+1} - eta)          (c_K = +inf)
                omk = np.concatenate([np.ones((x2.shape[0], 1)), om[:, 1:], np.ones((x2.shape[0], 1))], axis=1)
                prob = lo * hi * omk[:, None, :]
                rel = np.concatenate([zero, (1.0 - s) * e_a], axis=2) + np.concatenate([s * e_a, zero], axis=2) + 32 * U
                T["prob"], T["e_prob"] = prob, prob * rel
    for k in ("e_mean", "e_var", "e_prob", "e_em"):
        if k in T:
            T[k] = T[k] + SUB
    return T


def _fin(a):
    return np.where(np.isfinite(a), a, 0.0)


def reference(T, logw=None, has_y=True):
    """The definitions of smcnuts_amd/predict.py -> dict(lpd_i, n_inf_i, mean_i, var_i, prob, ess, n_particles)."""
    M = T["ll"].shape[0]
    keep, lW = _norm_weights(logw, M)
    W = np.exp(lW)
    out = dict(ess=float(1.0 / np.sum(np.exp(2.0 * lW))), n_particles=int(np.sum(keep)))
    with np.errstate(all="ignore"):
        if has_y:
            ll = T["ll"][keep]
            out["lpd_i"] = _lse0(lW[:, None] + ll)
            out["n_inf_i"] = np.sum(np.isneginf(ll), axis=0).astype(np.float64)
        if "mean" in T:
            mean, var = T["mean"][keep], T["var"][keep]
            bad = np.any(~np.isfinite(mean) | ~np.isfinite(var), axis=0)
            mz, vz = _fin(mean), _fin(var)
            mu = np.sum(W[:, None] * mz, axis=0)
            mu = mu + np.sum(W[:, None] * (mz - mu), axis=0)         # (second pass)
            between = np.sum(W[:, None] * (mz - mu) ** 2, axis=0)
            out["between_i"] = np.where(bad, np.nan, between)
            out["mean_i"] = np.where(bad, np.nan, mu)
            out["var_i"] = np.where(bad, np.nan, np.sum(W[:, None] * vz, axis=0) + between)
        if "em" in T:
            em = T["em"][keep]
            bad = np.any(~np.isfinite(em), axis=0)
            out["mean_i"] = np.where(bad, np.nan, np.sum(W[:, None] * _fin(em), axis=0))
        if "prob" in T:
            pr = T["prob"][keep]
            bad = np.any(~np.isfinite(pr), axis=(0, 2))
            if "em" in T:
                bad = bad | np.any(~np.isfinite(T["em"][keep]), axis=0)
            out["prob"] = np.where(bad[:, None], np.nan, np.sum(W[:, None, None] * _fin(pr), axis=0))
    return out


def bounds(T, logw, ref, has_y=True):
    """Per-element |device - reference| bounds (module docstring); non-finite reference entries: irrelevant."""
    M0 = T["ll"].shape[0]
    keep, lW = _norm_weights(logw, M0)
    M = int(np.sum(keep))
    W = np.exp(lW)[:, None]
    b = {}
    with np.errstate(all="ignore"):
        if has_y:
            ll, e = T["ll"][keep], T["e_ll"][keep]
            E = np.max(np.where(np.isfinite(ll), e, 0.0), axis=0)
            b["lpd_i"] = E + (M + 16) * U + 4 * U * np.abs(ref["lpd_i"])
        if "mean" in T:
            mean, e_mean, var, e_var = (_fin(T[k][keep]) for k in ("mean", "e_mean", "var", "e_var"))
            cmax = np.max(np.abs(mean), axis=0)
            b["mean_i"] = np.sum(W * e_mean, axis=0) + (M + 16) * U * np.sum(W * (np.abs(mean) + cmax), axis=0) \
                + 4 * U * np.abs(ref["mean_i"])
            Em = np.max(e_mean, axis=0)
            v = _fin(ref["between_i"])
            m2 = v + (np.max(mean, axis=0) - np.min(mean, axis=0)) ** 2
            b["var_i"] = np.sum(W * e_var, axis=0) + (M + 16) * U * np.sum(W * np.abs(var), axis=0) \
                + 2.0 * np.sqrt(v) * Em + Em * Em + 3 * (M + 16) * U * m2 + 4 * U * np.abs(ref["var_i"])
        if "em" in T:
            em, e_em = _fin(T["em"][keep]), _fin(T["e_em"][keep])
            b["mean_i"] = np.sum(W * e_em, axis=0) + (M + 16) * U * np.sum(W * np.abs(em), axis=0) + 4 * U * np.abs(ref["mean_i"])
        if "prob" in T:
            pr, e_pr = _fin(T["prob"][keep]), _fin(T["e_prob"][keep])
            b["prob"] = np.sum(W[:, :, None] * e_pr, axis=0) + (M + 16) * U * np.sum(W[:, :, None] * pr, axis=0)
    return {k: _fin(v) for k, v in b.items()}


def weight_shift_bounds(T, logw, ref, delta):
    """How far the summaries move when every log-weight moves by at most delta (the rounding of lw + 1e5).  The
    normalised weights move by factors within exp(+-2 delta), r = expm1(2 delta): lpd_i by 2 delta; a weighted mean of
    q_p by r sum W |q_p - mean|; var_i = E[Var] + between by r sum W |Var_p - E[Var]| + r sum W a^2 + (r sum W |a|)^2,
    a = mean_p - mean_i (tests/_pointwise.py)."""
    keep, lW = _norm_weights(logw, T["ll"].shape[0])
    W = np.exp(lW)[:, None]
    r = math.expm1(2.0 * delta)
    b = {}
    with np.errstate(all="ignore"):
        if "lpd_i" in ref:
            b["lpd_i"] = np.full(T["ll"].shape[1], 2.0 * delta)
        if "mean" in T:
            mean, var = _fin(T["mean"][keep]), _fin(T["var"][keep])
            a = _fin(mean - ref["mean_i"])
            A1 = np.sum(W * np.abs(a), axis=0)
            b["mean_i"] = r * A1
            ev = np.sum(W * var, axis=0)
            b["var_i"] = r * np.sum(W * np.abs(var - ev), axis=0) + r * np.sum(W * a * a, axis=0) + (r * A1) ** 2
        if "em" in T:
            em = _fin(T["em"][keep])
            b["mean_i"] = r * np.sum(W * np.abs(_fin(em - ref["mean_i"])), axis=0)
        if "prob" in T:
            pr = _fin(T["prob"][keep])
            b["prob"] = r * np.sum(W[:, :, None] * np.abs(_fin(pr - ref["prob"][None])), axis=0)
    return {k: _fin(v) for k, v in b.items()}


def add_bounds(*bs):
    return {k: sum(b[k] for b in bs) for k in bs[0]}


def assert_prediction(got, ref, bnd, factor=1.0, what="", close=None, report=None):
    """Element by element, no element left out: the same non-finite pattern, |got - ref| <= factor * bound elsewhere.
    A field the reference has must be present in `got`; one it lacks must be None."""
    for k in FIELDS:
        g = getattr(got, k)
        if k not in ref:
            assert g is None, f"{what} {k}: expected None"
            continue
        assert g is not None, f"{what} {k}: missing"
        g, r, b = np.asarray(g), np.asarray(ref[k]), factor * bnd[k]
        assert g.shape == r.shape, f"{what} {k}: shape {g.shape} != {r.shape}"
        fin = np.isfinite(r)
        np.testing.assert_array_equal(np.isnan(g), np.isnan(r), err_msg=f"{what} {k}: NaN pattern")
        np.testing.assert_array_equal(g[~fin & ~np.isnan(r)], r[~fin & ~np.isnan(r)], err_msg=f"{what} {k}: infinities")
        err = np.abs(g[fin] - r[fin])
        if report is not None:
            with np.errstate(all="ignore"):
                report[k] = max(report.get(k, 0.0), float(np.max(err / np.maximum(b[fin], 1e-300), initial=0.0)))
        worst = int(np.argmax(err - b[fin])) if err.size else 0
        assert np.all(err <= b[fin]), (f"{what} {k}: |got - ref| = {err[worst]:.3e} > bound {b[fin][worst]:.3e} "
                                       f"(got {g[fin][worst]!r}, ref {r[fin][worst]!r})")
        if close is not None and err.size:
            close(g[fin], r[fin], rtol=0.0, atol=float(np.max(b[fin])), what=f"predict {k}")
    if "n_inf_i" in ref:
        np.testing.assert_array_equal(got.n_inf_i, ref["n_inf_i"], err_msg=f"{what} n_inf_i")


def assert_loglik(got, T, close=None, what=""):
    """The matrix against the terms: the same -inf pattern, |got - ll| <= e_ll elsewhere."""
    ll, e = T["ll"], T["e_ll"]
    fin = np.isfinite(ll)
    np.testing.assert_array_equal(got[~fin], ll[~fin], err_msg=f"{what}: non-finite pattern")
    err = np.abs(got[fin] - ll[fin])
    assert np.all(np.isfinite(got[fin])), f"{what}: non-finite where the reference is finite"
    worst = int(np.argmax(err - e[fin])) if err.size else 0
    assert np.all(err <= e[fin]), f"{what}: |got - ref| = {err[worst]:.3e} > bound {e[fin][worst]:.3e}"
    if close is not None and err.size:
        close(got[fin], ll[fin], rtol=0.0, atol=float(np.max(e[fin])), what="predict_loglik")


def numpy_partials(T, logw=None, kind="glm", K=0):
    """A partials block [1 + m][Q] from the per-pair arrays, by the documented layout (include/smcnuts_hip.h)."""
    from smcnuts_amd import predict as P
    ll = T["ll"]
    M, m = ll.shape
    lw = np.zeros(M) if logw is None else np.asarray(logw, dtype=np.float64)
    Q = P.n_cols(kind, K)
    out = np.zeros((1 + m, Q))
    keep = np.isfinite(lw)
    out[1:, MA] = -np.inf
    if kind == "glm":
        out[1:, C0] = np.nan
    if not np.any(keep):
        out[0, 0] = -np.inf
        return out
    mw = np.max(lw[keep])
    l = lw[keep] - mw
    w = np.exp(l)
    out[0, :4] = mw, np.sum(w), np.sum(w * w), np.sum(keep)
    llk = ll[keep]
    with np.errstate(all="ignore"):
        for i in range(m):
            col, r = llk[:, i], out[1 + i]
            fin = np.isfinite(col)
            r[NINF] = np.sum(~fin)
            if np.any(fin):
                a = l[fin] + col[fin]
                r[MA] = np.max(a)
                r[SA] = np.sum(np.exp(a - r[MA]))
            if kind == "glm":
                mu, va = T["mean"][keep][:, i], T["var"][keep][:, i]
                ok = np.isfinite(mu) & np.isfinite(va)
                r[NBAD] = np.sum(~ok)
                if np.any(ok):
                    r[C0] = mu[ok][0]
                    d = mu[ok] - r[C0]
                    r[SW], r[S1], r[S2] = np.sum(w[ok]), np.sum(w[ok] * d), np.sum(w[ok] * d * d)
                    r[VAR] = np.sum(w[ok] * va[ok])
            else:
                ok = np.ones(l.shape[0], dtype=bool)
                if "em" in T:
                    ok &= np.isfinite(T["em"][keep][:, i])
                if "prob" in T:
                    ok &= np.all(np.isfinite(T["prob"][keep][:, i, :]), axis=1)
                r[NBAD] = np.sum(~ok)
                if kind == "ord":
                    r[P.ORD_EM] = np.sum(w[ok] * T["em"][keep][ok, i])
                if "prob" in T:
                    p0 = P.CAT_P0 if kind == "cat" else P.ORD_P0
                    r[p0:p0 + K] = np.sum(w[ok, None] * T["prob"][keep][ok, i, :], axis=0)
    return out
