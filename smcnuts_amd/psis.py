"""Pareto-smoothed importance-sampling LOO (PSIS-LOO) from the device's three stages (include/smcnuts_hip.h, smcn_psis_*).

The weighted particles of an SMC run come from a proposal g with W_p proportional to pi(x_p) / g(x_p); the ratio from g to
the leave-one-out posterior of observation i is W_p / p(y_i | x_p).  With lw' = lw - max lw, ll = log p(y_i | x_p) and
lr = lw' - ll over the S contributing particles (finite log-weight), per observation:
  M = min(S // 5, ceil(3 sqrt(S))) candidates; mx = max lr, z = lr - mx, c the (M + 1)-th largest z; the tail is z > c
  (ties at c belong to the body).  Fewer than 5 tail entries: nothing is smoothed, pareto_k = +inf.  Otherwise the
  Zhang-Stephens fit of a generalised Pareto distribution to x = e^c expm1(z - c) gives (k, sigma), and the tail's z are
  replaced by min(log(q_j + e^c), 0), q_j the fitted quantile at (j - 0.5) / T (left as they are if k is not finite).
  elpd_loo_i = log sum r~ p(y_i | x) - log sum r~,  psis_ess_i = (sum r~)^2 / sum r~^2  over body and smoothed tail.
An observation for which some contributing particle has ll = -inf reports pareto_k = +inf, elpd_loo_i = -inf, psis_ess_i =
0, tail_len_i = 0 (criteria.py's rule for elpd_loo_i).  With equal weights this is PSIS-LOO as published (Vehtari, Gelman,
Gabry 2017; Vehtari, Simpson, Gelman, Yao, Gabry 2024); `pareto_k_i` above `k_threshold` marks an estimate not to be relied on.

`merge_candidates` and `merge_body` are the only host arithmetic of a sharded call; everything else runs on the device.
"""
import math

import numpy as np

from .criteria import Pointwise, _merge_lse, _se, combine_pointwise_partials

K, ELPD, ESS, TAIL, CUTOFF, SIGMA = range(6)
MAX_TAIL = 4095          # candidates the device selects per observation, less the cutoff's: S <= 1 863 225


def tail_len(S):
    """M = min(floor(S / 5), ceil(3 sqrt(S))), in integers."""
    S = int(S)
    if S < 1:
        return 0
    return min(S // 5, math.isqrt(9 * S - 1) + 1)


def merge_candidates(cands):
    """The ranks' candidate lists [(lr, ll), ...] (each [n][T_cap], descending, ties in particle order, padded with -inf;
    ranks in order) -> (lr, ll, cutoff): the T_cap largest of the union per observation in the same order, and the cutoff
    on the lr scale -- the largest candidate whose z = lr - mx is at or below c, +inf where the largest is +inf."""
    cands = list(cands)
    if not cands:
        raise ValueError("merge_candidates: no candidates")
    lr = np.concatenate([np.atleast_2d(np.asarray(a, dtype=np.float64)) for a, _ in cands], axis=1)
    ll = np.concatenate([np.atleast_2d(np.asarray(b, dtype=np.float64)) for _, b in cands], axis=1)
    cap = np.atleast_2d(cands[0][0]).shape[1]
    if lr.shape != ll.shape or any(np.atleast_2d(a).shape[1] != cap for a, _ in cands):
        raise ValueError("merge_candidates: every rank's lr and ll are [n][T_cap]")
    order = np.argsort(-lr, axis=1, kind="stable")[:, :cap]
    lr, ll = np.take_along_axis(lr, order, axis=1), np.take_along_axis(ll, order, axis=1)
    return lr, ll, cutoffs(lr)


def cutoffs(lr):
    """Per row of descending candidates [n][T_cap]: the body's upper end on the lr scale (see merge_candidates)."""
    lr = np.asarray(lr, dtype=np.float64)
    mx = lr[:, :1]
    with np.errstate(invalid="ignore"):
        z = lr - mx
        body = z <= z[:, -1:]
        cut = np.max(np.where(body, lr, -np.inf), axis=1)
    return np.where(mx[:, 0] < np.inf, cut, mx[:, 0])


def merge_body(bodies):
    """Body partials [n][4] = (mb, Sb, Sb2, Sw) of disjoint particle sets on one weight scale, merged in list order."""
    bodies = [np.asarray(b, dtype=np.float64) for b in bodies]
    acc = bodies[0].copy()
    for b in bodies[1:]:
        m, s, q = _merge_lse(acc[:, 0], acc[:, 1], b[:, 0], b[:, 1], acc[:, 2], b[:, 2])
        acc = np.stack([m, s, q, acc[:, 3] + b[:, 3]], axis=1)
    return acc


class PsisLoo:
    """PSIS-LOO of one fitted model: per-observation arrays of length n and their totals; `plain` is the criteria.Pointwise
    of the same particles (lppd, WAIC, plain importance-sampling LOO)."""

    def __init__(self, out, plain, n_particles):
        out = np.asarray(out, dtype=np.float64)
        self.pareto_k_i = out[:, K].copy()
        self.elpd_loo_i = out[:, ELPD].copy()
        self.psis_ess_i = out[:, ESS].copy()
        self.tail_len_i = out[:, TAIL].astype(np.int64)
        self.cutoff_i, self.sigma_i = out[:, CUTOFF].copy(), out[:, SIGMA].copy()
        self.plain = plain
        with np.errstate(invalid="ignore"):
            self.p_loo_i = plain.lppd_i - self.elpd_loo_i
        self.n_particles = int(n_particles)
        self.n_obs = int(out.shape[0])

    elpd_loo = property(lambda self: float(np.sum(self.elpd_loo_i)))
    p_loo = property(lambda self: float(np.sum(self.p_loo_i)))
    se_elpd_loo = property(lambda self: _se(self.elpd_loo_i))

    @property
    def k_threshold(self):
        """min(1 - 1 / log10(S), 0.7): the sample-size-specific threshold of Vehtari et al. (2024)."""
        S = self.n_particles
        return min(1.0 - 1.0 / math.log10(S), 0.7) if S > 1 else -math.inf

    @property
    def n_high_k(self):
        return int(np.sum(~(self.pareto_k_i <= self.k_threshold)))

    def summary(self):
        return dict(n_obs=self.n_obs, n_particles=self.n_particles, elpd_loo=self.elpd_loo, se_elpd_loo=self.se_elpd_loo,
                    p_loo=self.p_loo, k_threshold=self.k_threshold, n_high_k=self.n_high_k,
                    max_pareto_k=float(np.max(self.pareto_k_i)), min_psis_ess=float(np.min(self.psis_ess_i)),
                    elpd_loo_plain=self.plain.elpd_loo)


def compare_loo(a, b):
    """a against b on the same observations: the difference of the smoothed elpd_loo totals (a - b) and its paired
    standard error sqrt(n var_i(diff_i, ddof=1)), as criteria.compare."""
    if a.n_obs != b.n_obs:
        raise ValueError(f"compare_loo: the two were computed on different numbers of observations ({a.n_obs} and {b.n_obs})")
    with np.errstate(invalid="ignore"):
        d = a.elpd_loo_i - b.elpd_loo_i
    return dict(elpd_loo_diff=float(np.sum(d)), se_elpd_loo_diff=_se(d), n_obs=a.n_obs,
                n_high_k=(a.n_high_k, b.n_high_k))


def _check_size(S):
    if tail_len(S) > MAX_TAIL:
        raise ValueError(f"loo: {S} contributing particles give a tail of {tail_len(S)} candidates per observation; the "
                         f"device selects at most {MAX_TAIL} (S <= 1863225)")


def loo_from_context(ctx, comm=None, x=None, logw=None):
    """PsisLoo of the context's resident particles (x = None) or of the points x with log-weights logw.  With a
    communicator of several ranks every rank passes its own shard and returns the same object: the partials' headers
    give the global mw and S (one all-gather), the ranks' candidates are merged (one all-gather, merge_candidates), the
    body partials are merged (one all-gather), and every rank runs the fit."""
    part = ctx.pointwise_partials(x, logw)
    if comm is None or comm.world_size == 1:
        plain = combine_pointwise_partials([part])
        if part[0, 3] < 1:
            raise ValueError("loo: no particle with a finite log-weight")
        _check_size(part[0, 3])
        out, head = ctx.psis_loo(x, logw)
        return PsisLoo(out, plain, head[3])
    allp = np.asarray(comm.allgather(part.reshape(-1))).reshape((comm.world_size,) + part.shape)
    plain = combine_pointwise_partials(list(allp))
    cnt = allp[:, 0, 3]
    S = int(np.sum(cnt))
    if S < 1:
        raise ValueError("loo: no particle with a finite log-weight")
    _check_size(S)
    mw = float(np.max(allp[cnt > 0, 0, 0]))
    lr, ll = ctx.psis_candidates(mw, S, x, logw)
    every = np.asarray(comm.allgather(np.concatenate([lr.reshape(-1), ll.reshape(-1)])))
    every = every.reshape((comm.world_size, 2) + lr.shape)
    glr, gll, cut = merge_candidates([(e[0], e[1]) for e in every])
    body = ctx.psis_body(mw, S, cut, x, logw)
    bodies = np.asarray(comm.allgather(body.reshape(-1))).reshape((comm.world_size,) + body.shape)
    out = ctx.psis_fit(glr, gll, merge_body(list(bodies)), mw, S)
    return PsisLoo(out, plain, S)
