"""Posterior summaries: weighted quantiles and tail masses of the constrained parameters, selected on the device.

Definition (include/smcnuts_hip.h): for a constrained coordinate with values v_i and weights w_i >= 0 of total W,
Q(p) = min{v_j : sum_{v_i <= v_j} w_i >= p W} -- NumPy's quantile(..., method="inverted_cdf", weights=w) -- and
F(t) = sum_{v_i <= t} w_i / W.  The device counts masses as integers (units of 2^-52 of the total), so a summary depends
on the multiset of (value, weight) pairs alone, not on the order of the particles; every shard returns the same bits."""
import math
from fractions import Fraction

import numpy as np

MAX_PROBS = 16
DEFAULT_PROBS = (0.025, 0.25, 0.5, 0.75, 0.975)


def key_of(v):
    """The order-preserving 64-bit key of a double the selection kernels use (as a Python int): the sign bit of a
    non-negative value is flipped, every bit of a negative value inverted."""
    b = int(np.float64(v).view(np.uint64))
    return (~b) & (2 ** 64 - 1) if b >> 63 else b ^ (1 << 63)


def check_probs(probs):
    """probs as a 1-D array of 1 .. 16 probabilities in (0, 1]; ValueError otherwise."""
    try:
        p = np.atleast_1d(np.asarray(probs, dtype=np.float64))
    except (TypeError, ValueError):
        raise ValueError("probs must be numbers in (0, 1]") from None
    if p.ndim != 1 or p.size < 1:
        raise ValueError("probs must be a non-empty 1-D sequence of probabilities")
    if p.size > MAX_PROBS:
        raise ValueError(f"probs: at most {MAX_PROBS} probabilities per call, not {p.size}")
    if np.any(np.isnan(p)):
        raise ValueError("probs must not hold NaN")
    if np.any(p <= 0.0) or np.any(p > 1.0):
        raise ValueError("probs must lie in (0, 1]")
    return p


def check_at(at, Dc):
    """Thresholds of the tail masses as [Dc][T]: a scalar or a 1-D sequence of T <= 16 values applies to every coordinate, a
    2-D array gives each coordinate its own row.  None stays None; ValueError for any other shape."""
    if at is None:
        return None
    try:
        a = np.asarray(at, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("at must be a number or an array of thresholds") from None
    if a.ndim == 0:
        a = a.reshape(1)
    if a.ndim == 1:
        a = np.broadcast_to(a, (Dc, a.size))
    if a.ndim != 2 or a.shape[0] != Dc or not 1 <= a.shape[1] <= MAX_PROBS:
        raise ValueError(f"at must be a scalar, [T] or [{Dc}][T] with 1 <= T <= {MAX_PROBS}; got shape {np.shape(at)}")
    return np.ascontiguousarray(a)


def check_logw(logw, M):
    if logw is None:
        return None
    lw = np.asarray(logw, dtype=np.float64)
    if lw.shape != (M,):
        raise ValueError("logw must hold one log-weight per row of x")
    if np.any(np.isnan(lw)) or np.any(lw == np.inf):
        raise ValueError("logw must not hold NaN or +inf")
    return np.ascontiguousarray(lw)


class PosteriorSummary:
    """names [Dc]; mean, sd [Dc]; probs [nq]; quantiles [Dc][nq]; cdf [Dc][T] (the posterior mass at or below at[c][j]) or
    None, with at [Dc][T] or None; ess (Kish, of the weights); n_particles."""

    def __init__(self, names, mean, sd, probs, quantiles, cdf, at, ess, n_particles):
        self.names = list(names)
        self.mean, self.sd = np.asarray(mean, dtype=np.float64), np.asarray(sd, dtype=np.float64)
        self.probs = np.asarray(probs, dtype=np.float64)
        self.quantiles = np.asarray(quantiles, dtype=np.float64)
        self.cdf, self.at = cdf, at
        self.ess, self.n_particles = float(ess), int(n_particles)

    def quantile(self, p):
        """The column of a requested probability."""
        hit = np.flatnonzero(self.probs == float(p))
        if hit.size == 0:
            raise ValueError(f"probability {p} was not requested: summary(probs=...) had {tuple(self.probs)}")
        return self.quantiles[:, hit[0]]

    def interval(self, level):
        """The equal-tailed credible interval [Dc][2] of a level in (0, 1), from the requested probabilities."""
        level = float(level)
        if not 0.0 < level < 1.0:
            raise ValueError("level must lie in (0, 1)")
        lo, hi = (1.0 - level) / 2.0, 1.0 - (1.0 - level) / 2.0
        tol = 4.0 * np.finfo(np.float64).eps
        a, b = np.flatnonzero(np.abs(self.probs - lo) <= tol), np.flatnonzero(np.abs(self.probs - hi) <= tol)
        if a.size == 0 or b.size == 0:
            raise ValueError(f"interval({level:g}) needs the probabilities {lo:g} and {hi:g}: "
                             f"request summary(probs=(..., {lo:g}, {hi:g}))")
        return np.stack([self.quantiles[:, a[0]], self.quantiles[:, b[0]]], axis=1)

    def __str__(self):
        heads = ["mean", "sd"] + [f"{100.0 * p:g}%" for p in self.probs]
        cols = [self.mean, self.sd] + [self.quantiles[:, j] for j in range(self.probs.size)]
        if self.cdf is not None:
            for j in range(self.cdf.shape[1]):
                same = np.all(self.at[:, j] == self.at[0, j])
                heads.append(f"P(<={self.at[0, j]:g})" if same else f"P(<=at[{j}])")
                cols.append(self.cdf[:, j])
        w = max([len(n) for n in self.names] + [4])
        lines = [" " * w + "".join(f"{h:>12}" for h in heads)]
        for i, n in enumerate(self.names):
            lines.append(f"{n:<{w}}" + "".join(f"{c[i]:>12.4g}" for c in cols))
        lines.append(f"{self.n_particles} particles, ESS {self.ess:.1f}")
        return "\n".join(lines)

    __repr__ = __str__


def thresholds(probs, mass):
    """ceil(p * mass) in exact arithmetic, at least one unit."""
    return [max(1, math.ceil(Fraction(float(p)) * int(mass))) for p in probs]


def pick_digits(hist, thr):
    """hist [Dc][nl][256] integer masses (nl = 1 or nq), thr [Dc][nq]: per (coordinate, probability) the first digit whose
    cumulative mass reaches the threshold, and the threshold less the mass below that digit."""
    cum = np.cumsum(hist, axis=-1)
    cum = np.broadcast_to(cum, (thr.shape[0], thr.shape[1], 256))
    h = np.broadcast_to(hist, cum.shape)
    reach = cum >= thr[:, :, None]
    digit = np.where(reach.any(-1), reach.argmax(-1), 255)
    below = np.take_along_axis(cum - h, digit[:, :, None], axis=-1)[:, :, 0]
    return digit.astype(np.int32), np.maximum(thr - below, 1)


def device_summary(ctx, comm, probs, at, x=None, logw=None, v=None):
    """(quantiles [Dc][nq], cdf [Dc][T] or None, ess) of a staged population; probs and at already checked.  Several
    shards: every pass exchanges the ranks' histograms with one host all-gather and every rank takes the same digits."""
    W = 1 if comm is None else comm.world_size
    order = np.argsort(probs, kind="stable")
    ps = probs[order]
    nq = ps.size
    head, Dc = ctx.summary_begin(x, logw, v)
    heads = np.asarray(comm.allgather(head)) if W > 1 else head[None, :]
    live = heads[:, 3] > 0
    T = 0 if at is None else at.shape[1]
    if not live.any():          # no particle of positive weight anywhere
        return np.full((Dc, nq), np.nan), (None if at is None else np.full((Dc, T), np.nan)), 0.0
    gmax = float(np.max(heads[live, 0]))
    gsum = gsum2 = 0.0
    for r in range(W):          # in rank order: the same bits on every rank
        if live[r]:
            s = math.exp(heads[r, 0] - gmax)
            gsum += heads[r, 1] * s
            gsum2 += heads[r, 2] * s * s
    ess = gsum * gsum / gsum2
    local_mass = ctx.summary_weights(gmax, gsum)
    if W == 1:
        mass = local_mass
        ctx.summary_select(np.array(thresholds(ps, mass), dtype=np.float64))
        q, flags = ctx.summary_values(nq, Dc)
    else:
        thr = flags = None
        for k in range(8):
            got = np.asarray(comm.allgather(ctx.summary_hist(k, nq, Dc)))
            tot = got.astype(np.int64).sum(axis=0)          # integers below 2^53: exact
            hist = tot[:-Dc].reshape(Dc, 1 if k == 0 else nq, 256)
            if k == 0:
                mass = int(hist[0, 0].sum())
                flags = tot[-Dc:].astype(np.float64)
                thr = np.tile(np.array(thresholds(ps, mass), dtype=np.int64), (Dc, 1))
            digit, thr = pick_digits(hist, thr)
            ctx.summary_descend(k, digit, thr.astype(np.float64))
        q, _ = ctx.summary_values(nq, Dc)
    cdf = None
    if at is not None:
        c = ctx.summary_cdf(at)
        if W > 1:
            c = np.asarray(comm.allgather(c)).astype(np.int64).sum(axis=0).astype(np.float64)
        cdf = c[:Dc * T].reshape(Dc, T) / float(mass)
        cdf[c[Dc * T:] != 0.0] = np.nan
    q[flags != 0.0] = np.nan
    out = np.empty_like(q)
    out[:, order] = q
    return out, cdf, ess


def host_moments(v, logw):
    """Weighted mean and standard deviation of the rows of v (the plain two-pass form, on the host)."""
    with np.errstate(all="ignore"):
        if logw is None:
            w = np.full(v.shape[0], 1.0 / v.shape[0])
        else:
            fin = np.isfinite(logw)
            if not fin.any():
                return np.full(v.shape[1], np.nan), np.full(v.shape[1], np.nan)
            w = np.where(fin, np.exp(logw - np.max(logw[fin])), 0.0)
            w = w / w.sum()
        keep = w > 0.0
        vv, ww = v[keep], w[keep]
        mean = ww @ vv
        return mean, np.sqrt(ww @ np.square(vv - mean))


def target_summary(target, ctx, x, logw, probs, at, v=None):
    """summary() of a target at caller-supplied points: x through the device's constrain path, or v already constrained."""
    Dc = int(getattr(target, "constrained_dim", target.dim))
    probs = check_probs(probs)
    at = check_at(at, Dc)
    q, cdf, ess = device_summary(ctx, None, probs, at, x=None if v is not None else x, logw=logw, v=v)
    vals = v if v is not None else target.constrain(x)
    mean, sd = host_moments(np.atleast_2d(vals), logw)
    names = list(target.param_names())
    if len(names) != Dc:
        names = [f"x.{i + 1}" for i in range(Dc)]
    return PosteriorSummary(names, mean, sd, probs, q, cdf, at, ess, np.atleast_2d(vals).shape[0])
