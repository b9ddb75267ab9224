"""Posterior covariance and correlation of the constrained parameters, summed on the device (fp64 MFMA).

Definition (include/smcnuts_hip.h): over the particles with a finite log-weight, w_p = exp(lw_p - mw), W = sum w_p,
m_i = sum w_p v_ip / W and C_ij = sum w_p (v_ip - m_i)(v_jp - m_j) / W -- weights normalised to one, no small-sample
correction, so diag(C) is the variance estimate.  R_ij = C_ij / sqrt(C_ii C_jj), clipped to [-1, 1], its diagonal exactly 1
where C_ii > 0 and row and column i NaN where C_ii == 0.  The device returns the augmented sums [[G, S1], [S1', W]] about
a centre c near the mean (smcn_cov_partials); partials of disjoint particle sets with the same centre and maximum add, and
the host finishes: d = S1 / W, C = G / W - d d', m = c + d.  sum w v v' - m m' is never formed."""
import math

import numpy as np


def combine_cov_partials(parts, centre):
    """parts: the shards' augmented sums [Dc+1][Dc+1] about the same `centre` [Dc] and the same log-weight maximum, added
    in the order given (rank order).  Returns (mean [Dc], cov [Dc][Dc], corr [Dc][Dc], W).  No weight: NaN everywhere;
    a non-finite sum in coordinate i: row and column i of cov and corr, and mean[i], NaN and nothing else."""
    centre = np.asarray(centre, dtype=np.float64)
    Dc = centre.size
    parts = [np.asarray(p, dtype=np.float64) for p in parts]
    if not parts or any(p.shape != (Dc + 1, Dc + 1) for p in parts):
        raise ValueError(f"every partial must be [{Dc + 1}][{Dc + 1}] (the centre holds {Dc} values)")
    A = parts[0].copy()
    for p in parts[1:]:
        A = A + p
    A = np.triu(A) + np.triu(A, 1).T         # the upper triangle is the result (the device's partials are symmetric already)
    W = float(A[Dc, Dc])
    nan = np.full(Dc, np.nan)
    if not W > 0.0:
        return nan, np.full((Dc, Dc), np.nan), np.full((Dc, Dc), np.nan), 0.0
    with np.errstate(all="ignore"):
        G, S1 = A[:Dc, :Dc], A[Dc, :Dc]
        d = S1 / W
        cov = G / W - np.outer(d, d)
        mean = centre + d
        bad = ~(np.isfinite(S1) & np.isfinite(np.diagonal(G)) & np.isfinite(centre))
        i = np.arange(Dc)
        cov[i, i] = np.maximum(cov[i, i], 0.0)
        cov[bad, :] = np.nan
        cov[:, bad] = np.nan
        mean = np.where(bad, np.nan, mean)
        sd = np.sqrt(np.diagonal(cov))
        corr = np.clip(cov / np.outer(sd, sd), -1.0, 1.0)
        flat = ~(sd > 0.0)                       # C_ii == 0 (or NaN)
        corr[i, i] = 1.0
        corr[flat, :] = np.nan
        corr[:, flat] = np.nan
    return mean, cov, corr, W


class PosteriorCovariance:
    """names [Dc]; mean, sd [Dc]; cov, corr [Dc][Dc]; ess (Kish, of the weights); n_particles; centre [Dc]: the point the
    device summed about (None where unknown) -- the rounding error of cov scales with the second moment about it."""

    def __init__(self, names, mean, cov, corr, ess, n_particles, centre=None):
        self.names = list(names)
        self.mean = np.asarray(mean, dtype=np.float64)
        self.cov, self.corr = np.asarray(cov, dtype=np.float64), np.asarray(corr, dtype=np.float64)
        Dc = self.mean.size
        if self.cov.shape != (Dc, Dc) or self.corr.shape != (Dc, Dc) or len(self.names) != Dc:
            raise ValueError(f"PosteriorCovariance: {Dc} means need {Dc} names and [{Dc}][{Dc}] matrices")
        with np.errstate(invalid="ignore"):
            self.sd = np.sqrt(np.diagonal(self.cov))
        self.ess, self.n_particles = float(ess), int(n_particles)
        self.centre = None if centre is None else np.asarray(centre, dtype=np.float64)

    def contrast(self, a):
        """Posterior mean a'm and sd sqrt(a'Ca) of a linear combination: (float, float) for a vector [Dc], two arrays
        [k] for a matrix [k, Dc] of contrasts."""
        try:
            a = np.asarray(a, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("contrast: a must be numbers") from None
        Dc = self.mean.size
        if a.ndim not in (1, 2) or a.shape[-1] != Dc:
            raise ValueError(f"contrast: a must be [{Dc}] or [k, {Dc}], not shape {a.shape}")
        a2 = np.atleast_2d(a)
        with np.errstate(invalid="ignore"):
            m = a2 @ self.mean
            q = np.einsum("ki,ij,kj->k", a2, self.cov, a2)
            s = np.sqrt(np.maximum(q, 0.0))
        return (float(m[0]), float(s[0])) if a.ndim == 1 else (m, s)

    def pairs(self, min_abs_corr=0.0):
        """[(name_i, name_j, r)] of the pairs i < j with |r| >= min_abs_corr, the largest |r| first (NaN pairs left out)."""
        t = float(min_abs_corr)
        if not 0.0 <= t <= 1.0:
            raise ValueError("pairs: min_abs_corr must lie in [0, 1]")
        i, j = np.triu_indices(self.mean.size, 1)
        r = self.corr[i, j]
        with np.errstate(invalid="ignore"):
            keep = np.abs(r) >= t
        i, j, r = i[keep], j[keep], r[keep]
        order = np.argsort(-np.abs(r), kind="stable")
        return [(self.names[i[k]], self.names[j[k]], float(r[k])) for k in order]

    def __str__(self):
        w = max([len(n) for n in self.names] + [4])
        lines = [" " * w + f"{'mean':>12}{'sd':>12}"]
        for i, n in enumerate(self.names):
            lines.append(f"{n:<{w}}{self.mean[i]:>12.4g}{self.sd[i]:>12.4g}")
        Dc = self.mean.size
        if Dc <= 8:
            lines.append("correlation")
            lines.append(" " * w + "".join(f"{n[:9]:>10}" for n in self.names))
            for i, n in enumerate(self.names):
                lines.append(f"{n:<{w}}" + "".join(f"{self.corr[i, j]:>10.3f}" for j in range(Dc)))
        else:
            top = self.pairs()[:10]
            lines.append(f"largest correlations of {Dc * (Dc - 1) // 2} pairs")
            lines += [f"  {a} ~ {b}: {r:+.3f}" for a, b, r in top]
        lines.append(f"{self.n_particles} particles, ESS {self.ess:.1f}")
        return "\n".join(lines)

    __repr__ = __str__


def check_centre(centre, Dc):
    if centre is None:
        return None
    try:
        c = np.asarray(centre, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("centre must be numbers") from None
    if c.shape != (Dc,):
        raise ValueError(f"centre must hold {Dc} values, not shape {c.shape}")
    return np.ascontiguousarray(c)


def device_covariance(ctx, comm, centre=None, x=None, logw=None, v=None, slices=0):
    """(mean, cov, corr, ess, centre used) of a staged population: the resident particles, x through the device's
    constrain path, or v already constrained.  Several shards: one all-gather of the weights' headers, one of
    (W_r, mean_r) where the caller gives no centre, one of the partials; every rank returns the same bits."""
    world = 1 if comm is None else comm.world_size
    head, Dc = ctx.summary_begin(x, logw, v)
    centre = check_centre(centre, Dc)
    heads = np.asarray(comm.allgather(head)) if world > 1 else head[None, :]
    live = heads[:, 3] > 0
    if not live.any():          # no particle of positive weight anywhere
        nan = np.full((Dc, Dc), np.nan)
        return np.full(Dc, np.nan), nan, nan.copy(), 0.0, (np.zeros(Dc) if centre is None else centre)
    gmax = float(np.max(heads[live, 0]))
    gsum = gsum2 = 0.0
    Wr = np.zeros(world)
    for r in range(world):      # in rank order: the same bits on every rank
        if live[r]:
            s = math.exp(heads[r, 0] - gmax)
            Wr[r] = heads[r, 1] * s
            gsum += Wr[r]
            gsum2 += heads[r, 2] * s * s
    ess = gsum * gsum / gsum2
    if centre is None and world > 1:
        means = np.asarray(comm.allgather(ctx.cov_centre(gmax, Dc)))
        acc = np.zeros(Dc)
        with np.errstate(all="ignore"):
            for r in range(world):
                if Wr[r] > 0.0:
                    acc = acc + Wr[r] * means[r]
            centre = np.ascontiguousarray(acc / gsum)
    aug, used = ctx.cov_partials(gmax, Dc, centre, slices)
    parts = list(np.asarray(comm.allgather(aug))) if world > 1 else [aug]
    mean, cov, corr, _ = combine_cov_partials(parts, used)
    return mean, cov, corr, ess, used


def target_covariance(target, ctx, x, logw, v=None):
    """covariance() of a target at caller-supplied points: x through the device's constrain path, or v already
    constrained."""
    Dc = int(getattr(target, "constrained_dim", target.dim))
    mean, cov, corr, ess, used = device_covariance(ctx, None, x=None if v is not None else x, logw=logw, v=v)
    names = list(target.param_names())
    if len(names) != Dc:
        names = [f"x.{i + 1}" for i in range(Dc)]
    return PosteriorCovariance(names, mean, cov, corr, ess, np.atleast_2d(x).shape[0], centre=used)
