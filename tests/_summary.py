"""Exact reference of the posterior summaries (smcnuts_amd/summary.py) and their two acceptance rules.

Definition: Q(p) = min{v_j : sum_{v_i <= v_j} w_i >= p W}, F(t) = sum_{v_i <= t} w_i / W, with w_i = exp(logw_i - max)
as DOUBLES and every sum of them exact.  The doubles are dyadic rationals, so the Fractions of the definition are kept
as Python integers over one common power-of-two denominator (the same exact arithmetic, a thousand times faster); the
threshold test cum_j >= p W is the integer test cum_j * den(p) >= num(p) * W with Fraction(p) = num / den.

TOL(N) = (N + 16) * 4 * 2^-53 of the total mass (the bound tests/test_gpu_pointwise.py uses for the ESS of the same
weights): a few u per weight from the device's rounded exponential (the argument's rounding u |a| is weighted by e^-a,
so stays below u), at most 2 N u from the fixed-point unit of 2^-52 (rounding, and one unit at least for a positive
weight), and this reference's own rounded exp.

Rank window (always): a returned q for probability p is bit for bit one of the column's values, W_<(q) <= (p + TOL) W
and W_<=(q) >= (p - TOL) W.  Exact: where the reference's own choice has a margin -- the smaller of |W_<(q_ref) - p W| and
|W_<=(q_ref) - p W|, over W -- above 2 TOL, the device must return q_ref itself; `check(..., exact=True)` ASSERTS that
margin (the cases are chosen so that it holds) and then equality.  With EQUAL weights the margin is not the measure
(0.025 * 1000 lies 1e-18 above an integer for every seed): all fixed-point weights are then one and the same integer,
the selection is the order statistic sort(v)[ceil(p M) - 1] in exact arithmetic, and that is asserted instead."""
import itertools
import math
from fractions import Fraction

import numpy as np

from _tol import close

U = 2.0 ** -53
DEFAULT = (0.025, 0.25, 0.5, 0.75, 0.975)


def TOL(N):
    return (N + 16) * 4 * U


def weights(logw, M):
    """exp(logw - max) as doubles (ones for None; zeros if no log-weight is finite)."""
    if logw is None:
        return np.ones(M)
    logw = np.asarray(logw, dtype=np.float64)
    fin = np.isfinite(logw)
    if not fin.any():
        return np.zeros(M)
    with np.errstate(all="ignore"):
        return np.where(fin, np.exp(logw - np.max(logw[fin])), 0.0)


def exact_ints(w):
    """The doubles w >= 0 as Python integers over one common power-of-two denominator."""
    m, e = np.frexp(w)
    mi = (m * 2.0 ** 53).astype(np.int64)
    pos = w > 0
    if not pos.any():
        return [0] * len(w)
    emin = int(e[pos].min())
    return [(int(a) << (int(b) - emin)) if p else 0 for a, b, p in zip(mi, e, pos)]


class Column:
    """One coordinate: values v [M] with the exact weights wi (exact_ints)."""

    def __init__(self, v, wi):
        v = np.asarray(v, dtype=np.float64)
        keep = np.array([a > 0 for a in wi], dtype=bool)
        self.nan = bool(np.any(np.isnan(v[keep])))
        self.empty = not keep.any()
        if self.nan or self.empty:
            return
        vk = v[keep] + 0.0                                  # (-0.0 and +0.0 are equal)
        order = np.argsort(vk, kind="stable")
        self.sv = vk[order]
        wk = [a for a, k in zip(wi, keep) if k]
        self.cum = list(itertools.accumulate(wk[i] for i in order))
        self.W = self.cum[-1]

    def mass_lt(self, t):
        j = int(np.searchsorted(self.sv, t, side="left"))
        return self.cum[j - 1] if j else 0

    def mass_le(self, t):
        j = int(np.searchsorted(self.sv, t, side="right"))
        return self.cum[j - 1] if j else 0

    def quantile(self, p):
        """(Q(p), margin of the choice as a fraction of W)."""
        num, den = Fraction(float(p)).as_integer_ratio()
        need = num * self.W                                 # cum_j * den >= need
        lo, hi = 0, len(self.cum) - 1
        while lo < hi:
            mid = (lo + hi) // 2
            if self.cum[mid] * den >= need:
                hi = mid
            else:
                lo = mid + 1
        q = self.sv[lo]
        below, upto = self.mass_lt(q), self.mass_le(q)
        margin = min(abs(Fraction(below * den - need, den * self.W)), abs(Fraction(upto * den - need, den * self.W)))
        return q, float(margin)

    def cdf(self, t):
        return float(Fraction(self.mass_le(t), self.W))


def columns(v, logw):
    v = np.atleast_2d(np.asarray(v, dtype=np.float64))
    wi = exact_ints(weights(logw, v.shape[0]))
    return [Column(v[:, c], wi) for c in range(v.shape[1])]


def quantiles(v, logw, probs):
    """[Dc][nq] reference quantiles (NaN columns as the definition says)."""
    out = np.full((np.atleast_2d(v).shape[1], len(probs)), np.nan)
    for c, col in enumerate(columns(v, logw)):
        if not (col.nan or col.empty):
            out[c] = [col.quantile(p)[0] for p in probs]
    return out


def check(got_q, v, logw, probs, exact, what, got_cdf=None, at=None, n_total=None, cols=None):
    """Both acceptance rules for quantiles [Dc][nq] of the constrained values v [M][Dc]; tail masses within TOL.
    cols: columns(v, logw) where a caller checks several results against one population."""
    v = np.atleast_2d(np.asarray(v, dtype=np.float64))
    M, Dc = v.shape
    tol = TOL(M if n_total is None else n_total)
    assert got_q.shape == (Dc, len(probs)), what
    worst = 0.0
    cdf_err = 0.0
    for c, col in enumerate(columns(v, logw) if cols is None else cols):
        if col.nan or col.empty:
            assert np.all(np.isnan(got_q[c])), f"{what}: column {c} must be NaN"
            if got_cdf is not None:
                assert np.all(np.isnan(got_cdf[c])), f"{what}: cdf of column {c} must be NaN"
            continue
        members = set(v[:, c].view(np.uint64).tolist())
        for j, p in enumerate(probs):
            q = got_q[c, j]
            assert int(np.float64(q).view(np.uint64)) in members, f"{what}: column {c} p={p}: {q!r} is not a particle's value"
            lt, le = float(Fraction(col.mass_lt(q), col.W)), float(Fraction(col.mass_le(q), col.W))
            assert lt <= p + tol, f"{what}: column {c} p={p}: mass below {q!r} is {lt!r}"
            assert le >= p - tol, f"{what}: column {c} p={p}: mass up to {q!r} is {le!r}"
            worst = max(worst, (lt - p) / tol, (p - le) / tol)
            if exact:
                ref, margin = col.quantile(p)
                if logw is None:
                    # equal weights: every fixed-point weight is the SAME integer f, so the device's test
                    # (j + 1) f >= ceil(p M f) is j + 1 >= p M exactly -- the order statistic, whatever the margin
                    # (p M within an ulp of an integer, as 0.025 * 1000, leaves no margin and no ambiguity)
                    k = math.ceil(Fraction(float(p)) * M)
                    assert ref == np.sort(v[:, c] + 0.0)[k - 1], f"{what}: column {c} p={p}: reference vs order statistic"
                else:
                    assert margin > 2.0 * tol, (f"{what}: column {c} p={p}: the reference's margin {margin:.3e} <= 2 TOL "
                                                f"{2 * tol:.3e}")
                assert q == ref, f"{what}: column {c} p={p}: {q!r}, reference {ref!r}"
        if got_cdf is not None:
            for j in range(at.shape[1]):
                cdf_err = max(cdf_err, abs(got_cdf[c, j] - col.cdf(at[c, j])))
    # the share of TOL the rank window used (<= 0: the window held without it), and the tail masses' error
    close(max(worst, 0.0) * tol, 0.0, rtol=0.0, atol=tol, what="summary: rank window, excess over p as a share of TOL")
    if got_cdf is not None:
        close(cdf_err, 0.0, rtol=0.0, atol=tol, what="summary: tail masses")
    return worst


def dup_values(rng, M, D):
    """[M][D] standard normal rows, half of them copies of other rows (as after resampling)."""
    x = rng.standard_normal((M, D))
    if M > 1:
        src = rng.integers(0, M, M // 2)
        dst = rng.permutation(M)[:M // 2]
        x[dst] = x[src]
    return x
