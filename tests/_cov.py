"""Reference of the posterior covariance (smcnuts_amd/covariance.py) and its per-entry bound.

Definition: w_p = exp(lw_p - max) as DOUBLES (zero for a non-finite log-weight), W = sum w_p, m_i = sum w_p v_ip / W,
C_ij = sum w_p (v_ip - m_i)(v_jp - m_j) / W over the particles with w_p > 0.

`exact`: rational arithmetic (fractions) over the doubles w_p and v_p -- small cases.
`reference`: the float64 restatement, every entry's sum with math.fsum (an exactly rounded sum of the rounded terms),
about the rounded mean m~ and corrected for it: C_ij = sum w a_i a_j / W - e_i e_j with a = v - m~ and e = sum w a / W
(m~ is off by up to half an ulp of |m|, and e_i e_j is that offset's square: 1e-16 where v is near 1e8).
Past FSUM_TERMS terms in all (Dc = 256 at M = 4097 is 135 million, a minute of Python floats) the terms are formed and
summed in the platform's extended precision instead where it has one (x87, u = 2^-64: each term carries 2^-64 where the
fsum route carries 2^-53, and a pairwise sum of S terms adds log2(S) 2^-64); test_cov_host.py holds both routes against
the exact one and against each other.

Bound (derived, not tuned).  Every term w a_i a_j carries a few roundings and the weight's few ulp (the device's
exponential against NumPy's); a sum of S terms in any order errs by at most S u sum |terms|.  By Cauchy-Schwarz
sum w |a_i| |a_j| / W <= sqrt(C'_ii C'_jj) with C'_ii = C_ii + d_i^2 the second moment about the centre c the device
actually used (d = m - c).  So |C^_ij - C_ij| <= TOL(S) sqrt(C'_ii C'_jj), TOL(S) = 4 (S + 16) u -- tests/_summary.py's
bound for masses -- and |m^_i - m_i| <= TOL(S) sum w |v_i| / W.  S: the particles with a finite log-weight."""
import math
from fractions import Fraction

import numpy as np

import _summary as S
from _tol import close

U = 2.0 ** -53
FSUM_TERMS = 4_000_000
LD = np.longdouble
HAVE_LD = np.finfo(LD).eps <= 2.0 ** -63


def TOL(n):
    return 4.0 * (n + 16) * U


def weights(logw, M):
    return S.weights(logw, M)


def contributing(logw, M):
    return M if logw is None else int(np.isfinite(np.asarray(logw, dtype=np.float64)).sum())


def exact(v, w):
    """(mean [Dc], cov [Dc][Dc]) as Fractions (lists) of the doubles v [M][Dc], w [M]; rows of zero weight left out."""
    v = np.atleast_2d(np.asarray(v, dtype=np.float64))
    keep = np.flatnonzero(np.asarray(w) > 0)
    Dc = v.shape[1]
    ws = [Fraction(float(w[p])) for p in keep]
    W = sum(ws)
    cols = [[Fraction(float(v[p, i])) for p in keep] for i in range(Dc)]
    mean = [sum(a * b for a, b in zip(ws, col)) / W for col in cols]
    cov = [[None] * Dc for _ in range(Dc)]
    for i in range(Dc):
        wi = [a * b for a, b in zip(ws, cols[i])]
        for j in range(i, Dc):
            cov[i][j] = cov[j][i] = sum(a * b for a, b in zip(wi, cols[j])) / W - mean[i] * mean[j]
    return mean, cov


def exact_floats(v, w):
    m, c = exact(v, w)
    return np.array([float(a) for a in m]), np.array([[float(a) for a in row] for row in c])


def reference(v, w, route=None):
    """(mean, cov, absmean) in float64: absmean_i = sum w |v_i| / W (the mean's bound).  route: "fsum", "ld" or None
    (by size)."""
    v = np.atleast_2d(np.asarray(v, dtype=np.float64))
    keep = np.asarray(w) > 0
    vv, ww = v[keep], np.asarray(w, dtype=np.float64)[keep]
    n, Dc = vv.shape
    if route is None:
        route = "ld" if (HAVE_LD and n * Dc * (Dc + 1) // 2 > FSUM_TERMS) else "fsum"
    if route == "ld":
        wl, vl = ww.astype(LD), vv.astype(LD)
        W = wl.sum()
        mean = (wl[:, None] * vl).sum(axis=0) / W
        a = vl - mean
        wa = wl[:, None] * a
        e = wa.sum(axis=0) / W
        cov = np.empty((Dc, Dc))
        for i in range(Dc):
            row = (wa[:, i:i + 1] * a[:, i:]).sum(axis=0) / W - e[i] * e[i:]
            cov[i, i:] = cov[i:, i] = row.astype(np.float64)
        absmean = ((wl[:, None] * np.abs(vl)).sum(axis=0) / W).astype(np.float64)
        return mean.astype(np.float64), cov, absmean
    W = math.fsum(ww)
    mean = np.array([math.fsum(ww * vv[:, i]) / W for i in range(Dc)])
    a = vv - mean
    wa = ww[:, None] * a
    e = np.array([math.fsum(wa[:, i]) / W for i in range(Dc)])
    cov = np.empty((Dc, Dc))
    for i in range(Dc):
        for j in range(i, Dc):
            cov[i, j] = cov[j, i] = math.fsum(wa[:, i] * a[:, j]) / W - e[i] * e[j]
    absmean = np.array([math.fsum(ww * np.abs(vv[:, i])) / W for i in range(Dc)])
    return mean, cov, absmean


def bounds(mean, cov, absmean, centre, n):
    """(bound of the mean [Dc], bound of cov [Dc][Dc]) about the centre the device used."""
    d = mean - np.asarray(centre, dtype=np.float64)
    second = np.maximum(np.diagonal(cov), 0.0) + d * d
    return TOL(n) * absmean, TOL(n) * np.sqrt(np.outer(second, second))


def share(got, want, bound):
    """|got - want| / bound per entry; 0 where both the error and the bound are 0, inf where only the bound is."""
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    with np.errstate(all="ignore"):
        return np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))


def check(mean, cov, v, logw, centre, what, ref=None, n=None):
    """The device's (mean, cov) of the values v [M][Dc] against the reference inside the bound, element by element
    (recorded as the share of the bound used).  ref: reference(v, weights) where a caller shares it.  Returns it."""
    v = np.atleast_2d(np.asarray(v, dtype=np.float64))
    M, Dc = v.shape
    if ref is None:
        ref = reference(v, weights(logw, M))
    rm, rc, ram = ref
    bm, bc = bounds(rm, rc, ram, centre, contributing(logw, M) if n is None else n)
    assert mean.shape == (Dc,) and cov.shape == (Dc, Dc), what
    assert np.all(np.isfinite(mean)) and np.all(np.isfinite(cov)), f"{what}: non-finite result"
    close(share(mean, rm, bm), 0.0, rtol=0.0, atol=1.0, err_msg=what, what="covariance: mean, share of TOL(S) sum w|v| / W")
    close(share(cov, rc, bc), 0.0, rtol=0.0, atol=1.0, err_msg=what,
          what="covariance: entries, share of TOL(S) sqrt(C'_ii C'_jj)")
    return ref


def check_corr(corr, cov, what):
    """corr is cov scaled: symmetric bit for bit, in [-1, 1], diagonal exactly 1 where C_ii > 0, NaN rows where C_ii == 0."""
    assert corr.tobytes() == corr.T.copy().tobytes(), f"{what}: corr not symmetric"
    pos = np.diagonal(cov) > 0
    assert np.all(np.diagonal(corr)[pos] == 1.0), f"{what}: diagonal of corr"
    assert np.all(np.isnan(corr[~pos])) and np.all(np.isnan(corr[:, ~pos])), f"{what}: flat rows of corr must be NaN"
    inner = corr[np.ix_(pos, pos)]
    assert np.all((inner >= -1.0) & (inner <= 1.0)), f"{what}: corr outside [-1, 1]"
    sd = np.sqrt(np.diagonal(cov)[pos])
    with np.errstate(all="ignore"):
        want = np.clip(cov[np.ix_(pos, pos)] / np.outer(sd, sd), -1.0, 1.0)
    off = ~np.eye(int(pos.sum()), dtype=bool)
    np.testing.assert_array_equal(inner[off], want[off], err_msg=f"{what}: corr is not cov scaled")


def population(Dc, M, weighted, seed=0):
    """[M][Dc] values (column c about loc_c, with scale and correlation differing by column) and log-weights 3 N(0, 1)."""
    rng = np.random.default_rng(100000 * seed + 1000 * Dc + M)
    z = rng.standard_normal((M, Dc))
    common = rng.standard_normal((M, 1))
    scale = np.exp(np.linspace(-1.0, 1.0, Dc))
    x = np.linspace(-2.0, 2.0, Dc)[None, :] + scale * (0.8 * z + 0.6 * np.sin(np.arange(Dc))[None, :] * common)
    lw = 3.0 * rng.standard_normal(M)
    return x, (lw if weighted else None)


def int_population(Dc, M, seed=0):
    """Integer values |v| <= 8 without any symmetry between the rows, log-weights in {0, -inf} (at least one 0)."""
    rng = np.random.default_rng(7000 * seed + 100 * Dc + M)
    v = rng.integers(-8, 9, (M, Dc)).astype(np.float64)
    lw = np.where(rng.random(M) < 0.7, 0.0, -np.inf)
    lw[rng.integers(0, M)] = 0.0
    return v, lw


def int_gram(v, lw):
    """The augmented integer matrix [[v'v, sum v], [sum v', count]] over the rows with lw == 0."""
    k = v[np.isfinite(lw)]
    a = np.concatenate([k, np.ones((k.shape[0], 1))], axis=1)
    return a.T @ a                       # small integers: exact in float64


def numpy_partial(v, w, centre):
    """The augmented sums about `centre` as NumPy forms them (test_cov_host.py's shards)."""
    keep = np.asarray(w) > 0
    a = np.concatenate([v[keep] - centre, np.ones((int(keep.sum()), 1))], axis=1)
    return (a * np.asarray(w)[keep][:, None]).T @ a
