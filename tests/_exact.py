"""Exact references for the population reductions (log-sum-exp, ESS, normalised weights, weighted moments) and the
resampling indices, for the GPU tests of tests/test_gpu_reductions.py.

Precision: up to MP_MAX finite terms every quantity is computed with mpmath at 40 digits.  Beyond, in the x87 80-bit
long double (64-bit mantissa, unit roundoff 2^-64): each term is formed from the float64 inputs with one or two
roundings of 2^-64 and the sums of N <= 2^21 same-signed terms carry at most ~log2(N) * 2^-64 -- three orders below the
float64 eps the kernels are measured in.  Where long double is no wider than float64, the sums fall back to math.fsum
(one rounding of the exact sum of the float64 terms).  Every result is rounded to float64 once, at the end.
"""
import math

import numpy as np

try:
    import mpmath
except ImportError:          # pragma: no cover - the long-double / fsum path then covers every size
    mpmath = None

MP_MAX = 10_000
EPS = float(np.finfo(np.float64).eps)
LD = np.longdouble
WIDE_LD = float(np.finfo(LD).eps) < 1e-18


def _finite(logw):
    a = np.asarray(logw, dtype=np.float64)
    if np.any(np.isnan(a)) or np.any(a == np.inf):
        raise ValueError("exact references take finite or -inf log-weights")
    return a, np.isfinite(a)


def _use_mp(n):
    return mpmath is not None and n <= MP_MAX


def _ld_sum(v):
    """Sum of a long-double array: long double itself, or fsum of the float64 terms."""
    if WIDE_LD:
        return np.sum(np.asarray(v, dtype=LD), dtype=LD)
    return LD(math.fsum(np.asarray(v, dtype=np.float64).tolist()))


def lse_exact(logw):
    """log sum exp over the finite entries (-inf if there is none)."""
    a, fin = _finite(logw)
    f = a[fin]
    if f.size == 0:
        return -math.inf
    m = float(f.max())
    if _use_mp(f.size):
        with mpmath.workdps(40):
            s = mpmath.fsum(mpmath.exp(mpmath.mpf(float(v)) - m) for v in f)
            return float(mpmath.log(s) + m)
    if WIDE_LD:
        s = _ld_sum(np.exp(f.astype(LD) - LD(m)))
        return float(LD(m) + np.log(s))
    s = math.fsum(np.exp(f - m).tolist())
    return float(m + math.log(s))


def wn_exact(logw):
    """Normalised weights exp(logw - lse), exactly 0 at -inf (all zero if every entry is -inf)."""
    a, fin = _finite(logw)
    out = np.zeros(a.size)
    f = a[fin]
    if f.size == 0:
        return out
    m = float(f.max())
    if _use_mp(f.size):
        with mpmath.workdps(40):
            e = [mpmath.exp(mpmath.mpf(float(v)) - m) for v in f]
            s = mpmath.fsum(e)
            out[fin] = [float(t / s) for t in e]
        return out
    e = np.exp(f.astype(LD) - LD(m))
    out[fin] = (e / _ld_sum(e)).astype(np.float64)
    return out


def ess_exact(logw):
    """1 / sum wn^2 = (sum e)^2 / sum e^2 with e = exp(logw - max) (nan if every entry is -inf)."""
    a, fin = _finite(logw)
    f = a[fin]
    if f.size == 0:
        return math.nan
    m = float(f.max())
    if _use_mp(f.size):
        with mpmath.workdps(40):
            e = [mpmath.exp(mpmath.mpf(float(v)) - m) for v in f]
            return float(mpmath.fsum(e) ** 2 / mpmath.fsum(t * t for t in e))
    e = np.exp(f.astype(LD) - LD(m))
    return float(_ld_sum(e) ** 2 / _ld_sum(e * e))


def moments_exact(logw, cx):
    """Weighted mean sum wn c(x) and variance sum wn (c(x) - mean)^2 per coordinate, the second moment around the
    EXACT mean.  cx: [N][D] constrained particles (float64)."""
    a, fin = _finite(logw)
    cx = np.asarray(cx, dtype=np.float64).reshape(a.size, -1)
    f, X = a[fin], cx[fin]
    D = cx.shape[1]
    if f.size == 0:
        return np.full(D, np.nan), np.full(D, np.nan)
    m = float(f.max())
    if _use_mp(f.size) and f.size * D <= 4 * MP_MAX:
        with mpmath.workdps(40):
            e = [mpmath.exp(mpmath.mpf(float(v)) - m) for v in f]
            W = mpmath.fsum(e)
            mean, var = np.empty(D), np.empty(D)
            for c in range(D):
                col = [mpmath.mpf(float(v)) for v in X[:, c]]
                mu = mpmath.fsum(ei * xi for ei, xi in zip(e, col)) / W
                mean[c] = float(mu)
                var[c] = float(mpmath.fsum(ei * (xi - mu) ** 2 for ei, xi in zip(e, col)) / W)
        return mean, var
    e = np.exp(f.astype(LD) - LD(m))
    W = _ld_sum(e)
    mean, var = np.empty(D), np.empty(D)
    for c in range(D):
        xc = X[:, c].astype(LD)
        mu = _ld_sum(e * xc) / W
        mean[c] = float(mu)
        var[c] = float(_ld_sum(e * (xc - mu) ** 2) / W)
    return mean, var


def indices_exact(wn, keys, blocked_cumsum):
    """searchsorted(cdf / cdf[-1], keys, 'right') on the blocked prefix sum of the scan kernel (the oracle's
    `blocked_cumsum`, passed in): vectorised; on a non-decreasing cdf the same as the oracle's bisection loop."""
    cdf = blocked_cumsum(np.asarray(wn, dtype=np.float64))
    cdf = cdf / cdf[-1]
    return np.searchsorted(cdf, np.asarray(keys, dtype=np.float64), side="right").astype(np.int64)


def sum_depth(n, blocks):
    """Longest chain of additions in the two-stage block reduction of the library (kRedBlock = 256 threads):
    ceil(n / (blocks * 256)) sequential adds per thread, the 8-level tree of a block, then the `blocks` partials:
    ceil(blocks / 256) sequential adds per thread and another 8-level tree."""
    t = -(-max(n, 1) // (blocks * 256))
    tf = -(-blocks // 256)
    return t + 8 + tf + 8
