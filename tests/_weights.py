"""Exact references for the weight path: the small operations that turn a proposal into the next generation's log-weights
and temperature (re-weighting, the Metropolis test, the tempered weights with their ESS, the bisection on it).

Every operation is restated from the reference implementation's Python and from include/smcnuts_hip.h, never from a kernel:

    combine      log pi_phi = lpri + phi * llik, a non-finite value -> -inf         (model/bridgestan.py:45-49)
    reweight     logw + pi_1(x') - pi_1(x) + L - q                                   (samples/samples.py:183-196)
    accept       reject iff u > min(1., exp(H1 - H0)) or x' has an infinite coordinate   (proposal/utils.py:22-34)
    asymptotic   logw + pi_new(x) - pi_old(x)                                        (samples/samples.py:169-180)
    ratio        pi_num(x) - pi_den(x)                                               (estimate/estimate_from_tempered.py:47)
    init         pi_phi(x) - log q0(x)                                               (samples/samples.py:85)
    tempered     v = phi (pi_1 - pi_0) + pi_0 - pi_old; the rows with v = -inf masked; ESS = (sum e^v)^2 / sum e^2v
                                                                                     (tempering/adaptive_tempering.py:38-56)

VALUE AND CLASS.  A result row is (class, value).  The class -- finite, +inf, -inf or NaN -- is the one IEEE float64
arithmetic gives the reference's own expression, evaluated left to right as its Python writes it: 0 * -inf is NaN at
phi = 0, -inf - -inf is NaN, and combine maps whatever is not finite to -inf before it is used.  The device must reproduce
the class exactly.  The value of a finite row is that expression WITHOUT rounding: mpmath at 40 digits up to MP_MAX rows;
beyond, numpy.longdouble with the math.fsum fallback, exactly as tests/_exact.py.  (Inputs whose class depends on HOW
float64 evaluates a finite expression -- a product that overflows where a fused multiply-add does not -- are not built.)
A value is kept as a pair of doubles (hi, lo), hi + lo the 40-digit value to 2^-106 relative, so that the error of a device
double d is (d - hi) - lo in plain float64.

BOUNDS.  Worst-case forward bounds, first order in u = 2^-53, each derived in the docstring of its function and none tuned on
what the device returns.  `check` prints "bound (share used)"; the shares of a run are collected in SHARES.
"""
import functools
import math
from fractions import Fraction

import numpy as np

import mpmath

from _exact import LD, MP_MAX, _ld_sum

U = 2.0 ** -53
EPS = 2.0 ** -52
DPS = 40
LOG2PI = math.log(2.0 * math.pi)
XTOL, RTOL = 2e-12, 4.0 * EPS            # scipy/optimize/Zeros/bisect.c as the reference calls it
FINITE, PINF, NINF, NAN = 0, 1, 2, 3
SHARES = {}                               # what -> (largest bound, largest share of its bound the device used)


def classes(a):
    a = np.asarray(a, dtype=np.float64)
    c = np.zeros(a.shape, dtype=np.int8)
    c[a == np.inf] = PINF
    c[a == -np.inf] = NINF
    c[np.isnan(a)] = NAN
    return c


def _hp(fn):
    """Run fn at DPS digits (mpmath's working precision is global; this module leaves it as it found it)."""
    @functools.wraps(fn)
    def wrapped(*a, **k):
        with mpmath.workdps(DPS):
            return fn(*a, **k)
    return wrapped


def _mp(v):
    return mpmath.mpf(float(v))


@_hp
def split(vals):
    """40-digit values -> (hi, lo) doubles."""
    hi = np.array([float(v) for v in vals], dtype=np.float64)
    lo = np.array([float(v - _mp(h)) for v, h in zip(vals, hi)], dtype=np.float64)
    return hi, lo


class Rows:
    """Per-row reference: cls [n] int8, hi/lo [n] (meaningful where cls == FINITE), bound [n] (absolute)."""

    def __init__(self, cls, hi, lo, bound):
        self.cls, self.hi, self.lo, self.bound = cls, hi, lo, np.asarray(bound, dtype=np.float64)


def check(dev, ref, what):
    """Class exact on every row; |dev - value| <= bound on the finite rows.  -> "bound (share used)"."""
    dev = np.asarray(dev, dtype=np.float64)
    got = classes(dev)
    bad = np.nonzero(got != ref.cls)[0]
    assert bad.size == 0, f"{what}: class differs at rows {bad[:8].tolist()}: device {dev[bad[:8]].tolist()}, " \
                          f"reference classes {ref.cls[bad[:8]].tolist()} (0 finite, 1 +inf, 2 -inf, 3 NaN)"
    fin = ref.cls == FINITE
    if not fin.any():
        return "no finite row"
    err = np.abs((dev[fin] - ref.hi[fin]) - ref.lo[fin])
    b = ref.bound[fin]
    with np.errstate(all="ignore"):
        share = float(np.max(np.where(err == 0, 0.0, err / b)))
    worst = int(np.argmax(np.where(err == 0, 0.0, err / np.where(b > 0, b, 1.0))))
    bmed = float(np.median(b))                 # (the typical row: a row of 1e300 parts has a bound of 1e285 and says nothing)
    old = SHARES.get(what, (0.0, 0.0))
    SHARES[what] = (max(old[0], bmed), max(old[1], share))
    msg = f"{bmed:.1e} ({share:.2f})"
    assert share <= 1.0, f"{what}: bound {msg}; worst finite row #{worst}: error {err[worst]:.3e}, bound {b[worst]:.3e}"
    return msg


@_hp
def check_scalar(dev, exact, bound, what):
    """One finite scalar against its exact value (a float or an mpf) and an absolute bound."""
    err = abs(float(_mp(dev) - exact))
    share = 0.0 if err == 0 else err / bound
    old = SHARES.get(what, (0.0, 0.0))
    SHARES[what] = (max(old[0], float(bound)), max(old[1], share))
    assert share <= 1.0, f"{what}: device {dev!r}, exact {float(exact)!r}, error {err:.3e} > bound {bound:.3e}"
    return f"{bound:.1e} ({share:.2f})"


# ---- combine -----------------------------------------------------------------------------------------------------------------
def combine64(lpri, llik, phi):
    """The class rule, explicit: lp = lpri + phi * llik in IEEE float64, and a non-finite lp becomes -inf."""
    with np.errstate(all="ignore"):
        lp = np.asarray(lpri, dtype=np.float64) + float(phi) * np.asarray(llik, dtype=np.float64)
    return np.where(np.isfinite(lp), lp, -np.inf)


@_hp
def combine_mp(lpri, llik, phi):
    """Exact lpri + phi * llik per row where combine64 is finite, else None."""
    fin = np.isfinite(combine64(lpri, llik, phi))
    p = _mp(phi)
    return [(_mp(a) + p * _mp(b)) if f else None for a, b, f in zip(lpri, llik, fin)]


@_hp
def kinetic_mp(r):
    """Exact |r_i|^2 per row of r [n][D]."""
    return [mpmath.fsum(_mp(v) ** 2 for v in row) for row in np.atleast_2d(r)]


def _left_to_right(terms):
    """IEEE float64 value of t0 + t1 + ... in that order (signs folded into the terms), for the class."""
    with np.errstate(all="ignore"):
        s = np.array(terms[0], dtype=np.float64, copy=True)
        for t in terms[1:]:
            s = s + t
    return s


@_hp
def _rows(cls64, exact_terms, bound):
    """exact_terms: per row a list of mpf (or None where a term is not finite)."""
    cls = classes(cls64)
    vals = [mpmath.fsum(t) if c == FINITE else _mp(0.0) for t, c in zip(exact_terms, cls)]
    hi, lo = split(vals)
    return Rows(cls, hi, lo, bound)


# ---- re-weighting ------------------------------------------------------------------------------------------------------------
@_hp
def reweight_ref(logw, lpri0, llik0, lpri1, llik1, r, r_new, L=None, q=None, kin=None):
    """samples.py:183-196: logw + p(x') - p(x) + L - q, p = combine(., ., 1).  L = None: the forward L-kernel's
    N(-r'; 0, I) = -|r'|^2 / 2 - D/2 log 2 pi (forward_lkernel.py:35); q = None: the momentum proposal's N(r; 0, I).

    Bound per row: (D + 8) u (|logw| + |lpri0| + |llik0| + |lpri1| + |llik1| + k0/2 + k1/2 + D log 2 pi), a supplied L or
    q entering with |L|, |q| in place of its k/2 + D/2 log 2 pi.  Derivation: |r|^2 summed in any order carries at most
    D u |r|^2 (D - 1 additions and a rounding per product, or D fused steps); D/2 log 2 pi is the rounded constant times an
    exactly representable D/2, 2 u; each of L, q adds a halving (exact) and one subtraction; each combine one product and
    one sum; the final expression four additions.  Every rounding is relative to a partial result no larger than the sum
    S of the magnitudes in the bracket, and there are at most 2 + 2 + 2 + 4 = 10 of them besides the sums of squares, of
    which the two combines' products are exact at phi = 1: 8 u S, plus D u (k0 + k1) / 2 <= D u S."""
    D = np.atleast_2d(r).shape[1]
    n = len(logw)
    k0, k1 = kin if kin is not None else (kinetic_mp(r), kinetic_mp(r_new))      # (kin: the two, computed once by the caller)
    cst = _mp(D) * mpmath.log(2 * mpmath.pi) / 2
    Lx = [(-k / 2 - cst) for k in k1] if L is None else [_mp(v) if np.isfinite(v) else None for v in L]
    qx = [(-k / 2 - cst) for k in k0] if q is None else [_mp(v) if np.isfinite(v) else None for v in q]
    L64 = np.array([float(v) for v in Lx]) if L is None else np.asarray(L, dtype=np.float64)
    q64 = np.array([float(v) for v in qx]) if q is None else np.asarray(q, dtype=np.float64)
    pxn, px = combine64(lpri1, llik1, 1.0), combine64(lpri0, llik0, 1.0)
    cls64 = _left_to_right([logw, pxn, -px, L64, -q64])
    pxn_x, px_x = combine_mp(lpri1, llik1, 1.0), combine_mp(lpri0, llik0, 1.0)
    terms = []
    for i in range(n):
        if np.isfinite(cls64[i]):
            terms.append([_mp(logw[i]), pxn_x[i], -px_x[i], Lx[i], -qx[i]])
        else:
            terms.append(None)
    mag = np.abs(np.where(np.isfinite(logw), logw, 0.0))
    for a in (lpri0, llik0, lpri1, llik1):
        mag = mag + np.abs(np.where(np.isfinite(a), a, 0.0))
    mag = mag + (np.array([float(k) for k in k1]) / 2 + D * LOG2PI / 2 if L is None else np.abs(np.where(np.isfinite(L64), L64, 0.0)))
    mag = mag + (np.array([float(k) for k in k0]) / 2 + D * LOG2PI / 2 if q is None else np.abs(np.where(np.isfinite(q64), q64, 0.0)))
    return _rows(cls64, terms, (D + 8) * U * mag)


# ---- the two-temperature differences -----------------------------------------------------------------------------------------
@_hp
def tempered_difference_ref(logw, lpri, llik, phi_a, phi_b):
    """logw + combine(phi_a) - combine(phi_b), left to right (samples.py:180; logw = None: estimate_from_tempered.py:47,
    the difference alone).

    The two densities cancel by construction -- at equal temperatures to exactly 0 -- so no relative accuracy is claimed:
    the bound is ABSOLUTE, 8 u (|logw| + |lpri| + |llik|).  Each combine rounds its product and its sum, each rounding at
    most u (|lpri| + |llik|) for |phi| <= 1: 4 u (|lpri| + |llik|) for the two; the two additions round results no larger
    than |logw| + 2 (|lpri| + |llik|): with the first, 8 u (|logw| + |lpri| + |llik|) covers all six."""
    n = len(lpri)
    lw = np.zeros(n) if logw is None else np.asarray(logw, dtype=np.float64)
    ca, cb = combine64(lpri, llik, phi_a), combine64(lpri, llik, phi_b)
    cls64 = _left_to_right([lw, ca, -cb]) if logw is not None else _left_to_right([ca, -cb])
    xa, xb = combine_mp(lpri, llik, phi_a), combine_mp(lpri, llik, phi_b)
    terms = [[_mp(lw[i]), xa[i], -xb[i]] if np.isfinite(cls64[i]) else None for i in range(n)]
    mag = sum(np.abs(np.where(np.isfinite(a), a, 0.0)) for a in (lw, lpri, llik))
    return _rows(cls64, terms, 8 * U * mag)


# ---- initial weights ---------------------------------------------------------------------------------------------------------
@_hp
def init_weights_ref(lpri, llik, phi, x=None, logq0=None):
    """samples.py:85: combine(phi) - log q0(x); logq0 = None: N(x; 0, I) = -|x|^2 / 2 - D/2 log 2 pi.

    Bound: (D + 6) u (|lpri| + |llik| + |x|^2 / 2 + D/2 log 2 pi) (a supplied logq0: 4 u (|lpri| + |llik| + |logq0|)):
    the sum of squares D u |x|^2 as in reweight_ref, the constant 2 u, the closed form's subtraction, the combine's two
    roundings and the final subtraction, each relative to a partial result within the bracket."""
    n = len(lpri)
    c64, cx = combine64(lpri, llik, phi), combine_mp(lpri, llik, phi)
    if logq0 is None:
        D = x.shape[1]
        ss = kinetic_mp(x)
        cst = _mp(D) * mpmath.log(2 * mpmath.pi) / 2
        lqx = [(-s / 2 - cst) if mpmath.isfinite(s) else None for s in ss]
        lq64 = np.array([float(-s / 2 - cst) for s in ss])
        mag, k = np.array([float(s) for s in ss]) / 2 + D * LOG2PI / 2, D + 6
    else:
        lq64 = np.asarray(logq0, dtype=np.float64)
        lqx = [_mp(v) if np.isfinite(v) else None for v in lq64]
        mag, k = np.abs(np.where(np.isfinite(lq64), lq64, 0.0)), 4
    cls64 = _left_to_right([c64, -lq64])
    terms = [[cx[i], -lqx[i]] if np.isfinite(cls64[i]) else None for i in range(n)]
    mag = mag + sum(np.abs(np.where(np.isfinite(a), a, 0.0)) for a in (lpri, llik))
    return _rows(cls64, terms, k * U * mag)


# ---- the Metropolis test -----------------------------------------------------------------------------------------------------
EXP_UNDERFLOW = -745.2          # below: e^x < 2^-1075 rounds to 0 in float64 whatever the last ulps of an exp are
EXP_SUBNORMAL = -708.3          # below: e^x is subnormal and its relative error is no longer a few ulps


class Decisions:
    """Per row: prob (the exact min(1, e^dH) as an mpf; 1 for a NaN ratio), accept (bool) for the given u, margin (the
    relative distance |u - prob| / prob of u from the threshold; inf where float64 decides the row exactly as the exact
    arithmetic does whatever its rounding) and bound (on the relative error of the device's prob)."""

    def __init__(self, prob, accept, margin, bound, dH_cls, dH):
        self.prob, self.accept, self.margin, self.bound, self.dH_cls, self.dH = prob, accept, margin, bound, dH_cls, dH


@_hp
def decisions_ref(lpri0, llik0, lpri1, llik1, r, r_new, x_new, phi, u):
    """proposal/utils.py:22-34 per row: H = combine(phi) - |r|^2 / 2; ratio = exp(H1 - H0); prob = min(1., ratio), which
    is 1. for a NaN ratio (Python's min keeps its first argument when the comparison is false); rejected iff u > prob or
    np.any(np.isinf(x')) -- a NaN coordinate does not reject by that rule.

    Bound on H1 - H0: (D + 6) u (|lpri0| + |phi llik0| + |lpri1| + |phi llik1| + k0/2 + k1/2): the sums of squares
    D u k as in reweight_ref, per Hamiltonian the combine's two roundings and one subtraction, the difference one more --
    7 roundings, of which the halvings are exact, each within the bracket; 6 would do at first order, D + 6 is stated.  The
    device's prob is e^(dH + d), |d| <= that bound, times (1 + 2 ulp) of an exp: relative error bound + 4 u.
    Rows decided identically whatever the rounding (margin = inf): dH = -inf (prob 0: only u = 0 accepts), a NaN ratio
    (prob 1.), dH at least 100 bounds above 0 (prob exactly 1., and u <= 1 - 2^-53 never exceeds it), dH + bound below
    log 2^-1075 (the float64 ratio is 0, the exact prob is below every positive double: u = 0 accepts, any other rejects),
    and u = 0 (never greater than a prob >= 0)."""
    r, r_new, x_new = (np.atleast_2d(np.asarray(a, dtype=np.float64)) for a in (r, r_new, x_new))
    n, D = r.shape
    u = np.asarray(u, dtype=np.float64)
    k0, k1 = kinetic_mp(r), kinetic_mp(r_new)
    c1, c0 = combine64(lpri1, llik1, phi), combine64(lpri0, llik0, phi)
    x1, x0 = combine_mp(lpri1, llik1, phi), combine_mp(lpri0, llik0, phi)
    with np.errstate(all="ignore"):
        H1 = c1 - 0.5 * np.array([float(k) for k in k1])
        H0 = c0 - 0.5 * np.array([float(k) for k in k0])
        dcls = classes(H1 - H0)
    mag = np.array([float(a) / 2 + float(b) / 2 for a, b in zip(k0, k1)])
    for a, f in ((lpri0, 1.0), (llik0, abs(phi)), (lpri1, 1.0), (llik1, abs(phi))):
        a = np.asarray(a, dtype=np.float64)
        mag = mag + f * np.abs(np.where(np.isfinite(a), a, 0.0))
    bdH = (D + 6) * U * mag
    bound = bdH + 4 * U
    infx = np.isinf(x_new).any(axis=1)
    prob, accept, margin, dHs = [], np.zeros(n, dtype=bool), np.full(n, np.inf), np.full(n, np.nan)
    for i in range(n):
        ui = _mp(u[i])
        if dcls[i] == NAN or dcls[i] == PINF:
            p = _mp(1.0)
        elif dcls[i] == NINF:
            p = _mp(0.0)
        else:
            dH = (x1[i] - k1[i] / 2) - (x0[i] - k0[i] / 2)
            dHs[i] = float(dH)
            p = mpmath.exp(dH) if dH < 0 else _mp(1.0)
            sure = (u[i] == 0.0 or dH >= 100 * bdH[i] or float(dH) + bdH[i] < EXP_UNDERFLOW)
            if not sure:
                if float(dH) < EXP_SUBNORMAL:
                    margin[i] = 0.0 if u[i] < 1e-300 else np.inf      # subnormal prob: decided only by a u far above it
                else:
                    margin[i] = float(abs(ui - p) / p)
        prob.append(p)
        accept[i] = (not (ui > p)) and not infx[i]
    return Decisions(prob, accept, margin, bound, dcls, dHs)


def require_margins(dec, factor=100.0):
    """The guarantee of the input builders: every row's u is at least `factor` bounds (relative, on the device's prob) away
    from its threshold, so that a correct device decides every row as the exact arithmetic does and NO row has to be left
    out of the comparison.  Raises -- never skips -- when a row fails it."""
    bad = np.nonzero(dec.margin < factor * dec.bound)[0]
    if bad.size:
        i = int(bad[0])
        raise ValueError(f"Metropolis input on the threshold: row {i} has margin {dec.margin[i]:.3e} < {factor:g} x bound "
                         f"{dec.bound[i]:.3e} ({bad.size} such rows); choose another u")
    return dec


# ---- tempered weights, their partials and ESS --------------------------------------------------------------------------------
BV = 16.0     # |v_device - v| <= BV u (|lpri| + |llik|), derived in Tempered


def chain(n):
    """Longest chain of additions the bounds below allow a reduction over n terms: log2(n) + 16.  A reduction tree over n
    terms has depth log2(n); the 16 is room for a few sequential additions per thread in front of the tree and for the
    sequential merge of per-block partials behind it.  The bounds hold for every summation order within that depth; a
    reduction that adds many more terms one after the other would need the bound revisited, not the tests."""
    return math.ceil(math.log2(max(int(n), 2))) + 16


class Tempered:
    """adaptive_tempering.py:38-56 on density parts (lpri, llik) and the temperature phi_old the particles were moved at:
        logpri = combine(0), loglik = combine(1) - logpri, v(phi) = phi * loglik + logpri - combine(phi_old),
    rows with v = -inf left out, a NaN row making everything NaN (np.isneginf does not mask it, logsumexp returns NaN).

    Class per row by IEEE float64 on that expression; value of a finite row exactly (phi - phi_old) * llik.
    Error of a float64 evaluation of v, absolute: BV u (|lpri| + |llik|) with BV = 16 -- writing S = |lpri| + |llik|:
    combine(1) rounds once (u S), combine(phi_old) twice (2 u S), the difference d = p1 - p0 is at most 2 S (2 u S),
    phi d at most 2 S (2 u S), phi d + p0 at most 3 S (3 u S), the last subtraction at most 4 S (4 u S): 14 u S, stated as 16.

    Identical rows are grouped (after every resampling the population is full of exact duplicates), each group carrying
    its count.  Rows that are tied at the exact maximum must be identical (lpri, llik) pairs, and the runner-up must lie
    more than two v-errors below: otherwise which rows a float64 evaluation counts "at the maximum" is a matter of its
    rounding, and partials() raises."""

    def __init__(self, lpri, llik, phi_old):
        self.lpri = np.asarray(lpri, dtype=np.float64)
        self.llik = np.asarray(llik, dtype=np.float64)
        self.N = self.lpri.size
        self.phi_old = float(phi_old)
        pairs = np.stack([self.lpri, self.llik], axis=1).view(np.uint64)
        uq, self.inv, cnt = np.unique(pairs, axis=0, return_inverse=True, return_counts=True)
        self.inv = self.inv.reshape(-1)
        g = uq.view(np.float64)
        self.gl, self.gk, self.gc = g[:, 0].copy(), g[:, 1].copy(), cnt.astype(np.int64)
        with np.errstate(over="ignore"):
            S = np.abs(np.where(np.isfinite(self.gl), self.gl, 0.0)) + np.abs(np.where(np.isfinite(self.gk), self.gk, 0.0))
        self.gbv = BV * U * S
        self.mp = self.N <= MP_MAX
        self._memo = {}

    def v64(self, phi):
        """Group-wise v in float64 as the reference's Python evaluates it: for the classes."""
        p0, p1 = combine64(self.gl, self.gk, 0.0), combine64(self.gl, self.gk, 1.0)
        base = combine64(self.gl, self.gk, self.phi_old)
        with np.errstate(all="ignore"):
            return float(phi) * (p1 - p0) + p0 - base

    def rows_cls(self, phi):
        return classes(self.v64(phi))[self.inv]

    def partials(self, phi, strict=True):
        """The partials at phi, computed once per temperature (a bisection and the checks around its result ask for the same
        temperatures under several targets)."""
        key = (float(phi), bool(strict))
        if key not in self._memo:
            self._memo[key] = self._partials(phi, strict)
        return self._memo[key]

    @_hp
    def _partials(self, phi, strict):
        """dict(nan, mx (mpf / long double), mx64, cnt, s1, s2, ess (floats rounded once), bv (the largest v-error among the
        rows that matter), spread).  Every finite-class group enters; s1 leaves the groups at the maximum out, s2 does not."""
        cls = classes(self.v64(phi))
        if np.any(cls == NAN):
            return dict(nan=True, ess=math.nan)
        if np.any(cls == PINF):
            raise ValueError("a tempered weight of +inf: not a population these references cover")
        fin = cls == FINITE
        if not fin.any():
            raise ValueError("every tempered weight is -inf: the reference's logsumexp fails on the empty selection")
        k, c, bv = self.gk[fin], self.gc[fin], self.gbv[fin]
        if self.mp:
            with mpmath.workdps(DPS):
                dphi = _mp(phi) - _mp(self.phi_old)
                v = [dphi * _mp(t) for t in k]
                mx = max(v)
                top = np.array([t == mx for t in v])
                rest = [float(t) for t, f in zip(v, top) if not f]
                e = [mpmath.exp(t - mx) for t in v]
                s1 = mpmath.fsum(ci * ei for ci, ei, f in zip(c, e, top) if not f)
                s2 = mpmath.fsum(ci * ei * ei for ci, ei in zip(c, e))
                cnt = int(c[top].sum())
                ess = (cnt + s1) ** 2 / s2
                spread = float(max(mx - t for t in v))
                gap = float(mx) - max(rest) if rest else math.inf
                out = dict(mx=mx, s1=float(s1), s2=float(s2), ess=float(ess), s1x=s1, s2x=s2, essx=ess)
        else:
            dphi = LD(phi) - LD(self.phi_old)
            v = dphi * k.astype(LD)
            mx = v.max()
            top = v == mx
            e = np.exp(v - mx)
            s1 = _ld_sum((c * e)[~top]) if (~top).any() else LD(0)
            s2 = _ld_sum(c * e * e)
            cnt = int(c[top].sum())
            ess = (LD(cnt) + s1) ** 2 / s2
            spread = float((mx - v).max())
            gap = float(mx - v[~top].max()) if (~top).any() else math.inf
            out = dict(mx=mx, s1=float(s1), s2=float(s2), ess=float(ess), s1x=s1, s2x=s2, essx=ess)
        bvm = float(bv.max())
        if strict and (int(top.sum()) != 1 or gap <= 2 * bvm):
            raise ValueError(f"tempered weights tied at the maximum within rounding (gap {gap:.3e}, v-error {bvm:.3e}, "
                             f"{int(top.sum())} distinct rows at the exact maximum): the count is not decidable")
        out.update(nan=False, mx64=float(mx) + 0.0, cnt=cnt, bv=bvm,    # (+ 0.0: an exact zero carries no sign)
                   spread=min(spread, 746.0), gap=gap)
        return out

    def sum_bounds(self, p):
        """Relative bounds (e1, e2) on a float64 evaluation of s1 and s2 whose sums have at most chain(N) levels.
        A term is e^(v - mx): both v and mx carry the v-error bv, the subtraction rounds (u |v - mx|, and terms further
        than 746 below the maximum are 0), the exp is good to 2 ulp: relative error 2 bv + (spread + 2) u per term, twice
        that plus one rounding for its square; summing non-negative terms adds at most one u per level."""
        t = 2 * p["bv"] + (p["spread"] + 2) * U
        return t + chain(self.N) * U, 2 * t + (1 + chain(self.N)) * U

    def ess_bound(self, p, log_space=True):
        """ABSOLUTE bound on a float64 ESS at these partials.  (cnt + s1)^2 / s2: 2 e1 + e2 + 4 u relative (a sum, a
        square, a quotient).  log_space: the ESS taken as the reference takes it, through the log-likelihood
        ll = log1p(s1 / cnt) + log cnt + mx and sum wn^2 = s2 e^(2 (mx - ll)) -- ll and mx - ll round at
        u (|mx| + |ll|) each, the two logarithms and their sum at 4 u log N, and the doubled exponent turns these absolute
        errors into relative ones: + 4 u (|mx| + |ll| + 2 log N + 2)."""
        e1, e2 = self.sum_bounds(p)
        rel = 2 * e1 + e2 + 4 * U
        if log_space:
            ll = abs(p["mx64"]) + math.log(self.N)
            rel += 4 * U * (abs(p["mx64"]) + ll + 2 * math.log(max(self.N, 2)) + 2)
        return rel * p["ess"]

    def ess(self, phi):
        return self.partials(phi, strict=False)["ess"]

    def f(self, target):
        """f_exact(phi) = ESS(phi) - target, rounded once (NaN for a NaN population)."""
        @_hp
        def f_exact(phi):
            e = self.partials(phi, strict=False)
            if e["nan"]:
                return math.nan
            return float(e["essx"] - (LD(target) if not self.mp else _mp(target)))
        return f_exact

    def exactly_computable(self, phi):
        """True where every intermediate of the reference's expression for v is itself a double on every finite row
        (p1 = lpri + llik, p1 - p0, phi * (p1 - p0), that + p0, phi_old * llik, lpri + that, the final difference): then ANY
        float64 evaluation, fused or not, returns the exact v, and the maximum is the nearest double of the exact one --
        itself -- bit for bit."""
        fin = classes(self.v64(phi)) == FINITE
        a, b = self.gl[fin], self.gk[fin]
        if self.N <= 512:                          # small populations: rational arithmetic, any temperatures
            F = Fraction
            is_d = lambda q: F(float(q)) == q
            po, pn = F(self.phi_old), F(float(phi))
            for ai, bi in zip(a, b):
                ai, bi = F(ai), F(bi)
                if not all(is_d(s) for s in (ai + bi, pn * bi, pn * bi + ai, po * bi, ai + po * bi, (pn - po) * bi)):
                    return False
            return True
        # larger ones: phi_old = 0 and phi a power of two (or 0) make the products exact scalings; the sums by TwoSum
        if self.phi_old != 0.0 or math.frexp(float(phi))[0] not in (0.0, 0.5):
            return False

        def exact_sum(x, y):
            s = x + y
            yy = s - x
            return ((x - (s - yy)) + (y - yy)) == 0.0
        return bool(np.all(exact_sum(a, b)) and np.all(exact_sum(float(phi) * b, a)))


def bracket_width(T, phi, target, b_of):
    """The half-width w of the root property: w = 2 (xtol + rtol phi) + 2 b / |s| with xtol = 2e-12, rtol = 4 eps, b the
    bound on the evaluated ESS near phi and s the slope of f_exact across [phi - w, phi + w] -- the guarantee of bisect.c
    when its sign tests are right (the last bracket is no wider than xtol + rtol |x| on either side of the returned
    midpoint; doubled for the midpoint's own rounding and the final halving), widened by what a sign test decided inside
    the rounding of f can cost: a test can be wrong only where |f| <= b, i.e. within b / |s| of the root, on either side."""
    f = T.f(target)
    w0 = 2.0 * (XTOL + RTOL * abs(phi))
    b = b_of(T.partials(phi, strict=False))
    w = w0
    for _ in range(3):
        lo, hi = max(T.phi_old, phi - w), min(1.0, phi + w)
        s = (f(hi) - f(lo)) / (hi - lo)
        if s == 0 or not math.isfinite(s):
            raise ValueError("f_exact is flat across the interval: no slope to scale the ESS bound with")
        w = w0 + 2.0 * b / abs(s)
    return w, b, s


def check_root(T, phi, target, what, log_space=True):
    """f_exact changes sign over [phi - w, phi + w] (clipped to the bracket the bisection started from)."""
    w, b, s = bracket_width(T, phi, target, lambda p: T.ess_bound(p, log_space))
    f = T.f(target)
    lo, hi = max(T.phi_old, phi - w), min(1.0, phi + w)
    flo, fhi = f(lo), f(hi)
    assert flo * fhi <= 0.0, f"{what}: phi = {phi!r} is no root: f({lo!r}) = {flo:.3e}, f({hi!r}) = {fhi:.3e}, w = {w:.3e}"
    # how far inside: the distance from phi to the exact root over w, the root located by the secant of the two ends
    root = lo + (hi - lo) * flo / (flo - fhi) if flo != fhi else phi
    share = abs(root - phi) / w
    old = SHARES.get("bisect root", (0.0, 0.0))
    SHARES["bisect root"] = (max(old[0], w), max(old[1], share))
    return f"{w:.1e} ({share:.2f})"


def bisect_outcome(T, target):
    """What the reference's calculate_phi does on f_exact, as (status, phi): ESS(1) >= target returns 1; else the project's
    restatement of bisect.c -- status 0 and the root, 2 for its ValueError, 3 for its RuntimeError."""
    from smcnuts_amd.tempering.adaptive_tempering import bisect
    f = T.f(target)
    if f(1.0) >= 0:
        return 0, 1.0
    try:
        return 0, float(bisect(f, T.phi_old, 1.0))
    except ValueError:
        return 2, math.nan
    except RuntimeError:
        return 3, math.nan


def has_root(T, target):
    f = T.f(target)
    a, b = f(T.phi_old), f(1.0)
    return a > 0 > b


# ---- populations of the tempering tests (shared by the GPU file and the CPU stand-in) ----------------------------------------
TEMPER_N = (1, 2, 255, 257, 1000, 4097, 70001)
TEMPER_KINDS = ("distinct", "repeated", "identical", "overflow", "nan")
PHI_OLD = (0.0, 1e-4, 0.3)


def population(kind, N, seed=0):
    """(lpri, llik) of N rows.  The benign rows: lpri = -|z|^2 / 2 - 4 (a prior at a draw of its own), llik = -2 chi^2_2,
    whose weights e^(phi llik) have ESS(1) / N = 9 / 25 in expectation: a root for the targets 0.5 N and 0.9 N.  The values
    are multiples of 2^-20 of moderate size, so that sums of a few of them are exact doubles (exactly_computable)."""
    rng = np.random.default_rng(1000 * seed + N)
    m = N if kind != "repeated" else max(1, N // 8)
    z = rng.standard_normal((m, 3))
    q = lambda a: np.round(a * 2.0 ** 20) / 2.0 ** 20
    lpri = q(-0.5 * z[:, 0] ** 2 - 4.0)
    llik = q(-2.0 * (z[:, 1] ** 2 + z[:, 2] ** 2))
    if kind == "repeated":                 # copies of a row sit N // 8 apart: ties at the maximum in several blocks
        idx = np.arange(N) % m
        lpri, llik = lpri[idx], llik[idx]
    elif kind == "identical":
        lpri, llik = np.full(N, lpri[0]), np.full(N, llik[0])
    elif kind == "overflow":               # combine(1) overflows: v = -inf, masked
        bad = np.arange(N) % 7 == 3
        lpri[bad], llik[bad] = -1e308, -1e308
    elif kind == "masked":                 # more than half the rows masked
        bad = np.arange(N) % 5 != 1
        lpri[bad], llik[bad] = -1e308, -1e308
    elif kind == "nan":                    # a finite prior and llik = -inf: v is NaN
        llik[N // 2] = -np.inf
    elif kind == "steep":                  # likelihoods of order 1e9: a root inside a bracket of width 1e-9
        llik = llik * 2.0 ** 30
    elif kind != "distinct":
        raise KeyError(kind)
    return lpri, llik


def standin_partials(lpri, llik, phi_old, phi, chunk=37):
    """A float64 stand-in for a device: v as the reference's Python writes it, the four partials with the sums taken in
    another order (chunks of 37, the chunks in reverse)."""
    p0, p1, base = combine64(lpri, llik, 0.0), combine64(lpri, llik, 1.0), combine64(lpri, llik, phi_old)
    with np.errstate(all="ignore"):
        v = phi * (p1 - p0) + p0 - base
        if np.any(np.isnan(v)):
            return np.array([np.nan, np.nan, np.nan, np.nan])
        v = v[v != -np.inf]
        if v.size == 0:
            return np.array([-np.inf, 0.0, 0.0, 0.0])
        mx = v.max()
        e = np.exp(v - mx)
        top = v == mx
        def rsum(a):
            parts = [float(np.sum(a[i:i + chunk][::-1])) for i in range(0, a.size, chunk)]
            s = 0.0
            for t in parts[::-1]:
                s += t
            return s
        return np.array([mx, float(top.sum()), rsum(e[~top]), rsum(e * e)])

# ---- input builders shared by the GPU tests and their CPU counterparts -------------------------------------------------------
INF, NAN_ = math.inf, math.nan


def rows(idx, D, rng):
    x = rng.standard_normal((len(idx), D))
    x[:, 0] = idx
    return x


def benign_table(n, rng):
    return -0.5 * rng.chisquare(3, n) - 2.0, -3.0 * rng.chisquare(2, n)


def accept_inputs(D, N, phi, seed):
    """Table, proposal and u with the edge rows of the Metropolis test; every u at least 100 bounds off its threshold."""
    rng = np.random.default_rng(seed)
    tl, tk = benign_table(2 * N, rng)
    x, x_new = rows(np.arange(N), D, rng), rows(N + np.arange(N), D, rng)
    r, r_new = rng.standard_normal((N, D)), rng.standard_normal((N, D))
    u = rng.uniform(size=N)
    near = []
    if N >= 32:
        def same(i, shift=0.0):              # the parts at x' are those at x (+ shift on the prior)
            tl[N + i], tk[N + i] = tl[i] + shift, tk[i]

        same(0); r[0, 0] = 1.5; r_new[0] = 0.5 * r[0]; u[0] = 1.0 - 2.0 ** -53          # ratio > 1, the largest u
        for i in (1, 2):                                                                 # H1 - H0 = -800: prob underflows to 0
            same(i, -800.0); r_new[i] = r[i]
        u[1], u[2] = 0.0, 5e-324                                                         # u = 0 is accepted (u > prob is false)
        u[3] = 1.0 - 2.0 ** -53
        near = [4, 5, 20, 21]                                                            # u = prob (1 -+ 1e-9), set below
        for j, i in enumerate(near):
            same(i, -1.0 - 0.25 * j); r_new[i] = r[i]                                    # ratios e^-1 .. e^-1.75
        tl[6] = tl[N + 6] = -INF; u[6] = 0.9                                             # NaN ratio: accepted
        if D > 1:
            x_new[7, 1], u[7] = INF, 0.0                                                 # an infinite coordinate rejects
            x_new[8, D - 1], u[8] = -INF, 0.0
            x_new[9, 1], u[9] = NAN_, 1e-3                                                # a NaN coordinate does not
            same(9); r_new[9] = 0.5 * r[9]
        tl[10] = -INF                                                                    # H0 = -inf: ratio +inf
        tk[N + 11] = -INF; u[11] = 0.5                                                   # H1 = -inf: prob 0
        tk[N + 12] = -INF; u[12] = 0.0
        tk[13] = -INF                                                                    # 0 * -inf at phi = 0, -inf otherwise
        tk[N + 14] = INF; u[14] = 1e-300                                                 # a +inf part is a failed density
    return tl, tk, x, x_new, r, r_new, u, near


def set_near(dec, u, near):
    """u = prob (1 - 1e-9) and prob (1 + 1e-9) on the rows `near` (alternating), prob the exact one."""
    for j, i in enumerate(near):
        p = float(dec.prob[i])
        assert 0.0 < p < 1.0, "the rows next to the threshold need a ratio below 1"
        u[i] = p * (1.0 - 1e-9) if j % 2 == 0 else p * (1.0 + 1e-9)


def check_outcome(T, target, phi, st, what):
    """A population with a root: status 0 and f_exact changes sign over [phi - w, phi + w].  Every other: what the
    reference's calculate_phi does on f_exact, status and value."""
    if has_root(T, target):
        assert st == 0, f"{what}: status {st}"
        return "root " + check_root(T, phi, target, what)
    want_st, want = bisect_outcome(T, target)
    assert st == want_st, f"{what}: status {st}, the reference's bisection gives {want_st}"
    if st == 0:
        assert phi == want, f"{what}: phi {phi!r}, the reference's bisection on f_exact gives {want!r}"
    return f"status {st}" + (f" phi {phi!r}" if st == 0 else "")
