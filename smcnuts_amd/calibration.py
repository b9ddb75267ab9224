"""Calibration checks of a GLM fit from the device's mergeable partials (include/smcnuts_hip.h,
smcn_calibration_partials): does the fitted family describe these observations at all, and at which rows does it fail?

Per particle x_p and row i the predictive law F_{p,i} is family(eta_{p,i} [, e^tau_p]), eta and the dispersion as the
density forms them (the row's offset included), and
  lo = P(Y < y_i),  up = P(Y > y_i),  pmf = P(Y = y_i) = 1 - lo - up  (0 for `normal`).
Over the particles with posterior weights W_p, per row:
  pit_lo_i = sum_p W_p lo,   sf_i = sum_p W_p up,   pit_hi_i = 1 - sf_i
and the `_loo` forms with the leave-one-out weights W_p / p(y_i | x_p), the plain importance ratios of criteria.py's
IS-LOO (no Pareto smoothing).  The probability integral transform of row i is uniform on [pit_lo_i, pit_hi_i]: a point for
`normal` (pit = pit_lo), an interval of the mixture's pmf for the count families.  `randomised()` draws one value per row
from it, `quantile_residuals()` maps that draw through the inverse normal cdf (Dunn and Smyth's randomised quantile
residuals: standard normal if the model holds), `pit_histogram()` is the non-randomised histogram of Czado, Gneiting and
Held for count data.  A U-shaped histogram says the predictive laws are too narrow (overdispersed counts under a Poisson
fit), a humped one that they are too wide, a sloped one that they are biased.

Rules, continuing criteria.py: a particle with a non-finite log-weight contributes to nothing.  A contributing particle
whose term is -inf is counted in ninf[i]; a pair whose tail evaluation reaches the device's iteration bound (2048 per
tail: Poisson counts near 1e5 and beyond, at their mode) is counted in n_unconverged[i] and adds nothing.  A row with
either count > 0 reports NaN; the other rows are unaffected.
"""
import math

import numpy as np

# columns of a partials block (row 0: header [mw, sw, sw2, cnt, 0 ..]; row 1 + i: observation i)
SW, LO, UP, MB, SB, LOB, UPB, NINF, NUNC = range(9)
QC = 9


# ---- the inverse normal cdf: Wichura's AS 241 (PPND16), then Halley steps on erfc ----------------------------------------------
_A = (3.3871328727963666080e0, 1.3314166789178437745e+2, 1.9715909503065514427e+3, 1.3731693765509461125e+4,
      4.5921953931549871457e+4, 6.7265770927008700853e+4, 3.3430575583588128105e+4, 2.5090809287301226727e+3)
_B = (1.0, 4.2313330701600911252e+1, 6.8718700749205790830e+2, 5.3941960214247511077e+3, 2.1213794301586595867e+4,
      3.9307895800092710610e+4, 2.8729085735721942674e+4, 5.2264952788528545610e+3)
_C = (1.42343711074968357734e0, 4.63033784615654529590e0, 5.76949722146069140550e0, 3.64784832476320460504e0,
      1.27045825245236838258e0, 2.41780725177450611770e-1, 2.27238449892691845833e-2, 7.74545014278341407640e-4)
_D = (1.0, 2.05319162663775882187e0, 1.67638483018380384940e0, 6.89767334985100004550e-1, 1.48103976427480074590e-1,
      1.51986665636164571966e-2, 5.47593808499534494600e-4, 1.05075007164441684324e-9)
_E = (6.65790464350110377720e0, 5.46378491116411436990e0, 1.78482653991729133580e0, 2.96560571828504891230e-1,
      2.65321895265761230930e-2, 1.24266094738807843860e-3, 2.71155556874348757815e-5, 2.01033439929228813265e-7)
_F = (1.0, 5.99832206555887937690e-1, 1.36929880922735805310e-1, 1.48753612908506148525e-2, 7.86869131145613259100e-4,
      1.84631831751005468180e-5, 1.42151175831644588870e-7, 2.04426310338993978564e-15)


def _horner(c, r):
    v = c[-1]
    for k in c[-2::-1]:
        v = v * r + k
    return v


def _lower_quantile(p):
    """Phi^-1(p) for 0 < p <= 1/2 (<= 0)."""
    q = p - 0.5
    if abs(q) <= 0.425:
        r = 0.180625 - q * q
        x = q * _horner(_A, r) / _horner(_B, r)
    else:
        r = math.sqrt(-math.log(p))
        x = -(_horner(_C, r - 1.6) / _horner(_D, r - 1.6) if r <= 5.0 else _horner(_E, r - 5.0) / _horner(_F, r - 5.0))
    for _ in range(2):          # Halley on Phi(x) - p, relative to the density: keeps the tail's relative accuracy
        pdf = math.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
        if pdf == 0.0:
            break
        e = (0.5 * math.erfc(-x / math.sqrt(2.0)) - p) / pdf
        x -= e / (1.0 + 0.5 * x * e)
    return x


def norm_ppf(p=None, sf=None):
    """The inverse normal cdf, elementwise: Phi^-1(p), or from the upper tail, the x with 1 - Phi(x) = sf (give one of the
    two).  0 gives -inf (+inf from sf), 1 gives +inf; outside [0, 1] and NaN give NaN.  p above 1/2 goes through 1 - p:
    beyond 1 - 1e-16 give the upper tail itself."""
    if (p is None) == (sf is None):
        raise ValueError("norm_ppf: give p or sf")
    upper = p is None
    v = np.asarray(sf if upper else p, dtype=np.float64)
    out = np.full(v.shape, np.nan)
    it = np.nditer([v, out], op_flags=[["readonly"], ["writeonly"]])
    for a, o in it:
        a = float(a)
        if not 0.0 <= a <= 1.0:
            continue
        if a == 0.0 or a == 1.0:
            x = -math.inf if a == 0.0 else math.inf
        elif a <= 0.5:
            x = _lower_quantile(a)
        else:
            x = -_lower_quantile(1.0 - a)
        o[...] = -x if upper else x
    return out if out.ndim else float(out)


# ---- partials --------------------------------------------------------------------------------------------------------------
def merge_calibration_partials(a, b):
    """The partials of the union of two disjoint particle sets (a's particles first)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or a.ndim != 2 or a.shape[1] != QC or a.shape[0] < 2:
        raise ValueError(f"partials blocks of one model have the same shape [1 + n][{QC}]")
    if b[0, 3] == 0.0:
        return a.copy()
    if a[0, 3] == 0.0:
        return b.copy()
    out = np.zeros_like(a)
    mw = max(a[0, 0], b[0, 0])
    da, db = a[0, 0] - mw, b[0, 0] - mw                 # (<= 0, one of them 0)
    fa, fb = np.exp(da), np.exp(db)
    out[0, 0] = mw
    out[0, 1] = a[0, 1] * fa + b[0, 1] * fb
    out[0, 2] = a[0, 2] * fa * fa + b[0, 2] * fb * fb
    out[0, 3] = a[0, 3] + b[0, 3]
    A, B, O = a[1:], b[1:], out[1:]
    for col in (SW, LO, UP):
        O[:, col] = A[:, col] * fa + B[:, col] * fb
    # the leave-one-out sums around the larger of the two maxima
    ha, hb = A[:, SB] > 0.0, B[:, SB] > 0.0
    m1, m2 = A[:, MB] + da, B[:, MB] + db
    with np.errstate(invalid="ignore", over="ignore"):
        m = np.where(ha, np.where(hb, np.maximum(m1, m2), m1), m2)
        e1 = np.where(ha, np.exp(np.where(ha, m1 - m, 0.0)), 0.0)
        e2 = np.where(hb, np.exp(np.where(hb, m2 - m, 0.0)), 0.0)
    O[:, MB] = m
    for col in (SB, LOB, UPB):
        O[:, col] = A[:, col] * e1 + B[:, col] * e2
    O[:, NINF] = A[:, NINF] + B[:, NINF]
    O[:, NUNC] = A[:, NUNC] + B[:, NUNC]
    return out


class Calibration:
    """Per-observation calibration of one fitted model (arrays of length n): pit_lo = P(Y < y_i), sf = P(Y > y_i) and
    pit_hi = 1 - sf under the posterior predictive law, pit_lo_loo, pit_hi_loo and sf_loo under the leave-one-out one
    (plain importance ratios), ninf and n_unconverged (a row with either > 0 is NaN), and the contributing particles with
    the effective sample size of their weights.  `pit` is pit_lo: the PIT value of a continuous family."""

    def __init__(self, pit_lo, pit_hi, sf, pit_lo_loo, pit_hi_loo, sf_loo, ninf, n_unconverged, n_particles, ess):
        self.pit_lo, self.pit_hi, self.sf = pit_lo, pit_hi, sf
        self.pit_lo_loo, self.pit_hi_loo, self.sf_loo = pit_lo_loo, pit_hi_loo, sf_loo
        self.ninf, self.n_unconverged = ninf, n_unconverged
        self.n_particles = int(n_particles)       # contributing particles (finite log-weight)
        self.ess = float(ess)                     # effective sample size of the weights
        self.n_obs = int(np.shape(pit_lo)[0])

    pit = property(lambda self: self.pit_lo)
    pit_loo = property(lambda self: self.pit_lo_loo)

    def _bounds(self, loo):
        return (self.pit_lo_loo, self.pit_hi_loo, self.sf_loo) if loo else (self.pit_lo, self.pit_hi, self.sf)

    @staticmethod
    def _uniforms(seed, n):
        """v_i in [0, 1): the i-th double of numpy's Philox stream keyed by `seed` -- a function of (seed, i) alone."""
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or seed < 0:
            raise ValueError("Calibration: seed must be a non-negative integer")
        return np.random.Generator(np.random.Philox(key=int(seed))).random(n)

    def randomised(self, seed, loo=False):
        """u_i = pit_lo_i + v_i (pit_hi_i - pit_lo_i): uniform on (0, 1) if the model holds."""
        lo, hi, _ = self._bounds(loo)
        return lo + self._uniforms(seed, self.n_obs) * (hi - lo)

    def quantile_residuals(self, seed, loo=False):
        """Phi^-1(u_i) of randomised(seed)'s u_i, from the smaller tail: where u_i > 1/2 from
        1 - u_i = sf_i + (1 - v_i) (pit_hi_i - pit_lo_i), so that a large positive residual keeps its accuracy."""
        lo, hi, sf = self._bounds(loo)
        v = self._uniforms(seed, self.n_obs)
        with np.errstate(invalid="ignore"):
            pm = np.maximum(hi - lo, 0.0)
            u, s = lo + v * pm, sf + (1.0 - v) * pm
            low = u <= 0.5
            nan = np.isnan(u) | np.isnan(s)
        r = np.where(low, norm_ppf(p=np.where(low & ~nan, u, 0.5)), norm_ppf(sf=np.where(~low & ~nan, s, 0.5)))
        return np.where(nan, np.nan, r)

    def pit_histogram(self, bins=10, loo=False):
        """The non-randomised PIT histogram: bin b of `bins` gets the mean over the rows of G_i(b / B) - G_i((b - 1) / B),
        G_i(u) = clip((u - lo_i) / (hi_i - lo_i), 0, 1) -- a step at lo_i where hi_i == lo_i -- with G_i(0) = 0 and
        G_i(1) = 1.  Sums to 1; flat (1 / B each) if the model holds.  NaN rows are left out (all NaN: NaN)."""
        if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or not 1 <= bins <= 1000:
            raise ValueError("Calibration.pit_histogram: bins must be an integer in 1..1000")
        lo, hi, _ = self._bounds(loo)
        ok = ~(np.isnan(lo) | np.isnan(hi))
        lo, hi = np.clip(lo[ok], 0.0, 1.0), np.clip(hi[ok], 0.0, 1.0)
        if lo.size == 0:
            return np.full(int(bins), np.nan)
        hi = np.maximum(hi, lo)
        u = (np.arange(int(bins) + 1) / int(bins))[None, :]
        w = (hi - lo)[:, None]
        with np.errstate(invalid="ignore", divide="ignore"):
            G = np.where(w > 0.0, np.clip((u - lo[:, None]) / w, 0.0, 1.0), (u >= lo[:, None]).astype(np.float64))
        G[:, 0], G[:, -1] = 0.0, 1.0
        return np.diff(G, axis=1).mean(0)

    def summary(self):
        """dict(n_obs, n_particles, ess, n_nonfinite, rows): one row per observation, dict(i, pit_lo, pit_hi, sf,
        pit_lo_loo, pit_hi_loo, sf_loo, ninf, n_unconverged)."""
        keys = ("pit_lo", "pit_hi", "sf", "pit_lo_loo", "pit_hi_loo", "sf_loo")
        rows = []
        for i in range(self.n_obs):
            r = dict(i=i)
            r.update({k: float(getattr(self, k)[i]) for k in keys})
            r.update(ninf=int(self.ninf[i]), n_unconverged=int(self.n_unconverged[i]))
            rows.append(r)
        return dict(n_obs=self.n_obs, n_particles=self.n_particles, ess=self.ess,
                    n_nonfinite=int(np.sum(np.isnan(self.pit_lo))), rows=rows)


def combine_calibration_partials(partials):
    """Merges partials blocks of disjoint particle sets in list order and finishes them -> Calibration."""
    partials = list(partials)
    if not partials:
        raise ValueError("combine_calibration_partials: no partials")
    acc = np.array(partials[0], dtype=np.float64, copy=True)
    if acc.ndim != 2 or acc.shape[1] != QC or acc.shape[0] < 2:
        raise ValueError(f"a partials block is [1 + n][{QC}]")
    for p in partials[1:]:
        acc = merge_calibration_partials(acc, p)
    sw, sw2, cnt = acc[0, 1], acc[0, 2], acc[0, 3]
    P = acc[1:]
    n = P.shape[0]
    if cnt == 0.0:
        nan = lambda: np.full(n, np.nan)            # noqa: E731
        return Calibration(nan(), nan(), nan(), nan(), nan(), nan(), np.zeros(n), np.zeros(n), 0, 0.0)
    bad = (P[:, NINF] > 0.0) | (P[:, NUNC] > 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        fin = lambda v: np.where(bad, np.nan, v)    # noqa: E731
        lo, up = fin(P[:, LO] / P[:, SW]), fin(P[:, UP] / P[:, SW])
        lol, upl = fin(P[:, LOB] / P[:, SB]), fin(P[:, UPB] / P[:, SB])
    return Calibration(lo, 1.0 - up, up, lol, 1.0 - upl, upl, P[:, NINF].copy(), P[:, NUNC].copy(), cnt, sw * sw / sw2)
