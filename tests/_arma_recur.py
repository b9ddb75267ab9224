"""Exact emulation of the arma recurrence of smcn_nuts3.hpp (ArmaLaneModel::recur) on the host: every fp64 fma is
computed in rational arithmetic and rounded once, so the full form and the two-phase form (mu-sensitivity no longer
updated once it repeats with period <= 2 on every row of a wavefront) can be compared bit for bit without a device."""
import math
from fractions import Fraction

import numpy as np

TRIP = 32          # the wavefront asks "settled?" after every TRIP full steps


def fma(a, b, c):
    """round(a * b + c), one rounding (int / int true division of Fraction.__float__ rounds to nearest even)."""
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        with np.errstate(all="ignore"):
            return float(np.float64(a) * np.float64(b) + np.float64(c))     # NaN / inf: the class of the result is what counts
    r = Fraction(a) * Fraction(b) + Fraction(c)
    if r == 0:
        # an exact zero: the product's and the addend's zero signs combine as in a * b + c; a cancellation gives +0
        return a * b + c if (a == 0.0 or b == 0.0) else 0.0
    return float(r)


def f_mu(nth, dm):
    return fma(nth, dm, -1.0)


def settle_step(theta, beta, limit):
    """The first n <= limit at which dm_n (after n full steps from -(1 + beta)) satisfies f(f(dm)) == dm, and the period
    (1 or 2) it has there; (None, None) if there is none.  Once true it stays true: the orbit repeats."""
    nth = -theta
    dm = -(1.0 + beta)
    for n in range(limit + 1):
        d1 = f_mu(nth, dm)
        d2 = f_mu(nth, d1)
        if d2 == dm:                         # (False for NaN)
            return n, (1 if d1 == dm else 2)
        dm = d1
    return None, None


def expected_switch(settle, T):
    """The switch step of a wavefront whose rows settle at `settle` (None: never), on a series of T observations: the
    first multiple m of TRIP with m >= every row's settle step and m <= T - 1 (the steps there are); 0 if none."""
    if any(s is None for s in settle):
        return 0
    m = max(TRIP, -(-max(settle) // TRIP) * TRIP)
    return m if m <= T - 1 else 0


class _Row:
    __slots__ = ("mu", "nth", "nbeta", "err", "dm", "db", "dt", "d1", "ss", "gm", "gb", "gt")

    def __init__(self, x, y0):
        mu, beta, theta = float(x[0]), float(x[1]), float(x[2])
        self.mu, self.nth, self.nbeta = mu, -theta, -beta
        self.err = fma(self.nbeta, mu, y0 - mu)
        self.dm, self.db, self.dt, self.d1 = -(1.0 + beta), -mu, 0.0, 0.0
        with np.errstate(all="ignore"):
            self.ss, self.gm, self.gb = (float(np.float64(self.err) * np.float64(v)) for v in (self.err, self.dm, self.db))
        self.gt = 0.0

    def step(self, settled, k, yp, yt):
        nth = self.nth
        self.dt = fma(nth, self.dt, -self.err)
        if not settled:
            self.dm = fma(nth, self.dm, -1.0)
        self.db = fma(nth, self.db, -yp)
        c = fma(self.nbeta, yp, yt - self.mu)
        self.err = fma(nth, self.err, c)
        self.ss = fma(self.err, self.err, self.ss)
        self.gm = fma(self.err, self.d1 if (settled and not (k & 1)) else self.dm, self.gm)
        self.gb = fma(self.err, self.db, self.gb)
        self.gt = fma(self.err, self.dt, self.gt)


def recur_wave(y, X, two_phase):
    """The four sums of every row of X (<= 64 rows: one wavefront) on the series y, and the wavefront's switch step.
    The groups of steps are those of the kernel: full trips of 32 up to the switch, settled trips of 32 (two rounds of 16,
    the parity restarting in each) while 32 steps are left, then the FULL step again for the last 0..31 (an even number of
    settled steps leaves dm where the full step expects it)."""
    y = [float(v) for v in y]
    T = len(y)
    rows = [_Row(x, y[0]) for x in X]
    t = 1                                    # steps done + 1; the next step reads y[t - 1], y[t]

    def group(settled, n):
        nonlocal t
        for k in range(n):
            for r in rows:
                r.step(settled, k, y[t - 1], y[t])
            t += 1

    sw = 0
    if two_phase:
        while t + TRIP <= T:
            group(False, 16)
            group(False, 16)
            for r in rows:
                r.d1 = f_mu(r.nth, r.dm)
            if not any(not (f_mu(r.nth, r.d1) == r.dm) for r in rows):
                sw = t - 1
                break
        if sw:
            while t + TRIP <= T:
                group(True, 16)
                group(True, 16)
    while t + 16 <= T:
        group(False, 16)
    rem = T - t
    for n in (8, 4, 2, 1):
        if rem >= n:
            group(False, n)
            rem -= n
    assert t == T
    return np.array([[r.ss, r.gm, r.gb, r.gt] for r in rows], dtype=np.float64).reshape(len(rows), 4), sw


def recur_float(y, X):
    """The four sums in extended precision without exactness (vectorised over rows): the reference of a 1e-12 tolerance."""
    L = np.longdouble
    y = np.asarray(y, dtype=L)
    X = np.asarray(X, dtype=L)
    mu, beta, theta = X[:, 0], X[:, 1], X[:, 2]
    with np.errstate(all="ignore"):
        err = y[0] - mu - beta * mu
        dm, db, dt = -(1 + beta), -mu, np.zeros_like(mu)
        ss, gm, gb, gt = err * err, err * dm, err * db, np.zeros_like(mu)
        for t in range(1, len(y)):
            dt = -theta * dt - err
            dm = -theta * dm - 1
            db = -theta * db - y[t - 1]
            err = y[t] - mu - beta * y[t - 1] - theta * err
            ss, gm, gb, gt = ss + err * err, gm + err * dm, gb + err * db, gt + err * dt
    return np.stack([ss, gm, gb, gt], axis=1).astype(np.float64)


def two_cycle_thetas(beta, count, seed=0, limit=96, hi=0.45):
    """`count` values of theta in (0.02, hi) whose mu-sensitivity ends, within `limit` steps, in a genuine 2-cycle."""
    rng = np.random.default_rng(seed)
    out = []
    for th in rng.uniform(0.02, hi, size=4000):
        n, period = settle_step(float(th), beta, limit)
        if period == 2:
            out.append(float(th))
            if len(out) == count:
                break
    return out
