"""Host references for the wide GLM target (smcnuts_amd.WideGLMTarget; SMCN_MODEL_WGLM): the model is GLMTarget's, so the
densities are tests/_glm.py's and tests/_glm_disp.py's.  What is added here is the tolerance of the trajectory tests at
65..256 coordinates, which is measured instead of assumed:

`tape_reference` runs oracle/pynuts.PyNUTS over the NumPy density and again over `FsumDensity` -- the same density with
every sum (the linear predictor, the log-likelihood, the column sums of the gradient, the prior) taken by math.fsum: two
correct host evaluations of the same trajectories.  The largest difference between the two sets of end points is the
spread two correct evaluations show at this D, n and tree length; the device is allowed 10 times that (the rule of
tests/_tol.py).  The two runs must take the same trees -- a difference is a slice or U-turn comparison within the
rounding of the two, a tie, and the case's seed is changed rather than a particle excluded."""
import functools
import math

import numpy as np

import _glm
import _glm_disp as gd

from oracle.pynuts import PyNUTS

DISP = ("normal", "neg_binomial_2_log")


def synthetic(family, n, p, seed, scale=None):
    return (gd.synthetic if family in DISP else _glm.synthetic)(family, n, p, seed, scale=scale)


def numpy_model(X, y, family, prior_sd=2.0, dispersion_prior=(0.0, 1.0), intercept=True):
    if family in DISP:
        return gd.GLMDispNumpy(X, y, family, prior_sd, dispersion_prior, intercept)
    return _glm.GLMNumpy(X, y, family, prior_sd, intercept)


def wide_target(X, y, family, prior_sd=2.0, dispersion_prior=(0.0, 1.0), intercept=True):
    from smcnuts_amd import WideGLMTarget
    kw = dict(dispersion_prior=dispersion_prior) if family in DISP else {}
    return WideGLMTarget(X, y, family=family, prior_sd=prior_sd, intercept=intercept, **kw)


def _fsum_rows(a):
    return np.array([math.fsum(r) for r in a.tolist()])


class FsumDensity:
    """A GLMNumpy / GLMDispNumpy with the StanModel surface whose sums are math.fsum's (one point at a time)."""

    def __init__(self, model):
        self.m, self.dim = model, model.dim
        self.disp = hasattr(model, "Dc")
        self.Dc = model.Dc if self.disp else model.dim
        self._at, self._parts = None, None

    def parts(self, x):
        """(NUTS asks for the gradient and then the value at one point: the second call is served from the first)"""
        x = np.asarray(x, dtype=np.float64).reshape(-1)
        if self._at is None or not np.array_equal(self._at, x):
            self._at, self._parts = x.copy(), self._evaluate(x)
        return self._parts

    def _evaluate(self, x):
        m = self.m
        eta = _fsum_rows(m.Z * x[:self.Dc])[None, :]
        if self.disp:
            tau = x[-1:]
            tau = np.where(m.bad(tau), 0.0, tau)
            f = gd.normal_obs if m.family == "normal" else gd.nb_obs
            args = (m.y[None, :], eta, tau[:, None]) + ((m.lgy[None, :],) if m.family != "normal" else ())
            term, d, gt = f(*args)[:3]
            mean, s = m.m, m.s
        else:
            # (GLMNumpy.terms computes eta itself: restated here on the fsum eta)
            _, term, d = _TermsOn(m, eta).terms()
            gt, mean, s = None, 0.0, m.s
        v = x - mean
        lpri = math.fsum((-0.5 * (v / s) ** 2 - np.log(s) - _glm.HALF_LOG_2PI).tolist())
        llik = math.fsum(term[0].tolist()) if np.all(np.isfinite(term[0])) else -np.inf
        if self.disp and m.bad(x[-1]):
            llik = -np.inf
        with np.errstate(invalid="ignore"):
            glik = _fsum_rows((d[0][:, None] * m.Z).T)
        if self.disp:
            glik = np.concatenate([glik, [math.fsum(gt[0].tolist())]])
        return lpri, llik, -v / s ** 2, glik

    def logpdf(self, x, phi=1.0):
        lpri, llik, _, _ = self.parts(x)
        lp = lpri + phi * llik
        return lp if np.isfinite(lp) else -np.inf

    def logpdfgrad(self, x, phi=1.0):
        lpri, llik, gpri, glik = self.parts(x)
        if not np.isfinite(lpri + phi * llik):
            return np.full(self.dim, -np.inf)
        return gpri + phi * glik


class _TermsOn:
    """GLMNumpy.terms with a given linear predictor."""

    def __init__(self, m, eta):
        self.m, self.eta = m, eta

    def terms(self):
        m, eta, y = self.m, self.eta, self.m.y
        with np.errstate(over="ignore", invalid="ignore"):
            if m.family == "bernoulli_logit":
                t = np.exp(-np.abs(eta))
                term = np.where(y != 0.0, np.minimum(eta, 0.0), -np.maximum(eta, 0.0)) - np.log1p(t)
                d = y - np.where(eta >= 0.0, 1.0 / (1.0 + t), t / (1.0 + t))
            else:
                mu = np.exp(eta)
                term = (np.where(y == 0.0, 0.0, y * eta) - mu) - m.lgy
                term = np.where(np.isfinite(mu), term, -np.inf)
                d = y - mu
        return eta, term, d


class _PyNUTSDepth(PyNUTS):
    """PyNUTS recording the number of doublings of its tree (the depth the device reports)."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self._lvl, self.top = 0, -1

    def build_tree(self, x, r, grad, logu, direction, depth, phi):
        if self._lvl == 0:
            self.top = depth
        self._lvl += 1
        try:
            return super().build_tree(x, r, grad, logu, direction, depth, phi)
        finally:
            self._lvl -= 1


def _run(model, eps, x, r, tapes):
    N = len(x)
    xo, ro = np.zeros_like(x), np.zeros_like(r)
    nleap, depth, ndraws = np.zeros(N, np.int64), np.zeros(N, np.int64), np.zeros(N, np.int64)
    for i in range(N):
        ref = _PyNUTSDepth(model, eps)
        xo[i:i + 1], ro[i:i + 1] = ref.rvs(x[i:i + 1], r[i:i + 1], 1.0, tapes=[tapes[i]])
        nleap[i], depth[i], ndraws[i] = ref.nleap, ref.top + 1, ref.ndraws[0]
    return xo, ro, nleap, depth, ndraws


N_TAPE, N_OBS = 12, 130


@functools.lru_cache(maxsize=None)
def tape_reference(family, D, eps, seed):
    """The tape case (family, D): data, start points, tapes, the NumPy reference's end points and tree statistics, and
    `tol`, 10 times the spread between the NumPy and the fsum evaluation of the same trajectories."""
    disp = family in DISP
    X, y = synthetic(family, N_OBS, D - 1 - disp, seed, scale=0.5)
    m = numpy_model(X, y, family)
    rng = np.random.default_rng(7 * D + len(family) + seed)
    x = rng.standard_normal((N_TAPE, D)) * 0.1
    if disp:
        x[:, -1] = np.log(0.7 if family == "normal" else 3.0) + 0.1 * rng.standard_normal(N_TAPE)
    r = rng.standard_normal((N_TAPE, D))
    tapes = [np.concatenate([[rng.exponential()], rng.random(2100)]) for _ in range(N_TAPE)]
    xa, ra, nleap, depth, ndraws = _run(m, eps, x, r, tapes)
    xb, rb, nleap_b, depth_b, ndraws_b = _run(FsumDensity(m), eps, x, r, tapes)
    same = np.array_equal(nleap, nleap_b) and np.array_equal(depth, depth_b) and np.array_equal(ndraws, ndraws_b)
    assert same, ("the two host evaluations took different trees (a tie): change this case's seed", family, D,
                  np.flatnonzero((nleap != nleap_b) | (ndraws != ndraws_b)).tolist())
    spread = max(float(np.max(np.abs(xa - xb))), float(np.max(np.abs(ra - rb))))
    return dict(X=X, y=y, model=m, x=x, r=r, tapes=tapes, want_x=xa, want_r=ra, nleap=nleap, depth=depth, ndraws=ndraws,
                spread=spread, tol=10.0 * spread)
