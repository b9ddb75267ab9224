"""The step-size probe restated in NumPy (smcnuts_amd/csrc/smcn_stepsize.hpp): the same leapfrog order, statistic,
divergence rule, subsampling and weighted reduction, over lp(x) / grad(x) callbacks ([M][D] -> [M] / [M][D]); analytic
callbacks for the targets that have a closed form in a few lines; and the case table the host and GPU tests share.
NumPy only: importing this module touches neither the library nor a device."""
import json
import math
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_LEAP = 8
OCTAVES = 2.0 ** (-6.0 + np.arange(16) / 2.0)       # the ladder of the per-particle comparisons
BAND = 20.0                                         # |dH| beyond which rounding has been amplified out of the exact class
CAP = 0.25                                          # entries beyond the band: at most this share of a case's L * M


def probe_reference(lp, grad, x, r, ladder, n=N_LEAP, logw=None, delta_max=100.0, max_particles=None):
    """dict(accept [L][Mp], first_bad [L][Mp], max_dh [L][Mp] (largest |dH_t| met, inf for a non-finite one), dh
    [L][Mp][n] (dH_t of the steps taken, NaN behind a stop), excluded [Mp], index [Mp], partials [1 + L][4]).  r
    [Mp][D]: the momenta of the probed particles."""
    x = np.asarray(x, dtype=np.float64)
    M = x.shape[0]
    Mp = M if max_particles is None else min(M, int(max_particles))
    idx = (np.arange(Mp, dtype=np.int64) * M) // Mp
    lw = np.zeros(M) if logw is None else np.asarray(logw, dtype=np.float64)
    xs, lws, r = x[idx], lw[idx], np.asarray(r, dtype=np.float64)
    assert r.shape == xs.shape
    ladder = np.asarray(ladder, dtype=np.float64)
    L = ladder.size
    with np.errstate(all="ignore"):
        lp0, g0 = np.asarray(lp(xs), dtype=np.float64), np.asarray(grad(xs), dtype=np.float64)
        excl = ~np.isfinite(lp0) | ~np.isfinite(lws)
        H0 = 0.5 * np.sum(r * r, axis=1) - lp0
        accept, first_bad, max_dh = np.zeros((L, Mp)), np.zeros((L, Mp), dtype=np.int32), np.zeros((L, Mp))
        dh = np.full((L, Mp, n), np.nan)
        for j, eps in enumerate(ladder):
            xx, rr, g = xs.copy(), r.copy(), g0.copy()
            done, acc = excl.copy(), np.zeros(Mp)
            for t in range(1, n + 1):
                act = ~done
                if not act.any():
                    break
                rr[act] += 0.5 * eps * g[act]
                xx[act] += eps * rr[act]
                lpt, gt = np.asarray(lp(xx), dtype=np.float64), np.asarray(grad(xx), dtype=np.float64)
                g[act] = gt[act]
                rr[act] += 0.5 * eps * g[act]
                dH = 0.5 * np.sum(rr * rr, axis=1) - lpt - H0
                dh[j, act, t - 1] = dH[act]
                bad = act & (~np.isfinite(dH) | (dH > delta_max))
                ok = act & ~bad
                first_bad[j, bad] = t
                done |= bad
                acc[ok] += np.minimum(1.0, np.exp(-dH[ok]))
                a = np.where(np.isfinite(dH), np.abs(dH), np.inf)
                max_dh[j, act] = np.maximum(max_dh[j, act], a[act])
            accept[j] = np.where(excl, 0.0, acc / n)
        fin = np.isfinite(lws)
        m = lws[fin].max() if fin.any() else -np.inf
        part = np.zeros((1 + L, 4))
        part[0] = (m, Mp, excl.sum(), 0.0)
        w = np.where(excl, 0.0, np.exp(lws - m))
        for j in range(L):
            d = (first_bad[j] != 0) & ~excl
            part[1 + j] = (np.sum(w * accept[j]), np.sum(w * d), np.sum(w), d.sum())
    return dict(accept=accept, first_bad=first_bad, max_dh=max_dh, dh=dh, excluded=excl, index=idx, partials=part)


def beyond_band(ref):
    """Entries whose reference |dH| left the band (or that the reference calls divergent): not compared in the exact class."""
    return (ref["max_dh"] > BAND) | (ref["first_bad"] != 0)


def compare_entries(ref, accept, first_bad, close, **tol):
    """The per-particle comparison of a case.  Entries inside the band: accept through `close` (the exact class) and the
    same first-bad step.  Beyond it rounding has been amplified geometrically: where the reference says divergent, the
    divergent flag; otherwise accept <= exp(-BAND) where every step of the reference lies beyond the band on the
    divergent side -- and for the rest (the energy error left the band at step t* only, or left it downwards, so the
    statistic is NOT small) the steps before t* are still exact: their share of the statistic bounds it from below, and
    that share plus one per later step from above.  Returns the share of entries beyond the band."""
    far = beyond_band(ref)
    share = float(np.mean(far))
    assert share <= CAP, f"{share:.3f} of the entries lie beyond the band: change the case, not the cap"
    assert accept.shape == far.shape and first_bad.shape == far.shape
    near = ~far
    np.testing.assert_array_equal(first_bad[near], 0)
    close(accept[near], ref["accept"][near], **tol)
    div = ref["first_bad"] != 0
    assert np.all(first_bad[div] != 0), "pairs the reference calls divergent"
    rest = far & ~div
    dh = ref["dh"]
    n = dh.shape[2]
    small = math.exp(-BAND)
    for j, k in zip(*np.nonzero(rest)):
        d = dh[j, k]
        if np.all(d > BAND):
            assert accept[j, k] <= small
            continue
        t0 = int(np.argmax(np.abs(d) > BAND))                  # steps [0, t0) are inside the band
        lo = float(np.sum(np.minimum(1.0, np.exp(-d[:t0])))) / n
        assert lo - 1e-9 <= accept[j, k] <= lo + (n - t0) / n + 1e-9
    return share


# ---- analytic callbacks -------------------------------------------------------------------------------------------------
def gaussian(D, s=1.0):
    """N(0, s^2 I)."""
    c = -D * math.log(s) - 0.5 * D * math.log(2.0 * math.pi)
    return (lambda x: -0.5 * np.sum(x * x, axis=1) / (s * s) + c), (lambda x: -x / (s * s))


def _eta(X, x, intercept, offset):
    eta = x[:, 1:] @ X.T + x[:, :1] if intercept else x @ X.T
    return eta if offset is None else eta + offset


def _design_grad(X, resid, intercept):
    g = resid @ X
    return np.concatenate([resid.sum(axis=1, keepdims=True), g], axis=1) if intercept else g


def logistic(X, y, prior_sd=2.5, intercept=True):
    """Logistic regression with N(0, prior_sd^2) priors; the intercept is coordinate 0."""
    def lp(x):
        eta = _eta(X, x, intercept, None)
        return np.sum(y * eta - np.logaddexp(0.0, eta), axis=1) - 0.5 * np.sum(x * x, axis=1) / prior_sd ** 2 \
            - x.shape[1] * (math.log(prior_sd) + 0.5 * math.log(2.0 * math.pi))

    def grad(x):
        eta = _eta(X, x, intercept, None)
        return _design_grad(X, y - 1.0 / (1.0 + np.exp(-eta)), intercept) - x / prior_sd ** 2
    return lp, grad


def poisson(X, y, prior_sd=2.5, intercept=True, offset=None, weights=None):
    """Poisson regression with a log link, optional offsets and weights."""
    w = np.ones_like(y) if weights is None else weights
    lgy = np.array([math.lgamma(v + 1.0) for v in y])

    def lp(x):
        eta = _eta(X, x, intercept, offset)
        return np.sum(w * (y * eta - np.exp(eta) - lgy), axis=1) - 0.5 * np.sum(x * x, axis=1) / prior_sd ** 2 \
            - x.shape[1] * (math.log(prior_sd) + 0.5 * math.log(2.0 * math.pi))

    def grad(x):
        eta = _eta(X, x, intercept, offset)
        return _design_grad(X, w * (y - np.exp(eta)), intercept) - x / prior_sd ** 2
    return lp, grad


def target_callbacks(target, phi=1.0):
    """Any other target: its own logpdf / logpdfgrad (which have parity tests of their own)."""
    return (lambda x: target.logpdf(np.ascontiguousarray(x), phi=phi)), \
        (lambda x: target.logpdfgrad(np.ascontiguousarray(x), phi=phi))


# ---- the case table -------------------------------------------------------------------------------------------------------
# A builder returns dict(make: () -> target (imports the product), callbacks: (lp, grad) or None: the target's own, D).
# Starting points and momenta: case_points(); the ladder: case_ladder().
GLM_M = 37


def _xy(seed, n, p, scale):
    rng = np.random.default_rng(seed)
    X = scale * rng.standard_normal((n, p))
    b = 0.5 * rng.standard_normal(p)
    return rng, X, X @ b


def _gauss(D):
    def build():
        def make():
            from smcnuts_amd import GaussianTarget
            return GaussianTarget(D)
        return dict(make=make, callbacks=gaussian(D), D=D)
    return build


def _logistic(p, seed):
    def build():
        rng, X, eta = _xy(seed, 40, p, 0.35)
        y = (rng.random(40) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)

        def make():
            from smcnuts_amd import LogisticRegression
            return LogisticRegression(X, y)
        return dict(make=make, callbacks=logistic(X, y), D=p + 1)
    return build


def _poisson_ow(p, seed):
    def build():
        rng, X, eta = _xy(seed, 40, p, 0.4)
        off = 0.3 * rng.standard_normal(40)
        w = rng.integers(0, 3, 40).astype(np.float64)
        w[0] = 1.0
        y = rng.poisson(np.exp(eta + off)).astype(np.float64)

        def make():
            from smcnuts_amd import PoissonRegression
            return PoissonRegression(X, y, offset=off, weights=w)
        return dict(make=make, callbacks=poisson(X, y, offset=off, weights=w), D=p + 1)
    return build


def _negbin(p, seed, ow=False):
    def build():
        rng, X, eta = _xy(seed, 40, p, 0.4)
        y = rng.poisson(np.exp(eta) * rng.gamma(3.0, 1.0 / 3.0, 40)).astype(np.float64)
        kw = dict(offset=0.2 * rng.standard_normal(40), weights=rng.integers(1, 3, 40).astype(np.float64)) if ow else {}

        def make():
            from smcnuts_amd import NegativeBinomialRegression
            return NegativeBinomialRegression(X, y, **kw)
        return dict(make=make, callbacks=None, D=p + 2)
    return build


def _logistic_ow(p, seed):
    def build():
        rng, X, eta = _xy(seed, 40, p, 0.5)
        off = 0.3 * rng.standard_normal(40)
        y = (rng.random(40) < 1.0 / (1.0 + np.exp(-eta - off))).astype(np.float64)
        w = rng.integers(1, 3, 40).astype(np.float64)

        def make():
            from smcnuts_amd import LogisticRegression
            return LogisticRegression(X, y, offset=off, weights=w)
        return dict(make=make, callbacks=None, D=p + 1)
    return build


def _hier(seed):
    def build():
        rng, X, eta = _xy(seed, 40, 2, 0.5)
        groups = rng.integers(0, 3, 40)
        y = (rng.random(40) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)

        def make():
            from smcnuts_amd import HierarchicalGLM
            return HierarchicalGLM(X, y, groups, n_groups=3)
        return dict(make=make, callbacks=None, D=3 + 3 + 1)
    return build


def _multi(seed):
    def build():
        rng, X, eta = _xy(seed, 40, 2, 0.5)
        g1, g2, z = rng.integers(0, 3, 40), rng.integers(0, 4, 40), 0.5 * rng.standard_normal(40)
        y = rng.poisson(np.exp(0.5 * eta)).astype(np.float64)

        def make():
            from smcnuts_amd import MultilevelGLM
            return MultilevelGLM(X, y, [(g1, None, 3), (g2, z, 4)], family="poisson_log")
        return dict(make=make, callbacks=None, D=3 + 3 + 4 + 2)
    return build


def _wide(p, seed):
    def build():
        rng, X, eta = _xy(seed, 40, p, 0.25)
        y = (rng.random(40) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)

        def make():
            from smcnuts_amd import WideGLMTarget
            return WideGLMTarget(X, y)
        return dict(make=make, callbacks=logistic(X, y), D=p + 1)
    return build


def _cat(K, p, seed):
    def build():
        rng, X, _ = _xy(seed, 40, p, 0.5)
        y = rng.integers(0, K, 40)
        y[:K] = np.arange(K)

        def make():
            from smcnuts_amd import CategoricalRegression
            return CategoricalRegression(X, y, n_classes=K)
        return dict(make=make, callbacks=None, D=(K - 1) * (p + 1))
    return build


def _ord(K, p, seed):
    def build():
        rng, X, _ = _xy(seed, 40, p, 0.5)
        y = rng.integers(0, K, 40)
        y[:K] = np.arange(K)

        def make():
            from smcnuts_amd import OrdinalRegression
            return OrdinalRegression(X, y, n_classes=K)
        return dict(make=make, callbacks=None, D=p + K - 1)
    return build


def _arma(tmp_path):
    """The shipped series truncated to T = 20, through a JSON in tmp_path."""
    src = os.path.join(ROOT, "smcnuts_amd", "model", "data", "arma.json")
    d = json.load(open(src))
    d["y"], d["T"] = list(d["y"])[:20], 20
    path = os.path.join(str(tmp_path), "arma20.json")
    json.dump(d, open(path, "w"))
    from smcnuts_amd import ArmaModel
    return ArmaModel(path)


def _prmwcd(tmp_path):
    from smcnuts_amd import PRMwCDModel
    return PRMwCDModel()


CASES = {
    # name: (builder or None: made by `SPECIAL[name](tmp_path)` (needs the product), M, spread of the starts, octaves the
    # ladder is shifted by: stiffer targets meet the stability limit earlier, and the cap is a condition on the case)
    "gauss_d3": (_gauss(3), 5, 1.0, 0),
    "gauss_d5": (_gauss(5), 37, 1.0, 0),
    "gauss_d65": (_gauss(65), 9, 1.0, 0),
    "gauss_d257": (_gauss(257), 3, 1.0, 0),
    "arma_t20": (None, 70, 0.3, -4),
    "logistic_d5": (_logistic(4, 11), GLM_M, 0.5, -1),
    "logistic_d17": (_logistic(16, 12), GLM_M, 0.5, -1),
    "negbin_d4": (_negbin(2, 13), GLM_M, 0.3, -2),
    "negbin_d9": (_negbin(7, 14), GLM_M, 0.3, -2),
    "poisson_ow_d5": (_poisson_ow(4, 15), GLM_M, 0.3, -2),
    "negbin_ow_d4": (_negbin(2, 16, ow=True), GLM_M, 0.3, -2),
    "negbin_ow_d9": (_negbin(7, 17, ow=True), GLM_M, 0.3, -2),
    "logistic_ow_d17": (_logistic_ow(16, 18), GLM_M, 0.5, -1),
    "hier_j3": (_hier(19), GLM_M, 0.3, -1),
    "multi_r2": (_multi(20), GLM_M, 0.3, -2),
    "wide_d65": (_wide(64, 21), GLM_M, 0.3, 0),
    "wide_d129": (_wide(128, 22), GLM_M, 0.3, 0),
    "cat_3x2": (_cat(3, 1, 23), GLM_M, 0.5, -1),
    "cat_4x4": (_cat(4, 3, 24), GLM_M, 0.5, -1),
    "ord_d4": (_ord(3, 2, 25), GLM_M, 0.3, -2),
    "ord_d12": (_ord(5, 8, 26), GLM_M, 0.3, -2),
    "prmwcd": (None, GLM_M, 0.2, -5),
}
SPECIAL = {"arma_t20": _arma, "prmwcd": _prmwcd}


def case_ladder(name):
    return OCTAVES * 2.0 ** CASES[name][3]


ANALYTIC = [k for k, v in CASES.items() if v[0] is not None and v[0]()["callbacks"] is not None]


def case_points(name, D):
    """(x [M][D], r [M][D]) of a case: starts spread about the origin, standard normal momenta, seeded by the name."""
    _, M, spread, _ = CASES[name]
    rng = np.random.default_rng(sum(ord(ch) * (i + 1) for i, ch in enumerate(name)))
    return spread * rng.standard_normal((M, D)), rng.standard_normal((M, D))
