"""The Gaussian-approximation L-kernel against a 50-digit reference: the reference, the populations and the driver shared by
tests/test_glk_host.py (CPU) and tests/test_gpu_glk.py (device).

exact()       the reference's formulation (lkernel/gaussian_lkernel.py:39-66: mean, np.cov with N - 1, the inverse of c_xx,
              B = c_rx c_xx^-1, cov = c_rr - B c_xr + 1e-6 I, log-density of N(m0 + B (x - mu_x), cov) at -r) in mpmath at 50
              digits on the float64 inputs taken exactly.  Where both matrices are positive definite the reference's pinv is
              the inverse and scipy's eigh-based pseudo-determinant / pseudo-inverse are the determinant and the inverse,
              so this is what its calls compute, without their rounding.
exact_sums()  the moment sums of smcn_gauss_lkernel_sums (E singles, upper triangle of the products of X - shift), each with
              the sum of the magnitudes of its terms.
host_L, chol_L  two float64 restatements (the reference's own pinv / eigh calls; a plain Cholesky route).  They are
              YARDSTICKS: their error against exact() is what float64 costs on a population, and the device is allowed
              MARGIN times the larger of the two.  Neither is the code under test.
population()  fixed-seed populations by name (CASES), every one built like the population of
              test_gpu_parity.py::test_gaussian_lkernel_algebra_on_the_device.
read_L()      the device's L values, bit for bit, through the public entry points.
"""
import functools
import math

import numpy as np

import mpmath

from _exact import LD, MP_MAX, WIDE_LD, _ld_sum

U64 = 2.0 ** -53
DPS = 50
RIDGE = 1e-6                   # gaussian_lkernel.py:68, the double nearest to 1e-6 (what np.eye(D) * 1e-6 adds)
MAX_COND = 1e8                 # kGlkMaxCond (smcn_glk.hpp): the estimate beyond which the device refuses
MARGIN = 8.0                   # the device may be MARGIN x the yardstick away from exact()
YARD_FLOOR = 16 * U64
MP_WORK = 200_000              # exact_sums: mpmath up to this many products per call (and MP_MAX terms per sum)

# name: D, N, and what shapes the population.  decades: the columns of x scaled over that many decades; far: the mean of
# x (r gets a quarter of it, negated); uniq: N particles drawn with replacement from that many distinct ones.
CASES = {
    "d1_n2": dict(D=1, N=2),
    "d1": dict(D=1, N=257),
    "d2": dict(D=2, N=65),
    "d3": dict(D=3, N=1000),
    "d5_2d2": dict(D=5, N=12),
    "d5_d3": dict(D=5, N=8),
    "d5_d1": dict(D=5, N=6),
    "d5_d": dict(D=5, N=5),
    "d5_255": dict(D=5, N=255),
    "d5_256": dict(D=5, N=256),
    "d5_257": dict(D=5, N=257),
    "d13_s2": dict(D=13, N=513, decades=2.0),
    "d13_s3": dict(D=13, N=513, decades=3.0),
    "d13_s45": dict(D=13, N=513, decades=4.5),
    "d8_far": dict(D=8, N=513, far=1e6),
    "d13_u40": dict(D=13, N=1024, uniq=40),
    "d13_u27": dict(D=13, N=1024, uniq=27),
    "d13_u20": dict(D=13, N=1024, uniq=20),
    "d13_u13": dict(D=13, N=1024, uniq=13),
    "d16": dict(D=16, N=257),
    "d17": dict(D=17, N=257),
    "d32_70": dict(D=32, N=70),
    "d32_65": dict(D=32, N=65),
}
# what the case list is built to contain (test_glk_host.py asserts that the exact condition numbers put them there)
INTENDED = {"d13_s2": "accept", "d5_d": "refuse", "d13_s45": "refuse", "d13_u13": "refuse", "d13_s3": "either"}
# must-refuse cases on which the reference's own calls (pinv's cut-off, eigh) still give finite values
HOST_ANSWERS = ("d5_d", "d13_s45", "d13_u13")
SEED = 7


@functools.lru_cache(maxsize=None)
def population(name):
    """(r_new, x_new), each [N][D] float64 and read-only: x = z A (* column scales) (+ mean), r correlated with x."""
    c = CASES[name]
    D, N = c["D"], c["N"]
    rng = np.random.default_rng(c.get("seed", SEED))
    M = c.get("uniq") or N
    A = rng.standard_normal((D, D)) / np.sqrt(D) + np.eye(D)
    x = rng.standard_normal((M, D)) @ A
    if "decades" in c:
        x = x * 10.0 ** np.linspace(0.0, -c["decades"], D)
    r = 0.4 * x @ rng.standard_normal((D, D)) / np.sqrt(D) + rng.standard_normal((M, D)) * rng.uniform(0.5, 2.0, D)
    if "far" in c:
        x = x + c["far"]
        r = r - 0.25 * c["far"]
    if "uniq" in c:
        idx = rng.integers(0, M, N)
        idx[:M] = np.arange(M)                 # every distinct particle is there at least once
        x, r = x[idx], r[idx]
    r, x = np.ascontiguousarray(r), np.ascontiguousarray(x)
    r.setflags(write=False)
    x.setflags(write=False)
    return r, x


# ---- the 50-digit reference --------------------------------------------------------------------------------------------------
def _mp(v):
    return mpmath.mpf(float(v))


def _cond(Mx):
    """Exact 2-norm condition number of a symmetric matrix: (cond or inf, singular) -- singular: an eigenvalue <= 0 or a
    condition number beyond 1e30 (an exactly singular matrix at 50 digits)."""
    ev = mpmath.eigsy(Mx, eigvals_only=True)
    ev = sorted(ev[i] for i in range(len(ev)))
    if ev[0] <= 0 or ev[-1] / ev[0] > mpmath.mpf(10) ** 30:
        return math.inf, True
    return float(ev[-1] / ev[0]), False


def _key(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a.tobytes(), a.shape


def exact(r_new, x_new):
    """dict(singular, cond_xx, cond_cov, and unless singular: L [N], c0, scale [N] = |c0| + maha / 2, maha [N],
    mu_x, m0 [D], B, U = Lc^-T [D][D] -- everything rounded to float64 once)."""
    (rb, shape), (xb, _) = _key(r_new), _key(x_new)
    return _exact_cached(rb, xb, shape)


@functools.lru_cache(maxsize=None)
def _exact_cached(rb, xb, shape):
    r = np.frombuffer(rb, dtype=np.float64).reshape(shape)
    x = np.frombuffer(xb, dtype=np.float64).reshape(shape)
    N, D = shape
    E = 2 * D
    with mpmath.workdps(DPS):
        cols = [[_mp(-v) for v in r[:, c]] for c in range(D)] + [[_mp(v) for v in x[:, c]] for c in range(D)]
        mu = [mpmath.fsum(col) / N for col in cols]
        cen = [[v - m for v in col] for col, m in zip(cols, mu)]
        C = mpmath.zeros(E, E)
        for a in range(E):
            for b in range(a, E):
                C[a, b] = C[b, a] = mpmath.fdot(cen[a], cen[b]) / (N - 1)
        c_rr, c_rx, c_xx = C[:D, :D], C[:D, D:], C[D:, D:]
        cond_xx, singular = _cond(c_xx)
        if singular:
            return dict(singular=True, cond_xx=math.inf, cond_cov=math.nan)
        B = c_rx * mpmath.inverse(c_xx)
        cov = c_rr - B * c_rx.T + mpmath.eye(D) * _mp(RIDGE)
        cond_cov, bad = _cond(cov)
        if bad:
            return dict(singular=True, cond_xx=cond_xx, cond_cov=math.inf)
        Lc = mpmath.cholesky(cov)
        Li = mpmath.inverse(Lc)                                  # U^T = Lc^-1: |Lc^-1 d|^2 = d^T cov^-1 d
        c0 = -(D * mpmath.log(2 * mpmath.pi) + 2 * mpmath.fsum(mpmath.log(Lc[k, k]) for k in range(D))) / 2
        m0, mu_x = mu[:D], mu[D:]
        # identical particles (a population just after resampling) share their value
        rows = np.hstack([r, x]).view(np.uint64)
        _, first, inv = np.unique(rows, axis=0, return_index=True, return_inverse=True)
        maha_u = []
        for i in first:
            dx = [cols[D + d][i] - mu_x[d] for d in range(D)]
            dev = [cols[c][i] - m0[c] - mpmath.fdot([B[c, d] for d in range(D)], dx) for c in range(D)]
            z = [mpmath.fdot([Li[e, c] for c in range(D)], dev) for e in range(D)]
            maha_u.append(mpmath.fsum(v * v for v in z))
        inv = np.asarray(inv).reshape(-1)
        L = np.array([float(c0 - maha_u[j] / 2) for j in inv])
        maha = np.array([float(maha_u[j]) for j in inv])
        f = lambda Mx: np.array([[float(Mx[i, j]) for j in range(D)] for i in range(D)])
        out = dict(singular=False, cond_xx=cond_xx, cond_cov=cond_cov, L=L, c0=float(c0), maha=maha,
                   scale=abs(float(c0)) + 0.5 * maha, mu_x=np.array([float(v) for v in mu_x]),
                   m0=np.array([float(v) for v in m0]), B=f(B), U=f(Li).T.copy())
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def exact_case(name):
    return exact(*population(name))


def decision(ex, D):
    """The class of a population from its exact condition numbers: the device's estimate e of a matrix satisfies
    cond <= e <= D^1.5 cond (trace <= D lambda_max, |M^-1|_F <= sqrt(D) / lambda_min), and it answers iff both estimates are
    below MAX_COND.  1 % on either side for the rounding of the estimate itself."""
    if ex["singular"] or max(ex["cond_xx"], ex["cond_cov"]) > 1.01 * MAX_COND:
        return "refuse"
    if 1.01 * D ** 1.5 * max(ex["cond_xx"], ex["cond_cov"]) < MAX_COND:
        return "accept"
    return "either"


# ---- the moment sums ---------------------------------------------------------------------------------------------------------
def exact_sums(r_new, x_new, shift):
    """(sums, mags), each [E + E (E + 1) / 2] in the order of smcn_gauss_lkernel_sums: the E sums of X - shift, then the
    upper triangle (row-major) of the sums of products, X = [-r_new, x_new]; mags the sums of the terms' magnitudes.
    mpmath at 50 digits up to MP_MAX terms per sum (and MP_WORK products in all); beyond, long double with pairwise sums
    (numpy along the contiguous axis), math.fsum where long double is no wider than float64 -- as tests/_exact.py."""
    r, x = np.asarray(r_new, dtype=np.float64), np.asarray(x_new, dtype=np.float64)
    N, D = x.shape
    E = 2 * D
    nq = E + E * (E + 1) // 2
    shift = np.asarray(shift, dtype=np.float64)
    sums, mags = np.empty(nq), np.empty(nq)
    if N <= MP_MAX and nq * N <= MP_WORK:
        with mpmath.workdps(DPS):
            cols = [[_mp(-v) - _mp(shift[c]) for v in r[:, c]] for c in range(D)] + \
                   [[_mp(v) - _mp(shift[D + c]) for v in x[:, c]] for c in range(D)]
            q = E
            for a in range(E):
                sums[a] = float(mpmath.fsum(cols[a]))
                mags[a] = float(mpmath.fsum(abs(v) for v in cols[a]))
                for b in range(a, E):
                    t = [u * v for u, v in zip(cols[a], cols[b])]
                    sums[q] = float(mpmath.fsum(t))
                    mags[q] = float(mpmath.fsum(abs(v) for v in t))
                    q += 1
        return sums, mags
    Xt = np.ascontiguousarray(np.hstack([-r, x]).T).astype(LD) - shift.astype(LD)[:, None]     # [E][N]
    q = E
    for a in range(E):
        sums[a] = float(_ld_sum(Xt[a]))
        mags[a] = float(_ld_sum(np.abs(Xt[a])))
        P = Xt[a] * Xt[a:]                                       # [E - a][N], the terms of a row of the triangle
        if WIDE_LD:
            sums[q:q + E - a] = np.sum(P, axis=1, dtype=LD).astype(np.float64)
            mags[q:q + E - a] = np.sum(np.abs(P), axis=1, dtype=LD).astype(np.float64)
        else:
            sums[q:q + E - a] = [float(_ld_sum(p)) for p in P]
            mags[q:q + E - a] = [float(_ld_sum(np.abs(p))) for p in P]
        q += E - a
    return sums, mags


def sums_depth(N, D):
    """Longest chain of additions of one moment sum on the device, read off the loops of glk_sums_kernel and
    sum_final_kernel (smcn_weights.hpp) as smcn_gauss_lkernel_sums launches them:

        TP = 256 (D <= 16) or 64 particles per tile; ntiles = ceil(N / TP); nb = min(ntiles, kMaxPart = 1024) blocks
        one():           a lane adds its terms k = lane, lane + 64, ... of the tile      ceil(TP / 64)
        wave_sum:        the wavefront's butterfly                                        6
        acc[q] += s:     once per tile of the block's grid-stride loop                    ceil(ntiles / nb)
        sum_final_kernel: a thread adds partials i, i + 256, ...                          ceil(nb / 256)
                          block_sum over 256 threads                                      8

    A change of either kernel's loop structure changes this sum, and the bound of test_gpu_glk.py with it."""
    TP = 256 if D <= 16 else 64
    ntiles = -(-N // TP)
    nb = min(ntiles, 1024)
    return -(-TP // 64) + 6 + -(-ntiles // nb) + -(-nb // 256) + 8


# ---- float64 yardsticks ------------------------------------------------------------------------------------------------------
class _Dim:
    def __init__(self, D):
        self.dim = D


def host_L(r_new, x_new):
    """GaussianApproxLKernel.calculate_L: the reference's own np.cov / pinv / eigh calls."""
    from smcnuts_amd.lkernel.gaussian_lkernel import GaussianApproxLKernel
    r, x = np.asarray(r_new), np.asarray(x_new)
    return GaussianApproxLKernel(_Dim(x.shape[1]), x.shape[0]).calculate_L(r, x)


def logpdf_np(r_new, x_new, mu_x, m0, B, U, c0):
    """L_i = c0 - |U^T (-r_i - m0 - B (x_i - mu_x))|^2 / 2 in plain NumPy."""
    dev = (-np.asarray(r_new)) - (m0 + (np.asarray(x_new) - mu_x) @ B.T)
    return c0 - 0.5 * np.sum(np.square(dev @ U), axis=1)


def chol_L(r_new, x_new):
    """The same formulas by a plain Cholesky route (np.linalg.cholesky, explicit inverses of the factors)."""
    r, x = np.asarray(r_new), np.asarray(x_new)
    D = x.shape[1]
    X = np.hstack([-r, x])
    mu, C = np.mean(X, axis=0), np.atleast_2d(np.cov(X.T))
    c_rr, c_rx, c_xx = C[:D, :D], C[:D, D:], C[D:, D:]
    Li = np.linalg.inv(np.linalg.cholesky(c_xx))
    B = c_rx @ (Li.T @ Li)
    cov = c_rr - B @ c_rx.T + np.eye(D) * RIDGE
    Lc = np.linalg.cholesky(cov)
    c0 = -0.5 * (D * np.log(2 * np.pi) + 2.0 * np.sum(np.log(np.diag(Lc))))
    return logpdf_np(r, x, mu[D:], mu[:D], B, np.linalg.inv(Lc).T, c0)


def rel_err(L, ex):
    """max_i |L_i - exact_i| / scale_i over EVERY particle (inf if any value is not finite)."""
    L = np.asarray(L, dtype=np.float64)
    if not np.all(np.isfinite(L)):
        return math.inf
    return float(np.max(np.abs(L - ex["L"]) / ex["scale"]))


def yardstick(r_new, x_new, ex, others=()):
    """max(err(host_L), err(chol_L), 16 u) relative to scale -- what float64 costs on this population."""
    errs = [rel_err(host_L(r_new, x_new), ex), rel_err(chol_L(r_new, x_new), ex)] + [rel_err(o, ex) for o in others]
    return max(errs + [YARD_FLOOR])


# ---- the driver --------------------------------------------------------------------------------------------------------------
def gauss_ctx(N, D):
    from smcnuts_amd import GaussianTarget, _capi
    t = GaussianTarget(D)
    return _capi.Context(N, t.model_id, t.model_data)


def load(ctx, r_new, x_new):
    """The state read_L needs: x = x_new and logw = 0, the proposal (r, x_new, r_new) -- both density evaluations on the
    same values, so p(x') - p(x) is exactly 0 -- and q = 0."""
    from smcnuts_amd import _capi
    x, r = np.ascontiguousarray(x_new, dtype=np.float64), np.ascontiguousarray(r_new, dtype=np.float64)
    ctx.set_state(x=x, logw=np.zeros(ctx.N))
    ctx.call("smcn_set_proposal", _capi.dptr(r), _capi.dptr(x), _capi.dptr(r))
    ctx.call("smcn_set_lkernel_values", None, _capi.dptr(np.zeros(ctx.N)))


def read_L(ctx):
    """The L values the last L-kernel call left on the device, bit for bit: after load(), smcn_reweight computes
    ((0 + p) - p) + L - 0 = L (reweight_kernel, smcn_weights.hpp).  Raises SmcnError where no L value is set."""
    from smcnuts_amd import _capi
    ctx.call("smcn_reweight", _capi.LKERNEL_GAUSSIAN)
    return ctx.get_proposal(r=False, x_new=False, r_new=False, logw_new=True)[3]
