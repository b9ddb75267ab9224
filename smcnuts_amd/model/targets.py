"""Device-native targets with the reference's StanModel surface.

Mirror of smcnuts/model/bridgestan.py:7-146 (`StanModel`): `.dim`,
`.constrained_dim`, `.param_names`, `.logpdf(x, phi=1.0)`,
`.logpdfgrad(x, phi=1.0)`, `.constrain(x)`.  The reference's back end is
BridgeStan (host-only, one compiled Stan model per .so); here each model is a
device functor restated from its .stan text (smcnuts_amd/csrc/smcn_models.hpp)
and the temperature phi is a kernel argument (the reference rewrites the JSON
data file and reloads the model on every change, bridgestan.py:122-146).
"""
import json
import math
import os

import numpy as np

from .. import _capi
from .. import _checks
from .. import covariance as _covariance
from .. import forecast as _forecast
from .. import residuals as _residuals
from .. import stepsize as _stepsize
from .. import summary as _summary
from .._checks import GLM_DISPERSION, GLM_FAMILIES, GLM_MAX_DIM
from ..predict import PredictiveDraws, PredictMixin

DATA_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")


class DeviceTarget:
    """Base: a model id + flat fp64 data block understood by the HIP library."""

    model_id = None

    def __init__(self, model_data, dim, param_names):
        self.model_data = np.ascontiguousarray(model_data, dtype=np.float64)
        self.dim = int(dim)
        self.constrained_dim = int(dim)
        self._param_names = list(param_names)
        self._ctx = None     # small private context for the host-facing batched calls
        self.device = 0

    def param_names(self):
        return list(self._param_names)

    def _context(self, M):
        if self._ctx is None or self._ctx.N < M:
            if self._ctx is not None:
                self._ctx.close()
            self._ctx = _capi.Context(max(int(M), 256), self.model_id, self.model_data, device=self.device)
        return self._ctx

    # bridgestan.py:28-58: 1-D -> scalar, 2-D -> [N]; failures -> -inf
    def logpdf(self, x, phi=1.0, adjust_transform=True):
        x = np.asarray(x, dtype=np.float64)
        x2 = np.atleast_2d(x)
        lp = self._context(x2.shape[0]).target_eval(x2, phi)[0]
        return float(lp[0]) if x.ndim == 1 else lp

    # bridgestan.py:60-90
    def logpdfgrad(self, x, phi=1.0, adjust_transform=True):
        x = np.asarray(x, dtype=np.float64)
        x2 = np.atleast_2d(x)
        g = self._context(x2.shape[0]).target_eval(x2, phi, want_grad=True)[1]
        return g[0] if x.ndim == 1 else g

    def logpdf_parts(self, x):
        """(log prior incl. Jacobian, log likelihood); log pi_phi = lpri + phi*llik."""
        x2 = np.atleast_2d(np.asarray(x, dtype=np.float64))
        _, _, a, b = self._context(x2.shape[0]).target_eval(x2, 1.0, want_parts=True)
        return a, b

    # bridgestan.py:93-120
    def constrain(self, x, include_tparams=True, include_gqs=True):
        x = np.asarray(x, dtype=np.float64)
        x2 = np.atleast_2d(x)
        c = self._context(x2.shape[0]).constrain(x2)
        return c[0] if x.ndim == 1 else c

    # pointwise criteria (smcnuts_amd/criteria.py): GLMTarget only
    def _no_pointwise(self):
        raise NotImplementedError(
            f"{type(self).__name__}: pointwise log-likelihood and the criteria built on it (WAIC, IS-LOO, fitted values) "
            "are implemented for GLMTarget (bernoulli_logit, poisson_log, normal, neg_binomial_2_log) only")

    def pointwise_loglik(self, x):
        self._no_pointwise()

    def pointwise(self, x, logw=None):
        self._no_pointwise()

    def loo(self, x, logw=None):
        self._no_pointwise()

    # calibration checks (smcnuts_amd/calibration.py): GLMTarget only
    def _no_calibration(self):
        raise NotImplementedError(
            f"{type(self).__name__}: calibration checks (PIT values, randomised quantile residuals) are implemented for "
            "GLMTarget (bernoulli_logit, poisson_log, normal, neg_binomial_2_log) only")

    def calibration_points(self, x):
        self._no_calibration()

    def calibration_partials(self, x, logw=None):
        self._no_calibration()

    def calibration(self, x, logw=None):
        self._no_calibration()

    def summary(self, x, logw=None, probs=_summary.DEFAULT_PROBS, at=None):
        """summary.PosteriorSummary of the points x [M][D] (unconstrained) with log-weights logw (None: equal): weighted
        quantiles at `probs` (at most 16, each in (0, 1]) and, with `at` (a scalar, [T] or [Dc][T], T <= 16), the mass at
        or below each threshold, of every constrained coordinate -- constrained and selected on the device."""
        x2 = _checks.points(type(self).__name__, x, self.dim)
        lw = _summary.check_logw(logw, x2.shape[0])
        probs, at = _summary.check_probs(probs), _summary.check_at(at, self.constrained_dim)
        return _summary.target_summary(self, self._context(x2.shape[0]), np.ascontiguousarray(x2), lw, probs, at)

    def covariance(self, x, logw=None):
        """covariance.PosteriorCovariance of the points x [M][D] (unconstrained) with log-weights logw (None: equal):
        weighted mean, covariance and correlation of the constrained coordinates -- constrained and summed on the device
        (one fp64 MFMA product) about the points' own weighted mean."""
        x2 = _checks.points(type(self).__name__, x, self.dim)
        lw = _summary.check_logw(logw, x2.shape[0])
        return _covariance.target_covariance(self, self._context(x2.shape[0]), np.ascontiguousarray(x2), lw)

    def probe_step_size(self, x, logw=None, phi=1.0, target_accept=_stepsize.TARGET_ACCEPT,
                        n_leapfrog=_stepsize.N_LEAPFROG, max_particles=_stepsize.MAX_PARTICLES, seed=0, r=None,
                        ladder=None, refine=True, delta_max=100.0):
        """stepsize.StepSizeProbe of the points x [M][D] (unconstrained) with log-weights logw (None: equal) at temperature
        phi: n_leapfrog leapfrogs from each of min(M, max_particles) points at every step size of `ladder` (None:
        stepsize.default_ladder()) on the device, and the largest step size whose weighted mean of min(1, exp(-dH))
        stays at target_accept -- refined by a second pass between the two neighbours that bracket it.  Momenta: r
        [min(M, max_particles)][D], or standard normal draws under `seed`."""
        ladder = _stepsize.check_probe_args(target_accept, n_leapfrog, max_particles, ladder, phi, delta_max)
        x2 = _checks.points(type(self).__name__, x, self.dim)
        lw = _summary.check_logw(logw, x2.shape[0])
        one_pass = _stepsize.context_pass(self._context(x2.shape[0]), None, x=np.ascontiguousarray(x2), logw=lw, r=r,
                                          n_leapfrog=int(n_leapfrog), phi=float(phi), delta_max=float(delta_max),
                                          seed=seed, max_particles=int(max_particles))
        return _stepsize.run_probe(one_pass, ladder, float(target_accept), refine)


class GaussianTarget(DeviceTarget):
    """prior N(0, prior_sd^2 I) x optional likelihood N(x | lik_mean 1, lik_sd^2 I)."""
    model_id = _capi.MODEL_GAUSS

    def __init__(self, dim, prior_sd=1.0, lik_mean=None, lik_sd=1.0):
        has = 0.0 if lik_mean is None else 1.0
        data = [dim, prior_sd, has, 0.0 if lik_mean is None else lik_mean, lik_sd]
        super().__init__(data, dim, [f"x.{i + 1}" for i in range(dim)])


class IsoGaussian(GaussianTarget):
    """log pi = -|x|^2/2 - D/2 log 2 pi (BASELINE config 5)."""

    def __init__(self, dim):
        super().__init__(dim)


class HostTarget:
    """Adapter for targets evaluated on the HOST: any object with the reference's StanModel surface
    (smcnuts/model/bridgestan.py:7-146: `.dim`, `.logpdf(x, phi)`, `.logpdfgrad(x, phi)`, optional
    `.constrain(x)` / `.constrained_dim` / `.param_names()`), e.g. a BridgeStan model that has no device
    functor here.  The NUTS tree building, the weights, the resampling and the estimates still run on
    the GPU; the library calls back for the density (`smcn_set_host_target`), in lock step for all
    particles -- one call per leapfrog of the longest tree: the generality path, not the fast one.

    The callback hands the library log prior and log likelihood separately, taken from the wrapped
    model the way the reference's tempering does (adaptive_tempering.py:44-49):
    lpri = logpdf(x, phi=0), llik = logpdf(x, phi=1) - lpri (the same for the gradients)."""
    model_id = _capi.MODEL_HOST
    host_evaluated = True

    def __init__(self, target):
        self.target = target
        self.dim = int(target.dim)
        self.constrained_dim = int(getattr(target, "constrained_dim", self.dim))
        self.model_data = np.array([float(self.dim)])
        self.device = 0
        self.calls = 0
        self._keep = []          # the ctypes trampolines must outlive the contexts they are registered with

    def param_names(self):
        f = getattr(self.target, "param_names", None)
        return list(f()) if callable(f) else [f"x.{i + 1}" for i in range(self.dim)]

    def logpdf(self, x, phi=1.0, **kw):
        return self.target.logpdf(x, phi=phi)

    def logpdfgrad(self, x, phi=1.0, **kw):
        return self.target.logpdfgrad(x, phi=phi)

    def logpdf_parts(self, x):
        with np.errstate(all="ignore"):
            a = np.asarray(self.target.logpdf(x, phi=0.0), dtype=np.float64)
            return a, np.asarray(self.target.logpdf(x, phi=1.0), dtype=np.float64) - a

    def constrain(self, x, **kw):
        f = getattr(self.target, "constrain", None)
        return f(x) if callable(f) else np.array(x, copy=True)

    def pointwise_loglik(self, x):
        DeviceTarget._no_pointwise(self)

    def pointwise(self, x, logw=None):
        DeviceTarget._no_pointwise(self)

    def loo(self, x, logw=None):
        DeviceTarget._no_pointwise(self)

    def calibration_points(self, x):
        DeviceTarget._no_calibration(self)

    def calibration_partials(self, x, logw=None):
        DeviceTarget._no_calibration(self)

    def calibration(self, x, logw=None):
        DeviceTarget._no_calibration(self)

    def summary(self, x, logw=None, probs=_summary.DEFAULT_PROBS, at=None):
        """DeviceTarget.summary with the wrapped model's own constrain() on the host and the selection on the device."""
        x2 = _checks.points("HostTarget", x, self.dim)
        lw = _summary.check_logw(logw, x2.shape[0])
        probs, at = _summary.check_probs(probs), _summary.check_at(at, self.constrained_dim)
        v = np.ascontiguousarray(np.atleast_2d(self.constrain(x2)), dtype=np.float64)
        if v.shape != (x2.shape[0], self.constrained_dim):
            raise ValueError(f"HostTarget: constrain() returned shape {v.shape}, not {(x2.shape[0], self.constrained_dim)}")
        ctx = getattr(self, "_sum_ctx", None)
        if ctx is None:
            ctx = self._sum_ctx = _capi.Context(256, self.model_id, self.model_data, device=self.device)
        return _summary.target_summary(self, ctx, x2, lw, probs, at, v=v)

    def covariance(self, x, logw=None):
        """DeviceTarget.covariance with the wrapped model's own constrain() on the host and the sums on the device."""
        x2 = _checks.points("HostTarget", x, self.dim)
        lw = _summary.check_logw(logw, x2.shape[0])
        v = np.ascontiguousarray(np.atleast_2d(self.constrain(x2)), dtype=np.float64)
        if v.shape != (x2.shape[0], self.constrained_dim):
            raise ValueError(f"HostTarget: constrain() returned shape {v.shape}, not {(x2.shape[0], self.constrained_dim)}")
        ctx = getattr(self, "_sum_ctx", None)
        if ctx is None:
            ctx = self._sum_ctx = _capi.Context(256, self.model_id, self.model_data, device=self.device)
        return _covariance.target_covariance(self, ctx, x2, lw, v=v)

    def probe_step_size(self, x, logw=None, **kw):
        raise NotImplementedError("HostTarget: the step-size probe runs its trajectories through a device functor, and a "
                                  "host-evaluated target has none; pass step_size as a number")

    def attach(self, ctx):
        """Register the density callback with a context created for this target."""
        import ctypes as C
        D = self.dim

        def trampoline(user, n, d, x, want_grad, lpri, llik, gpri, glik):
            try:
                xs = np.ctypeslib.as_array(x, shape=(n, d))
                with np.errstate(all="ignore"):
                    a = np.asarray(self.target.logpdf(xs, phi=0.0), dtype=np.float64).reshape(n)
                    b = np.asarray(self.target.logpdf(xs, phi=1.0), dtype=np.float64).reshape(n)
                    np.ctypeslib.as_array(lpri, shape=(n,))[:] = a
                    np.ctypeslib.as_array(llik, shape=(n,))[:] = b - a
                    if want_grad:
                        ga = np.asarray(self.target.logpdfgrad(xs, phi=0.0), dtype=np.float64).reshape(n, d)
                        gb = np.asarray(self.target.logpdfgrad(xs, phi=1.0), dtype=np.float64).reshape(n, d)
                        np.ctypeslib.as_array(gpri, shape=(n, d))[:] = ga
                        np.ctypeslib.as_array(glik, shape=(n, d))[:] = gb - ga
                self.calls += 1
                return 0
            except Exception as e:      # the library turns this into an error of the calling entry point
                self.last_error = e
                return 1

        fn = _capi.HOST_TARGET_FN(trampoline)
        self._keep.append(fn)
        ctx.call("smcn_set_host_target", fn, None)
        return ctx


def as_target(target):
    """Device-native targets pass through; anything else with the StanModel surface is wrapped."""
    if hasattr(target, "model_id"):
        return target
    for name in ("dim", "logpdf", "logpdfgrad"):
        if not hasattr(target, name):
            raise TypeError(f"target needs .{name} (the reference's StanModel interface, model/bridgestan.py)")
    return HostTarget(target)


def _load_json(path):
    s = open(path).read().rstrip()
    if s.endswith('"phi":'):       # the shipped PRMwCD.json is truncated
        s += " 1.0}"
    return json.loads(s)


class ArmaModel(DeviceTarget):
    """stan_models/arma/arma.stan; unconstrained (mu, beta, theta, log sigma)."""
    model_id = _capi.MODEL_ARMA

    def __init__(self, data_path=None, *, y=None):
        """The series from a JSON file {"T": .., "y": [..]} (None: the shipped one), or as an array y (1-D, finite, at
        least one value)."""
        if y is not None:
            if data_path is not None:
                raise ValueError("ArmaModel: give the series as data_path or as y, not both")
            try:
                y = np.asarray(y, dtype=np.float64)
            except (TypeError, ValueError):
                raise ValueError("ArmaModel: y must be numeric") from None
            if y.ndim != 1 or y.size < 1:
                raise ValueError("ArmaModel: y must be a 1-D series of at least one value")
            if not np.all(np.isfinite(y)):
                raise ValueError("ArmaModel: y must be finite")
        else:
            d = _load_json(data_path or os.path.join(DATA_DIR, "arma.json"))
            y = np.asarray(d["y"], dtype=np.float64)
            if int(d["T"]) != y.size:
                raise ValueError("arma data: T != len(y)")
        super().__init__(np.concatenate([[float(y.size)], y]), 4, ["mu", "beta", "theta", "sigma"])

    # ---- forecasts (smcnuts_amd/forecast.py); every argument check runs on the host, before a context exists ----
    def _forecast_args(self, who, horizon, y_future=None, at=None):
        H = _forecast.check_horizon(who, horizon)
        return H, _forecast.check_y_future(who, y_future, H), _forecast.check_at(who, at, H)

    def forecast_points(self, x, horizon, y_future=None):
        """Per point of x ([4] or [M, 4]) the h-step laws of y_{T+1..T+H}: dict(err_T [M], m [M, H], v [M, H]) and, with
        y_future, marginal [M, H] (log N(yf_h | m_h, v_h)) and joint [M, H] (the cumulative log density of yf_1..yf_h
        given the series).  A point with a non-finite coordinate gives NaN."""
        H, yf, _ = self._forecast_args("ArmaModel.forecast_points", horizon, y_future)
        x2 = _checks.points("ArmaModel", x, self.dim)
        ctx = self._context(x2.shape[0])
        ctx.forecast_set(H, yf)
        o = ctx.forecast_points(x2)
        out = dict(err_T=o[:, 0], m=o[:, 1:1 + H], v=o[:, 1 + H:1 + 2 * H])
        if yf is not None:
            out.update(marginal=o[:, 1 + 2 * H:1 + 3 * H], joint=o[:, 1 + 3 * H:1 + 4 * H])
        return out

    def forecast_partials(self, x, horizon, logw=None, y_future=None, at=None):
        """The mergeable partials of x's rows over the horizon ([1 + H][10 + Tn], include/smcnuts_hip.h)."""
        H, yf, a = self._forecast_args("ArmaModel.forecast", horizon, y_future, at)
        x2 = _checks.points("ArmaModel", x, self.dim)
        if logw is not None and np.shape(logw) != (x2.shape[0],):
            raise ValueError("ArmaModel.forecast: logw must hold one log-weight per row of x")
        ctx = self._context(x2.shape[0])
        ctx.forecast_set(H, yf, a)
        return ctx.forecast_partials(x2, logw)

    def forecast(self, x, horizon, logw=None, y_future=None, at=None):
        """Posterior predictive summaries of y_{T+1..T+H} from the weighted points (x [M, 4], logw unnormalised or None
        for equal weights) -> forecast.Forecast: mean, var, sd; with `at` (a scalar, [Tn] or [H][Tn], Tn <= 16) the
        mixture's cdf there; with y_future [H] the log predictive densities lpd_marginal and lpd_joint."""
        part = self.forecast_partials(x, horizon, logw, y_future, at)
        a = _forecast.check_at("ArmaModel.forecast", at, int(horizon))
        return _forecast.combine_forecast_partials([part], 0 if a is None else a.shape[1], y_future is not None, a)

    def forecast_draws(self, x, horizon, n_draws, seed=0, logw=None, ancestors=None):
        """n_draws simulated paths y_{T+1..T+H} from the weighted points (x [M, 4], logw unnormalised or None for equal
        weights; ancestors: the particle of each path instead of the systematic resampling) -> predict.PredictiveDraws
        (y [n_draws][H]): mean(), interval() and pvalue() give predictive intervals and path statistics."""
        H = _forecast.check_horizon("ArmaModel.forecast_draws", horizon)
        x2 = _checks.points("ArmaModel", x, self.dim)
        M = x2.shape[0]
        S, ancestors = _forecast.check_draws("ArmaModel.forecast_draws", n_draws, ancestors, M)
        if logw is not None and np.shape(logw) != (M,):
            raise ValueError("ArmaModel.forecast_draws: logw must hold one log-weight per row of x")
        ctx = self._context(M)
        ctx.forecast_set(H)
        return PredictiveDraws(*ctx.forecast_draws(S, seed, x2, logw, ancestors))

    # ---- one-step residual checks (smcnuts_amd/residuals.py); the argument checks run before a context exists ----
    @property
    def T(self):
        return int(self.model_data[0])

    def _residual_args(self, who, lags, levels=()):
        """(L, levels, the chi-square 1 - level quantiles on L degrees of freedom: Q's thresholds; none with L = 0)."""
        L = _residuals.check_lags(who, lags, self.T)
        lv = _residuals.check_levels(who, levels) if L else ()
        return L, lv, np.array([_residuals.chi2_isf(v, L) for v in lv], dtype=np.float64)

    def residual_points(self, x, lags=None):
        """Per point of x ([4] or [M, 4]) the in-sample one-step quantities: dict(nu [M, T] the one-step means, r [M, T] the
        standardised residuals) and, with lags > 0 (None: min(10, T // 5)), rho [M, L] the residual autocorrelations and
        Q [M] the Ljung-Box statistic.  A point with a non-finite coordinate gives NaN."""
        L, _, _ = self._residual_args("ArmaModel.residual_points", lags)
        x2 = _checks.points("ArmaModel", x, self.dim)
        ctx = self._context(x2.shape[0])
        ctx.residuals_set(L)
        o, T = ctx.residuals_points(x2), self.T
        out = dict(nu=o[:, :T], r=o[:, T:2 * T])
        if L:
            out.update(rho=o[:, 2 * T:2 * T + L], Q=o[:, 2 * T + L])
        return out

    def _residual_partials(self, who, x, logw, L, q):
        """residual_partials' body behind the checks of `who`'s lags and thresholds (q: [Tn] or None)."""
        x2 = _checks.points("ArmaModel", x, self.dim)
        if logw is not None and np.shape(logw) != (x2.shape[0],):
            raise ValueError(f"{who}: logw must hold one log-weight per row of x")
        ctx = self._context(x2.shape[0])
        ctx.residuals_set(L, q)
        return ctx.residuals_partials(x2, logw)

    def residual_partials(self, x, logw=None, lags=None, q_at=None):
        """The mergeable partials of x's rows ([1 + T (+ L + 1)][20], include/smcnuts_hip.h); q_at: at most 8 thresholds of
        the Ljung-Box statistic (with lags > 0 only)."""
        who = "ArmaModel.residual_partials"
        L, _, _ = self._residual_args(who, lags)
        q = None
        if q_at is not None:
            try:
                q = np.atleast_1d(np.asarray(q_at, dtype=np.float64))
            except (TypeError, ValueError):
                raise ValueError(f"{who}: q_at must be numeric") from None
            if q.ndim != 1 or not 1 <= q.size <= _residuals.MAX_LEVELS or not np.all(np.isfinite(q)):
                raise ValueError(f"{who}: q_at must hold 1 to {_residuals.MAX_LEVELS} finite thresholds")
            if not L:
                raise ValueError(f"{who}: q_at holds thresholds of the Ljung-Box statistic, which lags = 0 does not compute")
        return self._residual_partials(who, x, logw, L, q)

    def residuals(self, x, logw=None, lags=None, levels=(0.05,)):
        """One-step residual checks from the weighted points (x [M, 4], logw unnormalised or None for equal weights) ->
        residuals.OneStepResiduals: the one-step predictive mean, sd and log density of every y_t, the posterior mean of
        the standardised residuals and PIT values, and with lags > 0 (None: min(10, T // 5)) the residual autocorrelations
        and the Ljung-Box statistic with the posterior probability that it exceeds the chi-square 1 - level quantiles."""
        who = "ArmaModel.residuals"
        L, lv, q = self._residual_args(who, lags, levels)
        return _residuals.combine_residual_partials([self._residual_partials(who, x, logw, L, q if q.size else None)], L, lv)


class PRMwCDModel(DeviceTarget):
    """stan_models/PRMwCD/PRMwCD.stan; unconstrained (Beta[1..M], log Gamma)."""
    model_id = _capi.MODEL_PRMWCD

    def __init__(self, data_path=None):
        d = _load_json(data_path or os.path.join(DATA_DIR, "PRMwCD.json"))
        M = int(d["M"])
        data = np.concatenate([[float(d["N"]), float(M), float(d["Clength"]), float(d["q"])],
                               np.asarray(d["y"], dtype=np.float64), np.asarray(d["Xkernel"], dtype=np.float64)])
        if M != int(d["Clength"]) + 1:
            raise ValueError("PRMwCD data: M must equal Clength + 1")
        super().__init__(data, M + 1, [f"Beta.{i + 1}" for i in range(M)] + ["Gamma"])
        # the data shape the device functors are specialised for (unrolled observation loop, wave-per-tree finisher):
        # trees that want more than 9 doublings are then parked and finished one per wavefront (Samples: nuts_cap="auto")
        self.two_phase_default = (9, True, 8) if (96 < int(d["N"]) <= 100 and int(d["Clength"]) == 11 and float(d["q"]) == 0.5) else None


WGLM_MAX_DIM = 256                         # WideGLMTarget: GLM_MAX_DIM < D <= this
_NO_PRIOR = _checks.NO_PRIOR


def _coefficient_names(ic, p):
    return (["Intercept"] if ic else []) + [f"beta.{j + 1}" for j in range(p)]


def _glm_setup(self, limit, X, y, family, prior_sd, intercept, dispersion_prior, offset=None, weights=None):
    """GLMTarget's and WideGLMTarget's constructor: the checks (messages prefixed with the class's name), the
    attributes and the SMCN_MODEL_GLM data block -- with `offset` or `weights` (GLMTarget only), SMCN_MODEL_OGLM's.
    `limit(what, D)` raises where the class does not cover D."""
    who = type(self).__name__
    _checks.family(who, family)
    tau_prior = _checks.dispersion_prior(who, family, dispersion_prior)
    disp = tau_prior is not None
    X = _checks.design(who, X)
    n, p = X.shape
    y = _checks.response(who, y, n)            # before the rows are counted: the other targets count first
    _checks.some_rows(who, n)
    ic = 1 if intercept else 0
    Dc = p + ic
    D = Dc + (1 if disp else 0)
    if Dc < 1:
        raise ValueError(f"{who}: no coefficients (p = 0 without an intercept)")
    limit(f"D = {D} coefficients" if not disp else f"D = {D} coordinates ({Dc} coefficients and tau)", D)
    _checks.finite(who, "X", X)
    _checks.family_response(who, family, y)
    s = _checks.prior_sds(who, "prior_sd", prior_sd, (Dc,),
                          f"a scalar or one value per coefficient ({Dc})" if disp
                          else f"a scalar or one value per coefficient (D = {D})")
    self.family, self.intercept = family, bool(intercept)
    self.X, self.y, self.prior_sd = X.copy(), y.copy(), s.copy()
    self.dispersion_prior = tau_prior
    self.offset = self.weights = None
    if offset is not None:
        o = _checks.row_vector(who, "offset", offset, n, f"the n = {n} observations' offsets")
        self.offset = _checks.finite(who, "offset", o).copy()
    if weights is not None:
        w = _checks.row_vector(who, "weights", weights, n, f"the n = {n} observations' weights")
        if not np.all(np.isfinite(w) & (w >= 0.0)):
            raise ValueError(f"{who}: weights must be finite and >= 0")
        if not np.any(w > 0.0):
            raise ValueError(f"{who}: at least one weight must be > 0")
        self.weights = w.copy()
    flags = (1 if self.offset is not None else 0) | (2 if self.weights is not None else 0)
    head = [float(GLM_FAMILIES.index(family)), float(n), float(p), float(ic)]
    if flags:
        self.model_id = _capi.MODEL_OGLM
        head.append(float(flags))
    data = np.concatenate([head, s, tau_prior or [], y,
                           self.offset if flags & 1 else [], self.weights if flags & 2 else [], X.reshape(-1)])
    names = _coefficient_names(ic, p)
    if disp:
        names.append(GLM_DISPERSION[family])
    DeviceTarget.__init__(self, data, D, names)


class GLMTarget(PredictMixin, DeviceTarget):
    """GLM on the device, eta = [b_0 +] X b, independent N(0, prior_sd_c^2) priors on the Dc = p + intercept
    coefficients (the intercept is coordinate 0):
      bernoulli_logit:    y_i ~ bernoulli_logit(eta_i)
      poisson_log:        y_i ~ poisson_log(eta_i)
      normal:             y_i ~ normal(eta_i, sigma)
      neg_binomial_2_log: y_i ~ neg_binomial_2_log(eta_i, phi)   (Stan's parameterisation: mean e^eta, var mu + mu^2 / phi)
    The two last families sample tau = log sigma / log phi as the last coordinate (D = Dc + 1), with the prior
    tau ~ N(m, s^2) for dispersion_prior = (m, s) -- sigma / phi ~ lognormal(m, s); `constrain` reports sigma / phi.
    Coordinates are unconstrained; log pi_phi = lpri + phi * llik.  D <= 64 (65..256: WideGLMTarget; beyond: HostTarget).

    offset (a vector o of n finite values) enters the linear predictor, eta_i = [b_0 +] X_i b + o_i: log(exposure) of a
    Poisson or negative-binomial regression on rates.  weights (a vector w of n finite values >= 0, not all 0) multiply
    the observations' terms, llik = sum_i w_i log p(y_i | eta_i): frequency or survey weights, k successes out of m as
    two rows with weights k and m - k; a row with weight 0 is dropped whatever its term is.  With either, the object is
    SMCN_MODEL_OGLM's (model_id, block); with neither, it is what it was without the keywords.  After a fit with
    weights, predict() and predict_draws() work (new rows carry weight 1) and pointwise(), pointwise_loglik() and loo()
    raise NotImplementedError.

    Data block (include/smcnuts_hip.h, SMCN_MODEL_GLM):
    [family (0 bernoulli_logit, 1 poisson_log), n, p, intercept, s_1..s_D, y_1..y_n, X (n x p, row-major)], or
    [family (2 normal, 3 neg_binomial_2_log), n, p, intercept, s_1..s_Dc, m, s, y_1..y_n, X];
    with offset / weights (SMCN_MODEL_OGLM): [family, n, p, intercept, flags (1 offset | 2 weights), s_1..s_Dc, (m, s),
    y_1..y_n, o_1..o_n (flags & 1), w_1..w_n (flags & 2), X]."""
    model_id = _capi.MODEL_GLM

    def __init__(self, X, y, family="bernoulli_logit", prior_sd=2.5, intercept=True, dispersion_prior=_NO_PRIOR,
                 offset=None, weights=None):
        def limit(what, D):
            if D > GLM_MAX_DIM:
                raise ValueError(f"GLMTarget: {what}; the device functor covers D <= {GLM_MAX_DIM}. "
                                 f"WideGLMTarget covers the same model for {GLM_MAX_DIM} < D <= {WGLM_MAX_DIM}; beyond that, "
                                 "wrap a model object with .dim / .logpdf / .logpdfgrad in HostTarget instead.")
        _glm_setup(self, limit, X, y, family, prior_sd, intercept, dispersion_prior, offset, weights)

    _PW_CHUNK = 1 << 25          # doubles of ll the device holds at once (256 MB)

    def _refuse_weighted(self):
        if self.weights is not None:
            raise NotImplementedError(
                "GLMTarget: pointwise log-likelihoods, the criteria built on them (WAIC, IS-LOO, fitted values) and LOO "
                "are not implemented for a fit with weights: what a weighted row's leave-one-out term and the standard "
                "error of the sum should be is not settled (predict() and predict_draws() do work)")

    def _points(self, x):
        self._refuse_weighted()
        return _checks.points("GLMTarget", x, self.dim)      # the literal name, for a subclass as well

    def pointwise_loglik(self, x):
        """ll[p, i] = log p(y_i | x_p): [n] for a 1-D x, [M, n] for 2-D (sum over i: logpdf_parts(x)[1]).  The matrix is
        formed on the device in slabs of particles; it has to fit on the host."""
        x2 = self._points(x)
        M, n = x2.shape[0], self.y.shape[0]
        step = max(1, min(M, self._PW_CHUNK // n))
        ctx = self._context(step)
        out = np.empty((M, n))
        for m0 in range(0, M, step):
            out[m0:m0 + step] = ctx.pointwise_loglik(x2[m0:m0 + step])
        return out[0] if np.ndim(x) == 1 else out

    def pointwise_partials(self, x, logw=None):
        """The mergeable partials of x's rows ([1 + n][Q], include/smcnuts_hip.h)."""
        x2 = self._points(x)
        return self._context(x2.shape[0]).pointwise_partials(x2, logw)

    def pointwise(self, x, logw=None):
        """Per-observation lppd, WAIC, IS-LOO and fitted values of the weighted points (x [M, D], logw unnormalised or None
        for equal weights) -> criteria.Pointwise.  The matrix ll is never formed."""
        from ..criteria import combine_pointwise_partials
        return combine_pointwise_partials([self.pointwise_partials(x, logw)])

    def calibration_points(self, x):
        """(lo, up) = (P(Y < y_i), P(Y > y_i)) under every point of x: [n, 2] for a 1-D x, [M, n, 2] for 2-D.  NaN where the
        term is not finite or the tail evaluation reached the device's iteration bound (calibration.py)."""
        x2 = self._points(x)
        M, n = x2.shape[0], self.y.shape[0]
        step = max(1, min(M, self._PW_CHUNK // (2 * n)))
        ctx = self._context(step)
        out = np.empty((M, n, 2))
        for m0 in range(0, M, step):
            out[m0:m0 + step] = ctx.calibration_points(x2[m0:m0 + step])
        return out[0] if np.ndim(x) == 1 else out

    def calibration_partials(self, x, logw=None):
        """The mergeable calibration partials of x's rows ([1 + n][Qc], include/smcnuts_hip.h)."""
        x2 = self._points(x)
        if logw is not None and np.shape(logw) != (x2.shape[0],):
            raise ValueError("GLMTarget.calibration_partials: logw must hold one log-weight per row of x")
        return self._context(x2.shape[0]).calibration_partials(x2, logw)

    def calibration(self, x, logw=None):
        """Calibration of the weighted points (x [M, D], logw unnormalised or None for equal weights) ->
        calibration.Calibration: per observation the predictive cdf just below and at y_i (PIT bounds) and the survival
        function, under the posterior and the leave-one-out weights; randomised PIT values, quantile residuals and the
        non-randomised PIT histogram are its methods."""
        from ..calibration import combine_calibration_partials
        return combine_calibration_partials([self.calibration_partials(x, logw)])

    def loo(self, x, logw=None):
        """Pareto-smoothed importance-sampling LOO of the weighted points (x [M, D], logw unnormalised or None for equal
        weights) -> psis.PsisLoo: elpd_loo_i from the smoothed ratios, pareto_k_i as its diagnostic, and `plain`, the
        Pointwise of the same call.  Selection, fit and smoothing run on the device; the matrix ll is never downloaded."""
        from ..psis import loo_from_context
        x2 = self._points(x)
        return loo_from_context(self._context(x2.shape[0]), None, x2, logw)


class WideGLMTarget(DeviceTarget):
    """GLMTarget's model -- the same four families, priors, arguments, coordinates and constrained space -- for
    64 < D <= 256 coordinates (D = p + intercept, + 1 for tau in the dispersion families): dummy-coded factors,
    interactions, spline bases.  The device functor holds up to four coordinates per lane of one wavefront
    (smcn_models.hpp: GlmWideModel).  D <= 64 is GLMTarget's; D > 256 runs host-evaluated (HostTarget).  Sampling with the
    forward and the asymptotic L-kernel, tempering, shards, moments, summary() and covariance(); the pointwise criteria,
    LOO, prediction and GaussianApproxLKernel are not implemented for wide rows.

    Data block (include/smcnuts_hip.h, SMCN_MODEL_WGLM): SMCN_MODEL_GLM's, word for word."""
    model_id = _capi.MODEL_WGLM

    def __init__(self, X, y, family="bernoulli_logit", prior_sd=2.5, intercept=True, dispersion_prior=_NO_PRIOR):
        def limit(what, D):
            if D <= GLM_MAX_DIM:
                raise ValueError(f"WideGLMTarget: {what}; the wide functor covers {GLM_MAX_DIM} < D <= {WGLM_MAX_DIM}. "
                                 f"D <= {GLM_MAX_DIM} is GLMTarget's.")
            _checks.dim_limit("WideGLMTarget", D, what, WGLM_MAX_DIM)
        _glm_setup(self, limit, X, y, family, prior_sd, intercept, dispersion_prior)


class ContinuousGLM(DeviceTarget):
    """Regression for a continuous response on the device: GLMTarget's linear predictor and priors, eta = [b_0 +] X b with
    independent N(0, prior_sd_c^2) priors on the Dc = p + intercept coefficients (the intercept is coordinate 0), and
      gamma_log:  y_i ~ gamma(shape, shape / e^eta_i)   (mean e^eta_i, variance mean^2 / shape; y finite and > 0)
      student_t:  y_i ~ student_t(df, eta_i, sigma)     (df fixed by the caller, finite and > 0; y finite)
    The last coordinate is tau = log shape / log sigma (D = Dc + 1 <= 64), with the prior tau ~ N(m, s^2) for
    dispersion_prior = (m, s); `constrain` reports shape / sigma.  Coordinates are unconstrained;
    log pi_phi = lpri + phi * llik.  Sampling with every L-kernel, tempering, shards, moments, summary(), covariance()
    and the step-size probe as for any device target; the pointwise criteria, LOO, calibration and prediction are not
    implemented for these families, and df is not estimated.

    Data block (include/smcnuts_hip.h, SMCN_MODEL_CGLM):
    [family (0 gamma_log, 1 student_t), n, p, intercept, df (0 for gamma_log), s_1..s_Dc, m, s, y_1..y_n, X (n x p,
    row-major)]."""
    model_id = _capi.MODEL_CGLM

    def __init__(self, X, y, family="gamma_log", prior_sd=2.5, intercept=True, dispersion_prior=(0.0, 2.5),
                 df=_checks.DEFAULT_DF):
        who = type(self).__name__
        _checks.continuous_family(who, family)
        dfv = _checks.student_df(who, family, df)
        tau_prior = _checks.scale_prior(who, dispersion_prior)
        X = _checks.design(who, X)
        n, p = X.shape
        y = _checks.response(who, y, n)
        _checks.some_rows(who, n)
        ic = 1 if intercept else 0
        Dc = p + ic
        D = Dc + 1
        if Dc < 1:
            raise ValueError(f"{who}: no coefficients (p = 0 without an intercept)")
        _checks.dim_limit(who, D, f"D = {D} coordinates ({Dc} coefficients and tau)")
        _checks.finite(who, "X", X)
        _checks.continuous_response(who, family, y)
        s = _checks.prior_sds(who, "prior_sd", prior_sd, (Dc,), f"a scalar or one value per coefficient ({Dc})")
        self.family, self.intercept = family, bool(intercept)
        self.df = dfv if family == "student_t" else None
        self.X, self.y, self.prior_sd = X.copy(), y.copy(), s.copy()
        self.dispersion_prior = tau_prior
        head = [float(_checks.CONTINUOUS_FAMILIES.index(family)), float(n), float(p), float(ic), dfv]
        data = np.concatenate([head, s, tau_prior, y, X.reshape(-1)])
        super().__init__(data, D, _coefficient_names(ic, p) + [_checks.CONTINUOUS_SCALE[family]])


class HierarchicalGLM(PredictMixin, DeviceTarget):
    """Varying-intercept GLM on the device, non-centred: observations fall into J groups, group j has the intercept
    alpha_j = tau z_j,
      eta_i = [b_0 +] X_i b + tau z_{g_i},   y_i ~ family(eta_i [, e^ld])   (GLMTarget's four families, same terms)
      b_c ~ N(0, prior_sd_c^2),  z_j ~ N(0, 1),  tau ~ half-normal(group_sd_prior) (sampled as lt = log tau, with its
      Jacobian),  e^ld ~ lognormal(m, s) for dispersion_prior = (m, s) (families normal / neg_binomial_2_log).
    x = (b_1..b_Dc, z_1..z_J, lt [, ld]), D = Dc + J + 1 (+ 1) <= 64 (larger models: HostTarget); Dc = p + intercept may
    be 0.  `groups` holds each observation's group in 0..J-1, J = max + 1 unless n_groups is given (groups without
    observations keep their prior).  `constrain` reports (b, alpha_1..alpha_J, tau [, sigma | phi]).

    Data block (include/smcnuts_hip.h, SMCN_MODEL_HGLM):
    [family, n, p, intercept, J, s_1..s_Dc, s_tau, (m, s: families 2, 3), y_1..y_n, g_1..g_n, X (n x p, row-major)]."""
    model_id = _capi.MODEL_HGLM

    def __init__(self, X, y, groups, family="bernoulli_logit", prior_sd=2.5, group_sd_prior=1.0, intercept=True,
                 dispersion_prior=_NO_PRIOR, n_groups=None):
        who = "HierarchicalGLM"
        _checks.family(who, family)
        ld_prior = _checks.dispersion_prior(who, family, dispersion_prior)
        disp = ld_prior is not None
        try:                                   # one number here; MultilevelGLM's is a vector, one per term
            s_tau = float(group_sd_prior)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: group_sd_prior must be a number") from None
        if not (math.isfinite(s_tau) and s_tau > 0.0):
            raise ValueError(f"{who}: group_sd_prior must be finite and > 0")
        X = _checks.design(who, X)
        n, p = X.shape
        _checks.some_rows(who, n)
        y = _checks.response(who, y, n)
        gf = _checks.index_vector(who, groups, n, "groups")
        J = _checks.n_groups(who, gf, n_groups)
        ic = 1 if intercept else 0
        Dc = p + ic
        D = Dc + J + 1 + (1 if disp else 0)
        _checks.dim_limit(who, D, f"D = {D} coordinates ({Dc} coefficients, {J} groups, tau"
                                  f"{', ' + GLM_DISPERSION[family] if disp else ''})")
        _checks.finite(who, "X", X)
        _checks.family_response(who, family, y)
        s = _checks.prior_sds(who, "prior_sd", prior_sd, (Dc,), f"a scalar or one value per coefficient ({Dc})")
        self.family, self.intercept, self.n_groups = family, bool(intercept), J
        self.X, self.y, self.groups, self.prior_sd = X.copy(), y.copy(), gf.astype(np.int64), s.copy()
        self.group_sd_prior = s_tau
        self.dispersion_prior = ld_prior
        head = [float(GLM_FAMILIES.index(family)), float(n), float(p), float(ic), float(J)]
        data = np.concatenate([head, s, [s_tau], ld_prior or [], y, gf, X.reshape(-1)])
        names = _coefficient_names(ic, p) + [f"alpha.{j + 1}" for j in range(J)] + ["tau"]
        if disp:
            names.append(GLM_DISPERSION[family])
        super().__init__(data, D, names)


ML_MAX_TERMS = 4


class MultilevelGLM(DeviceTarget):
    """Multilevel GLM on the device, non-centred: R = 1..4 independent varying terms, term r with J_r levels, a level
    g_ir and a multiplier z_ir per observation (z = 1: a varying intercept; z = a covariate: a varying slope; two terms
    may use the same factor -- `(1 + days || subject)` -- or crossed ones -- `(1 | subject) + (1 | item)`),
      eta_i = [b_0 +] X_i b + sum_r z_ir tau_r u_{r,g_ir},   y_i ~ family(eta_i [, e^ld])   (GLMTarget's four families)
      b_c ~ N(0, prior_sd_c^2),  u_rj ~ N(0, 1),  tau_r ~ half-normal(group_sd_prior_r) (sampled as lt_r = log tau_r, with
      its Jacobian),  e^ld ~ lognormal(m, s) for dispersion_prior = (m, s) (families normal / neg_binomial_2_log).
    x = (b_1..b_Dc, u_1,1..u_1,J1, .., u_R,1..u_R,JR, lt_1..lt_R [, ld]), D = Dc + sum J_r + R (+ 1) <= 64 (larger
    models: HostTarget); Dc = p + intercept may be 0.  `terms` is a sequence of (groups,), (groups, z) or
    (groups, z, n_groups): groups in 0..J_r-1 with J_r = max + 1 unless n_groups is given, z=None for ones.  `constrain`
    reports (b, alpha.r.j = tau_r u_rj .., tau.1..tau.R [, sigma | phi]).  With one term and z = None this is
    HierarchicalGLM's density.  Held-out prediction and the pointwise criteria do not cover this target.

    Data block (include/smcnuts_hip.h, SMCN_MODEL_MLGLM):
    [family, n, p, intercept, R, J_1..J_4 (0 beyond R), s_1..s_Dc, s_tau_1..s_tau_R, (m, s: families 2, 3), y_1..y_n,
     g_1 (n), z_1 (n), .., g_R (n), z_R (n), X (n x p, row-major)]."""
    model_id = _capi.MODEL_MLGLM

    def __init__(self, X, y, terms, family="bernoulli_logit", prior_sd=2.5, group_sd_prior=1.0, intercept=True,
                 dispersion_prior=_NO_PRIOR):
        who = "MultilevelGLM"
        _checks.family(who, family)
        ld_prior = _checks.dispersion_prior(who, family, dispersion_prior)
        disp = ld_prior is not None
        try:
            terms = [tuple(t) for t in terms]
        except TypeError:
            raise ValueError(f"{who}: terms must be a sequence of (groups,), (groups, z) or (groups, z, n_groups)") \
                from None
        R = len(terms)
        if not 1 <= R <= ML_MAX_TERMS:
            raise ValueError(f"{who}: terms must hold 1 to {ML_MAX_TERMS} varying terms, not {R}")
        if any(not 1 <= len(t) <= 3 for t in terms):
            raise ValueError(f"{who}: every term must be (groups,), (groups, z) or (groups, z, n_groups)")
        try:                                   # one per term here; HierarchicalGLM's is one number
            s_tau = np.asarray(group_sd_prior, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: group_sd_prior must be a number or one per term") from None
        s_tau = _checks.prior_sds(who, "group_sd_prior", s_tau, (R,), f"a scalar or one value per term ({R})")
        X = _checks.design(who, X)
        n, p = X.shape
        _checks.some_rows(who, n)
        y = _checks.response(who, y, n)
        gs, zs, Js = [], [], []
        for r, t in enumerate(terms):
            pre = f"term {r + 1}: "
            gf = _checks.index_vector(who, t[0], n, pre + "groups")
            if len(t) < 2 or t[1] is None:
                z = np.ones(n)
            else:
                try:
                    z = np.asarray(t[1], dtype=np.float64)
                except (TypeError, ValueError):
                    raise ValueError(f"{who}: {pre}z must be numbers") from None
                _checks.finite(who, pre + "z", _checks.per_row(who, pre + "z", z, n))
            J = _checks.n_groups(who, gf, t[2] if len(t) == 3 else None, pre)
            gs.append(gf), zs.append(z.copy()), Js.append(J)
        ic = 1 if intercept else 0
        Dc = p + ic
        D = Dc + sum(Js) + R + (1 if disp else 0)
        _checks.dim_limit(who, D, f"D = {D} coordinates ({Dc} coefficients, {' + '.join(map(str, Js))} levels, "
                                  f"{R} tau{', ' + GLM_DISPERSION[family] if disp else ''})")
        _checks.finite(who, "X", X)
        _checks.family_response(who, family, y)
        s = _checks.prior_sds(who, "prior_sd", prior_sd, (Dc,), f"a scalar or one value per coefficient ({Dc})")
        self.family, self.intercept, self.n_groups = family, bool(intercept), tuple(Js)
        self.X, self.y, self.prior_sd = X.copy(), y.copy(), s.copy()
        self.term_groups, self.term_z = [g.astype(np.int64) for g in gs], zs
        self.group_sd_prior = s_tau.copy()
        self.dispersion_prior = ld_prior
        head = [float(GLM_FAMILIES.index(family)), float(n), float(p), float(ic), float(R)] \
            + [float(J) for J in Js] + [0.0] * (ML_MAX_TERMS - R)
        gz = [v for r in range(R) for v in (gs[r], zs[r])]
        data = np.concatenate([head, s, s_tau, ld_prior or [], y] + gz + [X.reshape(-1)])
        names = _coefficient_names(ic, p) \
            + [f"alpha.{r + 1}.{j + 1}" for r in range(R) for j in range(Js[r])] + [f"tau.{r + 1}" for r in range(R)]
        if disp:
            names.append(GLM_DISPERSION[family])
        super().__init__(data, D, names)


CAT_MAX_CLASSES = 16


class CategoricalRegression(PredictMixin, DeviceTarget):
    """Categorical (multinomial logistic) regression on the device, Stan's categorical_logit with class 0 the
    reference: y_i in {0, .., K-1},
      eta_i0 = 0,  eta_ik = [b_k0 +] X_i b_k  (k = 1..K-1),  log p(y_i) = eta_{i,y_i} - logsumexp_k eta_ik,
      b_kj ~ N(0, prior_sd_kj^2).
    x = (b_1,1..b_1,Dc, b_2,1.., .., b_K-1,Dc) class-major, Dc = p + intercept, D = (K - 1) Dc <= 64 and K <= 16
    (larger models: HostTarget).  n_classes defaults to max(y) + 1; classes without observations are allowed.
    prior_sd: a scalar, one value per column (Dc, shared by the classes) or a (K - 1, Dc) array.  constrain() is the
    identity.

    Data block (include/smcnuts_hip.h, SMCN_MODEL_CATEGORICAL): [K, n, p, intercept, s_1..s_D, y_1..y_n, X (n x p,
    row-major)]."""
    model_id = _capi.MODEL_CATEGORICAL

    def __init__(self, X, y, n_classes=None, prior_sd=2.5, intercept=True):
        who = "CategoricalRegression"
        X = _checks.design(who, X)
        n, p = X.shape
        _checks.some_rows(who, n)
        yf = _checks.index_vector(who, y, n, "y", "the labels y")
        K = _checks.n_classes(who, yf, n_classes)
        if K > CAT_MAX_CLASSES:
            raise ValueError(f"{who}: K = {K} classes; the device functor holds K <= {CAT_MAX_CLASSES}. "
                             "Wrap a model object with .dim / .logpdf / .logpdfgrad in HostTarget instead.")
        _checks.below(who, "the labels y", yf, K, "n_classes")
        ic = 1 if intercept else 0
        Dc = p + ic
        if Dc < 1:
            raise ValueError(f"{who}: no coefficients (p = 0 without an intercept)")
        D = (K - 1) * Dc
        _checks.dim_limit(who, D, f"D = (K - 1) Dc = {K - 1} x {Dc} = {D} coefficients")
        _checks.finite(who, "X", X)
        s = np.asarray(prior_sd, dtype=np.float64)
        if s.shape == (Dc,):                   # one value per column, shared by the classes
            s = np.tile(s, (K - 1, 1))
        s = _checks.prior_sds(who, "prior_sd", s, (K - 1, Dc), f"a scalar, one value per column ({Dc}) or a "
                                                               f"(K - 1, Dc) = ({K - 1}, {Dc}) array")
        self.intercept, self.n_classes = bool(intercept), K
        self.X, self.y, self.prior_sd = X.copy(), yf.astype(np.int64), s.copy()
        data = np.concatenate([[float(K), float(n), float(p), float(ic)], s.reshape(-1), yf, X.reshape(-1)])
        names = [name for k in range(1, K)
                 for name in (([f"Intercept.{k}"] if ic else []) + [f"beta.{k}.{j + 1}" for j in range(p)])]
        super().__init__(data, D, names)


class OrdinalRegression(PredictMixin, DeviceTarget):
    """Ordinal (ordered-logistic) regression on the device, Stan's ordered_logistic with y shifted to 0..K-1:
      eta_i = X_i b (no intercept: the cutpoints take its place),
      P(y_i = k) = logit^-1(eta_i - c_k) - logit^-1(eta_i - c_{k+1})  (c_0 = -inf, c_K = +inf),
      b_j ~ N(0, prior_sd_j^2),  c_k ~ N(0, cutpoint_prior_sd_k^2)  (the ordering's normalising constant left out).
    The cutpoints c_1 < .. < c_{K-1} are sampled through Stan's `ordered` transform, c_1 = u_1, c_k = c_{k-1} + e^u_k,
    with its log-Jacobian sum_{k>=2} u_k: x = (b_1..b_p, u_1..u_{K-1}), D = p + K - 1 <= 64 (larger models: HostTarget).
    n_classes defaults to max(y) + 1; classes without observations are allowed.  prior_sd: a scalar or one value per
    column; cutpoint_prior_sd: a scalar or one value per cutpoint.  `constrain` reports (b, c_1..c_{K-1}).

    Data block (include/smcnuts_hip.h, SMCN_MODEL_ORDINAL): [K, n, p, s_1..s_p, t_1..t_{K-1}, y_1..y_n, X (n x p,
    row-major)]."""
    model_id = _capi.MODEL_ORDINAL

    def __init__(self, X, y, n_classes=None, prior_sd=2.5, cutpoint_prior_sd=5.0):
        who = "OrdinalRegression"
        X = _checks.design(who, X)
        n, p = X.shape
        _checks.some_rows(who, n)
        yf = _checks.index_vector(who, y, n, "y", "the labels y")
        K = _checks.n_classes(who, yf, n_classes)
        _checks.below(who, "the labels y", yf, K, "n_classes")
        D = p + K - 1
        _checks.dim_limit(who, D, f"D = p + K - 1 = {p} + {K - 1} = {D} coordinates")
        _checks.finite(who, "X", X)
        s = _checks.prior_sds(who, "prior_sd", prior_sd, (p,), f"a scalar or one value per column ({p})")
        t = _checks.prior_sds(who, "cutpoint_prior_sd", cutpoint_prior_sd, (K - 1,),
                              f"a scalar or one value per cutpoint (K - 1 = {K - 1})")
        self.n_classes = K
        self.X, self.y, self.prior_sd, self.cutpoint_prior_sd = X.copy(), yf.astype(np.int64), s.copy(), t.copy()
        data = np.concatenate([[float(K), float(n), float(p)], s, t, yf, X.reshape(-1)])
        names = [f"beta.{j + 1}" for j in range(p)] + [f"cutpoint.{k}" for k in range(1, K)]
        super().__init__(data, D, names)


def LogisticRegression(X, y, prior_sd=2.5, intercept=True, offset=None, weights=None):
    """Bayesian logistic regression: GLMTarget(X, y, family="bernoulli_logit", ...)."""
    return GLMTarget(X, y, family="bernoulli_logit", prior_sd=prior_sd, intercept=intercept, offset=offset,
                     weights=weights)


def _exposure_offset(who, offset, exposure):
    """offset, or log(exposure): one of the two at the most (GLMTarget checks the length, as an offset's)."""
    if exposure is None:
        return offset
    if offset is not None:
        raise ValueError(f"{who}: give offset or exposure, not both (exposure is offset = log(exposure))")
    try:
        e = np.asarray(exposure, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: exposure must be numeric") from None
    if e.ndim != 1:
        raise ValueError(f"{who}: exposure must be a vector of the observations' exposures")
    if not np.all(np.isfinite(e) & (e > 0.0)):
        raise ValueError(f"{who}: exposure must be finite and > 0")
    return np.log(e)


def PoissonRegression(X, y, prior_sd=2.5, intercept=True, offset=None, weights=None, exposure=None):
    """Bayesian Poisson regression with a log link: GLMTarget(X, y, family="poisson_log", ...).  exposure (finite, > 0)
    is offset = log(exposure): y_i ~ poisson(exposure_i e^eta_i)."""
    offset = _exposure_offset("PoissonRegression", offset, exposure)
    return GLMTarget(X, y, family="poisson_log", prior_sd=prior_sd, intercept=intercept, offset=offset, weights=weights)


def LinearRegression(X, y, prior_sd=2.5, dispersion_prior=(0.0, 2.5), intercept=True, offset=None, weights=None):
    """Bayesian linear regression, y ~ normal(eta, sigma) with log sigma ~ N(m, s^2):
    GLMTarget(X, y, family="normal", ...).  The last coordinate is log sigma; constrain() reports sigma."""
    return GLMTarget(X, y, family="normal", prior_sd=prior_sd, intercept=intercept, dispersion_prior=dispersion_prior,
                     offset=offset, weights=weights)


def NegativeBinomialRegression(X, y, prior_sd=2.5, dispersion_prior=(0.0, 2.5), intercept=True, offset=None,
                               weights=None, exposure=None):
    """Bayesian negative-binomial (NB2) regression with a log link, y ~ neg_binomial_2_log(eta, phi) with
    log phi ~ N(m, s^2): GLMTarget(X, y, family="neg_binomial_2_log", ...).  The last coordinate is log phi;
    constrain() reports phi.  exposure (finite, > 0) is offset = log(exposure)."""
    offset = _exposure_offset("NegativeBinomialRegression", offset, exposure)
    return GLMTarget(X, y, family="neg_binomial_2_log", prior_sd=prior_sd, intercept=intercept,
                     dispersion_prior=dispersion_prior, offset=offset, weights=weights)


def GammaRegression(X, y, prior_sd=2.5, dispersion_prior=(0.0, 2.5), intercept=True):
    """Bayesian gamma regression with a log link, y ~ gamma(shape, shape / e^eta) with log shape ~ N(m, s^2):
    ContinuousGLM(X, y, family="gamma_log", ...).  The last coordinate is log shape; constrain() reports shape."""
    return ContinuousGLM(X, y, family="gamma_log", prior_sd=prior_sd, intercept=intercept,
                         dispersion_prior=dispersion_prior)


def RobustRegression(X, y, df=_checks.DEFAULT_DF, prior_sd=2.5, dispersion_prior=(0.0, 2.5), intercept=True):
    """Bayesian robust linear regression, y ~ student_t(df, eta, sigma) with df fixed and log sigma ~ N(m, s^2):
    ContinuousGLM(X, y, family="student_t", df=df, ...).  The last coordinate is log sigma; constrain() reports sigma."""
    return ContinuousGLM(X, y, family="student_t", prior_sd=prior_sd, intercept=intercept,
                         dispersion_prior=dispersion_prior, df=df)


def StanModel(model_name, model_path=None, data_path=None):
    """Same call shape as the reference's StanModel(model_name, model_path,
    data_path) (bridgestan.py:13); resolves the model NAME to its device
    functor -- arbitrary .stan files are not compiled here."""
    name = str(model_name).lower()
    if name == "arma":
        return ArmaModel(data_path)
    if name == "prmwcd":
        return PRMwCDModel(data_path)
    raise NotImplementedError(
        f"no device-native functor for Stan model {model_name!r} (available: arma, PRMwCD).  Pass the model "
        "object itself -- anything with .dim / .logpdf(x, phi) / .logpdfgrad(x, phi), e.g. the reference's "
        "StanModel over BridgeStan -- as `target`: it is evaluated on the host through HostTarget.")
