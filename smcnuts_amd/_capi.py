"""ctypes binding of libsmcnuts_hip.so (include/smcnuts_hip.h).

There is no CPU fallback: if the library is missing or no GPU is visible the
product raises."""
import ctypes as C
import os

import numpy as np

from . import build as _build

MODEL_GAUSS, MODEL_ARMA, MODEL_PRMWCD, MODEL_HOST = 0, 1, 2, 3
MODEL_GLM = 4
MODEL_HGLM = 5
MODEL_CATEGORICAL = 6
MODEL_ORDINAL = 7
MODEL_MLGLM = 8
MODEL_WGLM = 9
MODEL_OGLM = 10
MODEL_CGLM = 12                            # (11 is unassigned)
HOST_TARGET_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_double), C.c_int,
                             C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                             C.POINTER(C.c_double))
LKERNEL_FORWARD, LKERNEL_GAUSSIAN = 0, 1

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_lp = C.POINTER(C.c_int64)
_ctx = C.c_void_p

SIGNATURES = {
    "smcn_version": ([], C.c_int),
    "smcn_last_error": ([_ctx], C.c_char_p),
    "smcn_ctx_create": ([C.POINTER(_ctx), C.c_int, C.c_int64, C.c_int64, C.c_int, _dp, C.c_int64], C.c_int),
    "smcn_ctx_destroy": ([_ctx], None),
    "smcn_dim": ([_ctx], C.c_int),
    "smcn_constrained_dim": ([_ctx], C.c_int),
    "smcn_fused_transitions": ([_ctx], C.c_int),
    "smcn_set_stream": ([_ctx, C.c_void_p], C.c_int),
    "smcn_synchronize": ([_ctx], C.c_int),
    "smcn_set_seed": ([_ctx, C.c_uint64], C.c_int),
    "smcn_set_state": ([_ctx, _dp, _dp], C.c_int),
    "smcn_get_state": ([_ctx, _dp, _dp, _dp], C.c_int),
    "smcn_get_proposal": ([_ctx, _dp, _dp, _dp, _dp], C.c_int),
    "smcn_set_momentum": ([_ctx, _dp], C.c_int),
    "smcn_set_proposal": ([_ctx, _dp, _dp, _dp], C.c_int),
    "smcn_target_eval": ([_ctx, _dp, C.c_int64, C.c_double, _dp, _dp, _dp, _dp], C.c_int),
    "smcn_target_constrain": ([_ctx, _dp, C.c_int64, _dp], C.c_int),
    "smcn_init_particles_std_normal": ([_ctx, C.c_double], C.c_int),
    "smcn_init_weights": ([_ctx, C.c_double, _dp], C.c_int),
    "smcn_normalise_partials": ([_ctx, _dp], C.c_int),
    "smcn_normalise_apply": ([_ctx, C.c_double], C.c_int),
    "smcn_normalise": ([_ctx, _dp, _dp], C.c_int),
    "smcn_moment_sums": ([_ctx, _dp, _dp], C.c_int),
    "smcn_resample_multinomial": ([_ctx, _dp, C.c_double, C.c_double, C.c_int64, _lp], C.c_int),
    "smcn_propose_nuts": ([_ctx, C.c_double, C.c_double, C.c_int, C.c_double, C.c_int64, _dp, _lp], C.c_int),
    "smcn_get_tree_stats": ([_ctx, _ip, _ip, _ip, _ip], C.c_int),
    "smcn_last_leapfrogs": ([_ctx, _lp], C.c_int),
    "smcn_get_density_parts": ([_ctx, _dp, _dp, _dp, _dp], C.c_int),
    "smcn_set_lkernel_values": ([_ctx, _dp, _dp], C.c_int),
    "smcn_reweight": ([_ctx, C.c_int], C.c_int),
    "smcn_accept_reject": ([_ctx, C.c_double, _dp, C.c_int64], C.c_int),
    "smcn_reweight_asymptotic": ([_ctx, C.c_double, C.c_double], C.c_int),
    "smcn_set_logw_density_ratio": ([_ctx, C.c_double, C.c_double], C.c_int),
    "smcn_gauss_lkernel_sums": ([_ctx, _dp, _dp], C.c_int),
    "smcn_gauss_lkernel_logpdf": ([_ctx, _dp, _dp, _dp, _dp, C.c_double], C.c_int),
    "smcn_gauss_lkernel_device": ([_ctx, _dp], C.c_int),
    "smcn_gauss_lkernel_buffers": ([_ctx, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)], C.c_int),
    "smcn_gauss_lkernel_stage": ([_ctx, C.c_int, C.c_int, C.c_double, _dp], C.c_int),
    "smcn_set_nuts_cap": ([_ctx, C.c_int, C.c_int], C.c_int),
    "smcn_set_nuts_requeue": ([_ctx, C.c_int], C.c_int),
    "smcn_nuts_parked": ([_ctx, C.POINTER(C.c_int64)], C.c_int),
    "smcn_temper_partials": ([_ctx, C.c_double, C.c_double, _dp], C.c_int),
    "smcn_temper_bisect": ([_ctx, C.c_double, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_int)], C.c_int),
    "smcn_temper_bisect_pass": ([_ctx, C.c_int, C.c_double], C.c_int),
    "smcn_temper_bisect_buffers": ([_ctx, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)], C.c_int),
    "smcn_temper_bisect_decide": ([_ctx, C.c_int, C.c_int, C.c_double, C.c_double], C.c_int),
    "smcn_temper_bisect_result": ([_ctx, C.POINTER(C.c_double), C.POINTER(C.c_int)], C.c_int),
    "smcn_eval_proposed_parts": ([_ctx, C.c_int], C.c_int),
    "smcn_commit": ([_ctx, _lp], C.c_int),
    "smcn_fast_begin": ([_ctx, C.c_int64, C.c_int, C.c_int], C.c_int),
    "smcn_fast_buffers": ([_ctx, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int)], C.c_int),
    "smcn_set_resample_uniforms": ([_ctx, _dp], C.c_int),
    "smcn_step_begin": ([_ctx, C.c_int64], C.c_int),
    "smcn_step_finish": ([_ctx, C.c_int64, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int,
                          C.c_double, C.c_int, C.c_int, _dp, _lp], C.c_int),
    "smcn_fast_read": ([_ctx, _dp, _dp, _dp], C.c_int),
    "smcn_fast_read_from": ([_ctx, _dp, _dp, _dp, C.c_int64], C.c_int),
    "smcn_history_download": ([_ctx, C.c_int64, C.c_int64, _dp, _dp], C.c_int),
    "smcn_fuse_begin": ([_ctx, C.c_int, C.c_int], C.c_int),
    "smcn_fuse_buffers": ([_ctx, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int)], C.c_int),
    "smcn_fuse_run": ([_ctx, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int,
                       C.c_double, C.c_int], C.c_int),
    "smcn_set_resample_scheme": ([_ctx, C.c_int], C.c_int),
    "smcn_set_wide_eval": ([_ctx, C.c_int], C.c_int),
    "smcn_set_phase_paths": ([_ctx, C.c_int], C.c_int),
    "smcn_set_tree_align": ([_ctx, C.c_int], C.c_int),
    "smcn_get_wave_iterations": ([_ctx, C.POINTER(C.c_uint32), C.c_int64], C.c_int),
    "smcn_set_lane_grid": ([_ctx, C.c_int64], C.c_int),
    "smcn_set_lane_segments": ([_ctx, C.c_int], C.c_int),
    "smcn_set_host_target": ([_ctx, HOST_TARGET_FN, C.c_void_p], C.c_int),
    "smcn_moment_sums_of": ([_ctx, _dp, C.c_int, _dp, _dp], C.c_int),
    "smcn_block_resample_local": ([_ctx, C.c_int64], C.c_int),
    "smcn_block_launch": ([_ctx, C.c_int64, C.c_int, C.c_double, C.c_double, C.c_int, C.c_double], C.c_int),
    "smcn_block_post": ([_ctx, C.c_int64, C.c_int, C.c_int], C.c_int),
    "smcn_block_partials_get": ([_ctx, C.c_int, _dp], C.c_int),
    "smcn_block_partials_set": ([_ctx, C.c_int, C.c_int, _dp], C.c_int),
    "smcn_block_stats": ([_ctx, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int], C.c_int),
    "smcn_block_wait": ([_ctx, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)], C.c_int),
    "smcn_block_commit": ([_ctx, C.c_int64, C.c_int], C.c_int),
    "smcn_set_block_post": ([_ctx, C.c_int], C.c_int),
    "smcn_block_ess": ([_ctx, C.c_int, _dp], C.c_int),
    "smcn_fuse_decide": ([_ctx, C.c_int64, C.c_int, C.c_int, C.c_double, C.c_double, C.POINTER(C.c_int)], C.c_int),
    "smcn_fuse_finish": ([_ctx, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double,
                          C.POINTER(C.c_int)], C.c_int),
    "smcn_partials_get": ([_ctx, _dp], C.c_int),
    "smcn_partials_set_gathered": ([_ctx, _dp, C.c_int], C.c_int),
    "smcn_timers": ([_ctx, _dp, C.c_int], C.c_int),
    "smcn_selftest_math": ([_ctx, _dp, C.c_int64, _dp], C.c_int),
    "smcn_measure_peaks": ([_ctx, _dp], C.c_int),
    "smcn_selftest_wide": ([_ctx, C.c_int, _dp, C.c_int64, _dp], C.c_int),
    "smcn_selftest_recur": ([_ctx, _dp, C.c_int64, _dp], C.c_int),
    "smcn_device_cache_trim": ([C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)], C.c_int),
    "smcn_debug_profile": ([_ctx, C.POINTER(C.c_uint64), C.c_int], C.c_int),
    "smcn_bench_resample": ([_ctx, C.c_int, C.c_int64, _dp], C.c_int),
    "smcn_comm_unique_id": ([C.c_char_p], C.c_int),
    "smcn_comm_init": ([_ctx, C.c_int, C.c_int, C.c_char_p], C.c_int),
    "smcn_comm_destroy": ([_ctx], C.c_int),
    "smcn_comm_info": ([_ctx, C.POINTER(C.c_int)], C.c_int),
    "smcn_comm_allgather": ([_ctx, C.c_void_p, C.c_void_p, C.c_int64], C.c_int),
    "smcn_comm_allgather_host": ([_ctx, _dp, C.c_int64, _dp], C.c_int),
    "smcn_comm_alltoallv": ([_ctx, C.c_void_p, _lp, C.c_void_p, _lp, C.c_int], C.c_int),
    "smcn_buf_get": ([_ctx, C.c_void_p, C.c_int64, _dp], C.c_int),
    "smcn_buf_set": ([_ctx, C.c_void_p, C.c_int64, _dp], C.c_int),
    "smcn_buf_copy": ([_ctx, C.c_void_p, C.c_void_p, C.c_int64], C.c_int),
    "smcn_gres_begin": ([_ctx, C.c_int, _dp], C.c_int),
    "smcn_gres_buffers": ([_ctx] + [C.POINTER(C.c_void_p)] * 6, C.c_int),
    "smcn_gres_plan": ([_ctx, C.c_int, C.c_int, _dp, C.c_int64, _ip], C.c_int),
    "smcn_gres_set_order": ([_ctx, _ip], C.c_int),
    "smcn_gres_reserve": ([_ctx, C.c_int64], C.c_int),
    "smcn_gres_serve": ([_ctx, C.c_int, C.c_int, C.c_int64], C.c_int),
    "smcn_gres_finish": ([_ctx, C.c_int, _dp], C.c_int),
    "smcn_pointwise_dims": ([_ctx, _lp, C.POINTER(C.c_int)], C.c_int),
    "smcn_pointwise_loglik": ([_ctx, _dp, C.c_int64, _dp], C.c_int),
    "smcn_pointwise_partials": ([_ctx, _dp, _dp, C.c_int64, _dp], C.c_int),
    "smcn_pointwise_last_ms": ([_ctx, _dp], C.c_int),
    "smcn_calibration_dims": ([_ctx, _lp, C.POINTER(C.c_int)], C.c_int),
    "smcn_calibration_points": ([_ctx, _dp, C.c_int64, _dp], C.c_int),
    "smcn_calibration_partials": ([_ctx, _dp, _dp, C.c_int64, _dp], C.c_int),
    "smcn_calibration_last_ms": ([_ctx, _dp], C.c_int),
    "smcn_psis_candidates": ([_ctx, _dp, _dp, C.c_int64, C.c_double, C.c_int64, _dp], C.c_int),
    "smcn_psis_body": ([_ctx, _dp, _dp, C.c_int64, C.c_double, C.c_int64, _dp, _dp], C.c_int),
    "smcn_psis_fit": ([_ctx, _dp, _dp, C.c_int64, C.c_double, C.c_int64, _dp], C.c_int),
    "smcn_psis_loo": ([_ctx, _dp, _dp, C.c_int64, _dp, _dp], C.c_int),
    "smcn_psis_last_ms": ([_ctx, _dp], C.c_int),
    "smcn_predict_set_data": ([_ctx, _dp, C.c_int64, C.c_int], C.c_int),
    "smcn_predict_dims": ([_ctx, _lp, C.POINTER(C.c_int), C.POINTER(C.c_int)], C.c_int),
    "smcn_predict_loglik": ([_ctx, _dp, C.c_int64, _dp], C.c_int),
    "smcn_predict_partials": ([_ctx, _dp, _dp, C.c_int64, _dp], C.c_int),
    "smcn_predict_last_ms": ([_ctx, _dp], C.c_int),
    "smcn_predict_draws": ([_ctx, _dp, _dp, C.c_int64, C.c_int64, C.c_uint64, _lp, _lp, C.c_int64, C.c_int64, _dp, _lp,
                            _lp], C.c_int),
    "smcn_predict_draws_last_ms": ([_ctx, _dp], C.c_int),
    "smcn_summary_begin": ([_ctx, _dp, _dp, _dp, C.c_int64, C.c_int, _dp], C.c_int),
    "smcn_summary_weights": ([_ctx, C.c_double, C.c_double, _dp], C.c_int),
    "smcn_summary_select": ([_ctx, C.c_int, _dp], C.c_int),
    "smcn_summary_hist": ([_ctx, C.c_int, C.c_int, _dp], C.c_int),
    "smcn_summary_descend": ([_ctx, C.c_int, C.c_int, _ip, _dp], C.c_int),
    "smcn_summary_values": ([_ctx, C.c_int, _dp, _dp], C.c_int),
    "smcn_summary_cdf": ([_ctx, C.c_int, _dp, _dp], C.c_int),
    "smcn_summary_last_ms": ([_ctx, _dp], C.c_int),
    "smcn_summary_pass_ms": ([_ctx, _dp], C.c_int),
    "smcn_cov_partials": ([_ctx, C.c_double, _dp, C.c_int64, _dp, _dp], C.c_int),
    "smcn_cov_dims": ([_ctx, C.POINTER(C.c_int64)], C.c_int),
    "smcn_cov_last_ms": ([_ctx, _dp], C.c_int),
    "smcn_stepsize_probe": ([_ctx, _dp, _dp, C.c_int64, _dp, _dp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_uint64,
                             C.c_int64, _dp, _dp, _ip], C.c_int),
    "smcn_stepsize_last_ms": ([_ctx], C.c_double),
    "smcn_forecast_set": ([_ctx, C.c_int64, _dp, _dp, C.c_int], C.c_int),
    "smcn_forecast_dims": ([_ctx, _lp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)], C.c_int),
    "smcn_forecast_slices": ([_ctx, C.c_int64, _lp], C.c_int),
    "smcn_forecast_points": ([_ctx, _dp, C.c_int64, _dp], C.c_int),
    "smcn_forecast_partials": ([_ctx, _dp, _dp, C.c_int64, _dp], C.c_int),
    "smcn_forecast_draws": ([_ctx, _dp, _dp, C.c_int64, C.c_int64, C.c_uint64, _lp, C.c_int64, C.c_int64, _dp, _lp, _lp],
                            C.c_int),
    "smcn_forecast_last_ms": ([_ctx, _dp], C.c_int),
    "smcn_residuals_set": ([_ctx, C.c_int, _dp, C.c_int], C.c_int),
    "smcn_residuals_dims": ([_ctx, _lp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)], C.c_int),
    "smcn_residuals_points": ([_ctx, _dp, C.c_int64, _dp], C.c_int),
    "smcn_residuals_partials": ([_ctx, _dp, _dp, C.c_int64, _dp], C.c_int),
    "smcn_residuals_last_ms": ([_ctx, _dp], C.c_int),
}

_lib = None


class SmcnError(RuntimeError):
    pass


def lib():
    """Load libsmcnuts_hip.so; raises if it has not been built."""
    global _lib
    if _lib is None:
        path = os.environ.get("SMCN_LIB") or _build.LIB     # SMCN_LIB: diagnostic / A-B builds of the same ABI
        if not os.path.exists(path):
            raise SmcnError(
                f"{path} is missing: build the HIP extension first "
                "(python -c 'import __graft_entry__ as g; g.build()').  There is no CPU fallback.")
        _lib = C.CDLL(path)
        for name, (args, res) in SIGNATURES.items():
            fn = getattr(_lib, name)
            fn.argtypes, fn.restype = args, res
    return _lib


def dptr(a):
    if a is None:
        return None
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_dp)


def iptr(a):
    return None if a is None else a.ctypes.data_as(_ip)


def lptr(a):
    return None if a is None else a.ctypes.data_as(_lp)


def trim_device_cache(device=-1):
    """Streams and device buffers of closed contexts stay pooled in the library (include/smcnuts_hip.h,
    smcn_device_cache_trim): give the idle buffers of `device` (-1: all) back to the driver.  Returns
    (bytes released, bytes that were idle)."""
    rel, idle = C.c_int64(0), C.c_int64(0)
    rc = lib().smcn_device_cache_trim(int(device), C.byref(rel), C.byref(idle))
    if rc:
        raise RuntimeError("smcn_device_cache_trim failed")
    return rel.value, idle.value


class Context:
    """One GPU shard of N particles (smcn_ctx)."""

    def __init__(self, n_particles, model_id, model_data, device=0, particle_base=0):
        self._lib = lib()
        self.N = int(n_particles)
        self.particle_base = int(particle_base)
        md = np.ascontiguousarray(model_data, dtype=np.float64)
        h = _ctx()
        rc = self._lib.smcn_ctx_create(C.byref(h), int(device), self.N, self.particle_base, int(model_id),
                                       dptr(md), md.size)
        if rc != 0:
            raise SmcnError(self._lib.smcn_last_error(None).decode())
        self._h = h
        self.D = self._lib.smcn_dim(h)
        self.Dc = self._lib.smcn_constrained_dim(h)
        self.fused_transitions = self._lib.smcn_fused_transitions(h) == 1

    def close(self):
        if getattr(self, "_h", None):
            self._lib.smcn_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def call(self, name, *args):
        rc = getattr(self._lib, name)(self._h, *args)
        if rc != 0:
            raise SmcnError(f"{name}: {self._lib.smcn_last_error(self._h).decode()}")

    def _particles(self, x, logw):
        """(x, logw, M) as the post-fit entry points take them: x=None: the resident particles and weights."""
        if x is None:
            return None, None, self.N
        x = np.ascontiguousarray(np.atleast_2d(x), dtype=np.float64)
        lw = None if logw is None else np.ascontiguousarray(logw, dtype=np.float64)
        if lw is not None and lw.shape != (x.shape[0],):
            raise ValueError("logw must hold one log-weight per row of x")
        return dptr(x), dptr(lw), x.shape[0]

    def _last_ms(self, name, n=0):
        """What the timer entry point `name` reports: a number, or n of them."""
        ms = np.zeros(max(n, 1))
        if getattr(self._lib, name)(self._h, dptr(ms)) != 0:
            raise SmcnError(f"{name} failed")
        return ms if n else float(ms[0])

    # ---- convenience wrappers -------------------------------------------------
    def set_seed(self, seed):
        self.call("smcn_set_seed", C.c_uint64(int(seed) & (2 ** 64 - 1)))

    def set_state(self, x=None, logw=None):
        x = None if x is None else np.ascontiguousarray(x, dtype=np.float64)
        logw = None if logw is None else np.ascontiguousarray(logw, dtype=np.float64)
        self.call("smcn_set_state", dptr(x), dptr(logw))

    def get_state(self, x=True, logw=True, wn=False):
        X = np.empty((self.N, self.D)) if x else None
        lw = np.empty(self.N) if logw else None
        w = np.empty(self.N) if wn else None
        self.call("smcn_get_state", dptr(X), dptr(lw), dptr(w))
        return X, lw, w

    def get_proposal(self, r=True, x_new=True, r_new=True, logw_new=False):
        R = np.empty((self.N, self.D)) if r else None
        Xn = np.empty((self.N, self.D)) if x_new else None
        Rn = np.empty((self.N, self.D)) if r_new else None
        lw = np.empty(self.N) if logw_new else None
        self.call("smcn_get_proposal", dptr(R), dptr(Xn), dptr(Rn), dptr(lw))
        return R, Xn, Rn, lw

    def target_eval(self, x, phi=1.0, want_grad=False, want_parts=False):
        x = np.ascontiguousarray(np.atleast_2d(x), dtype=np.float64)
        M = x.shape[0]
        lp = np.empty(M)
        g = np.empty((M, self.D)) if want_grad else None
        a = np.empty(M) if want_parts else None
        b = np.empty(M) if want_parts else None
        self.call("smcn_target_eval", dptr(x), M, float(phi), dptr(lp), dptr(g), dptr(a), dptr(b))
        return lp, g, a, b

    def constrain(self, x):
        x = np.ascontiguousarray(np.atleast_2d(x), dtype=np.float64)
        out = np.empty((x.shape[0], self.Dc))
        self.call("smcn_target_constrain", dptr(x), x.shape[0], dptr(out))
        return out

    def normalise_partials(self):
        p = np.empty(4)
        self.call("smcn_normalise_partials", dptr(p))
        return p

    def temper_partials(self, phi_old, phi_new):
        p = np.empty(4)
        self.call("smcn_temper_partials", float(phi_old), float(phi_new), dptr(p))
        return p

    def moment_sums(self, mean=None):
        s = np.empty(self.Dc)
        m = None if mean is None else np.ascontiguousarray(mean, dtype=np.float64)
        self.call("smcn_moment_sums", dptr(m), dptr(s))
        return s

    def resample(self, loglik, log_n_total, iteration, u=None, want_idx=False):
        u = None if u is None else np.ascontiguousarray(u, dtype=np.float64)
        idx = np.empty(self.N, dtype=np.int64) if want_idx else None
        self.call("smcn_resample_multinomial", dptr(u), float(loglik), float(log_n_total), int(iteration), lptr(idx))
        return idx

    def propose_nuts(self, step_size, phi, iteration, max_depth=10, delta_max=100.0, tape=None, tape_off=None):
        if tape is not None:
            tape = np.ascontiguousarray(tape, dtype=np.float64)
            tape_off = np.ascontiguousarray(tape_off, dtype=np.int64)
            if tape_off.size != self.N + 1:
                raise ValueError("tape_off must have N+1 entries")
        self.call("smcn_propose_nuts", float(step_size), float(phi), int(max_depth), float(delta_max),
                  int(iteration), dptr(tape), lptr(tape_off))

    def tree_stats(self):
        a, b, c, d = (np.empty(self.N, dtype=np.int32) for _ in range(4))
        self.call("smcn_get_tree_stats", iptr(a), iptr(b), iptr(c), iptr(d))
        return dict(nleap=a, depth=b, ndraws=c, flags=d)

    def last_leapfrogs(self):
        v = C.c_int64(0)
        self.call("smcn_last_leapfrogs", C.byref(v))
        return v.value

    def density_parts(self):
        a, b, c, d = (np.empty(self.N) for _ in range(4))
        self.call("smcn_get_density_parts", dptr(a), dptr(b), dptr(c), dptr(d))
        return a, b, c, d

    def commit(self, count_moved=True):
        v = C.c_int64(0)
        self.call("smcn_commit", C.byref(v) if count_moved else None)
        return v.value

    # ---- device-resident loop ----------------------------------------------------
    def fast_begin(self, K, save_history, world=1):
        self.call("smcn_fast_begin", int(K), int(bool(save_history)), int(world))
        a, b, n = C.c_void_p(), C.c_void_p(), C.c_int()
        self.call("smcn_fast_buffers", C.byref(a), C.byref(b), C.byref(n))
        self.lp_ptr, self.gath_ptr, self.nq = a.value, b.value, n.value

    def step_begin(self, k):
        self.call("smcn_step_begin", int(k))

    def step_finish(self, k, world, rank, n_total, step_size, phi, max_depth=10, delta_max=100.0, last=False,
                    tape=None, tape_off=None):
        if tape is not None:
            tape = np.ascontiguousarray(tape, dtype=np.float64)
            tape_off = np.ascontiguousarray(tape_off, dtype=np.int64)
        self.call("smcn_step_finish", int(k), int(world), int(rank), float(n_total), float(step_size), float(phi),
                  int(max_depth), float(delta_max), LKERNEL_FORWARD, int(bool(last)), dptr(tape), lptr(tape_off))

    def fast_read(self, K, save_history, xs=None, lw=None, k_from=0):
        """Scalar history and, with save_history, x_saved / logw_saved -- into the caller's arrays when given (already
        touched memory: a fresh 100 MB array costs more in page faults than its bytes cost on the bus)."""
        hs = 6 + 2 * self.Dc
        hist = np.empty((K + 1, hs))
        if save_history:
            ok = lambda a, shape: a is not None and a.shape == shape and a.dtype == np.float64 and a.flags.c_contiguous
            xs = xs if ok(xs, (K + 1, self.N, self.D)) else np.empty((K + 1, self.N, self.D))
            lw = lw if ok(lw, (K + 1, self.N)) else np.empty((K + 1, self.N))
        else:
            xs = lw = None
        self.call("smcn_fast_read_from", dptr(hist), dptr(xs), dptr(lw), int(k_from))
        return hist, xs, lw

    def partials_get(self):
        p = np.empty(self.nq)
        self.call("smcn_partials_get", dptr(p))
        return p

    def partials_set_gathered(self, g):
        g = np.ascontiguousarray(g, dtype=np.float64)
        self.call("smcn_partials_set_gathered", dptr(g), int(g.shape[0]))

    # ---- pointwise criteria (SMCN_MODEL_GLM) -----------------------------------------
    def pointwise_dims(self):
        n, q = C.c_int64(0), C.c_int(0)
        self.call("smcn_pointwise_dims", C.byref(n), C.byref(q))
        return n.value, q.value

    def pointwise_loglik(self, x):
        x = np.ascontiguousarray(np.atleast_2d(x), dtype=np.float64)
        n, _ = self.pointwise_dims()
        out = np.empty((x.shape[0], n))
        self.call("smcn_pointwise_loglik", dptr(x), x.shape[0], dptr(out))
        return out

    def pointwise_partials(self, x=None, logw=None):
        """[1 + n][Q] mergeable partials (include/smcnuts_hip.h); x=None: the resident particles and weights."""
        n, q = self.pointwise_dims()
        out = np.empty((1 + n, q))
        self.call("smcn_pointwise_partials", *self._particles(x, logw), dptr(out))
        return out

    def pointwise_last_ms(self):
        """Device time of the last pointwise_partials' kernels (HIP events on the context's stream)."""
        return self._last_ms("smcn_pointwise_last_ms")

    # ---- calibration (SMCN_MODEL_GLM; include/smcnuts_hip.h, smcn_calibration_*) --------
    def calibration_dims(self):
        n, q = C.c_int64(0), C.c_int(0)
        self.call("smcn_calibration_dims", C.byref(n), C.byref(q))
        return n.value, q.value

    def calibration_points(self, x):
        """[M][n][2]: (lo, up) = (P(Y < y_i), P(Y > y_i)) under every point of x; NaN for an unconverged pair."""
        x = np.ascontiguousarray(np.atleast_2d(x), dtype=np.float64)
        n, _ = self.calibration_dims()
        out = np.empty((x.shape[0], n, 2))
        self.call("smcn_calibration_points", dptr(x), x.shape[0], dptr(out))
        return out

    def calibration_partials(self, x=None, logw=None):
        """[1 + n][Qc] mergeable partials (include/smcnuts_hip.h); x=None: the resident particles and weights."""
        n, q = self.calibration_dims()
        out = np.empty((1 + n, q))
        self.call("smcn_calibration_partials", *self._particles(x, logw), dptr(out))
        return out

    def calibration_last_ms(self):
        """Device time of the last calibration_partials' kernels (HIP events on the context's stream)."""
        return self._last_ms("smcn_calibration_last_ms")

    # ---- Pareto-smoothed LOO (SMCN_MODEL_GLM; include/smcnuts_hip.h, smcn_psis_*) ------
    def psis_candidates(self, mw, S, x=None, logw=None):
        """(lr, ll), each [n][T_cap]: this rank's T_cap largest ratios per observation, descending."""
        from .psis import tail_len
        xp, lp_, M = self._particles(x, logw)
        n, _ = self.pointwise_dims()
        out = np.empty((2, n, tail_len(S) + 1))
        self.call("smcn_psis_candidates", xp, lp_, M, float(mw), int(S), dptr(out))
        return out[0], out[1]

    def psis_body(self, mw, S, cutoff, x=None, logw=None):
        """[n][4] body partials (mb, Sb, Sb2, Sw) of the particles at or below the per-observation cutoffs."""
        xp, lp_, M = self._particles(x, logw)
        n, _ = self.pointwise_dims()
        cutoff = np.ascontiguousarray(cutoff, dtype=np.float64)
        if cutoff.shape != (n,):
            raise ValueError("cutoff must hold one value per observation")
        out = np.empty((n, 4))
        self.call("smcn_psis_body", xp, lp_, M, float(mw), int(S), dptr(cutoff), dptr(out))
        return out

    def psis_fit(self, lr, ll, body, mw, S):
        """[n][6] = pareto_k, elpd_psis, psis_ess, tail_len, cutoff, sigma from merged candidates and body partials."""
        from .psis import tail_len
        cand = np.ascontiguousarray(np.stack([lr, ll]), dtype=np.float64)
        body = np.ascontiguousarray(body, dtype=np.float64)
        n = cand.shape[1]
        if cand.ndim != 3 or cand.shape[2] != tail_len(S) + 1 or body.shape != (n, 4):
            raise ValueError("psis_fit: candidates are [n][tail_len(S) + 1] and body partials [n][4]")
        out = np.empty((n, 6))
        self.call("smcn_psis_fit", dptr(cand), dptr(body), n, float(mw), int(S), dptr(out))
        return out

    def psis_loo(self, x=None, logw=None):
        """([n][6], header [mw, sw, sw2, S]) of one rank's particles: the three stages without a host round trip."""
        xp, lp_, M = self._particles(x, logw)
        n, _ = self.pointwise_dims()
        out, head = np.empty((n, 6)), np.empty(4)
        self.call("smcn_psis_loo", xp, lp_, M, dptr(out), dptr(head))
        return out, head

    def psis_last_ms(self):
        """Device time [candidates, body, fit, whole psis_loo] of the last calls (HIP events on the context's stream)."""
        return self._last_ms("smcn_psis_last_ms", 4)

    # ---- held-out prediction (GLM, hierarchical, categorical, ordinal) ----------------
    def predict_set_data(self, block, has_y):
        """The new rows as the model's data block without the priors (include/smcnuts_hip.h)."""
        block = np.ascontiguousarray(block, dtype=np.float64)
        self.call("smcn_predict_set_data", dptr(block), block.size, int(bool(has_y)))

    def predict_dims(self):
        m, q, hy = C.c_int64(0), C.c_int(0), C.c_int(0)
        self.call("smcn_predict_dims", C.byref(m), C.byref(q), C.byref(hy))
        return m.value, q.value, bool(hy.value)

    def predict_loglik(self, x):
        x = np.ascontiguousarray(np.atleast_2d(x), dtype=np.float64)
        m, _, _ = self.predict_dims()
        out = np.empty((x.shape[0], m))
        self.call("smcn_predict_loglik", dptr(x), x.shape[0], dptr(out))
        return out

    def predict_partials(self, x=None, logw=None):
        """[1 + m][Q] mergeable partials (include/smcnuts_hip.h); x=None: the resident particles and weights."""
        m, q, _ = self.predict_dims()
        out = np.empty((1 + m, q))
        self.call("smcn_predict_partials", *self._particles(x, logw), dptr(out))
        return out

    def predict_last_ms(self):
        """Device time of the last predict_partials' kernels (HIP events on the context's stream)."""
        return self._last_ms("smcn_predict_last_ms")

    def _draws(self, fn, width, noun, S, seed, x, logw, ancestors, s_first, s_count, grouped=False, new_group=None):
        """The body of predict_draws and forecast_draws: `width` values per `noun`; grouped: `fn` takes new_group."""
        S = int(S)
        n = S - int(s_first) if s_count is None else int(s_count)
        y, anc, nbad = np.empty((max(n, 0), width)), np.empty(max(n, 0), dtype=np.int64), C.c_int64(0)
        a_in = None if ancestors is None else np.ascontiguousarray(ancestors, dtype=np.int64)
        if a_in is not None and a_in.shape != (S,):
            raise ValueError(f"ancestors must hold one particle index per {noun}")
        g_in = None if new_group is None else np.ascontiguousarray(new_group, dtype=np.int64)
        if g_in is not None and g_in.shape != (width,):
            raise ValueError("new_group must hold one label per new row")
        self.call(fn, *self._particles(x, logw), S, C.c_uint64(int(seed) & (2 ** 64 - 1)), lptr(a_in),
                  *((lptr(g_in),) if grouped else ()), int(s_first), n, dptr(y), lptr(anc), C.byref(nbad))
        return y, anc, nbad.value

    def predict_draws(self, S, seed, x=None, logw=None, ancestors=None, new_group=None, s_first=0, s_count=None):
        """(y [s_count][m], ancestors [s_count], n_bad): posterior predictive draws of the slots s_first .. of S at the
        rows of the last predict_set_data (include/smcnuts_hip.h); x=None: the resident particles and weights."""
        return self._draws("smcn_predict_draws", self.predict_dims()[0], "draw", S, seed, x, logw, ancestors, s_first, s_count,
                           True, new_group)

    def predict_draws_last_ms(self):
        """Device time of the last predict_draws' kernels (HIP events on the context's stream)."""
        return self._last_ms("smcn_predict_draws_last_ms")

    # ---- posterior summaries (every model) ---------------------------------------------
    def summary_begin(self, x=None, logw=None, v=None):
        """Stage a population (include/smcnuts_hip.h): x=None and v=None: the resident particles and log-weights; x [M][D]
        unconstrained points; v [M][Dv] constrained values.  Returns (header [4] of this shard's log-weights, columns)."""
        head = np.empty(4)
        if x is None and v is None:
            self.call("smcn_summary_begin", None, None, None, self.N, 0, dptr(head))
            return head, self.Dc
        ap, lp_, M = self._particles(x if v is None else v, logw)
        if v is None:
            self.call("smcn_summary_begin", ap, lp_, None, M, 0, dptr(head))
            return head, self.Dc
        self.call("smcn_summary_begin", None, lp_, ap, M, np.atleast_2d(v).shape[1], dptr(head))
        return head, np.atleast_2d(v).shape[1]

    def summary_weights(self, lw_max, lw_sum):
        m = C.c_double(0.0)
        self.call("smcn_summary_weights", float(lw_max), float(lw_sum), C.byref(m))
        return int(m.value)

    def summary_select(self, thresholds):
        t = np.ascontiguousarray(thresholds, dtype=np.float64)
        self.call("smcn_summary_select", t.size, dptr(t))

    def summary_hist(self, k, nq, Dc):
        out = np.empty(Dc * (1 if k == 0 else nq) * 256 + Dc)
        self.call("smcn_summary_hist", int(k), int(nq), dptr(out))
        return out

    def summary_descend(self, k, digits, residual):
        d = np.ascontiguousarray(digits, dtype=np.int32)
        r = np.ascontiguousarray(residual, dtype=np.float64)
        self.call("smcn_summary_descend", int(k), d.shape[1], iptr(d), dptr(r))

    def summary_values(self, nq, Dc):
        out, flags = np.empty((Dc, nq)), np.empty(Dc)
        self.call("smcn_summary_values", int(nq), dptr(out), dptr(flags))
        return out, flags

    def summary_cdf(self, at):
        at = np.ascontiguousarray(at, dtype=np.float64)
        Dc, T = at.shape
        out = np.empty(Dc * T + Dc)
        self.call("smcn_summary_cdf", T, dptr(at), dptr(out))
        return out

    def summary_last_ms(self):
        """Device time of the summary kernels since the last summary_begin (HIP events on the context's stream)."""
        return self._last_ms("smcn_summary_last_ms")

    def summary_pass_ms(self):
        return self._last_ms("smcn_summary_pass_ms", 8)

    # ---- posterior covariance (every model; the population staged by summary_begin) -----
    def cov_dims(self):
        """(M, Dc, the slice rule's count, the most slices a call may ask for) of the staged population."""
        out = (C.c_int64 * 4)()
        if self._lib.smcn_cov_dims(self._h, out) != 0:
            raise SmcnError("smcn_cov_dims: call summary_begin first")
        return tuple(int(v) for v in out)

    def cov_partials(self, lw_max, Dc, centre=None, slices=0):
        """(augmented sums [Dc+1][Dc+1] = [[G, S1], [S1', W]] about the centre, the centre [Dc] the device used) of the
        staged population against the log-weight maximum lw_max of all shards (include/smcnuts_hip.h)."""
        out, cen = np.empty((Dc + 1, Dc + 1)), np.empty(Dc)
        c = None if centre is None else np.ascontiguousarray(centre, dtype=np.float64)
        if c is not None and c.shape != (Dc,):
            raise ValueError(f"centre must hold {Dc} values")
        self.call("smcn_cov_partials", float(lw_max), dptr(c), int(slices), dptr(out), dptr(cen))
        return out, cen

    def cov_centre(self, lw_max, Dc):
        """The staged shard's own weighted mean [Dc] (zeros where it has no weight): the centre kernel alone."""
        cen = np.empty(Dc)
        self.call("smcn_cov_partials", float(lw_max), None, 0, None, dptr(cen))
        return cen

    def cov_last_ms(self):
        """Device time of the last cov_partials' kernels (HIP events on the context's stream)."""
        return self._last_ms("smcn_cov_last_ms")

    # ---- step-size probe (every device-native model) -----------------------------------
    def stepsize_probe(self, ladder, x=None, logw=None, r=None, n_leapfrog=8, phi=1.0, delta_max=100.0, seed=0,
                       max_particles=4096, want_particles=False):
        """(partials [1 + L][4], accept [L][Mp], first_bad [L][Mp]) of one pass over `ladder` (include/smcnuts_hip.h); the
        last two None unless want_particles.  x=None: the resident particles and weights.  r [Mp][D]: the momenta of
        the probed particles (None: Philox under `seed`)."""
        lad = np.ascontiguousarray(ladder, dtype=np.float64).reshape(-1)
        if x is None:
            if logw is not None:
                raise ValueError("the resident particles come with their resident log-weights (x=None: logw=None)")
        else:
            x = np.ascontiguousarray(np.atleast_2d(x), dtype=np.float64)
            if x.shape[1] != self.D:
                raise ValueError(f"x must hold {self.D} coordinates per row")
        xp, lp_, M = self._particles(x, logw)
        Mp = min(M, int(max_particles))
        if r is not None:
            r = np.ascontiguousarray(r, dtype=np.float64)
            if r.shape != (Mp, self.D):
                raise ValueError(f"r must hold the momenta of the {Mp} probed particles, [{Mp}][{self.D}]")
        part = np.empty((1 + lad.size, 4))
        acc = np.empty((lad.size, Mp)) if want_particles else None
        fb = np.empty((lad.size, Mp), dtype=np.int32) if want_particles else None
        self.call("smcn_stepsize_probe", xp, lp_, M, dptr(r), dptr(lad), lad.size, int(n_leapfrog), float(phi),
                  float(delta_max), C.c_uint64(int(seed) & (2 ** 64 - 1)), int(max_particles), dptr(part), dptr(acc),
                  iptr(fb))
        return part, acc, fb

    def stepsize_last_ms(self):
        """Device time of the last stepsize_probe's kernels (HIP events on the context's stream)."""
        return float(self._lib.smcn_stepsize_last_ms(self._h))

    # ---- forecasts (SMCN_MODEL_ARMA; include/smcnuts_hip.h, smcn_forecast_*) --------------
    def forecast_set(self, horizon, y_future=None, at=None):
        """The horizon H, the held-out continuation [H] (or None) and the thresholds [H][Tn] (or None)."""
        yf = None if y_future is None else np.ascontiguousarray(y_future, dtype=np.float64)
        a = None if at is None else np.ascontiguousarray(at, dtype=np.float64)
        if yf is not None and yf.shape != (int(horizon),):
            raise ValueError("y_future must hold one value per horizon")
        if a is not None and (a.ndim != 2 or a.shape[0] != int(horizon)):
            raise ValueError("at must be [H][Tn]")
        Tn = 0 if a is None else a.shape[1]
        self.call("smcn_forecast_set", int(horizon), dptr(yf), dptr(a) if Tn else None, Tn)

    def forecast_dims(self):
        H, q, hy, tn = C.c_int64(0), C.c_int(0), C.c_int(0), C.c_int(0)
        self.call("smcn_forecast_dims", C.byref(H), C.byref(q), C.byref(hy), C.byref(tn))
        return H.value, q.value, bool(hy.value), tn.value

    def forecast_slices(self, M):
        """The particle slices a forecast_partials call over M particles is merged from."""
        n = C.c_int64(0)
        self.call("smcn_forecast_slices", int(M), C.byref(n))
        return n.value

    def forecast_points(self, x):
        """[M][1 + 2H (+ 2H)]: err_T, m_1..m_H, v_1..v_H and, with y_future, the marginal and the cumulative joint terms."""
        x = np.ascontiguousarray(np.atleast_2d(x), dtype=np.float64)
        H, _, hy, _ = self.forecast_dims()
        out = np.empty((x.shape[0], 1 + (4 if hy else 2) * H))
        self.call("smcn_forecast_points", dptr(x), x.shape[0], dptr(out))
        return out

    def forecast_partials(self, x=None, logw=None):
        """[1 + H][Q] mergeable partials (include/smcnuts_hip.h); x=None: the resident particles and weights."""
        H, q, _, _ = self.forecast_dims()
        out = np.empty((1 + H, q))
        self.call("smcn_forecast_partials", *self._particles(x, logw), dptr(out))
        return out

    def forecast_draws(self, S, seed, x=None, logw=None, ancestors=None, s_first=0, s_count=None):
        """(y [s_count][H], ancestors [s_count], n_bad): simulated paths of the slots s_first .. of S over the horizon of
        the last forecast_set (include/smcnuts_hip.h); x=None: the resident particles and weights."""
        return self._draws("smcn_forecast_draws", self.forecast_dims()[0], "path", S, seed, x, logw, ancestors, s_first,
                           s_count)

    def forecast_last_ms(self):
        """Device time [partials, draws] of the last forecast calls' kernels (HIP events on the context's stream)."""
        return self._last_ms("smcn_forecast_last_ms", 2)

    # ---- one-step residual checks (SMCN_MODEL_ARMA; include/smcnuts_hip.h, smcn_residuals_*) --------------
    def residuals_set(self, lags, q_at=None):
        """The number of lags L and the thresholds [Tn] of the Ljung-Box statistic (or None)."""
        q = None if q_at is None else np.ascontiguousarray(q_at, dtype=np.float64).reshape(-1)
        Tn = 0 if q is None else q.size
        self.call("smcn_residuals_set", int(lags), dptr(q) if Tn else None, Tn)

    def residuals_dims(self):
        T, L, q, tn = C.c_int64(0), C.c_int(0), C.c_int(0), C.c_int(0)
        self.call("smcn_residuals_dims", C.byref(T), C.byref(L), C.byref(q), C.byref(tn))
        return T.value, L.value, q.value, tn.value

    def residuals_points(self, x):
        """[M][2T (+ L + 1)]: nu_1..nu_T, r_1..r_T and, with lags, rho_1..rho_L and Q."""
        x = np.ascontiguousarray(np.atleast_2d(x), dtype=np.float64)
        T, L, _, _ = self.residuals_dims()
        out = np.empty((x.shape[0], 2 * T + (L + 1 if L else 0)))
        self.call("smcn_residuals_points", dptr(x), x.shape[0], dptr(out))
        return out

    def residuals_partials(self, x=None, logw=None):
        """[1 + T (+ L + 1)][Qc] mergeable partials (include/smcnuts_hip.h); x=None: the resident particles and weights."""
        T, L, q, _ = self.residuals_dims()
        out = np.empty((1 + T + (L + 1 if L else 0), q))
        self.call("smcn_residuals_partials", *self._particles(x, logw), dptr(out))
        return out

    def residuals_last_ms(self):
        """Device time of the last residuals_partials call's kernels (HIP events on the context's stream)."""
        return self._last_ms("smcn_residuals_last_ms")

    def timers(self, reset=False):
        t = np.zeros(6)
        self.call("smcn_timers", dptr(t), int(bool(reset)))
        return t
