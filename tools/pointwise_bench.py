"""Pointwise criteria (smcn_pointwise_partials) on one MI355X: one JSON line per case, also appended to
profiles/pointwise_bench.jsonl.

    python tools/pointwise_bench.py [--N 65536] [--reps 9] [--slice 2048] [--numpy-n 1000] [--out profiles/pointwise_bench.jsonl]

GPU only; run every invocation under `timeout`.  Cases: bernoulli_logit with (n, D) in {(100, 8), (1 000, 16), (1 000, 17),
(1 000, 25), (10 000, 64)} and the three other families at (1 000, 25) (D counts tau), N resident particles drawn
0.3 N(0, 1) with log-weights 3 N(0, 1).  Per case, after two warm-up calls, the median and the min / max of --reps calls:
  stats_ms      smcn_pointwise_partials on the resident state: its kernels between two HIP events on the context's
                stream (smcn_pointwise_last_ms); stats_wall_ms the whole call (wait and download of [1 + n][Q] included)
  eval_ms       (a) smcn_eval_proposed_parts: one batched density evaluation (value and gradient) of the same particles
                with the existing kernels, wall time of the call (it waits for the stream)
  loglik_ms     (b) pointwise_loglik of --slice particles (upload and the download of the matrix included), and
                loglik_scaled_ms = loglik_ms N / slice: what materialising the matrix would cost
  numpy_s       (c) the chunked NumPy reference (criteria_reference on chunks of 64 observations), for n <= --numpy-n
stats_over_eval sets the kernels' time against (a)'s wall time; stats_wall_over_eval sets wall time against wall time.
Also terms / s, and the share of 2 n D N flop (eta alone) against the 78.6 TF fp64 peak the other tools use.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK_FP64 = 78.6e12
CASES = [("bernoulli_logit", 100, 8), ("bernoulli_logit", 1000, 16), ("bernoulli_logit", 1000, 17),
         ("bernoulli_logit", 1000, 25), ("bernoulli_logit", 10000, 64), ("poisson_log", 1000, 25), ("normal", 1000, 25),
         ("neg_binomial_2_log", 1000, 25)]


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--slice", type=int, default=2048)
    ap.add_argument("--numpy-n", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pointwise_bench.jsonl"))
    a = ap.parse_args()
    import _glm
    import _glm_disp
    import _pointwise as pw
    from smcnuts_amd import GLMTarget, _capi
    out = open(a.out, "a")
    for family, n, D in CASES:
        disp = family in _glm_disp.DISP_FAMILIES
        if disp:
            X, y = _glm_disp.synthetic(family, n, D - 2, 1000 + D, scale=0.5)
            t = GLMTarget(X, y, family=family, prior_sd=2.0, dispersion_prior=(0.0, 2.5))
            model = _glm_disp.GLMDispNumpy(X, y, family, 2.0, (0.0, 2.5))
        else:
            X, y = _glm.synthetic(family, n, D - 1, 1000 + D, scale=0.5)
            t = GLMTarget(X, y, family=family, prior_sd=2.0)
            model = _glm.GLMNumpy(X, y, family, 2.0)
        rng = np.random.default_rng(D + n)
        x = 0.3 * rng.standard_normal((a.N, D))
        lw = 3.0 * rng.standard_normal(a.N)
        ctx = _capi.Context(a.N, t.model_id, t.model_data)
        ctx.set_state(x=x, logw=lw)
        ev, wall, ea = [], [], []
        for r in range(a.reps + 2):
            t0 = time.perf_counter()
            part = ctx.pointwise_partials()
            w = time.perf_counter() - t0
            ms = ctx.pointwise_last_ms()
            t0 = time.perf_counter()
            ctx.call("smcn_eval_proposed_parts", 0)
            e = time.perf_counter() - t0
            if r >= 2:
                ev.append(ms)
                wall.append(w * 1e3)
                ea.append(e * 1e3)
        M = min(a.slice, a.N)
        lk = []
        for r in range(5):
            t0 = time.perf_counter()
            ctx.pointwise_loglik(x[:M])
            if r >= 2:
                lk.append((time.perf_counter() - t0) * 1e3)
        rec = dict(case=f"{family}_n{n}_D{D}", family=family, n=n, D=D, N=a.N, reps=a.reps, stats_ms=stats(ev),
                   stats_wall_ms=stats(wall), eval_ms=stats(ea), loglik_slice=M, loglik_ms=stats(lk))
        rec["loglik_scaled_ms"] = rec["loglik_ms"]["median"] * a.N / M
        rec["stats_over_eval"] = rec["stats_ms"]["median"] / rec["eval_ms"]["median"]
        rec["stats_wall_over_eval"] = rec["stats_wall_ms"]["median"] / rec["eval_ms"]["median"]     # (wall against wall)
        rec["terms_per_s"] = a.N * n / (rec["stats_ms"]["median"] * 1e-3)
        rec["fp64_fraction_of_peak"] = 2.0 * n * D * a.N / (rec["stats_ms"]["median"] * 1e-3) / PEAK_FP64
        if n <= a.numpy_n:
            t0 = time.perf_counter()
            for i0 in range(0, n, 64):
                sl = slice(i0, min(n, i0 + 64))
                sub = type(model)(X[sl], y[sl], family, 2.0, (0.0, 2.5)) if disp else type(model)(X[sl], y[sl], family, 2.0)
                ll, _, mean, _ = pw.terms(sub, x)
                pw.criteria_reference(ll, lw, mean)
            rec["numpy_s"] = time.perf_counter() - t0
        ctx.close()
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()


if __name__ == "__main__":
    main()
