"""Calibration partials (smcn_calibration_partials) beside the pointwise criteria (smcn_pointwise_partials) on one
MI355X: one JSON line per case, also appended to profiles/calibration_bench.jsonl.

    python tools/calibration_bench.py [--N 65536] [--reps 9] [--out profiles/calibration_bench.jsonl]

GPU only; run every invocation under `timeout`.  Cases: the four families at (n, D) = (1 000, 25) (D counts tau), and
poisson_log at (100, 8) and (1 000, 17), with tools/pointwise_bench.py's data, N resident particles drawn 0.3 N(0, 1) and
log-weights 3 N(0, 1).  Per case, after two warm-up calls, the median and the min / max of --reps calls of either entry
point on the resident state: its kernels between two HIP events on the context's stream (smcn_calibration_last_ms,
smcn_pointwise_last_ms).  calibration_over_pointwise is the ratio of the medians; pairs_per_s the (particle, observation)
pairs of the calibration call per second.  For the record: no ratio is required of it.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = [("bernoulli_logit", 1000, 25), ("poisson_log", 1000, 25), ("normal", 1000, 25), ("neg_binomial_2_log", 1000, 25),
         ("poisson_log", 100, 8), ("poisson_log", 1000, 17)]


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "calibration_bench.jsonl"))
    a = ap.parse_args()
    import _glm
    import _glm_disp
    from smcnuts_amd import GLMTarget, _capi
    from smcnuts_amd.calibration import combine_calibration_partials
    out = open(a.out, "a")
    for family, n, D in CASES:
        if family in _glm_disp.DISP_FAMILIES:
            X, y = _glm_disp.synthetic(family, n, D - 2, 1000 + D, scale=0.5)
            t = GLMTarget(X, y, family=family, prior_sd=2.0, dispersion_prior=(0.0, 2.5))
        else:
            X, y = _glm.synthetic(family, n, D - 1, 1000 + D, scale=0.5)
            t = GLMTarget(X, y, family=family, prior_sd=2.0)
        rng = np.random.default_rng(D + n)
        x = 0.3 * rng.standard_normal((a.N, D))
        lw = 3.0 * rng.standard_normal(a.N)
        ctx = _capi.Context(a.N, t.model_id, t.model_data)
        ctx.set_state(x=x, logw=lw)
        cal, pw = [], []
        for r in range(a.reps + 2):
            part = ctx.calibration_partials()
            c = ctx.calibration_last_ms()
            ctx.pointwise_partials()
            p = ctx.pointwise_last_ms()
            if r >= 2:
                cal.append(c)
                pw.append(p)
        res = combine_calibration_partials([part])
        rec = dict(case=f"{family}_n{n}_D{D}", family=family, n=n, D=D, N=a.N, reps=a.reps, calibration_ms=stats(cal),
                   pointwise_ms=stats(pw), max_y=float(np.max(y)), n_unconverged=float(np.sum(res.n_unconverged)),
                   n_nan_rows=int(np.sum(np.isnan(res.pit_lo))))
        rec["calibration_over_pointwise"] = rec["calibration_ms"]["median"] / rec["pointwise_ms"]["median"]
        rec["pairs_per_s"] = a.N * n / (rec["calibration_ms"]["median"] * 1e-3)
        ctx.close()
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()


if __name__ == "__main__":
    main()
