"""Pareto-smoothed LOO (smcn_psis_loo) on one MI355X: one JSON line per case, also appended to profiles/psis_bench.jsonl.

    python tools/psis_bench.py [--N 65536] [--reps 9] [--cases 0,1,..] [--out profiles/psis_bench.jsonl]

GPU only; run every invocation under `timeout`.  Cases: those of tools/pointwise_bench.py -- bernoulli_logit with (n, D) in
{(100, 8), (1 000, 16), (1 000, 17), (1 000, 25), (10 000, 64)} and the three other families at (1 000, 25) (D counts tau),
N resident particles drawn 0.3 N(0, 1) with log-weights 3 N(0, 1).  Per case, after two warm-up calls, the median and the
min / max of --reps calls:
  candidates_ms, body_ms, fit_ms, psis_ms   the stages of smcn_psis_loo on the resident state and the whole of it, between
                HIP events on the context's stream (smcn_psis_last_ms); psis_wall_ms the whole call (wait and download of
                [n][6] included)
  stats_ms      smcn_pointwise_partials on the same state (smcn_pointwise_last_ms) and stats_wall_ms its call: plain IS-LOO,
                the number this library had before
psis_over_stats sets the kernels' times against each other, psis_wall_over_stats_wall the calls.
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
    ap.add_argument("--cases", default=",".join(str(i) for i in range(len(CASES))))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "psis_bench.jsonl"))
    a = ap.parse_args()
    import _glm
    import _glm_disp
    from smcnuts_amd import GLMTarget, _capi
    out = open(a.out, "a")
    for family, n, D in [CASES[int(i)] for i in a.cases.split(",")]:
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
        stage, wall, pev, pwall = [], [], [], []
        for r in range(a.reps + 2):
            t0 = time.perf_counter()
            res, _ = ctx.psis_loo()
            w = time.perf_counter() - t0
            ms = ctx.psis_last_ms()
            t0 = time.perf_counter()
            ctx.pointwise_partials()
            pw_ = time.perf_counter() - t0
            if r >= 2:
                stage.append(ms)
                wall.append(w * 1e3)
                pev.append(ctx.pointwise_last_ms())
                pwall.append(pw_ * 1e3)
        stage = np.array(stage)
        rec = dict(case=f"{family}_n{n}_D{D}", family=family, n=n, D=D, N=a.N, reps=a.reps,
                   candidates_ms=stats(stage[:, 0]), body_ms=stats(stage[:, 1]), fit_ms=stats(stage[:, 2]),
                   psis_ms=stats(stage[:, 3]), psis_wall_ms=stats(wall), stats_ms=stats(pev), stats_wall_ms=stats(pwall),
                   tail_len=int(res[0, 3]), max_pareto_k=float(np.max(res[:, 0])),
                   n_high_k=int(np.sum(~(res[:, 0] <= 0.7))))
        rec["psis_over_stats"] = rec["psis_ms"]["median"] / rec["stats_ms"]["median"]
        rec["psis_wall_over_stats_wall"] = rec["psis_wall_ms"]["median"] / rec["stats_wall_ms"]["median"]
        ctx.close()
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()


if __name__ == "__main__":
    main()
