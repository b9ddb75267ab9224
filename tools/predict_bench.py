"""Held-out prediction (smcn_predict_partials) on one MI355X: one JSON line per case, also appended to
profiles/predict_bench.jsonl.

    python tools/predict_bench.py [--N 65536] [--reps 9] [--numpy-m 1000] [--only SUBSTR] [--out profiles/predict_bench.jsonl]

GPU only; run every invocation under `timeout`.  Cases: the (n, D) cases of tools/pointwise_bench.py with the new rows
m = n (bernoulli_logit at (100, 8), (1 000, 16), (1 000, 17), (1 000, 25), (10 000, 64); the three other families at
(1 000, 25)), and at m = 1 000: hierarchical (poisson_log, Dc = 9, J = 40), categorical K = 5 (Dc = 8) and K = 16
(Dc = 4), ordinal K = 7 (p = 10).  N resident particles drawn 0.3 N(0, 1) with log-weights 3 N(0, 1); the context's
training data are the same rows, so that (a) and the pointwise pass work on the rows the predict pass works on.  Per case,
after two warm-up calls, the median and the min / max of --reps calls:
  predict_ms     smcn_predict_partials on the resident state: its kernels between two HIP events on the context's stream
                 (smcn_predict_last_ms); predict_wall_ms the whole call (wait and download of [1 + m][Q] included)
  pointwise_ms   smcn_pointwise_partials on the same context with the SAME rows as its training data (GLM families
                 only): the same walk with other accumulators; predict_over_pointwise is the ratio of the kernel times
  eval_ms        (a) smcn_eval_proposed_parts: one batched density evaluation (value and gradient) of the same particles
                 on a context whose training data are the same rows, wall time of the call
  numpy_s        the chunked NumPy reference of the tests (terms + reference on chunks of 64 rows, 8 for the class
                 models), for m <= --numpy-m
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

GLM_CASES = [("bernoulli_logit", 100, 8), ("bernoulli_logit", 1000, 16), ("bernoulli_logit", 1000, 17),
             ("bernoulli_logit", 1000, 25), ("bernoulli_logit", 10000, 64), ("poisson_log", 1000, 25), ("normal", 1000, 25),
             ("neg_binomial_2_log", 1000, 25)]


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


def cases():
    """(name, target on the rows themselves, NumPy model class and arguments for a slice of rows, rows)"""
    import _cat
    import _glm
    import _glm_disp
    import _hglm
    import _ord
    from smcnuts_amd import CategoricalRegression, GLMTarget, HierarchicalGLM, OrdinalRegression
    for family, m, D in GLM_CASES:
        if family in _glm_disp.DISP_FAMILIES:
            X, y = _glm_disp.synthetic(family, m, D - 2, 1000 + D, scale=0.5)
            yield (f"{family}_m{m}_D{D}", GLMTarget(X, y, family=family, prior_sd=2.0, dispersion_prior=(0.0, 2.5)),
                   lambda sl, X=X, y=y, f=family: _glm_disp.GLMDispNumpy(X[sl], y[sl], f, 2.0, (0.0, 2.5)), (X, y, None), True)
        else:
            X, y = _glm.synthetic(family, m, D - 1, 1000 + D, scale=0.5)
            yield (f"{family}_m{m}_D{D}", GLMTarget(X, y, family=family, prior_sd=2.0),
                   lambda sl, X=X, y=y, f=family: _glm.GLMNumpy(X[sl], y[sl], f, 2.0), (X, y, None), True)
    X, y, g = _hglm.synthetic("poisson_log", 1000, 8, 40, 7)
    yield ("hier_poisson_m1000_Dc9_J40", HierarchicalGLM(X, y, g, family="poisson_log", n_groups=40),
           lambda sl: _hglm.HGLMNumpy(X[sl], y[sl], g[sl], "poisson_log", n_groups=40), (X, y, g), False)
    for K, p in ((5, 7), (16, 3)):
        Xc, yc = _cat.synthetic(K, 1000, p, 8)
        yield (f"cat_m1000_K{K}_Dc{p + 1}", CategoricalRegression(Xc, yc, n_classes=K),
               lambda sl, Xc=Xc, yc=yc, K=K: _cat.CategoricalNumpy(Xc[sl], yc[sl], K), (Xc, yc, None), False)
    Xo, yo = _ord.synthetic(7, 1000, 10, 9)
    yield ("ord_m1000_K7_p10", OrdinalRegression(Xo, yo, n_classes=7),
           lambda sl: _ord.OrdinalNumpy(Xo[sl], yo[sl], 7), (Xo, yo, None), False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--numpy-m", type=int, default=1000)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predict_bench.jsonl"))
    a = ap.parse_args()
    import _predict as pr
    from smcnuts_amd import _capi
    out = open(a.out, "a")
    for name, t, model_of, (X, y, g), glm in cases():
        if a.only not in name:
            continue
        m = X.shape[0]
        rng = np.random.default_rng(m + t.dim)
        x = 0.3 * rng.standard_normal((a.N, t.dim))
        lw = 3.0 * rng.standard_normal(a.N)
        ctx = _capi.Context(a.N, t.model_id, t.model_data)
        ctx.set_state(x=x, logw=lw)
        block, has_y = t._predict_block(X, y, g)
        ctx.predict_set_data(block, has_y)
        ev, wall, ea, pwm = [], [], [], []
        for r in range(a.reps + 2):
            t0 = time.perf_counter()
            ctx.predict_partials()
            w = time.perf_counter() - t0
            ms = ctx.predict_last_ms()
            t0 = time.perf_counter()
            ctx.call("smcn_eval_proposed_parts", 0)
            e = time.perf_counter() - t0
            if glm:
                ctx.pointwise_partials()
            if r >= 2:
                ev.append(ms)
                wall.append(w * 1e3)
                ea.append(e * 1e3)
                if glm:
                    pwm.append(ctx.pointwise_last_ms())
        rec = dict(case=name, m=m, D=t.dim, N=a.N, reps=a.reps, predict_ms=stats(ev), predict_wall_ms=stats(wall),
                   eval_ms=stats(ea))
        if glm:
            rec["pointwise_ms"] = stats(pwm)
            rec["predict_over_pointwise"] = rec["predict_ms"]["median"] / rec["pointwise_ms"]["median"]
        rec["predict_over_eval"] = rec["predict_ms"]["median"] / rec["eval_ms"]["median"]
        rec["pairs_per_s"] = a.N * m / (rec["predict_ms"]["median"] * 1e-3)
        if m <= a.numpy_m:
            t0 = time.perf_counter()
            step = 64 if glm else 8                      # (the class models hold [N][rows][K] arrays)
            for i0 in range(0, m, step):
                T = pr.terms(model_of(slice(i0, min(m, i0 + step))), x)
                pr.reference(T, lw)
            rec["numpy_s"] = time.perf_counter() - t0
        ctx.close()
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()


if __name__ == "__main__":
    main()
