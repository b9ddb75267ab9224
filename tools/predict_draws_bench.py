"""Posterior predictive draws (smcn_predict_draws) on one MI355X: one JSON line per case, also appended to
profiles/predict_draws_bench.jsonl.

    python tools/predict_draws_bench.py [--N 65536] [--S 1000] [--reps 9] [--only SUBSTR] [--out profiles/predict_draws_bench.jsonl]

GPU only; run every invocation under `timeout`.  Cases: those of tools/predict_bench.py (the rows are the context's
training rows).  N resident particles drawn 0.3 N(0, 1) with log-weights 3 N(0, 1), S draws.  At that scale every mean of
the count families is below 10 (inversion only), so each of them is timed a second time, `_wide`, with the particles
drawn 2.4 N(0, 1): mu then spans the inversion and the PTRS branch.  Per case, after two warm-up
calls, the median and the min / max of --reps calls:
  draws_ms        smcn_predict_draws on the resident state: its kernels (header, weights, scan, ancestors, gather, the
                  model's draw kernel and, in the two-pass form, the sampling kernel) between two HIP events on the
                  context's stream (smcn_predict_draws_last_ms); draws_wall_ms the whole call (wait and download of
                  [S][m] included)
  loglik_wall_ms  the yardstick: smcn_predict_loglik on the SAME S gathered particles and the same rows -- the same walk,
                  a matrix of the same size written and downloaded -- wall time of the call (it has no event timer; the
                  upload of the S particles is in it); draws_over_loglik is the ratio of the two wall times
  attempts        the rejection samplers' mean attempts per draw (Poisson from mu = 10, NB2: gamma and Poisson), from the
                  NumPy restatement of tests/_predict_draws.py on the first 64 rows of the first 32 draws
  n_bad           NaN draws of the last call
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
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=65536)
    ap.add_argument("--S", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predict_draws_bench.jsonl"))
    a = ap.parse_args()
    import _predict as pr
    import _predict_draws as dr
    from predict_bench import cases, stats
    from smcnuts_amd import _capi
    out = open(a.out, "a")
    variants = []
    for c in cases():
        variants.append(c + (0.3,))
        if getattr(c[1], "family", "") in ("poisson_log", "neg_binomial_2_log"):
            variants.append((c[0] + "_wide",) + c[1:] + (2.4,))
    for name, t, model_of, (X, y, g), glm, scale in variants:
        if a.only not in name:
            continue
        m = X.shape[0]
        rng = np.random.default_rng(m + t.dim)
        x = scale * rng.standard_normal((a.N, t.dim))
        lw = 3.0 * rng.standard_normal(a.N)
        ctx = _capi.Context(a.N, t.model_id, t.model_data)
        ctx.set_state(x=x, logw=lw)
        block, has_y = t._predict_block(X, y, g)
        ctx.predict_set_data(block, has_y)
        ev, wall, yard = [], [], []
        for r in range(a.reps + 2):
            t0 = time.perf_counter()
            yv, anc, nbad = ctx.predict_draws(a.S, 7)
            w = time.perf_counter() - t0
            ms = ctx.predict_draws_last_ms()
            xa = x[anc]
            t0 = time.perf_counter()
            ctx.predict_loglik(xa)
            yw = time.perf_counter() - t0
            if r >= 2:
                ev.append(ms)
                wall.append(w * 1e3)
                yard.append(yw * 1e3)
        rec = dict(case=name, m=m, D=t.dim, N=a.N, S=a.S, reps=a.reps, x_scale=scale, draws_ms=stats(ev), draws_wall_ms=stats(wall),
                   loglik_wall_ms=stats(yard), n_bad=int(nbad))
        rec["draws_over_loglik"] = rec["draws_wall_ms"]["median"] / rec["loglik_wall_ms"]["median"]
        rec["draws_per_s"] = a.S * m / (rec["draws_ms"]["median"] * 1e-3)
        fam = getattr(t, "family", "")
        if fam in ("poisson_log", "neg_binomial_2_log"):
            sl = slice(0, min(m, 64))
            mean = pr.terms(model_of(sl), x[anc[:32]])["mean"]
            s, i = np.broadcast_arrays(np.arange(mean.shape[0])[:, None], np.arange(mean.shape[1])[None, :])
            if fam == "poisson_log":
                _, _, att = dr.poisson(mean, 0.0, 7, s, i)
                rec["attempts"] = dict(poisson=float(np.nanmean(np.where(att > 0, att, np.nan))), poisson_max=float(att.max()),
                                       share_ptrs=float(np.mean(mean >= 10.0)))
            else:
                phi = np.broadcast_to(np.exp(x[anc[:32], -1:]), mean.shape)
                _, _, (ng, npo) = dr.nb2(mean, 0.0, phi, 0.0, 7, s, i)
                rec["attempts"] = dict(gamma=float(ng.mean()), gamma_max=float(ng.max()), poisson=float(npo.mean()),
                                       poisson_max=float(npo.max()))
        ctx.close()
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()


if __name__ == "__main__":
    main()
