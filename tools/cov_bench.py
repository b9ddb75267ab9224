"""Posterior covariance (smcn_cov_partials, fp64 MFMA) on one MI355X: one JSON line per case, also appended to
profiles/cov_bench.jsonl.

    python tools/cov_bench.py [--reps 9] [--host-reps 2] [--out profiles/cov_bench.jsonl]

GPU only; run every invocation under `timeout`.  Cases: logistic-regression contexts with Dc in {8, 25, 64} at N = 65 536,
Dc = 64 at N = 262 144, a Gaussian with D = 256 at N = 131 072 and a wide logistic regression with D = 200 at N = 65 536.
The resident particles are loc_c + 0.3 N(0, 1) with loc spread over [-2, 2], half the rows duplicated, log-weights
3 N(0, 1) (tools/summary_bench.py's population).  Per case, after two warm-up calls, the median and min / max of --reps
calls:
  device_ms   the kernels of smcn_cov_partials between HIP events on the context's stream (weights, partials, the two
              combine stages; smcn_cov_last_ms); begin_ms the staging of smcn_summary_begin before it
              (smcn_summary_last_ms); wall_ms the whole covariance.device_covariance call (staging, waits, the download of
              [Dc+1][Dc+1] doubles and the finish on the host included)
  image_GBs   8 N Dc bytes, one read of the staged image, over device_ms, beside copy_GBs, the streaming copy rate
              smcn_measure_peaks reports in this run (the small-Dc cases are a read of the image)
  mfma_share  2 Dp^2 N flop (Dp: Dc + 1 rounded up to 16 -- the whole square, of which the kernel forms the upper
              triangle's tiles) over 78.6 TF, over device_ms
  host_ms     what a user does without this call, on the same population in the same run: get_state (download of x and
              logw), target.constrain, np.cov(aweights=) (--host-reps runs); max_rel the largest |device - host| entry
              over sqrt(C_ii C_jj)
csrc_sha stamps the kernel sources the numbers belong to (bench.py's hash)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = [("logistic", 65536, 8), ("logistic", 65536, 25), ("logistic", 65536, 64), ("logistic", 262144, 64),
         ("gaussian", 131072, 256), ("wide_logistic", 65536, 200)]
PEAK_F64_MATRIX = 78.6e12


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--slices", type=int, default=0)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cov_bench.jsonl"))
    a = ap.parse_args()
    import _glm
    from bench import csrc_hash
    from smcnuts_amd import GaussianTarget, LogisticRegression, WideGLMTarget, _capi
    from smcnuts_amd import covariance as cv
    out = open(a.out, "a")
    copy_gbs = None
    for kind, N, D in CASES:
        if kind == "gaussian":
            t = GaussianTarget(D)
        else:
            X, y = _glm.synthetic("bernoulli_logit", 200, D - 1, 1000 + D, scale=0.5)
            t = (WideGLMTarget if kind == "wide_logistic" else LogisticRegression)(X, y)
        rng = np.random.default_rng(N + D)
        x = np.linspace(-2.0, 2.0, D)[None, :] + 0.3 * rng.standard_normal((N, D))
        x[rng.permutation(N)[:N // 2]] = x[rng.integers(0, N, N // 2)]
        lw = 3.0 * rng.standard_normal(N)
        ctx = _capi.Context(N, t.model_id, t.model_data)
        ctx.set_state(x=x, logw=lw)
        if copy_gbs is None:
            pk = (C.c_double * 3)()
            ctx.call("smcn_measure_peaks", pk)
            copy_gbs = float(pk[0])
        host, want = [], None
        for r in range(a.host_reps):
            t0 = time.perf_counter()
            xs, lws, _ = ctx.get_state()
            v = t.constrain(xs)
            want = np.atleast_2d(np.cov(v, rowvar=False, ddof=0, aweights=np.exp(lws - lws.max())))
            host.append((time.perf_counter() - t0) * 1e3)
        ev, begin, wall = [], [], []
        for r in range(a.reps + 2):
            t0 = time.perf_counter()
            mean, cov, corr, ess, _ = cv.device_covariance(ctx, None, slices=a.slices)
            wl = (time.perf_counter() - t0) * 1e3
            if r >= 2:
                ev.append(ctx.cov_last_ms())
                begin.append(ctx.summary_last_ms())
                wall.append(wl)
        _, Dc, rule, cap = ctx.cov_dims()
        Dp = (Dc + 1 + 15) // 16 * 16
        sd = np.sqrt(np.diagonal(want))
        rec = dict(case=f"{kind}_N{N}_D{D}", label=a.label, kind=kind, N=N, D=D, Dc=Dc, Dp=Dp, reps=a.reps,
                   slices=int(a.slices or rule), slice_cap=cap, device_ms=stats(ev), begin_ms=stats(begin),
                   wall_ms=stats(wall), host_ms=stats(host), copy_GBs=copy_gbs, ess=float(ess),
                   max_rel=float(np.max(np.abs(cov - want) / np.outer(sd, sd))), csrc_sha=csrc_hash())
        dev_s = rec["device_ms"]["median"] * 1e-3
        rec["image_GBs"] = 8.0 * N * Dc / dev_s / 1e9
        rec["mfma_share"] = 2.0 * Dp * Dp * N / PEAK_F64_MATRIX / dev_s
        rec["host_over_wall"] = rec["host_ms"]["median"] / rec["wall_ms"]["median"]
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()
        ctx.close()


if __name__ == "__main__":
    main()
