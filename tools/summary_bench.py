"""Posterior summaries (smcn_summary_*) on one MI355X: one JSON line per case, also appended to
profiles/summary_bench.jsonl.

    python tools/summary_bench.py [--reps 9] [--host-reps 2] [--out profiles/summary_bench.jsonl]

GPU only; run every invocation under `timeout`.  Cases: logistic-regression contexts with Dc in {8, 25, 64} at N = 65 536,
Dc = 64 at N = 262 144, and a Gaussian with D = 256 at N = 131 072; 5 and 16 probabilities each.  The resident particles are
loc_c + 0.3 N(0, 1) with loc spread over [-2, 2] (so the columns differ in sign and binade), half the rows duplicated,
log-weights 3 N(0, 1).  Per case, after two warm-up calls, the median and min / max of --reps calls:
  device_ms   the summary's kernels between HIP events on the context's stream (smcn_summary_last_ms: staging, header,
              fixed-point weights, the eight passes); wall_ms the whole summary.device_summary call (waits and the
              download of [Dc][nq] doubles included)
  pass_ms     each of the eight passes (histogram, memset and pick; smcn_summary_pass_ms), and pass_GBs: the bytes a pass
              reads (8 B per value, 8 B per particle for the weight) over its time, beside copy_GBs, the streaming copy
              rate smcn_measure_peaks reports in this run (what bench.py prints as roofline.peak_measured.copy_GBs)
  host_ms     what a user does without this call, on the same population in the same run: get_state (download of x and
              logw), target.constrain, np.quantile(..., method="inverted_cdf", weights=...) per column (--host-reps runs)
  mismatches  how many of the Dc * nq quantiles differ from that NumPy result (NumPy forms its cumulative weights in
              doubles: a difference needs a near-tie in mass)
csrc_sha stamps the kernel sources the numbers belong to (bench.py's hash).
"""
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
         ("gaussian", 131072, 256)]
P5 = (0.025, 0.25, 0.5, 0.75, 0.975)
P16 = tuple(np.linspace(0.02, 0.98, 16))


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "summary_bench.jsonl"))
    a = ap.parse_args()
    import _glm
    from bench import csrc_hash
    from smcnuts_amd import GaussianTarget, LogisticRegression, _capi
    from smcnuts_amd import summary as sm
    out = open(a.out, "a")
    copy_gbs = None
    for kind, N, D in CASES:
        if kind == "logistic":
            X, y = _glm.synthetic("bernoulli_logit", 200, D - 1, 1000 + D, scale=0.5)
            t = LogisticRegression(X, y)
        else:
            t = GaussianTarget(D)
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
            w = np.exp(lws - lws.max())
            want = {nq: np.stack([np.quantile(v[:, c], p, method="inverted_cdf", weights=w) for c in range(D)])
                    for nq, p in ((5, P5),)}
            host.append((time.perf_counter() - t0) * 1e3)
        for probs in (P5, P16):
            p = np.asarray(probs)
            ev, wall, passes = [], [], []
            for r in range(a.reps + 2):
                t0 = time.perf_counter()
                q, _, ess = sm.device_summary(ctx, None, p, None)
                wl = (time.perf_counter() - t0) * 1e3
                if r >= 2:
                    ev.append(ctx.summary_last_ms())
                    wall.append(wl)
                    passes.append(ctx.summary_pass_ms())
            pm = np.median(np.array(passes), axis=0)
            pass_bytes = 8.0 * N * D + 8.0 * N
            rec = dict(case=f"{kind}_N{N}_D{D}_q{len(probs)}", kind=kind, N=N, D=D, nq=len(probs), reps=a.reps,
                       device_ms=stats(ev), wall_ms=stats(wall), pass_ms=[float(v) for v in pm],
                       pass_GBs=[float(pass_bytes / (v * 1e-3) / 1e9) for v in pm], copy_GBs=copy_gbs,
                       host_ms=stats(host), host_probs=5, ess=float(ess), csrc_sha=csrc_hash())
            if len(probs) == 5:
                rec["mismatches"] = int(np.sum(q != want[5]))
            rec["host_over_wall"] = rec["host_ms"]["median"] / rec["wall_ms"]["median"]
            line = json.dumps(rec)
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()
        ctx.close()


if __name__ == "__main__":
    main()
