"""Arma one-step residual checks (smcn_residuals_partials) on one MI355X: one JSON line per case, also appended to
profiles/residuals_bench.jsonl.

    python tools/residuals_bench.py [--reps 9] [--cases 0,1,2,3] [--out profiles/residuals_bench.jsonl]

GPU only; run every invocation under `timeout`.  Cases (N, T, L): the shipped series (T = 200) with L = 10 lags at
N = 65 536, 1 024 and 1 048 576, and a synthetic series of T = 4 000 with L = 20 at N = 65 536.  The resident particles
are (0.3, 0.5, -0.3, -0.5) + 0.1 N(0, 1) with log-weights 2 N(0, 1); one threshold of Q, the chi-square 5 % critical
value.  Per case, after two warm-up calls, the median and min / max of --reps calls:
  device_ms   the kernels of smcn_residuals_partials between HIP events on the context's stream (header, slices, the
              two merge stages; smcn_residuals_last_ms); wall_ms the whole call with the download of the block and the
              finish
  host_ms     the route this replaces, on the same population in the same run, once: get_state (download of x and logw)
              and the NumPy restatement in one pass over t (tests/_residuals.py: mixture_stream); host_state_ms the
              download alone
  max_share   the largest |device - host| over the magnitudes of tests/_residuals.py; share_of_bound that over
              (N + T) 2^-53, the bound of tests/test_gpu_residuals.py::test_the_window_edge
  chain_est_us   an estimate of the chain alone: T steps of two dependent fp64 fma at 8 cycles each at 2.4 GHz (not a
              measurement)
csrc_sha stamps the kernel sources the numbers belong to (bench.py's hash)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = [(65536, 200, 10), (1024, 200, 10), (1048576, 200, 10), (65536, 4000, 20)]


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--cases", default="0,1,2,3")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "residuals_bench.jsonl"))
    a = ap.parse_args()
    import _forecast as fref
    import _residuals as ref
    from bench import csrc_hash
    from smcnuts_amd import ArmaModel, _capi
    from smcnuts_amd.residuals import chi2_isf, combine_residual_partials
    out = open(a.out, "a")
    for N, T, L in [CASES[int(i)] for i in a.cases.split(",")]:
        ser = fref.shipped_series() if T == 200 else fref.synthetic_series(T, 1)
        assert ser.size == T
        t = ArmaModel(y=ser)
        rng = np.random.default_rng(N + T)
        x = np.array([0.3, 0.5, -0.3, -0.5])[None, :] + 0.1 * rng.standard_normal((N, 4))
        lw = 2.0 * rng.standard_normal(N)
        q_at = [chi2_isf(0.05, L)]
        ctx = _capi.Context(N, t.model_id, t.model_data)
        ctx.set_state(x=x, logw=lw)
        ctx.residuals_set(L, q_at)
        t0 = time.perf_counter()
        xs, lws, _ = ctx.get_state()
        state = (time.perf_counter() - t0) * 1e3
        want, sc = ref.mixture_stream(ser, xs, lws, L, q_at)
        host = (time.perf_counter() - t0) * 1e3
        ev, wall = [], []
        for r in range(a.reps + 2):
            t0 = time.perf_counter()
            res = combine_residual_partials([ctx.residuals_partials()], L, (0.05,))
            wl = (time.perf_counter() - t0) * 1e3
            if r >= 2:
                ev.append(ctx.residuals_last_ms())
                wall.append(wl)
        got = ref.of(res)
        keys = ref.KEYS_T + ref.KEYS_L + ("ljung_box", "ljung_box_var")
        shares = {k: ref.share(got[k], want[k], sc[k]) for k in keys}
        rec = dict(case=f"arma_N{N}_T{T}_L{L}", label=a.label, N=N, T=T, L=L, reps=a.reps, slices=-(-N // 256),
                   device_ms=stats(ev), wall_ms=stats(wall), host_ms=host, host_state_ms=state, ess=float(res.ess),
                   ljung_box=float(res.ljung_box), exceed=float(res.exceed[0]), host_exceed=float(want["exceed"][0]),
                   max_share=max(shares.values()), worst=max(shares, key=shares.get),
                   share_of_bound=max(shares.values()) / ((N + T) * 2.0 ** -53),
                   chain_est_us=T * 2 * 8 / 2.4e3, csrc_sha=csrc_hash())
        rec["host_over_wall"] = rec["host_ms"] / rec["wall_ms"]["median"]
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()
        ctx.close()


if __name__ == "__main__":
    main()
