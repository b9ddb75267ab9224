"""Arma forecasts (smcn_forecast_partials, smcn_forecast_draws) on one MI355X: one JSON line per case, also appended to
profiles/forecast_bench.jsonl.

    python tools/forecast_bench.py [--reps 9] [--host-reps 2] [--out profiles/forecast_bench.jsonl]

GPU only; run every invocation under `timeout`.  Cases (N, H, Tn) on the shipped series (T = 200), first N = 65 536,
H = 24, Tn = 4.  The resident particles are (0.3, 0.5, -0.3, -0.5) + 0.1 N(0, 1) with log-weights 2 N(0, 1); a held-out
continuation is given.  Per case, after two warm-up calls, the median and min / max of --reps calls:
  device_ms   the kernels of smcn_forecast_partials between HIP events on the context's stream (header, slices, the two
              merge stages; smcn_forecast_last_ms); wall_ms the whole call with the download of [1 + H][Q] and the finish
  host_ms     the route this replaces, on the same population in the same run: get_state (download of x and logw) and
              the NumPy restatement of the mixture (tests/_forecast.py: mixture; --host-reps runs), host_state_ms the
              download alone; max_share the largest |device - host| over the magnitudes of tests/_forecast.py
  draws_*     the same for 1000 paths: smcn_forecast_draws' kernels, the call, get_state plus the NumPy paths
  chain_est_us   an estimate of the chain alone: T steps of two dependent fp64 fma at 8 cycles each at
              2.4 GHz (not a measurement)
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

CASES = [(65536, 24, 4), (65536, 512, 16), (1048576, 24, 4), (1024, 24, 4)]
N_PATHS = 1000


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forecast_bench.jsonl"))
    a = ap.parse_args()
    import _forecast as ref
    from bench import csrc_hash
    from smcnuts_amd import ArmaModel, _capi
    from smcnuts_amd.forecast import combine_forecast_partials
    out = open(a.out, "a")
    t = ArmaModel()
    ser = ref.shipped_series()
    for N, H, Tn in CASES:
        rng = np.random.default_rng(N + H)
        x = np.array([0.3, 0.5, -0.3, -0.5])[None, :] + 0.1 * rng.standard_normal((N, 4))
        lw = 2.0 * rng.standard_normal(N)
        yf = ref.synthetic_series(H, 1)
        at = np.tile(np.linspace(-1.0, 2.0, Tn), (H, 1))
        ctx = _capi.Context(N, t.model_id, t.model_data)
        ctx.set_state(x=x, logw=lw)
        ctx.forecast_set(H, yf, at)
        host, state, want = [], [], None
        for r in range(a.host_reps if N * H * Tn <= 1e7 else 1):
            t0 = time.perf_counter()
            xs, lws, _ = ctx.get_state()
            state.append((time.perf_counter() - t0) * 1e3)
            want = ref.mixture(ser, xs, lws, H, yf, at)
            host.append((time.perf_counter() - t0) * 1e3)
        ev, wall = [], []
        for r in range(a.reps + 2):
            t0 = time.perf_counter()
            f = combine_forecast_partials([ctx.forecast_partials()], Tn, True, at)
            wl = (time.perf_counter() - t0) * 1e3
            if r >= 2:
                ev.append(ctx.forecast_last_ms()[0])
                wall.append(wl)
        sc = ref.mixture_scales(ser, x, lw, H, yf, at)
        dhost, dev_d, wall_d = [], [], []
        for r in range(a.host_reps if N * H * Tn <= 1e7 else 1):
            t0 = time.perf_counter()
            xs, lws, _ = ctx.get_state()
            anc, _ = ref.ancestors(lws, N, N_PATHS, 7)
            ref.paths(ser, xs, anc, 7, H)
            dhost.append((time.perf_counter() - t0) * 1e3)
        for r in range(a.reps + 2):
            t0 = time.perf_counter()
            ctx.forecast_draws(N_PATHS, 7)
            wl = (time.perf_counter() - t0) * 1e3
            if r >= 2:
                dev_d.append(ctx.forecast_last_ms()[1])
                wall_d.append(wl)
        rec = dict(case=f"arma_N{N}_H{H}_Tn{Tn}", label=a.label, N=N, T=int(ser.size), H=H, Tn=Tn, reps=a.reps,
                   slices=ctx.forecast_slices(N), device_ms=stats(ev), wall_ms=stats(wall), host_ms=stats(host),
                   host_state_ms=stats(state), ess=float(f.ess),
                   max_share=max(ref.share(getattr(f, k), want[k], sc[k]) for k in sc),
                   n_paths=N_PATHS, draws_device_ms=stats(dev_d), draws_wall_ms=stats(wall_d), draws_host_ms=stats(dhost),
                   chain_est_us=ser.size * 2 * 8 / 2.4e3, csrc_sha=csrc_hash())
        rec["host_over_wall"] = rec["host_ms"]["median"] / rec["wall_ms"]["median"]
        rec["draws_host_over_wall"] = rec["draws_host_ms"]["median"] / rec["draws_wall_ms"]["median"]
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()
        ctx.close()


if __name__ == "__main__":
    main()
