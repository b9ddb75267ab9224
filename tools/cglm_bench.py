"""ContinuousGLM (SMCN_MODEL_CGLM: gamma_log, student_t) throughput on one MI355X next to GLMTarget(family="normal") --
the same table walk with a cheaper observation body -- at the same shapes in the same process: one JSON line per shape,
printed and appended to profiles/cglm_bench.jsonl.

    python tools/cglm_bench.py [--K 10] [--N 65536] [--n 1000] [--dims 8,25,64] [--repeats 5]

GPU only; run every invocation under `timeout`.  Shapes: N = 65 536 particles, n = 1 000 observations, D in {8, 25, 64}
(D counts tau: 8 is the 8-lane shape, 25 and 64 one wavefront per particle); synthetic data from fixed seeds
(tests/_cglm.py, tests/_glm_disp.py).  Each family's step size is the largest of tools/glm_bench.py's halving ladder
whose pilot NUTS launch averages >= 8 leapfrogs per tree.  After a warm-up run of each, the three targets are run
alternately `repeats` times (K generations of SMCSampler, forward L-kernel, device-resident loop): per family the median
leapfrog/s with its min..max, the spread (max - min) / median, milliseconds per NUTS launch, and the ratios of the medians
to normal's.  A ratio below 0.5 is flagged (`below_half_of_normal`): look for spills or an un-hoisted constant before
accepting it.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

OUT = os.path.join(ROOT, "profiles", "cglm_bench.jsonl")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=10)
    ap.add_argument("--N", type=int, default=65536)
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--dims", default="8,25,64")
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import _cglm
    import _glm_disp
    from glm_bench import pick_step, run
    from smcnuts_amd import ContinuousGLM, GLMTarget
    for D in (int(v) for v in a.dims.split(",")):
        n, p = a.n, D - 2
        targets = {}
        X, y = _glm_disp.synthetic("normal", n, p, 1000 + D, scale=0.5)
        targets["normal"] = GLMTarget(X, y, family="normal", prior_sd=2.0, dispersion_prior=(0.0, 2.5))
        for family in _cglm.FAMILIES:
            X, y = _cglm.synthetic(family, n, p, 1000 + D, scale=0.5)
            targets[family] = ContinuousGLM(X, y, family=family, prior_sd=2.0, dispersion_prior=(0.0, 2.5))
        steps = {}
        for name, t in targets.items():
            steps[name] = pick_step(t, a.N, 5)
            run(t, a.N, 2, steps[name][0], 6)                    # warm-up: code objects, allocations
        runs = {name: [] for name in targets}
        for _ in range(a.repeats):
            for name, t in targets.items():
                runs[name].append(run(t, a.N, a.K, steps[name][0], 7))
        r = dict(case=f"cglm_n{n}_D{D}", n=n, D=D, N=a.N, K=a.K, repeats=a.repeats)
        for name, rs in runs.items():
            v = sorted(q["leapfrog_per_s"] for q in rs)
            ms = sorted(q["nuts_ms_per_launch"] for q in rs)[len(rs) // 2]
            r[name] = dict(median=v[len(v) // 2], min=v[0], max=v[-1], spread=(v[-1] - v[0]) / v[len(v) // 2],
                           step_size=steps[name][0], pilot_nleap=steps[name][1], nleap_mean=rs[-1]["nleap_mean"],
                           nuts_ms_per_launch=ms, repeatable=all(q["leapfrogs"] == rs[0]["leapfrogs"] for q in rs))
        for family in _cglm.FAMILIES:
            r[f"ratio_{family}_over_normal"] = r[family]["median"] / r["normal"]["median"]
        r["below_half_of_normal"] = [f for f in _cglm.FAMILIES if r[f"ratio_{f}_over_normal"] < 0.5]
        line = json.dumps(r)
        print(line, flush=True)
        with open(OUT, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
