"""GLM targets (GLMTarget, SMCN_MODEL_GLM; HierarchicalGLM, SMCN_MODEL_HGLM; CategoricalRegression;
OrdinalRegression; MultilevelGLM, SMCN_MODEL_MLGLM) throughput on one MI355X: one JSON line per case.

    python tools/glm_bench.py [--K 10] [--N 65536] [--host-N 4096] [--families normal,neg_binomial_2_log]
                              [--models glm,hier,cat,ord,multi,wide,offset] [--wide-cases bernoulli_logit:65,normal:256]

GPU only; run every invocation under `timeout`.  Cases: bernoulli_logit at N = 65 536 with (n, D) in {(100, 8),
(1 000, 25), (10 000, 64), (1 000, 16), (1 000, 17)}, poisson_log at (1 000, 25), and normal and neg_binomial_2_log
(D counts tau) at (100, 8), (1 000, 16), (1 000, 25); synthetic data from fixed seeds (--families: a subset).  The step size of each case
is the largest of a halving ladder whose pilot NUTS launch averages >= 8 leapfrogs per tree (trees of 2^3-2^4).
Per case: leapfrog/s and mean leapfrogs per tree of a K-generation SMCSampler run (forward L-kernel, device-resident
loop), milliseconds per NUTS launch (smcn_timers), and the fp64 rate counted as 4 n D flop per leapfrog (eta and the
gradient: two multiply-adds per design entry) against the 78.6 TF peak bench.py uses.  The (1 000, 25) cases of
logistic, normal and NB are also run at --host-N particles both device-native and through HostTarget with the numpy
density of tests/_glm.py / tests/_glm_disp.py.
Hierarchical cases (varying intercepts, D = Dc + J + 1 (+ 1)): bernoulli_logit with n = 1 000, Dc = 5, J = 20 and
normal with n = 1 000, Dc = 3, J = 50, the same way; the logistic one also against HostTarget with tests/_hglm.py's
numpy density.  Their flop count is 4 n (Dc + 1) per leapfrog (eta's fixed part and its gradient, plus the group term).
Categorical cases (CategoricalRegression, D = (K - 1) Dc): (K, n, Dc) in {(3, 100, 4), (5, 1 000, 6), (16, 1 000, 4)},
the (5, 1 000, 6) one also against HostTarget with tests/_cat.py's numpy density; flop count 4 n D per leapfrog.
Ordinal cases (OrdinalRegression, D = p + K - 1): (K, n, p) in {(5, 100, 3), (5, 1 000, 20), (10, 1 000, 40)}, the
(5, 1 000, 20) one also against HostTarget with tests/_ord.py's numpy density; flop count 4 n p per leapfrog.
Multilevel cases (--models multi; MultilevelGLM, not in the default set): (a) the hierarchical logistic case (n = 1 000,
Dc = 5, J = 20) expressed as MultilevelGLM with one term and z = 1, against HierarchicalGLM on the same data, step and
seed in one process, the two alternated five times -- both medians, their min..max and the ratio of the medians; (b)
normal, n = 1 000, Dc = 3, an intercept and a slope on one factor of 18 levels.  Flop count 4 n (Dc + R) per leapfrog.
Wide cases (--models wide; WideGLMTarget, SMCN_MODEL_WGLM, not in the default set; run with --N 16384): n = 1 000,
bernoulli_logit at D = 65, 128, 129, 256 and normal at D = 128, 256 (--wide-cases: a subset, so that a caller can give
every case a process and a time limit of its own).  The step is the ladder's (pilot launch >= 8 leapfrogs per tree at
generation 0; the trees grow as the particles spread: 15 to 60 leapfrogs per tree over the run, `nleap_in_15_60`).  Per case the figures above and `fma_per_s` = 2 n DP leapfrog/s, DP = the row's padded
column count: the evaluation's multiply-adds (eta and the column sums) per second.  With the bernoulli_logit D = 65 case,
in the same process: GLMTarget at D = 64 on the first 63 columns of the same data (`wide_ref_glm_D64`: the per-FMA
efficiency of the one-coordinate-per-lane functor), and the D = 65 model at --host-N particles both device-native and
through HostTarget with the numpy density (`.._vs_host`: what a user had before).
Offset cases (--models offset; GLMTarget(offset=, weights=), SMCN_MODEL_OGLM, not in the default set): the (1 000, 16),
(1 000, 17) and (1 000, 25) cases of each family (--families: a subset) as GLMTarget and as the offset model with o = 0 and
w = 1 -- the same posterior -- on the same data, step and seed in one process, the two alternated five times: both
medians, their min..max and the ratio of the medians, one JSON line per case, also appended to
profiles/glm_offset_bench.jsonl.
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

# (the two D = 16 / 17 cases sit on either side of the boundary between the functor's two shapes)
CASES = [("bernoulli_logit", 100, 8), ("bernoulli_logit", 1000, 25), ("bernoulli_logit", 10000, 64),
         ("poisson_log", 1000, 25), ("bernoulli_logit", 1000, 16), ("bernoulli_logit", 1000, 17),
         ("normal", 100, 8), ("normal", 1000, 16), ("normal", 1000, 25),
         ("neg_binomial_2_log", 100, 8), ("neg_binomial_2_log", 1000, 16), ("neg_binomial_2_log", 1000, 25)]
HOST_CASES = (("bernoulli_logit", 1000, 25), ("normal", 1000, 25), ("neg_binomial_2_log", 1000, 25))
# hierarchical: (family, n, Dc, J)
HIER_CASES = [("bernoulli_logit", 1000, 5, 20), ("normal", 1000, 3, 50)]
HIER_HOST_CASES = (("bernoulli_logit", 1000, 5, 20),)
# categorical: (classes K, n, Dc); D = (K - 1) Dc: 8 (the 8-lane shape), 24, 60
CAT_CASES = [(3, 100, 4), (5, 1000, 6), (16, 1000, 4)]
CAT_HOST_CASES = ((5, 1000, 6),)
# ordinal: (classes K, n, p); D = p + K - 1: 7 (the 8-lane shape), 24, 49
ORD_CASES = [(5, 100, 3), (5, 1000, 20), (10, 1000, 40)]
ORD_HOST_CASES = ((5, 1000, 20),)
MULTI_REPEATS = 5
# wide: (family, D), n = 1 000; D counts tau
WIDE_CASES = [("bernoulli_logit", 65), ("bernoulli_logit", 128), ("bernoulli_logit", 129), ("bernoulli_logit", 256),
              ("normal", 128), ("normal", 256)]
WIDE_N_OBS = 1000
# offset: (n, D) of each family; D counts tau.  16 / 17 sit on either side of the canonical families' shape boundary; the
# dispersion families are one wavefront per particle at all three
OFFSET_CASES = [(1000, 16), (1000, 17), (1000, 25)]
OFFSET_FAMILIES = ("bernoulli_logit", "poisson_log", "normal", "neg_binomial_2_log")


def pick_step(target, N, seed):
    from smcnuts_amd import _capi
    ctx = _capi.Context(N, target.model_id, target.model_data)
    ctx.set_seed(seed)
    ctx.call("smcn_init_particles_std_normal", 1.0)
    x0, _, _ = ctx.get_state()
    eps = 0.4
    for _ in range(10):
        ctx.set_state(x=x0)                                   # generation 0's particles
        ctx.propose_nuts(eps, 1.0, 0)
        m = float(ctx.tree_stats()["nleap"].mean())
        if m >= 8.0:
            break
        eps *= 0.5
    ctx.close()
    return eps, m


def run(target, N, K, eps, seed):
    from smcnuts_amd import SMCSampler
    smc = SMCSampler(K=K, N=N, target=target, step_size=eps, seed=seed)
    ctx = smc.samples.ctx
    ctx.timers(reset=True)
    smc.sample(show_progress=False)
    ms, launches = ctx.timers()[:2]
    leaps = int(smc.leapfrogs.sum())
    return dict(run_s=smc.run_time, leapfrogs=leaps, leapfrog_per_s=leaps / smc.run_time,
                nleap_mean=leaps / (N * K), nuts_ms_per_launch=(ms / launches) if launches else None,
                launches=int(launches), device_resident=bool(smc.device_resident))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=10)
    ap.add_argument("--N", type=int, default=65536)
    ap.add_argument("--host-N", type=int, default=4096)
    ap.add_argument("--host-K", type=int, default=3)
    ap.add_argument("--families", default=None, help="comma-separated subset of the families (default: all)")
    ap.add_argument("--models", default="glm,hier,cat,ord",
                    help="comma-separated: glm (GLMTarget cases), hier (HierarchicalGLM cases), cat (CategoricalRegression), "
                         "ord (OrdinalRegression); multi (MultilevelGLM), wide (WideGLMTarget) and offset (GLMTarget with "
                         "offset= / weights=), not in the default set")
    ap.add_argument("--wide-cases", default=None, help="comma-separated family:D subset of the wide cases (default: all)")
    a = ap.parse_args()
    models = set(a.models.split(","))
    import _glm
    import _glm_disp
    from smcnuts_amd import GLMTarget
    fams = None if a.families is None else set(a.families.split(","))
    for family, n, D in (CASES if "glm" in models else []):
        if fams is not None and family not in fams:
            continue
        disp = family in _glm_disp.DISP_FAMILIES
        if disp:
            X, y = _glm_disp.synthetic(family, n, D - 2, 1000 + D, scale=0.5)
            t = GLMTarget(X, y, family=family, prior_sd=2.0, dispersion_prior=(0.0, 2.5))
            host_model = lambda: _glm_disp.GLMDispNumpy(X, y, family, 2.0, (0.0, 2.5))
        else:
            X, y = _glm.synthetic(family, n, D - 1, 1000 + D, scale=0.5)
            t = GLMTarget(X, y, family=family, prior_sd=2.0)
            host_model = lambda: _glm.GLMNumpy(X, y, family, 2.0)
        eps, pilot = pick_step(t, a.N, 5)
        run(t, a.N, 2, eps, 6)                                   # warm-up: code objects, allocations
        r = run(t, a.N, a.K, eps, 7)
        r.update(case=f"{family}_n{n}_D{D}", family=family, n=n, D=D, N=a.N, K=a.K, step_size=eps, pilot_nleap=pilot,
                 fp64_tflops=4.0 * n * D * r["leapfrog_per_s"] / 1e12)
        r["fp64_fraction_of_peak"] = r["fp64_tflops"] * 1e12 / PEAK_FP64
        print(json.dumps(r), flush=True)
        if (family, n, D) in HOST_CASES:
            dev = run(t, a.host_N, a.host_K, eps, 8)
            host = run(host_model(), a.host_N, a.host_K, eps, 8)
            print(json.dumps(dict(case=f"{family}_n{n}_D{D}_vs_host", N=a.host_N, K=a.host_K, step_size=eps,
                                  device=dev, host=host, same_leapfrogs=dev["leapfrogs"] == host["leapfrogs"],
                                  speedup=host["run_s"] / dev["run_s"])), flush=True)
    if "hier" in models:
        hier(a, fams)
    if "cat" in models:
        cat(a)
    if "ord" in models:
        ordinal(a)
    if "multi" in models:
        multi(a)
    if "wide" in models:
        wide(a)
    if "offset" in models:
        offset(a, fams)


def offset(a, fams):
    import _glm
    import _glm_disp
    from smcnuts_amd import GLMTarget, _capi
    out = os.path.join(ROOT, "profiles", "glm_offset_bench.jsonl")
    for family in OFFSET_FAMILIES:
        if fams is not None and family not in fams:
            continue
        for n, D in OFFSET_CASES:
            disp = family in _glm_disp.DISP_FAMILIES
            if disp:
                X, y = _glm_disp.synthetic(family, n, D - 2, 1000 + D, scale=0.5)
                kw = dict(family=family, prior_sd=2.0, dispersion_prior=(0.0, 2.5))
            else:
                X, y = _glm.synthetic(family, n, D - 1, 1000 + D, scale=0.5)
                kw = dict(family=family, prior_sd=2.0)
            tg = GLMTarget(X, y, **kw)
            to = GLMTarget(X, y, offset=np.zeros(n), weights=np.ones(n), **kw)
            assert tg.model_id == _capi.MODEL_GLM and to.model_id == _capi.MODEL_OGLM
            eps, pilot = pick_step(tg, a.N, 5)
            run(tg, a.N, 2, eps, 6)                              # warm-up: code objects, allocations
            run(to, a.N, 2, eps, 6)
            rg, ro = [], []
            for _ in range(MULTI_REPEATS):
                rg.append(run(tg, a.N, a.K, eps, 7))
                ro.append(run(to, a.N, a.K, eps, 7))

            def stats(rs):
                v = sorted(r["leapfrog_per_s"] for r in rs)
                return dict(median=v[len(v) // 2], min=v[0], max=v[-1])
            sg, so = stats(rg), stats(ro)
            ms = lambda rs: sorted(r["nuts_ms_per_launch"] for r in rs)[len(rs) // 2]
            r = dict(case=f"offset_{family}_n{n}_D{D}_vs_glm", family=family, n=n, D=D, N=a.N, K=a.K, step_size=eps,
                     pilot_nleap=pilot, repeats=MULTI_REPEATS, nleap_mean=ro[-1]["nleap_mean"],
                     offset_leapfrog_per_s=so, glm_leapfrog_per_s=sg, ratio_offset_over_glm=so["median"] / sg["median"],
                     offset_nuts_ms_per_launch=ms(ro), glm_nuts_ms_per_launch=ms(rg),
                     glm_spread=(sg["max"] - sg["min"]) / sg["median"],
                     same_leapfrogs=all(q["leapfrogs"] == rg[0]["leapfrogs"] for q in rg + ro))
            line = json.dumps(r)
            print(line, flush=True)
            with open(out, "a") as f:
                f.write(line + "\n")


def hier(a, fams):
    import _hglm
    from smcnuts_amd import HierarchicalGLM
    for family, n, Dc, J in HIER_CASES:
        if fams is not None and family not in fams:
            continue
        disp = family in _hglm.gd.DISP_FAMILIES
        D = Dc + J + 1 + (1 if disp else 0)
        X, y, g = _hglm.synthetic(family, n, Dc - 1, J, 2000 + D)
        kw = dict(dispersion_prior=(0.0, 2.5)) if disp else {}
        t = HierarchicalGLM(X, y, g, family=family, prior_sd=2.0, group_sd_prior=1.0, n_groups=J, **kw)
        host_model = lambda: _hglm.HGLMNumpy(X, y, g, family, 2.0, 1.0, (0.0, 2.5), n_groups=J)
        eps, pilot = pick_step(t, a.N, 5)
        run(t, a.N, 2, eps, 6)
        r = run(t, a.N, a.K, eps, 7)
        r.update(case=f"hier_{family}_n{n}_Dc{Dc}_J{J}", family=family, n=n, Dc=Dc, J=J, D=D, N=a.N, K=a.K,
                 step_size=eps, pilot_nleap=pilot, fp64_tflops=4.0 * n * (Dc + 1) * r["leapfrog_per_s"] / 1e12)
        r["fp64_fraction_of_peak"] = r["fp64_tflops"] * 1e12 / PEAK_FP64
        print(json.dumps(r), flush=True)
        if (family, n, Dc, J) in HIER_HOST_CASES:
            dev = run(t, a.host_N, a.host_K, eps, 8)
            host = run(host_model(), a.host_N, a.host_K, eps, 8)
            print(json.dumps(dict(case=f"hier_{family}_n{n}_Dc{Dc}_J{J}_vs_host", N=a.host_N, K=a.host_K, step_size=eps,
                                  device=dev, host=host, same_leapfrogs=dev["leapfrogs"] == host["leapfrogs"],
                                  speedup=host["run_s"] / dev["run_s"])), flush=True)


def cat(a):
    import _cat
    from smcnuts_amd import CategoricalRegression
    for K, n, Dc in CAT_CASES:
        D = (K - 1) * Dc
        X, y = _cat.synthetic(K, n, Dc - 1, 3000 + D, scale=0.5)
        t = CategoricalRegression(X, y, n_classes=K, prior_sd=2.0)
        host_model = lambda: _cat.CategoricalNumpy(X, y, n_classes=K, prior_sd=2.0)
        eps, pilot = pick_step(t, a.N, 5)
        run(t, a.N, 2, eps, 6)
        r = run(t, a.N, a.K, eps, 7)
        r.update(case=f"cat_K{K}_n{n}_Dc{Dc}", K_classes=K, n=n, Dc=Dc, D=D, N=a.N, K=a.K, step_size=eps,
                 pilot_nleap=pilot, fp64_tflops=4.0 * n * D * r["leapfrog_per_s"] / 1e12)
        r["fp64_fraction_of_peak"] = r["fp64_tflops"] * 1e12 / PEAK_FP64
        print(json.dumps(r), flush=True)
        if (K, n, Dc) in CAT_HOST_CASES:
            dev = run(t, a.host_N, a.host_K, eps, 8)
            host = run(host_model(), a.host_N, a.host_K, eps, 8)
            print(json.dumps(dict(case=f"cat_K{K}_n{n}_Dc{Dc}_vs_host", N=a.host_N, K=a.host_K, step_size=eps,
                                  device=dev, host=host, same_leapfrogs=dev["leapfrogs"] == host["leapfrogs"],
                                  speedup=host["run_s"] / dev["run_s"])), flush=True)


def ordinal(a):
    import _ord
    from smcnuts_amd import OrdinalRegression
    for K, n, p in ORD_CASES:
        D = p + K - 1
        X, y = _ord.synthetic(K, n, p, 4000 + D, scale=0.5)
        t = OrdinalRegression(X, y, n_classes=K, prior_sd=2.0, cutpoint_prior_sd=5.0)
        host_model = lambda: _ord.OrdinalNumpy(X, y, n_classes=K, prior_sd=2.0, cutpoint_prior_sd=5.0)
        eps, pilot = pick_step(t, a.N, 5)
        run(t, a.N, 2, eps, 6)
        r = run(t, a.N, a.K, eps, 7)
        r.update(case=f"ord_K{K}_n{n}_p{p}", K_classes=K, n=n, p=p, D=D, N=a.N, K=a.K, step_size=eps,
                 pilot_nleap=pilot, fp64_tflops=4.0 * n * p * r["leapfrog_per_s"] / 1e12)
        r["fp64_fraction_of_peak"] = r["fp64_tflops"] * 1e12 / PEAK_FP64
        print(json.dumps(r), flush=True)
        if (K, n, p) in ORD_HOST_CASES:
            dev = run(t, a.host_N, a.host_K, eps, 8)
            host = run(host_model(), a.host_N, a.host_K, eps, 8)
            print(json.dumps(dict(case=f"ord_K{K}_n{n}_p{p}_vs_host", N=a.host_N, K=a.host_K, step_size=eps,
                                  device=dev, host=host, same_leapfrogs=dev["leapfrogs"] == host["leapfrogs"],
                                  speedup=host["run_s"] / dev["run_s"])), flush=True)


def multi(a):
    import _hglm
    import _mlglm
    from smcnuts_amd import HierarchicalGLM, MultilevelGLM
    # (a) HIER_CASES[0] as one varying-intercept term, alternated with HierarchicalGLM
    family, n, Dc, J = HIER_CASES[0]
    D = Dc + J + 1
    X, y, g = _hglm.synthetic(family, n, Dc - 1, J, 2000 + D)
    th = HierarchicalGLM(X, y, g, family=family, prior_sd=2.0, group_sd_prior=1.0, n_groups=J)
    tm = MultilevelGLM(X, y, [(g, None, J)], family=family, prior_sd=2.0, group_sd_prior=1.0)
    eps, pilot = pick_step(th, a.N, 5)
    run(th, a.N, 2, eps, 6)
    run(tm, a.N, 2, eps, 6)
    rh, rm = [], []
    for _ in range(MULTI_REPEATS):
        rh.append(run(th, a.N, a.K, eps, 7))
        rm.append(run(tm, a.N, a.K, eps, 7))

    def stats(rs):
        v = sorted(r["leapfrog_per_s"] for r in rs)
        return dict(median=v[len(v) // 2], min=v[0], max=v[-1])
    sh, sm = stats(rh), stats(rm)
    r = dict(rm[-1])
    r.update(case=f"multi_R1_{family}_n{n}_Dc{Dc}_J{J}_vs_hier", family=family, n=n, Dc=Dc, J=[J], R=1, D=D, N=a.N,
             K=a.K, step_size=eps, pilot_nleap=pilot, repeats=MULTI_REPEATS, leapfrog_per_s=sm["median"],
             multi_leapfrog_per_s=sm, hier_leapfrog_per_s=sh, ratio_multi_over_hier=sm["median"] / sh["median"],
             hier_spread=(sh["max"] - sh["min"]) / sh["median"],
             same_leapfrogs=all(q["leapfrogs"] == rh[0]["leapfrogs"] for q in rh + rm),
             fp64_tflops=4.0 * n * (Dc + 1) * sm["median"] / 1e12)
    r["fp64_fraction_of_peak"] = r["fp64_tflops"] * 1e12 / PEAK_FP64
    print(json.dumps(r), flush=True)
    # (b) normal, an intercept and a slope on one factor of 18 levels
    family, n, Dc, J = "normal", 1000, 3, 18
    D = Dc + 2 * J + 2 + 1
    X, y, terms = _mlglm.synthetic(family, n, Dc - 1, [(J, 0), (J, 0)], 2000 + D)
    t = MultilevelGLM(X, y, terms, family=family, prior_sd=2.0, group_sd_prior=1.0, dispersion_prior=(0.0, 2.5))
    eps, pilot = pick_step(t, a.N, 5)
    run(t, a.N, 2, eps, 6)
    r = run(t, a.N, a.K, eps, 7)
    r.update(case=f"multi_R2_{family}_n{n}_Dc{Dc}_J{J}x2", family=family, n=n, Dc=Dc, J=[J, J], R=2, D=D, N=a.N, K=a.K,
             step_size=eps, pilot_nleap=pilot, fp64_tflops=4.0 * n * (Dc + 2) * r["leapfrog_per_s"] / 1e12)
    r["fp64_fraction_of_peak"] = r["fp64_tflops"] * 1e12 / PEAK_FP64
    print(json.dumps(r), flush=True)


def wide(a):
    import _glm
    import _glm_disp
    from smcnuts_amd import GLMTarget, WideGLMTarget
    n = WIDE_N_OBS
    want = None if a.wide_cases is None else {tuple(c.split(":")) for c in a.wide_cases.split(",")}
    for family, D in WIDE_CASES:
        if want is not None and (family, str(D)) not in want:
            continue
        disp = family in _glm_disp.DISP_FAMILIES
        Dc = D - (1 if disp else 0)
        if disp:
            X, y = _glm_disp.synthetic(family, n, Dc - 1, 5000 + D, scale=0.5)
            t = WideGLMTarget(X, y, family=family, prior_sd=2.0, dispersion_prior=(0.0, 2.5))
        else:
            X, y = _glm.synthetic(family, n, Dc - 1, 5000 + D, scale=0.5)
            t = WideGLMTarget(X, y, family=family, prior_sd=2.0)
        DP = (Dc + 1) // 2 * 2

        def line(name, target, dp, dim, **more):
            eps, pilot = pick_step(target, a.N, 5)
            run(target, a.N, 2, eps, 6)                          # warm-up: code objects, allocations
            r = run(target, a.N, a.K, eps, 7)
            r.update(case=name, family=family, n=n, D=dim, DP=dp, N=a.N, K=a.K, step_size=eps, pilot_nleap=pilot,
                     nleap_in_15_60=bool(15.0 <= r["nleap_mean"] <= 60.0), fma_per_s=2.0 * n * dp * r["leapfrog_per_s"],
                     fp64_tflops=4.0 * n * dp * r["leapfrog_per_s"] / 1e12, library=os.environ.get("SMCN_LIB", "built"), **more)
            r["fp64_fraction_of_peak"] = r["fp64_tflops"] * 1e12 / PEAK_FP64
            print(json.dumps(r), flush=True)
            return eps, r

        eps, r = line(f"wide_{family}_n{n}_D{D}", t, DP, D)
        if (family, D) == WIDE_CASES[0]:
            # the reference lines, in this process: the narrow functor on the first 63 columns, the host-evaluated model
            g = GLMTarget(X[:, :63], y, family=family, prior_sd=2.0)
            _, rg = line(f"wide_ref_glm_{family}_n{n}_D64", g, 64, 64)
            print(json.dumps(dict(case=f"wide_{family}_D{D}_over_glm_D64", leapfrog_rate_ratio=r["leapfrog_per_s"] / rg["leapfrog_per_s"],
                                  fma_rate_ratio=r["fma_per_s"] / rg["fma_per_s"])), flush=True)
            dev = run(t, a.host_N, a.host_K, eps, 8)
            host = run(_glm.GLMNumpy(X, y, family, 2.0), a.host_N, a.host_K, eps, 8)
            print(json.dumps(dict(case=f"wide_{family}_n{n}_D{D}_vs_host", N=a.host_N, K=a.host_K, step_size=eps,
                                  device=dev, host=host, same_leapfrogs=dev["leapfrogs"] == host["leapfrogs"],
                                  wide_full_N_leapfrog_per_s=r["leapfrog_per_s"],
                                  wide_faster_than_host=bool(r["leapfrog_per_s"] > host["leapfrog_per_s"]),
                                  speedup=host["run_s"] / dev["run_s"])), flush=True)


if __name__ == "__main__":
    main()
