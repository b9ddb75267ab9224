"""The step-size probe (SMCSampler.probe_step_size, smcn_stepsize_probe) on one MI355X: one JSON line per configuration,
also appended to profiles/stepsize_probe.jsonl.

    python tools/stepsize_report.py [--K 20] [--out profiles/stepsize_probe.jsonl]

GPU only; run every invocation under `timeout`.  Run by hand: nothing else reads its output but DESIGN.md 4.5.
Configurations: arma at N = 65 536 (hand-picked step size 0.01), a logistic regression with n = 1000, D = 10 and one
column scaled by 100 at N = 16 384 (0.05, the value of the regression examples), the iso-Gaussian with D = 256 at
N = 131 072 (0.25).  The hand-picked values are those of INTEGRATION.md's examples.  Per configuration:
  probe_ms        device time of the probe's kernels on generation 0, both passes (HIP events; StepSizeProbe.ms), and
                  probe_wall_ms, the whole probe_step_size() call
  chosen / hand   the step size the probe chose (target_accept 0.8, 8 leapfrogs, 4096 particles) next to the hand-picked one
  per step size   a K-iteration run: leapfrogs per particle and iteration, final ESS, run time
What this does NOT measure: effective samples per leapfrog of the estimates -- the ESS here is the weights' (Kish), which
says how evenly the particles are weighted, not how far they have moved."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def configs():
    from smcnuts_amd import ArmaModel, IsoGaussian, LogisticRegression
    rng = np.random.default_rng(2024)
    n, p = 1000, 9
    Z = rng.standard_normal((n, p))
    b = rng.standard_normal(p) * 0.7
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-(0.3 + Z @ b)))).astype(np.float64)
    X = Z.copy()
    X[:, 0] *= 100.0
    return [("arma_N65536", lambda: ArmaModel(), 65536, 0.01),
            ("logistic_n1000_D10_col100_N16384", lambda: LogisticRegression(X, y), 16384, 0.05),
            ("isogauss_D256_N131072", lambda: IsoGaussian(256), 131072, 0.25)]


def run(make, N, K, eps, seed=17):
    from smcnuts_amd import SMCSampler
    s = SMCSampler(K=K, N=N, target=make(), step_size=eps, seed=seed, save_history=False)
    s.sample(show_progress=False)
    return dict(step_size=float(eps), leapfrogs_per_particle_iteration=float(s.leapfrogs.sum()) / (N * K),
                final_ess=float(s.ess[-1]), run_time_s=float(s.run_time),
                mean_finite=bool(np.all(np.isfinite(s.mean_estimate[-1]))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stepsize_probe.jsonl"))
    a = ap.parse_args()
    from bench import csrc_hash
    from smcnuts_amd import SMCSampler
    out = open(a.out, "a")
    for name, make, N, hand in configs():
        s = SMCSampler(K=1, N=N, target=make(), step_size=hand, seed=17, save_history=False)
        s.probe_step_size(seed=1)                              # warm-up: code objects, buffers
        t0 = time.perf_counter()
        p = s.probe_step_size(seed=1)
        wall = (time.perf_counter() - t0) * 1e3
        coarse = p.coarse or p
        rec = dict(config=name, N=N, K=a.K, probe_ms=p.ms, probe_wall_ms=wall, chosen=p.step_size, hand_picked=hand,
                   bracketed=p.bracketed, n_particles=p.n_particles, n_excluded=p.n_excluded,
                   coarse_ladder=coarse.ladder.tolist(), coarse_accept=coarse.accept.tolist(),
                   coarse_divergent_share=coarse.divergent_share.tolist(),
                   with_chosen=run(make, N, a.K, p.step_size), with_hand_picked=run(make, N, a.K, hand),
                   csrc_sha=csrc_hash())
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()


if __name__ == "__main__":
    main()
