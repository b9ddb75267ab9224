"""Step-size probe: the device measures, the host chooses.

The library runs short leapfrog trajectories from a population's particles at a ladder of candidate step sizes
(smcn_stepsize_probe, csrc/smcn_stepsize.hpp): per particle i and ladder entry j, n leapfrogs from the same (x_i, r_i)
and the statistic a_ij = (1/n) sum_t min(1, exp(-dH_t)), 0 from the first step whose energy error is not finite or
exceeds delta_max.  It returns mergeable partials [1 + L][4]:

    row 0      (m, particles probed, particles excluded, 0)      m: the largest finite log-weight probed
    row 1 + j  (sum w a_j, sum w d_j, sum w, number divergent)   w = exp(logw - m), d_j: the pair diverged

This module holds everything around that call: the ladders, the combination of shards' partials, the choice of the step
size from the weighted acceptance curve, and the result class.  What the defaults rest on, and what nobody has
measured, is in DESIGN.md 4.5.
"""
import numpy as np

LADDER_MAX = 16           # entries of one pass (the library's limit)
LEAPFROG_MAX = 64         # leapfrogs per trajectory (the library's limit)
TARGET_ACCEPT = 0.8       # Stan's adapt_delta
N_LEAPFROG = 8            # a guess: long enough to leave the starting point's curvature, short enough to stay cheap
MAX_PARTICLES = 4096


def default_ladder():
    """16 octaves, 2**-12 .. 2**3."""
    return 2.0 ** np.arange(-12.0, 4.0)


def refine_ladder(lo, hi):
    """16 geometric steps from lo to hi (two neighbours of a coarser ladder), both ends included exactly."""
    lo, hi = float(lo), float(hi)
    if not (np.isfinite(lo) and np.isfinite(hi) and 0.0 < lo < hi):
        raise ValueError(f"refine_ladder: need 0 < lo < hi, both finite, not ({lo}, {hi})")
    lad = lo * (hi / lo) ** (np.arange(LADDER_MAX) / (LADDER_MAX - 1.0))
    lad[0], lad[-1] = lo, hi
    return lad


def check_ladder(ladder):
    lad = np.ascontiguousarray(np.asarray(ladder, dtype=np.float64).reshape(-1))
    if not 1 <= lad.size <= LADDER_MAX:
        raise ValueError(f"ladder: 1 .. {LADDER_MAX} step sizes per pass, not {lad.size} (probe a longer ladder in pieces)")
    if not (np.all(np.isfinite(lad)) and np.all(lad > 0.0) and np.all(np.diff(lad) > 0.0)):
        raise ValueError("ladder: finite, positive and strictly increasing step sizes")
    return lad


def check_probe_args(target_accept=TARGET_ACCEPT, n_leapfrog=N_LEAPFROG, max_particles=MAX_PARTICLES, ladder=None,
                     phi=1.0, delta_max=100.0):
    """The refusals of probe_step_size, before any device context is made.  Returns the ladder (default_ladder() for None)."""
    if not (isinstance(target_accept, (int, float, np.floating)) and 0.0 < float(target_accept) < 1.0):
        raise ValueError(f"target_accept must lie in (0, 1), not {target_accept!r} (0.8 is Stan's adapt_delta)")
    if int(n_leapfrog) != n_leapfrog or not 1 <= int(n_leapfrog) <= LEAPFROG_MAX:
        raise ValueError(f"n_leapfrog: 1 .. {LEAPFROG_MAX} leapfrogs per trajectory, not {n_leapfrog!r}")
    if int(max_particles) != max_particles or int(max_particles) < 1:
        raise ValueError(f"max_particles must be a positive integer, not {max_particles!r}")
    if not (np.isfinite(phi) and 0.0 <= float(phi) <= 1.0):
        raise ValueError(f"phi (the temperature) must lie in [0, 1], not {phi!r}")
    if not float(delta_max) > 0.0:
        raise ValueError(f"delta_max must be positive, not {delta_max!r}")
    return default_ladder() if ladder is None else check_ladder(ladder)


def combine_stepsize_partials(parts):
    """The shards' partials [1 + L][4] as one: shard r's weighted sums are rescaled by exp(m_r - m), m the largest of the
    shards' finite maxima, and added in the order given (rank order); counts add as they are.  A shard without a finite
    log-weight (all of its particles excluded) contributes its counts only."""
    parts = [np.asarray(p, dtype=np.float64) for p in parts]
    if not parts or any(p.ndim != 2 or p.shape != parts[0].shape or p.shape[1] != 4 or p.shape[0] < 2 for p in parts):
        raise ValueError("every partial must be [1 + L][4] with the same L >= 1")
    ms = np.array([p[0, 0] for p in parts])
    fin = np.isfinite(ms)
    m = float(ms[fin].max()) if fin.any() else -np.inf
    out = np.zeros_like(parts[0])
    out[0, 0] = m
    for p, mr, ok in zip(parts, ms, fin):
        out[0, 1:3] += p[0, 1:3]
        out[1:, 3] += p[1:, 3]
        if ok:
            out[1:, :3] += np.exp(mr - m) * p[1:, :3]
    return out


def curves_from_partials(part):
    """(weighted mean of a_j [L], weighted share of divergent pairs [L]); NaN where no particle counts."""
    part = np.asarray(part, dtype=np.float64)
    with np.errstate(all="ignore"):
        w = part[1:, 2]
        return np.where(w > 0.0, part[1:, 0] / w, np.nan), np.where(w > 0.0, part[1:, 1] / w, np.nan)


def first_below(accept, target_accept):
    """Index of the first entry, scanning from the smallest step size up, whose weighted mean falls below the target
    (a NaN counts as below); None: none does."""
    for j, a in enumerate(np.asarray(accept, dtype=np.float64)):
        if not a >= target_accept:
            return j
    return None


def choose_step_size(ladder, accept, target_accept=TARGET_ACCEPT):
    """(step_size, bracketed).  Scans the ladder from its smallest entry up; at the first entry whose weighted mean
    acceptance falls below the target, interpolates linearly in log eps between it and its predecessor.  None falls
    below: the largest entry, bracketed=False.  The smallest is already below: the smallest, bracketed=False."""
    ladder = np.asarray(ladder, dtype=np.float64).reshape(-1)
    accept = np.asarray(accept, dtype=np.float64).reshape(-1)
    if ladder.size < 1 or ladder.shape != accept.shape:
        raise ValueError("choose_step_size: one acceptance value per ladder entry")
    j = first_below(accept, target_accept)
    if j is None:
        return float(ladder[-1]), False
    if j == 0:
        return float(ladder[0]), False
    a0, a1 = accept[j - 1], accept[j]
    if not np.isfinite(a1):                    # nothing to interpolate towards: the last entry known to hold the target
        return float(ladder[j - 1]), True
    t = (a0 - target_accept) / (a0 - a1)
    return float(np.exp(np.log(ladder[j - 1]) + t * (np.log(ladder[j]) - np.log(ladder[j - 1])))), True


class StepSizeProbe:
    """step_size: the chosen value; ladder, accept, divergent_share [L]: the pass that decided it (the refined one when
    there is one; `coarse` then holds the first pass as a StepSizeProbe of its own, else None); n_particles probed and
    n_excluded (starting density or weight not finite) over all shards; target_accept; bracketed: the curve crossed the
    target inside the ladder (False: step_size is an end of the ladder -- probe again with another one); ms: device time
    of the probe's kernels, all passes."""

    def __init__(self, step_size, ladder, accept, divergent_share, n_particles, n_excluded, target_accept, bracketed, ms,
                 coarse=None):
        self.step_size = float(step_size)
        self.ladder = np.asarray(ladder, dtype=np.float64)
        self.accept = np.asarray(accept, dtype=np.float64)
        self.divergent_share = np.asarray(divergent_share, dtype=np.float64)
        self.n_particles = int(n_particles)
        self.n_excluded = int(n_excluded)
        self.target_accept = float(target_accept)
        self.bracketed = bool(bracketed)
        self.ms = float(ms)
        self.coarse = coarse

    def __repr__(self):
        return (f"StepSizeProbe(step_size={self.step_size:.6g}, bracketed={self.bracketed}, target_accept="
                f"{self.target_accept}, n_particles={self.n_particles}, n_excluded={self.n_excluded}, "
                f"ladder={self.ladder[0]:.3g}..{self.ladder[-1]:.3g}, ms={self.ms:.3f})")


def probe_from_partials(ladder, part, target_accept, ms):
    accept, div = curves_from_partials(part)
    eps, br = choose_step_size(ladder, accept, target_accept)
    return StepSizeProbe(eps, ladder, accept, div, part[0, 1], part[0, 2], target_accept, br, ms)


def run_probe(one_pass, ladder, target_accept, refine):
    """one_pass(ladder) -> (combined partials [1 + L][4], ms).  The first pass over `ladder`; bracketed and `refine`: a
    second pass over refine_ladder of the two neighbours, from the same particles and momenta."""
    part, ms = one_pass(ladder)
    res = probe_from_partials(ladder, part, target_accept, ms)
    if not (refine and res.bracketed):
        return res
    j = first_below(res.accept, target_accept)
    lad2 = refine_ladder(ladder[j - 1], ladder[j])
    part2, ms2 = one_pass(lad2)
    fine = probe_from_partials(lad2, part2, target_accept, ms + ms2)
    fine.coarse = res
    if not fine.bracketed:          # (the ends are the coarse pass's entries with the same momenta: not expected)
        fine.step_size, fine.bracketed = res.step_size, True
    return fine


def context_pass(ctx, comm, x=None, logw=None, r=None, n_leapfrog=N_LEAPFROG, phi=1.0, delta_max=100.0, seed=0,
                 max_particles=MAX_PARTICLES):
    """one_pass of run_probe on a context: its own partials, one host all-gather over the shards, combined in rank order."""
    def one_pass(ladder):
        part, _, _ = ctx.stepsize_probe(ladder, x=x, logw=logw, r=r, n_leapfrog=n_leapfrog, phi=phi, delta_max=delta_max,
                                        seed=seed, max_particles=max_particles)
        ms = ctx.stepsize_last_ms()
        if comm is not None and comm.world_size > 1:
            allp = np.asarray(comm.allgather(np.append(part.reshape(-1), ms))).reshape(comm.world_size, -1)
            return combine_stepsize_partials([p[:-1].reshape(part.shape) for p in allp]), float(allp[:, -1].max())
        return combine_stepsize_partials([part]), ms
    return one_pass
