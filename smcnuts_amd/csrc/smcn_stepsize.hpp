// Step-size probe (smcn_stepsize_probe): short leapfrog trajectories from a population's particles at a ladder of
// candidate step sizes, one pass; the host picks the largest step size that keeps the energy error in check
// (smcnuts_amd/stepsize.py).  Nothing here is called by the sampler's loops.
//
// Per probed particle i and ladder entry j the trajectory restarts from the SAME (x_i, r_i) -- common random numbers
// across the ladder -- and runs n leapfrogs of size eps_j:
//     r += eps/2 g;  x += eps r;  g = grad log pi_phi(x);  r += eps/2 g;  dH_t = H_t - H_0,  H = -log pi_phi + |r|^2 / 2
//     a_ij = (1/n) sum_t min(1, exp(-dH_t))
// The first t at which dH_t is not finite or exceeds delta_max marks the pair divergent (first_bad = t): that step and
// all later ones contribute 0 and the trajectory stops.  A particle whose starting density or log-weight is not finite
// is excluded (a = 0, first_bad = 0, excluded flag set).
//
// stepsize_probe_kernel mirrors eval_kernel (smcn_weights.hpp): the same coordinate layout, model.init, cooperative
// model.eval and a trip count that is equal for all lanes of a wavefront; lane_stepsize_probe_kernel mirrors
// lane_eval_kernel (smcn_nuts3.hpp).  x, r, g are [DL] registers; the start is re-read from memory per ladder entry.
#pragma once
#include "smcn_weights.hpp"

namespace smcn {

constexpr uint32_t kStreamStepsize = 24;   // Philox stream of the probe's momenta (no sampler kernel draws from it)
constexpr int kStepLadderMax = 16, kStepLeapMax = 64;

struct StepArgs {
    const double* x;        // particle i's coordinate c at x[i * rs + c * cs]
    int64_t rs, cs;
    const double* logw;     // [M]
    const double* r;        // [Mp][D] momenta of the probed particles, or null: Philox
    int64_t M, Mp;          // probed particle k is particle (k * M) / Mp
    int64_t particle_base;
    uint64_t seed;
    double ladder[kStepLadderMax];
    int L, n;
    double phi, delta_max;
    double* accept;         // [L][Mp]
    int32_t* first_bad;     // [L][Mp]
    int32_t* excluded;      // [Mp]
};

// momentum coordinate c of particle p: the draw normals_kernel makes for (pair c / 2, p), cosine for the even coordinate
__device__ __forceinline__ double stepsize_momentum(const StepArgs& a, int64_t p, int c) {
    const u32x4 o = philox4x32_10({(uint32_t)(c >> 1), (uint32_t)(a.particle_base + p), 0u, kStreamStepsize},
                                  (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
    const double u1 = u53(o.a, o.b), u2 = u53(o.c, o.d);
    const double rad = sqrt(-2.0 * log1p(-u1));
    double sn, cs;
    sincospi(2.0 * u2, &sn, &cs);
    return rad * ((c & 1) ? sn : cs);
}
// one step's share of the statistic; returns false where the pair has just diverged
__device__ __forceinline__ bool stepsize_step(double dH, double delta_max, double& acc) {
    if (!finite_d(dH) || dH > delta_max) return false;
    const double e = exp(-dH);
    acc += e < 1.0 ? e : 1.0;
    return true;
}

// log pi_phi up to an additive constant, and the two gradient parts.  Only differences of H enter the statistic, so a
// functor that offers its sums before the normalising constant is added (HAS_PARTIAL: the Gaussians) is evaluated without
// it: a constant such as -D log s is large against dH_t and its rounding would be all of dH_t's error -- and without it
// the probe of N(0, s^2 I) at x = s u with the ladder times s is, for s a power of two, the probe of N(0, I) bit for bit
template <class Model, class = void>
struct probe_has_partial { static constexpr bool value = false; };
template <class Model>
struct probe_has_partial<Model, decltype((void)Model::HAS_PARTIAL)> { static constexpr bool value = Model::HAS_PARTIAL; };
template <class Model>
__device__ __forceinline__ double probe_logp(const Model& model, const double (&x)[Model::DL], double phi,
                                             double (&gp)[Model::DL], double (&gl)[Model::DL]) {
    if constexpr (probe_has_partial<Model>::value) {
        double ss, sl;
        model.eval_partial(x, ss, sl, gp, gl);
        ss = group_sum<Model::G>(ss);
        double lp = -0.5 * ss * model.inv0;
        if (model.has) lp += phi * (-0.5 * group_sum<Model::G>(sl) * model.inv1);
        return lp;
    } else {
        double lpri, llik;
        model.eval(x, lpri, llik, gp, gl);
        return lpri + phi * llik;
    }
}

template <class Model>
__global__ void __launch_bounds__(256) stepsize_probe_kernel(const double* mdata, StepArgs a) {
    constexpr int G = Model::G, DL = Model::DL;
    static_assert(Model::DIST, "coordinate c = lg + G * k lives on lane lg");
    extern __shared__ double step_lds[];
    const int lg = (int)(threadIdx.x & (G - 1));
    Model model;
    model.init(mdata, lg, step_lds);
    const int D = model.dim();
    const int64_t ngroups = (int64_t)gridDim.x * (blockDim.x / G);
    const int64_t g0 = (int64_t)blockIdx.x * (blockDim.x / G) + threadIdx.x / G;
    // every lane of a wavefront runs the same number of trips, ladder entries and leapfrogs (eval is cooperative)
    const int64_t trips = (a.Mp + ngroups - 1) / ngroups;
    for (int64_t tr = 0; tr < trips; ++tr) {
        const int64_t k = g0 + tr * ngroups;
        const bool live = k < a.Mp;
        const int64_t i = live ? (k * a.M) / a.Mp : 0;
        const double lw = live ? a.logw[i] : -kInf;
        bool excl = !finite_d(lw);
        for (int j = 0; j < a.L; ++j) {
            const double eps = a.ladder[j], heps = 0.5 * eps;
            double xv[DL], rv[DL], gv[DL];
#pragma unroll
            for (int q = 0; q < DL; ++q) {
                const int c = lg + G * q;
                const bool on = live && c < D;
                xv[q] = on ? a.x[i * a.rs + c * a.cs] : 0.0;
                rv[q] = on ? (a.r ? a.r[k * D + c] : stepsize_momentum(a, i, c)) : 0.0;
            }
            double H0, kin = 0.0;
            {
                double gp[DL], gl[DL];
                const double lp0 = probe_logp(model, xv, a.phi, gp, gl);
#pragma unroll
                for (int q = 0; q < DL; ++q) {
                    gv[q] = (lg + G * q < D) ? fma(a.phi, gl[q], gp[q]) : 0.0;
                    kin = fma(rv[q], rv[q], kin);
                }
                H0 = 0.5 * group_sum<G>(kin) - lp0;
                excl = excl || !finite_d(lp0);
            }
            bool done = excl || !live;
            int fb = 0;
            double acc = 0.0;
            for (int t = 1; t <= a.n; ++t) {
                if (__all(done)) break;          // (wavefront-uniform)
                if (!done) {
#pragma unroll
                    for (int q = 0; q < DL; ++q) {
                        rv[q] = fma(heps, gv[q], rv[q]);
                        xv[q] = fma(eps, rv[q], xv[q]);
                    }
                }
                double gp[DL], gl[DL];
                const double lp = probe_logp(model, xv, a.phi, gp, gl);
                kin = 0.0;
#pragma unroll
                for (int q = 0; q < DL; ++q) {
                    if (!done) {
                        gv[q] = (lg + G * q < D) ? fma(a.phi, gl[q], gp[q]) : 0.0;
                        rv[q] = fma(heps, gv[q], rv[q]);
                    }
                    kin = fma(rv[q], rv[q], kin);
                }
                const double H = 0.5 * group_sum<G>(kin) - lp;
                if (!done && !stepsize_step(H - H0, a.delta_max, acc)) {
                    fb = t;
                    done = true;
                }
            }
            if (live && lg == 0) {
                a.accept[(int64_t)j * a.Mp + k] = excl ? 0.0 : acc / (double)a.n;
                a.first_bad[(int64_t)j * a.Mp + k] = excl ? 0 : fb;
            }
        }
        if (live && lg == 0) a.excluded[k] = excl ? 1 : 0;
    }
}

// One thread per probed particle (LaneModel: Model::D coordinates in registers, eval by the lane alone)
template <class Model>
__global__ void __launch_bounds__(256) lane_stepsize_probe_kernel(const double* mdata, StepArgs a) {
    constexpr int D = Model::D;
    Model model;
    model.init(mdata);
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < a.Mp; k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = (k * a.M) / a.Mp;
        const double lw = a.logw[i];
        bool excl = !finite_d(lw);
        for (int j = 0; j < a.L; ++j) {
            const double eps = a.ladder[j], heps = 0.5 * eps;
            double xv[D], rv[D], gv[D], lpri, llik, gp[D], gl[D];
#pragma unroll
            for (int q = 0; q < D; ++q) {
                xv[q] = a.x[i * a.rs + q * a.cs];
                rv[q] = a.r ? a.r[k * D + q] : stepsize_momentum(a, i, q);
            }
            model.eval(xv, lpri, llik, gp, gl);
            double kin = 0.0;
#pragma unroll
            for (int q = 0; q < D; ++q) {
                gv[q] = fma(a.phi, gl[q], gp[q]);
                kin = fma(rv[q], rv[q], kin);
            }
            const double lp0 = lpri + a.phi * llik;
            const double H0 = 0.5 * kin - lp0;
            excl = excl || !finite_d(lp0);
            int fb = 0;
            double acc = 0.0;
            for (int t = 1; t <= a.n && !excl; ++t) {
#pragma unroll
                for (int q = 0; q < D; ++q) {
                    rv[q] = fma(heps, gv[q], rv[q]);
                    xv[q] = fma(eps, rv[q], xv[q]);
                }
                model.eval(xv, lpri, llik, gp, gl);
                kin = 0.0;
#pragma unroll
                for (int q = 0; q < D; ++q) {
                    gv[q] = fma(a.phi, gl[q], gp[q]);
                    rv[q] = fma(heps, gv[q], rv[q]);
                    kin = fma(rv[q], rv[q], kin);
                }
                const double H = 0.5 * kin - (lpri + a.phi * llik);
                if (!stepsize_step(H - H0, a.delta_max, acc)) {
                    fb = t;
                    break;
                }
            }
            a.accept[(int64_t)j * a.Mp + k] = excl ? 0.0 : acc / (double)a.n;
            a.first_bad[(int64_t)j * a.Mp + k] = excl ? 0 : fb;
        }
        a.excluded[k] = excl ? 1 : 0;
    }
}

// part [1 + L][4]: row 0 = (m, Mp, excluded, 0), m the largest finite log-weight probed (-inf: none); row 1 + j =
// (sum w a_j, sum w d_j, sum w, number divergent) over the particles that count, w = exp(logw - m), d_j the pair's
// divergent flag.  ONE block: a thread's terms in index order, then block_sum's fixed tree -- no atomics, so two calls
// give the same bits.
__global__ void __launch_bounds__(kRedBlock) stepsize_reduce_kernel(StepArgs a, double* part) {
    __shared__ double sh[16];
    double mx = -kInf, nex = 0.0;
    for (int64_t k = threadIdx.x; k < a.Mp; k += kRedBlock) {
        const double lw = a.logw[(k * a.M) / a.Mp];
        if (finite_d(lw)) mx = fmax(mx, lw);
        nex += a.excluded[k] ? 1.0 : 0.0;
    }
    mx = block_max(mx, sh);
    nex = block_sum(nex, sh);
    if (threadIdx.x == 0) {
        part[0] = mx;
        part[1] = (double)a.Mp;
        part[2] = nex;
        part[3] = 0.0;
    }
    for (int j = 0; j < a.L; ++j) {
        double v[4] = {0.0, 0.0, 0.0, 0.0};
        for (int64_t k = threadIdx.x; k < a.Mp; k += kRedBlock) {
            if (a.excluded[k]) continue;
            const double w = exp(a.logw[(k * a.M) / a.Mp] - mx);
            const double d = a.first_bad[(int64_t)j * a.Mp + k] != 0 ? 1.0 : 0.0;
            v[0] = fma(w, a.accept[(int64_t)j * a.Mp + k], v[0]);
            v[1] = fma(w, d, v[1]);
            v[2] += w;
            v[3] += d;
        }
        block_sum_n(v, sh);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) part[4 * (1 + j) + q] = v[q];
        }
    }
}

}  // namespace smcn
