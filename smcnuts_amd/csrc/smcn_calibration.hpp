// Calibration of the SMCN_MODEL_GLM families (and SMCN_MODEL_OGLM's with offsets): per (particle, observation) the two
// tails of the predictive law at the observed response, lo = P(Y < y_i | x_p) and up = P(Y > y_i | x_p), and their
// weighted sums OVER PARTICLES per observation under the posterior and the leave-one-out weights -- what the probability
// integral transform and the randomised quantile residuals are finished from (smcnuts_amd/calibration.py).
//
// Shape: pointwise_stats_kernel's (smcn_pointwise.hpp).  The walk hands the functor eta, y and the particle's dispersion
// constants beside the term it has formed; the tails come from glm_tails (smcn_glm_family.hpp), whose prefactor is
// exp(term).  A lane owns an observation, the particle is wave-uniform, so the trip counts of the tail loops differ
// between the lanes of a wavefront: a wavefront stays in a pair for as long as its slowest lane, at most kCalMaxIter
// iterations.  Every statistic accumulates in the lane's own registers: no cross-lane reduction, no LDS, no atomics.
// calibration_combine_kernel merges the slices per observation in slice order (groups of kPwGroup first, then the groups).
//
// Partials (column layout: include/smcnuts_hip.h, smcn_calibration_partials).  lw' = lw - mw, w = exp(lw').  Per
// observation, over the contributing particles whose term is finite and whose tails converged:
//   SW, LO, UP         sum w, sum w lo, sum w up
//   mb, Sb, LOb, UPb   running maximum of lw' - ll, sum exp(lw' - ll - mb), and the same sum times lo and times up
//   ninf, nunc         contributing particles with ll = -inf; with a tail that reached the iteration bound
#pragma once
#include "smcn_pw_walk.hpp"   // the kernels of this file are smcn_loo.hip's

namespace smcn {

constexpr int kCalCols = 9;
enum : int { CAL_SW = 0, CAL_LO, CAL_UP, CAL_MB, CAL_SB, CAL_LOB, CAL_UPB, CAL_NINF, CAL_NUNC };

// lo and up of every pair as out[(t * n + i) * 2 + {0, 1}]: NaN where the term is not finite or a tail did not converge
template <int DPMAX, bool DISP, bool OW = false>
__global__ void __launch_bounds__(64) calibration_points_kernel(PwArgs a, int64_t tiles, double* __restrict__ out) {
    const int64_t tile = blockIdx.x % tiles, slice = blockIdx.x / tiles;
    const int64_t i = tile * 64 + (threadIdx.x & 63u);
    const int fam = a.fam;
    pw_walk<DPMAX, DISP, OW>(
        a, tile, slice, [](int64_t, bool) { return 0.0; },
        [&](int64_t t, double, double, double term, double, double eta, double y, const TauConst& k) {
            double lo = __builtin_nan(""), up = __builtin_nan("");
            bool ok = false;
            if (finite_d(term)) ok = glm_tails(fam, eta, y, term, k, lo, up);
            if (i < a.n) {
                double* const o = out + (t * a.n + i) * 2;
                o[0] = ok ? lo : __builtin_nan("");
                o[1] = ok ? up : __builtin_nan("");
            }
        });
}

// the slices' partials of a tile: part[(slice * kCalCols + col) * npad + i]
template <int DPMAX, bool DISP, bool OW = false>
__global__ void __launch_bounds__(64) calibration_stats_kernel(PwArgs a, int64_t tiles, const double* __restrict__ lw,
                                                               const double* __restrict__ head, double* __restrict__ part) {
    const int64_t tile = blockIdx.x % tiles, slice = blockIdx.x / tiles;
    const int64_t i = tile * 64 + (threadIdx.x & 63u), npad = tiles * 64;
    const double mw = head[0];
    const int fam = a.fam;
    double SW = 0.0, LO = 0.0, UP = 0.0, mb = -kInf, Sb = 0.0, LOb = 0.0, UPb = 0.0, ninf = 0.0, nunc = 0.0;
    pw_walk<DPMAX, DISP, OW>(
        a, tile, slice, [&](int64_t t, bool have) { return have ? lw[t] - mw : -kInf; },
        [&](int64_t, double lwq, double wq, double term, double, double eta, double y, const TauConst& k) {
            const bool fin = term > -kInf;
            ninf += fin ? 0.0 : 1.0;
            double lo = 0.0, up = 0.0;
            bool ok = false;
            if (fin) ok = glm_tails(fam, eta, y, term, k, lo, up);
            nunc += (fin && !ok) ? 1.0 : 0.0;
            const double w = ok ? wq : 0.0;
            lo = ok ? lo : 0.0;
            up = ok ? up : 0.0;
            SW += w;
            LO = fma(w, lo, LO);
            UP = fma(w, up, UP);
            // the leave-one-out weights: the sums of lw' - ll around its running maximum, as pointwise_stats_kernel's Sb
            const double v = lwq - (ok ? term : 0.0), d = v - mb, e = pw_exp_neg(d);
            const bool gt = d > 0.0;
            const double Sn = gt ? fma(Sb, e, 1.0) : Sb + e;
            const double Ln = gt ? fma(LOb, e, lo) : fma(e, lo, LOb);
            const double Un = gt ? fma(UPb, e, up) : fma(e, up, UPb);
            Sb = ok ? Sn : Sb;
            LOb = ok ? Ln : LOb;
            UPb = ok ? Un : UPb;
            mb = (ok && gt) ? v : mb;
        });
    if (i < a.n) {
        double* const o = part + slice * kCalCols * npad + i;
        o[CAL_SW * npad] = SW;
        o[CAL_LO * npad] = LO;
        o[CAL_UP * npad] = UP;
        o[CAL_MB * npad] = mb;
        o[CAL_SB * npad] = Sb;
        o[CAL_LOB * npad] = LOb;
        o[CAL_UPB * npad] = UPb;
        o[CAL_NINF * npad] = ninf;
        o[CAL_NUNC * npad] = nunc;
    }
}

// Merges slice partials of one call (same mw) per observation, in slice order, in pointwise_combine_kernel's two stages:
// stage 1 (FINAL = false) merges the slices of group blockIdx.y into the slices' layout, stage 2 (FINAL = true) merges the
// groups into out[(1 + i) * kCalCols + col], row 0 the header.  calibration.py merges blocks of different calls the same way.
template <bool FINAL>
__global__ void calibration_combine_kernel(const double* __restrict__ part, const double* __restrict__ head, int64_t slices,
                                           int64_t n, int64_t npad, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (FINAL && i == 0) {
        for (int q = 0; q < kCalCols; ++q) out[q] = q < 4 ? head[q] : 0.0;
    }
    if (i >= n) return;
    const int64_t s0 = FINAL ? 0 : (int64_t)blockIdx.y * kPwGroup;
    const int64_t s1 = FINAL ? slices : (s0 + kPwGroup < slices ? s0 + kPwGroup : slices);
    double SW = 0.0, LO = 0.0, UP = 0.0, mb = -kInf, Sb = 0.0, LOb = 0.0, UPb = 0.0, ninf = 0.0, nunc = 0.0;
    for (int64_t s = s0; s < s1; ++s) {
        const double* const o = part + s * kCalCols * npad + i;
        SW += o[CAL_SW * npad];
        LO += o[CAL_LO * npad];
        UP += o[CAL_UP * npad];
        const double m2 = o[CAL_MB * npad], s2 = o[CAL_SB * npad];
        if (s2 > 0.0) {
            const double e = pw_exp_neg(m2 - mb);
            if (m2 > mb) {
                Sb = fma(Sb, e, s2);
                LOb = fma(LOb, e, o[CAL_LOB * npad]);
                UPb = fma(UPb, e, o[CAL_UPB * npad]);
                mb = m2;
            } else {
                Sb = fma(s2, e, Sb);
                LOb = fma(o[CAL_LOB * npad], e, LOb);
                UPb = fma(o[CAL_UPB * npad], e, UPb);
            }
        }
        ninf += o[CAL_NINF * npad];
        nunc += o[CAL_NUNC * npad];
    }
    double* const r = FINAL ? out + (1 + i) * kCalCols : out + (int64_t)blockIdx.y * kCalCols * npad + i;
    const int64_t st = FINAL ? 1 : npad;
    r[CAL_SW * st] = SW;
    r[CAL_LO * st] = LO;
    r[CAL_UP * st] = UP;
    r[CAL_MB * st] = mb;
    r[CAL_SB * st] = Sb;
    r[CAL_LOB * st] = LOb;
    r[CAL_UPB * st] = UPb;
    r[CAL_NINF * st] = ninf;
    r[CAL_NUNC * st] = nunc;
}

}  // namespace smcn
