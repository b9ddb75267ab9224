// Pointwise log-likelihood of the SMCN_MODEL_GLM families (and SMCN_MODEL_OGLM's, eta_i with the row's offset), ll[p, i] = log p(y_i | x_p), and its weighted reductions
// OVER PARTICLES per observation (lppd, WAIC, importance-sampling LOO, fitted values) without ever forming the matrix.
//
// Shape: the transpose of GlmModel<64, 1>.  A LANE owns an observation and keeps its table row in registers (DP <= 16 /
// 32 / 64 doubles: three instantiations), a wavefront owns a tile of 64 observations and walks a slice of the particles
// in chunks of 64: coordinate j of the chunk's 64 particles is ONE coalesced load from the [D][N] state (lane l holds
// particle p0 + l), and particle q's coefficients are read out of those registers as scalars (group_read<64>), so eta
// is DP fused multiply-adds with a scalar operand each.  What depends on a particle alone -- its log-weight, its
// weight, the dispersion families' TauConst -- is formed once per chunk, one particle per lane, and read out the same
// way.  Every statistic accumulates in the lane's own registers: no cross-lane reduction, no LDS, no atomics.  The grid
// is (observation tiles) x (particle slices); pointwise_combine_kernel merges the slices' partials per observation in
// slice order (groups of 16 first, then the groups), so a result depends on its inputs alone (the slice count follows
// from M and n: pointwise_slices).
//
// The per-observation terms are the density functors' own (smcn_glm_family.hpp: glm_canon_obs, which returns the fitted
// value mu / the sigmoid itself, and glm_tau_const / glm_disp_obs), so a term has the bits the density's sum took.
//
// Partials (column layout: include/smcnuts_hip.h, smcn_pointwise_partials).  lw' = lw - mw with mw the largest finite
// log-weight of the call; "contributing" particles are those with finite lw.  Per observation, over the contributing
// particles whose term is finite:
//   ma, Sa        running maximum of lw' + ll and sum exp(lw' + ll - ma)                       (lppd)
//   mb, Sb, Sb2   running maximum of lw' - ll, sum exp(lw' - ll - mb) and sum of its square    (IS-LOO and its ESS)
//   c, SW, S1, S2 the first such term, sum w, sum w (ll - c), sum w (ll - c)^2 with w = exp(lw') (mean and variance)
//   F             sum w E[y | x_p]
//   ninf          how many contributing particles have ll = -inf (the terms are finite or -inf)
#pragma once
#include "smcn_pw_walk.hpp"   // the walk itself and what its callers share: the kernels of this file are smcn_loo.hip's

namespace smcn {

// ll as [M][n] row-major
template <int DPMAX, bool DISP, bool OW = false>
__global__ void __launch_bounds__(64) pointwise_loglik_kernel(PwArgs a, int64_t tiles, double* __restrict__ out) {
    const int64_t tile = blockIdx.x % tiles, slice = blockIdx.x / tiles;
    const int64_t i = tile * 64 + (threadIdx.x & 63u);
    pw_walk<DPMAX, DISP, OW>(
        a, tile, slice, [](int64_t, bool) { return 0.0; },
        [&](int64_t t, double, double, double term, double) {
            if (i < a.n) out[t * a.n + i] = term;
        });
}

// header of a call's partials: {max finite lw, sum exp(lw - max), sum exp(2 (lw - max)), contributing particles}
__global__ void __launch_bounds__(kRedBlock) pointwise_header_kernel(const double* __restrict__ lw, int64_t M,
                                                                     double* __restrict__ head) {
    __shared__ double sh[4];
    double m = -kInf;
    for (int64_t t = threadIdx.x; t < M; t += kRedBlock) {
        const double v = lw[t];
        m = finite_d(v) ? fmax(m, v) : m;
    }
    m = block_max(m, sh);
    double s = 0.0, s2 = 0.0, cn = 0.0;
    for (int64_t t = threadIdx.x; t < M; t += kRedBlock) {
        const double v = lw[t];
        if (finite_d(v)) {
            const double w = pw_exp_neg(v - m);
            s += w;
            s2 += w * w;
            cn += 1.0;
        }
    }
    s = block_sum(s, sh);
    s2 = block_sum(s2, sh);
    cn = block_sum(cn, sh);
    if (threadIdx.x == 0) {
        head[0] = m;
        head[1] = s;
        head[2] = s2;
        head[3] = cn;
    }
}

// the slices' partials of a tile: part[(slice * kPwCols + col) * npad + i]
template <int DPMAX, bool DISP, bool OW = false>
__global__ void __launch_bounds__(64) pointwise_stats_kernel(PwArgs a, int64_t tiles, const double* __restrict__ lw,
                                                             const double* __restrict__ head, double* __restrict__ part) {
    const int64_t tile = blockIdx.x % tiles, slice = blockIdx.x / tiles;
    const int64_t i = tile * 64 + (threadIdx.x & 63u), npad = tiles * 64;
    const double mw = head[0];
    double ma = -kInf, Sa = 0.0, mb = -kInf, Sb = 0.0, Sb2 = 0.0;
    double c = __builtin_nan(""), SW = 0.0, S1 = 0.0, S2 = 0.0, F = 0.0, ninf = 0.0;
    pw_walk<DPMAX, DISP, OW>(
        a, tile, slice, [&](int64_t t, bool have) { return have ? lw[t] - mw : -kInf; },
        [&](int64_t, double lwq, double wq, double term, double mean) {
            const bool fin = term > -kInf;
            ninf += fin ? 0.0 : 1.0;
            const double tf = fin ? term : 0.0, w = fin ? wq : 0.0;
            {   // lppd: log-sum-exp of lw' + ll around its running maximum
                const double v = lwq + tf, d = v - ma, e = pw_exp_neg(d);
                const bool up = d > 0.0;
                const double Sn = up ? fma(Sa, e, 1.0) : Sa + e;
                Sa = fin ? Sn : Sa;
                ma = (fin && up) ? v : ma;
            }
            {   // IS-LOO: the same for lw' - ll, with the sum of squares beside it
                const double v = lwq - tf, d = v - mb, e = pw_exp_neg(d), e2 = e * e;
                const bool up = d > 0.0;
                const double Sn = up ? fma(Sb, e, 1.0) : Sb + e, Qn = up ? fma(Sb2, e2, 1.0) : Sb2 + e2;
                Sb = fin ? Sn : Sb;
                Sb2 = fin ? Qn : Sb2;
                mb = (fin && up) ? v : mb;
            }
            c = (fin && c != c) ? term : c;
            const double dl = fin ? term - c : 0.0, wd = w * dl;
            SW += w;
            S1 += wd;
            S2 = fma(wd, dl, S2);
            F = fin ? fma(w, mean, F) : F;
        });
    if (i < a.n) {
        double* const o = part + slice * kPwCols * npad + i;
        o[PW_MA * npad] = ma;
        o[PW_SA * npad] = Sa;
        o[PW_MB * npad] = mb;
        o[PW_SB * npad] = Sb;
        o[PW_SB2 * npad] = Sb2;
        o[PW_C * npad] = c;
        o[PW_SW * npad] = SW;
        o[PW_S1 * npad] = S1;
        o[PW_S2 * npad] = S2;
        o[PW_F * npad] = F;
        o[PW_NINF * npad] = ninf;
    }
}

// Merges slice partials of one call (same mw: the weights need no rescaling) per observation, in slice order.  Two
// stages, so that no thread walks more than kPwGroup + slices / kPwGroup partials one after the other (every step is a
// lone thread's dependent loads and exponentials, and small n has up to 1024 slices): stage 1 (FINAL = false) merges the
// slices of group g = blockIdx.y, [g kPwGroup, (g + 1) kPwGroup), into the same layout; stage 2 (FINAL = true) merges the
// groups into out[(1 + i) * kPwCols + col], row 0 the header.  The grouping follows from the slice count alone.
// criteria.py merges partials of different calls the same way.
template <bool FINAL>
__global__ void pointwise_combine_kernel(const double* __restrict__ part, const double* __restrict__ head, int64_t slices,
                                         int64_t n, int64_t npad, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (FINAL && i == 0) {
        for (int q = 0; q < kPwCols; ++q) out[q] = q < 4 ? head[q] : 0.0;
    }
    if (i >= n) return;
    const int64_t s0 = FINAL ? 0 : (int64_t)blockIdx.y * kPwGroup;
    const int64_t s1 = FINAL ? slices : (s0 + kPwGroup < slices ? s0 + kPwGroup : slices);
    double ma = -kInf, Sa = 0.0, mb = -kInf, Sb = 0.0, Sb2 = 0.0;
    double c = __builtin_nan(""), SW = 0.0, S1 = 0.0, S2 = 0.0, F = 0.0, ninf = 0.0;
    for (int64_t s = s0; s < s1; ++s) {
        const double* const o = part + s * kPwCols * npad + i;
        {
            const double m2 = o[PW_MA * npad], s2 = o[PW_SA * npad];
            if (s2 > 0.0) {
                const double e = pw_exp_neg(m2 - ma);
                if (m2 > ma) {
                    Sa = fma(Sa, e, s2);
                    ma = m2;
                } else {
                    Sa = fma(s2, e, Sa);
                }
            }
        }
        {
            const double m2 = o[PW_MB * npad], s2 = o[PW_SB * npad], q2 = o[PW_SB2 * npad];
            if (s2 > 0.0) {
                const double e = pw_exp_neg(m2 - mb);
                if (m2 > mb) {
                    Sb = fma(Sb, e, s2);
                    Sb2 = fma(Sb2, e * e, q2);
                    mb = m2;
                } else {
                    Sb = fma(s2, e, Sb);
                    Sb2 = fma(q2, e * e, Sb2);
                }
            }
        }
        // the moments are merged by re-centring the slice's on the first slice's shift
        const double sws = o[PW_SW * npad];
        const double c2 = o[PW_C * npad];
        if (c2 == c2) {
            if (c != c) {
                c = c2;
                S1 = o[PW_S1 * npad];
                S2 = o[PW_S2 * npad];
            } else {
                const double dl = c2 - c, s1 = o[PW_S1 * npad];
                S2 += o[PW_S2 * npad] + dl * (2.0 * s1 + dl * sws);
                S1 += s1 + dl * sws;
            }
        }
        SW += sws;
        F += o[PW_F * npad];
        ninf += o[PW_NINF * npad];
    }
    // stage 1: the group's partial in the slices' layout; stage 2: the observation's row
    double* const r = FINAL ? out + (1 + i) * kPwCols : out + (int64_t)blockIdx.y * kPwCols * npad + i;
    const int64_t st = FINAL ? 1 : npad;
    r[PW_MA * st] = ma;
    r[PW_SA * st] = Sa;
    r[PW_MB * st] = mb;
    r[PW_SB * st] = Sb;
    r[PW_SB2 * st] = Sb2;
    r[PW_C * st] = c;
    r[PW_SW * st] = SW;
    r[PW_S1 * st] = S1;
    r[PW_S2 * st] = S2;
    r[PW_F * st] = F;
    r[PW_NINF * st] = ninf;
}

}  // namespace smcn
