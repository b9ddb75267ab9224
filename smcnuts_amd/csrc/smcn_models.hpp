// Device-native target densities (value + gradient in one pass), evaluated
// cooperatively by the G lanes that own a particle.
//
// Replaces StanModel.logpdf / logpdfgrad (smcnuts/model/bridgestan.py:28-90),
// whose BridgeStan back end is host-only.  Math restated from the .stan text:
// stan_models/arma/arma.stan:14-30, stan_models/PRMwCD/PRMwCD.stan:17-38.
//
// Every model returns the log prior (+ log-Jacobian) and the log likelihood
// separately (log pi_phi = lpri + phi * llik; arma.stan:30), and the two
// gradient parts.
//
// Model concept:
//   static constexpr int  G     lanes per particle
//   static constexpr int  DL    coordinates held per lane
//   static constexpr bool DIST  true: coordinate c = lg + G*i lives on lane lg
//                               false: every lane holds all DL = D coordinates
//   static constexpr int SHARED   doubles of block-shared LDS the model wants
//   static constexpr int MIN_WAVES  waves per SIMD the NUTS kernel is compiled for (register budget)
//   static constexpr int LDS_LEVELS tree-stack levels kept in LDS when the stack itself lives in HBM
//   int  dim()
//   void init(const double* mdata, int lg, double* shared)   all threads of the block
//   void eval(x[DL], lpri, llik, gpri[DL], glik[DL])   all lanes of the group
#pragma once
#include "smcn_device.hpp"
#include "smcn_regdata.hpp"   // where the regression models' tables lie (glm_table_offset and its kin)
#include "smcn_glm_family.hpp"   // the regression families' per-observation terms

namespace smcn {

// ---------------------------------------------------------------------------
// Gaussian family: prior N(0, s0^2 I), optional likelihood N(x | m 1, s1^2 I).
// mdata = [D, s0, has_lik, m, s1].  Coordinates are distributed over lanes.
// ---------------------------------------------------------------------------
template <int G_, int DL_, int LEVELS = 2, int WAVES = 2>
struct GaussModel {
    static constexpr int G = G_, DL = DL_, SHARED = 0, MIN_WAVES = WAVES, LDS_LEVELS = LEVELS;
    static constexpr bool DIST = true;
    int D;
    double inv0, inv1, m, c0, c1;
    bool has;
    bool valid[DL];

    __device__ int dim() const { return D; }
    __device__ void init(const double* md, int lg, double*) {
        D = (int)md[0];
        const double s0 = md[1], s1 = md[4];
        has = md[2] != 0.0;
        m = md[3];
        inv0 = 1.0 / (s0 * s0);
        inv1 = 1.0 / (s1 * s1);
        c0 = -D * log(s0) - 0.5 * D * kLog2Pi;
        c1 = -D * log(s1) - 0.5 * D * kLog2Pi;
#pragma unroll
        for (int i = 0; i < DL; ++i) valid[i] = (lg + G * i) < D;
    }
    // the evaluation in two halves, so that a caller that owns the whole wavefront (G = 64) can put the two sums of
    // squares through ONE butterfly together with its own (the kinetic energy): this lane's share, then the totals
    static constexpr bool HAS_PARTIAL = true;
    __device__ __forceinline__ void eval_partial(const double (&x)[DL], double& ss, double& sl, double (&gp)[DL],
                                                 double (&gl)[DL]) const {
        ss = 0.0; sl = 0.0;
#pragma unroll
        for (int i = 0; i < DL; ++i) {
            const double xi = valid[i] ? x[i] : 0.0;
            const double d = valid[i] ? (x[i] - m) : 0.0;
            ss = fma(xi, xi, ss);
            sl = fma(d, d, sl);
            gp[i] = -xi * inv0;
            gl[i] = has ? -d * inv1 : 0.0;
        }
    }
    // nuts_wave_kernel (smcn_nuts_wave.hpp: one wavefront per particle, candidates by leaf index) is this model's NUTS kernel
    static constexpr bool WAVE_KERNEL = G_ == 64 && DL_ >= 2 && (DL_ % 2) == 0;
    // eval_partial with the two facts of the data that cost selects as compile-time constants: FULL (D = G * DL: every
    // slot is a coordinate) and HAS (there is a likelihood factor).  The same operations in the same order.
    template <bool FULL, bool HAS>
    __device__ __forceinline__ void eval_partial_t(const double (&x)[DL], double& ss, double& sl, double (&gp)[DL],
                                                   double (&gl)[DL]) const {
        ss = 0.0; sl = 0.0;
#pragma unroll
        for (int i = 0; i < DL; ++i) {
            const double xi = (FULL || valid[i]) ? x[i] : 0.0;
            ss = fma(xi, xi, ss);
            gp[i] = -xi * inv0;
            if constexpr (HAS) {
                const double d = (FULL || valid[i]) ? (x[i] - m) : 0.0;
                sl = fma(d, d, sl);
                gl[i] = -d * inv1;
            } else {
                gl[i] = 0.0;
            }
        }
    }
    __device__ __forceinline__ void finish(double ss_total, double sl_total, double& lpri, double& llik) const {
        lpri = -0.5 * ss_total * inv0 + c0;
        llik = has ? -0.5 * sl_total * inv1 + c1 : 0.0;
    }
    __device__ void eval(const double (&x)[DL], double& lpri, double& llik, double (&gp)[DL],
                         double (&gl)[DL]) const {
        double ss, sl;
        eval_partial(x, ss, sl, gp, gl);
        ss = group_sum<G>(ss);
        if (has) sl = group_sum<G>(sl);
        finish(ss, sl, lpri, llik);
    }
};

// ---------------------------------------------------------------------------
// PRMwCD with the particle state DISTRIBUTED over the group (coordinate c on lane c % G): the tree
// state of the NUTS kernel is then DL = ceil(13 / G) doubles per vector and lane instead of 13
// (a replicated form needed > 256 VGPRs and spilled).  One evaluation:
//   1. every lane reads all 13 coordinates from their owners (cross-lane reads),
//   2. lane lg accumulates the likelihood partials of observations lg, lg + G, ..,
//   3. the 13 gradient partials are summed over the group and lane c % G keeps column c,
//   4. prior terms are computed by the lane that owns the coordinate.
// RED must be 2 (see the static_assert below); its default of 0 is kept only because it is part of the template's
// parameter list, and with it of the kernels' mangled names.  Spell RED = 2 out.
// ---------------------------------------------------------------------------
template <int G_, int NOBS, int C_, int RED = 0, int LEVELS = 2, bool FAST = false, int WAVES = 2>
struct PrmwcdDistModel {
    // FAST (round 4; the shipped shape only -- other data take the generic loop): the observation loop unrolled over the
    // lane's S observations with everything that is not arithmetic taken out of it.  The generic loop issues 101
    // instructions per observation for 47 of arithmetic (tools/ubench/prm_eval: 458 cycles per observation, and the
    // launch of BASELINE config 4 is its longest tree's leaf latency): a v_mov_b64 in front of nine of the
    // twelve Horner steps of exp (constants in VGPRs: v_fmac needs its addend in the destination), seventeen selects and
    // compares for `live` and for poisson_lpmf's two edge cases, two branches around the y loads, address arithmetic.
    // Here: design rows padded to S * G_ (all lanes live except in the last pass, whose padded lanes are masked), y in
    // the row's free slot, rows at immediate offsets from one per-lane base, exp's constants as scalar operands
    // (v_fma_f64 with an SGPR pair), and the edge cases decided ONCE behind the loop from max(mu) and
    // min(mu + [y == 0]).  Same operations in the same order for every sum: bit-identical results.
    // RED: how the gradient partials are reduce-scattered; 2 = cross-lane sums only, without LDS scratch (the one form left)
    static_assert(RED == 2, "PrmwcdDistModel: RED = 2 is the only reduce-scatter");
    static constexpr int LDS_LEVELS = LEVELS;             // tree-stack levels kept in LDS (hybrid stack)
    static constexpr int G = G_, C = C_, M = C_ + 1, D_ = C_ + 2, DL = (C_ + 2 + G_ - 1) / G_;
    static constexpr int RS = (C_ + 1 + 1) & ~1;          // design row, padded to an even count
    static constexpr int PR = (D_ + 2) & ~1;              // partial row: 13 -> 14 doubles
    static constexpr int SG = ((NOBS + G_ - 1) / G_) * G_;                   // observations padded to whole passes
    static constexpr int XROWS = FAST ? SG : NOBS;
    static constexpr int DATA = XROWS * RS + 2 * NOBS + (FAST ? 2 * SG : 0);   // design, y, lgamma(y + 1) (+ FAST: [lgamma, y == 0] pairs)
    static constexpr int SHARED = (DATA + 1) & ~1, MIN_WAVES = WAVES;
    static constexpr bool DIST = true;
    static constexpr bool TWO_PHASE = true;               // nuts_kernel: park / resume at a doubling boundary
    // nuts_kernel: its groups (8 particles a wavefront) take a new particle only every 16th loop iteration -- trees of
    // hundreds of leaves lose nothing by the wait, and the groups then do their deep merges in the same iterations
    // (config 4: 1.47 -> 1.52 G leapfrog/s; 2 / 4 / 8 / 16 / 32 / 64 within 1 % of each other)
    static constexpr int STEP_ALIGN = 16;
    static constexpr int S = (NOBS + G - 1) / G;
    // NOBS and C_ are CAPACITIES: the data's own shape (nobs <= NOBS observations, cc <= C_ kernel columns, the
    // shipped file: 100 and 11) is read from mdata; unused design entries are zero, unused coordinates masked
    int lg, nobs, cc;
    double q;
    const double* X;  // [NOBS][RS] in LDS
    const double* y;  // [NOBS]     in LDS

    __device__ int dim() const { return cc + 2; }
    __device__ void init(const double* md, int lg_, double* shared) {
        lg = lg_;
        nobs = (int)md[0];
        cc = (int)md[2];
        q = md[3];
        for (int t = threadIdx.x; t < XROWS * RS; t += blockDim.x) {
            const int i = t / RS, j = t - i * RS;
            double v = (i < nobs && j < cc) ? md[4 + nobs + i * cc + j] : 0.0;
            if (FAST && j == RS - 1) v = i < nobs ? md[4 + i] : 0.0;          // y_i rides in the row's padding slot
            shared[t] = v;
        }
        for (int t = threadIdx.x; t < NOBS; t += blockDim.x) {
            shared[XROWS * RS + t] = t < nobs ? md[4 + t] : 0.0;
            shared[XROWS * RS + NOBS + t] = t < nobs ? lgamma(md[4 + t] + 1.0) : 0.0;   // data-only term of poisson_lpmf
        }
        if constexpr (FAST) {
            static_assert(!FAST || RS > C_, "FAST needs a free slot in the design row (odd column count)");
            for (int t = threadIdx.x; t < SG; t += blockDim.x) {
                shared[XROWS * RS + 2 * NOBS + 2 * t] = t < nobs ? lgamma(md[4 + t] + 1.0) : 0.0;
                shared[XROWS * RS + 2 * NOBS + 2 * t + 1] = (t < nobs && md[4 + t] != 0.0) ? 0.0 : 1.0;
            }
        }
        X = shared;
        y = shared + XROWS * RS;
        __syncthreads();
    }

    // One wavefront per particle (G_ = 64, FAST; the kernel that finishes the long trees a two-phase launch parks): the
    // evaluation built for LATENCY.  Coordinate c lives on lane c; the 13 coefficients are read out as scalars
    // (v_readlane) and enter the FMAs as SGPR operands; lane l evaluates observations l and l + 64 with the unrolled
    // loop's per-observation code; the 12 gradient sums, the log-likelihood and the two prior sums go through four
    // four-value butterflies (wave_sum4) and come back as scalars, which lane c picks its own from.  ~370 wave
    // instructions where the generic evaluation on 64 lanes issued ~1 000.  (The sums are associated differently
    // from the 8-lane kernel's: the same values to rounding -- the short-tree parity tests run with this functor, too -- and, on
    // this target's chaotic trajectories, another equally valid tree: DESIGN.md 2.)
    __device__ bool eval_wave(const double (&x)[DL], double& lpri, double& llik, double (&gp)[DL], double (&gl)[DL]) const {
        if constexpr (G_ == 64 && FAST && DL == 1) {
            if (!(nobs > 64 && nobs <= 2 * 64 && cc == C && q == 0.5)) return false;
            using d2 = double __attribute__((ext_vector_type(2)));
            using lds2 = const __attribute__((address_space(3))) d2*;
            double bs[D_];
#pragma unroll
            for (int j = 0; j < D_; ++j) bs[j] = lane_value(x[0], j);
            const double g = bs[M];
            const double egq = exp_fast(-0.5 * g), eg = egq * egq;
            const lds2 rows = (lds2)(X + lg * RS);
            const lds2 lz = (lds2)(y + 2 * NOBS) + lg;
            double pa[M], pll = 0.0;
#pragma unroll
            for (int j = 0; j < M; ++j) pa[j] = 0.0;
            bool edge = false;
#pragma unroll
            for (int o = 0; o < 2; ++o) {
                double row[RS];
#pragma unroll
                for (int j2 = 0; j2 < RS / 2; ++j2) {
                    const d2 t = rows[(o * 64 * RS) / 2 + j2];
                    row[2 * j2] = t.x; row[2 * j2 + 1] = t.y;
                }
                const d2 aux = lz[o * 64];
                double e = bs[0];
#pragma unroll
                for (int j = 0; j < C; ++j) e = fma(bs[j + 1], row[j], e);
                const double mu = exp_fast_s(e);
                const double yi = row[RS - 1];
                double t1, term;
                {
#pragma clang fp contract(off)
                    t1 = yi * e;
                    term = (t1 - mu) - aux.x;
                }
                double d = yi - mu;
                bool bad = !(mu < kInf) || (mu + aux.y) == 0.0;         // poisson_lpmf: lambda = inf; lambda = 0 with n != 0
                if (o == 1) {                                            // lanes past the data
                    const bool live = lg + 64 < nobs;
                    term = live ? term : 0.0; d = live ? d : 0.0; bad = live && bad;
                }
                edge = edge || bad;
                pll += term;
                pa[0] += d;
#pragma unroll
                for (int j = 0; j < C; ++j) pa[j + 1] = fma(d, row[j], pa[j + 1]);
            }
            // priors on the owning lane (PRMwCD.stan:21, 36-38), as in eval()
            double plp = 0.0, pdg = 0.0, gpl = 0.0;
            if (lg >= 1 && lg < M) {
                const double ab = fabs(x[0]);
                const double apm1 = rsqrt_nr(ab), apow = ab == 0.0 ? 0.0 : ab * apm1;
                const double p = apow * egq;
                plp = -g - p;
                pdg = -1.0 + 0.5 * p;
                const double sgn = (x[0] > 0.0) ? 1.0 : ((x[0] < 0.0) ? -1.0 : 0.0);
                gpl = -0.5 * sgn * apm1 * egq;
            } else if (lg == M) {
                plp = 2.0 * 0.26236426446749105203 - 3.0 * g - 1.3 * eg + g;
                pdg = -3.0 + 1.3 * eg + 1.0;
            }
            double S[16];
            wave_sum4(pa[0], pa[1], pa[2], pa[3], S[0], S[1], S[2], S[3]);
            wave_sum4(pa[4], pa[5], pa[6], pa[7], S[4], S[5], S[6], S[7]);
            wave_sum4(pa[8], pa[9], pa[10], pa[11], S[8], S[9], S[10], S[11]);
            wave_sum4(pll, plp, pdg, 0.0, S[12], S[13], S[14], S[15]);
            double glv = 0.0;
#pragma unroll
            for (int j = 0; j < M; ++j) glv = (lg == j) ? S[j] : glv;
            gl[0] = glv;
            gp[0] = (lg == M) ? S[14] : gpl;
            lpri = S[13];
            llik = (__ballot(edge) != 0ull) ? -kInf : S[12];
            return true;
        }
        return false;
    }

    __device__ void eval(const double (&x)[DL], double& lpri, double& llik, double (&gp)[DL],
                         double (&gl)[DL]) const {
        if constexpr (G_ == 64 && FAST && DL == 1) {
            if (eval_wave(x, lpri, llik, gp, gl)) return;
        }
        // ---- 1. all coordinates to every lane
        double b[PR];
#pragma unroll
        for (int j = 0; j < PR; ++j) b[j] = (j < D_) ? group_read<G>(x[j / G], j % G) : 0.0;
        const int Mr = cc + 1;                             // index of g = log Gamma
        double g = 0.0;
        if (FAST && Mr == M) g = b[M];                     // (the shipped shape: no 13-way select)
        else {
#pragma unroll
            for (int j = 1; j < PR; ++j) g = (j == Mr) ? b[j] : g;
        }
        if (Mr != M) {                                     // (fewer columns than the capacity: g must not meet a zero
#pragma unroll                                             //  design entry as inf * 0)
            for (int j = 1; j < PR; ++j) b[j] = (j < Mr) ? b[j] : 0.0;
        }
        const bool half = q == 0.5;                        // the shipped data; a branch, not a select
        double eg, egq;                                    // 1 / Gamma, Gamma^-q
        if (half) { egq = FAST ? exp_fast_s(-0.5 * g) : exp_fast(-0.5 * g); eg = egq * egq; }
        else { eg = exp(-g); egq = pow(eg, q); }
        // ---- 2. likelihood partials of this lane's observations (PRMwCD.stan:24-33)
        double ll = 0.0, acc[PR];
#pragma unroll
        for (int j = 0; j < PR; ++j) acc[j] = 0.0;
        const int Sr = (nobs + G - 1) / G;
        if (FAST && Sr == S && Mr == M) {      // (the shipped shape; other data take the loop below)
            using d2 = double __attribute__((ext_vector_type(2)));
            using lds2 = const __attribute__((address_space(3))) d2*;
            const lds2 rows = (lds2)(X + lg * RS);                            // this lane's first row; the next G * RS doubles on
            const lds2 lz = (lds2)(y + 2 * NOBS) + lg;                        // [lgamma(y + 1), y == 0] of its observations
            double mumax = 0.0, mmin = 1.0;
            auto one = [&](int k, bool masked) __attribute__((always_inline)) {
                double row[RS];
#pragma unroll
                for (int j2 = 0; j2 < RS / 2; ++j2) {
                    const d2 t = rows[(k * G * RS) / 2 + j2];
                    row[2 * j2] = t.x; row[2 * j2 + 1] = t.y;
                }
                const d2 aux = lz[k * G];
                double e = b[0];
#pragma unroll
                for (int j = 0; j < C; ++j) e = fma(b[j + 1], row[j], e);
                const double mu = exp_fast_s(e);
                const double yi = row[RS - 1];
                double t1, term;
                {
#pragma clang fp contract(off)
                    t1 = yi * e;                                             // (0 for y = 0, as the reference's select)
                    term = (t1 - mu) - aux.x;
                }
                double d = yi - mu, mz = mu + aux.y, mm = mu;
                if (masked) {                                                // the last pass: lanes past the data
                    const bool live = lg + G * k < nobs;
                    term = live ? term : 0.0; d = live ? d : 0.0; mz = live ? mz : 1.0; mm = live ? mm : 0.0;
                }
                mumax = fmax(mumax, mm);
                mmin = fmin(mmin, mz);
                ll += term;
                acc[0] += d;
#pragma unroll
                for (int j = 0; j < C; ++j) acc[j + 1] = fma(d, row[j], acc[j + 1]);
            };
#pragma unroll
            for (int k = 0; k < S; ++k) {
                one(k, k == S - 1 && SG != NOBS);
                if (k & 1) __builtin_amdgcn_sched_barrier(0);                // two observations in flight, not thirteen rows
            }
            // poisson_lpmf's edge cases (lambda = inf; lambda = 0 with n != 0), once: -inf as the reference
            if (!(mumax < kInf) || mmin == 0.0) ll = -kInf;
        } else
#pragma unroll 1
        for (int k = 0; k < Sr; ++k) {
            const int i = lg + G * k;
            const bool live = i < nobs;
            const double* row = X + (live ? i : 0) * RS;
            double eta = b[0];
#pragma unroll
            for (int j = 0; j < C; ++j) eta = fma(b[j + 1], row[j], eta);
            const double mu = exp_fast(eta);
            const double yi = live ? y[i] : 0.0;
            double term = (yi == 0.0 ? 0.0 : yi * eta) - mu - (live ? y[NOBS + i] : 0.0);
            term = (mu == 0.0 && yi != 0.0) ? -kInf : term;              // lambda == 0, n != 0
            term = finite_d(mu) ? term : -kInf;                          // poisson_lpmf(y | inf)
            const double d = live ? (yi - mu) : 0.0;
            ll += live ? term : 0.0;
            acc[0] += d;
#pragma unroll
            for (int j = 0; j < C; ++j) acc[j + 1] = fma(d, row[j], acc[j + 1]);
        }
        // ---- 3. reduce-scatter of the gradient partials: lane c % G ends with the sum of column c
#pragma unroll
        for (int j = 0; j < D_; ++j) acc[j] = group_sum<G>(acc[j]);
#pragma unroll
        for (int i = 0; i < DL; ++i) {
            double v = 0.0;
#pragma unroll
            for (int j = i * G; j < (i + 1) * G && j < D_; ++j) v = (j - i * G == lg) ? acc[j] : v;
            gl[i] = v;
        }
        // ---- 4. priors on the owning lane: inv_gamma(Gamma | 2, 1.3) + Jacobian for g,
        //         exponential-power terms for Beta_2..Beta_M (:36-38); Beta_1 is flat
        double lp = 0.0, dg = 0.0;
#pragma unroll
        for (int i = 0; i < DL; ++i) {
            const int c = lg + G * i;
            gp[i] = 0.0;
            if (c >= 1 && c < Mr) {
                const double ab = fabs(x[i]);
                double apow, apm1;                                         // |Beta_j|^q, |Beta_j|^(q-1)
                if (half) { apm1 = rsqrt_nr(ab); apow = ab == 0.0 ? 0.0 : ab * apm1; }
                else { apow = pow(ab, q); apm1 = apow / ab; }
                const double p = apow * egq;                               // (|Beta_j| / Gamma)^q
                lp += -g - p;
                dg += -1.0 + q * p;
                const double sgn = (x[i] > 0.0) ? 1.0 : ((x[i] < 0.0) ? -1.0 : 0.0);
                gp[i] = -q * sgn * apm1 * egq;                             // -q sgn |b|^(q-1) e^(-gq)
            } else if (c == Mr) {
                lp += 2.0 * 0.26236426446749105203 - 3.0 * g - 1.3 * eg + g;   // lgamma(2) = 0
                dg += -3.0 + 1.3 * eg + 1.0;
            }
        }
        llik = group_sum<G>(ll);
        lpri = group_sum<G>(lp);
        dg = group_sum<G>(dg);
#pragma unroll
        for (int i = 0; i < DL; ++i)
            if (lg + G * i == Mr) gp[i] = dg;
    }
};

// ---------------------------------------------------------------------------
// Flat GLM (SMCN_MODEL_GLM, SMCN_MODEL_OGLM): the likelihood of a linear predictor eta = X beta (+ intercept),
// independent Gaussian priors N(0, s_c^2) on the Dc <= 64 coefficients.  Two compile-time parameters:
//   DISP  false: the canonical-link families, 0 bernoulli_logit and 1 poisson_log; x = (b_1..b_Dc), D = Dc.
//         true:  the families with a dispersion coordinate, 2 normal and 3 neg_binomial_2_log (smcn_glm_family.hpp);
//                x = (b_1..b_Dc, tau), D = Dc + 1, tau last and unconstrained, prior N(m_tau, s_tau^2) on tau (= a
//                lognormal prior on sigma / phi = e^tau with its Jacobian).  tau is read like any coordinate and its
//                gradient is one more sum over the observations, which lands on the lane that owns coordinate Dc.
//                Everything that depends on tau alone is formed once per evaluation (TauConst).
//   OW    true:  per-observation offsets and weights (SMCN_MODEL_OGLM),
//                eta_i = [b_0 +] X_i b + o_i,   llik = sum_i w_i l(y_i | eta_i [, tau]),   grad = sum_i w_i d_i X_i
//                (tau: sum_i w_i gt_i).
// What differs is behind `if constexpr`: every instantiation compiles to the instruction stream it had when the four were
// separate structs (GlmModel, GlmDispModel, GlmOffModel, GlmOffDispModel; tools/asm_compare.py,
// profiles/glm_family_merge_asm.txt).  Within a pair the family is a wave-uniform runtime branch.
// The density works on the table reg_repack (smcn_regdata.hpp) lays behind the caller's data (glm_table_offset;
// oglm_table_offset: the same place whatever the flags): a row per observation, [1 (intercept only), X_i1 .. X_ip,
// 0 (to an even column count DP), y_i, lgamma(y_i + 1) (unused by `normal`)], RS = DP + 2 doubles, at a 128-byte
// boundary, zero rows up to a multiple of 64 -- every lane reads whole rows, unmasked, with 16-byte loads.  The design
// stays in global memory (L2 / Infinity Cache): the G lanes of every particle group of a wavefront read the same rows in
// the same instructions (nuts_kernel's lock step), so a row is fetched once per wavefront.
// OW rows are [.., y_i, lgamma(y_i + 1), o_i, w_i], RS = DP + 4 doubles; o_i = 0 and w_i = 1 where the caller gave none,
// and the kernels always read both.  A padding row is all zero, so its weight is 0: `w != 0` is the one test for "this row
// counts", and a row that does not count adds exactly 0 to every sum whatever its term is (-inf or NaN included: e^eta
// may overflow there) -- it is selected out, not multiplied out.
//   G = 8:  coordinate c on lane c % 8; every lane gathers the Dc coefficients, lane lg evaluates observations
//           lg, lg + 8, .. and the gradient partials are reduce-scattered over the group.  D <= 16 with two coordinates
//           per lane (canonical; its NUTS kernel is at 246 VGPRs), D <= 8 with one (DISP: the two-coordinate form spills).
//   G = 64: one particle per wavefront, coordinate c on lane c, D <= 64.  Observations go in chunks of 64, one per lane:
//           eta with the coefficients read out as scalars (v_readlane), then the chunk's 64 residuals read out
//           the same way and lane c accumulates column c of the chunk's rows -- the column sums come out on the
//           lane that owns the coordinate, with no butterfly at all.
// ---------------------------------------------------------------------------
template <int G_, int DL_, bool DISP = false, bool OW = false>
struct GlmModel {
    static constexpr int G = G_, DL = DL_, SHARED = 0, MIN_WAVES = 2, LDS_LEVELS = 2;
    static constexpr bool DIST = true;
    static constexpr int DMAX = G_ * DL_;
    static_assert(G_ == 64 ? DL_ == 1 : (DMAX % 2) == 0, "GlmModel: 64 lanes with one coordinate each, or an even capacity");
    static constexpr int HEAD = OW ? 5 : 4;   // doubles of the data block in front of the priors
    using d2 = double __attribute__((ext_vector_type(2)));
    int lg, D, Dc, DP, RS, n;
    bool alt;             // the pair's second family: poisson_log, or (DISP) neg_binomial_2_log
    const double* T;      // the repacked table
    double mc[DL], inv_s2[DL], lc[DL];   // (DISP) prior mean; 1 / s^2 and -log s - log(2 pi) / 2 of the lane's coordinates (0 beyond D)

    __device__ int dim() const { return D; }
    __device__ void init(const double* md, int lg_, double*) {
        lg = lg_;
        alt = DISP ? md[0] == 3.0 : md[0] != 0.0;
        n = (int)md[1];
        const int p = (int)md[2];
        Dc = p + (int)md[3];
        D = DISP ? Dc + 1 : Dc;
        DP = (Dc + 1) & ~1;
        RS = OW ? oglm_row_doubles(Dc) : glm_row_doubles(Dc);
        const int npri = DISP ? Dc + 2 : Dc;
        T = md + (OW ? oglm_table_offset(npri, n, p) : glm_table_offset(npri, n, p));
#pragma unroll
        for (int i = 0; i < DL; ++i) {
            const int c = lg + G * i;
            const double s = c < Dc ? md[HEAD + c] : ((DISP && c == Dc) ? md[HEAD + 1 + Dc] : 1.0);
            if constexpr (DISP) mc[i] = c == Dc ? md[HEAD + Dc] : 0.0;
            inv_s2[i] = c < D ? 1.0 / (s * s) : 0.0;
            lc[i] = c < D ? -log(s) - 0.5 * kLog2Pi : 0.0;
        }
    }
    // one observation: log-likelihood term, d term / d eta and (DISP) d term / d tau
    __device__ __forceinline__ void obs(const TauConst& k, double eta, d2 yl, double& term, double& d, double& g) const {
        if constexpr (DISP) {
            glm_disp_obs(alt, k, eta, yl.x, yl.y, term, d, g);
        } else {
            double mean;
            glm_canon_obs(alt, eta, yl.x, yl.y, term, mean);
            d = yl.x - mean;
        }
    }
    // (OW) o_i and w_i of a row.  Spelled at every use, not held in a local: it is one load either way, and a local that
    // the plain instantiations declare without using it changed their register allocation.
    __device__ __forceinline__ d2 ow(const d2* row) const { return row[(DP >> 1) + 1]; }
    // a row's share v of a sum: weighted (OW), and exactly 0 -- selected out, not multiplied out -- where the row does not
    // count
    __device__ __forceinline__ double share(bool live, const d2* row, double v) const {
        if constexpr (OW) v = ow(row).y * v;
        return live ? v : 0.0;
    }
    __device__ void eval(const double (&x)[DL], double& lpri, double& llik, double (&gp)[DL], double (&gl)[DL]) const {
        double ll = 0.0, lp = 0.0, gt = 0.0;
#pragma unroll
        for (int i = 0; i < DL; ++i) {
            double v = x[i];
            if constexpr (DISP) v = x[i] - mc[i];
            gp[i] = -v * inv_s2[i];
            lp += fma(-0.5 * v, v * inv_s2[i], lc[i]);
        }
        TauConst k{};
        if constexpr (DISP) {
            double xt = x[0];
#pragma unroll
            for (int i = 1; i < DL; ++i) xt = Dc / G == i ? x[i] : xt;
            k = glm_tau_const(alt, group_read<G>(xt, Dc % G));
        }
        if constexpr (G_ == 64) {
            // (four accumulators for the column sums and two for eta: one wavefront per SIMD is all the tree stack in LDS
            //  leaves room for, so dependent FMA chains are not hidden behind other wavefronts)
            double acc[4] = {0.0, 0.0, 0.0, 0.0};
            const int col = lg < DP ? lg : 0;
            const double xb = (!DISP || lg < Dc) ? x[0] : 0.0;   // (DISP: tau is not a coefficient: 0 on the pad column)
            for (int k0 = 0; k0 < n; k0 += 64) {
                const d2* const row = (const d2*)(T + (int64_t)(k0 + lg) * RS);
                double e0 = 0.0, e1 = 0.0;
                for (int j = 0; j < DP; j += 2) {          // (j wave-uniform: the coefficients are scalar operands)
                    const d2 v = row[j >> 1];
                    e0 = fma(group_read<64>(xb, j), v.x, e0);
                    e1 = fma(group_read<64>(xb, j + 1), v.y, e1);
                }
                const d2 yl = row[DP >> 1];
                double e = e0 + e1;
                if constexpr (OW) e += ow(row).x;
                double term, d, g;
                obs(k, e, yl, term, d, g);
                const bool live = OW ? ow(row).y != 0.0 : k0 + lg < n;   // (OW: a padding row's weight is 0)
                ll += share(live, row, term);
                if constexpr (DISP) gt += share(live, row, g);
                d = share(live, row, d);
                // column `lg` of the chunk's 64 rows, weighted by their residuals (read out as scalars)
                const double* const colp = T + (int64_t)k0 * RS + col;
#pragma unroll 16
                for (int i = 0; i < 64; ++i) acc[i & 3] = fma(lane_value(d, i), colp[(int64_t)i * RS], acc[i & 3]);
            }
            double L, P, GT, u1;
            // (the lane's column sum in front of the wave-wide sums, or behind them where tau's lane takes one of them: each
            //  case in the statement order its kernels have always been compiled from -- the other order moves registers)
            if constexpr (!DISP) gl[0] = lg < Dc ? (acc[0] + acc[1]) + (acc[2] + acc[3]) : 0.0;
            wave_sum4(ll, lp, gt, 0.0, L, P, GT, u1);
            if constexpr (DISP) gl[0] = lg < Dc ? (acc[0] + acc[1]) + (acc[2] + acc[3]) : (lg == Dc ? GT : 0.0);
            llik = (DISP && k.bad) ? -kInf : L;
            lpri = P;
        } else {
            // ---- 1. the Dc coefficients to every lane of the group (DISP: 0 in tau's slot and beyond)
            double b[DMAX];
#pragma unroll
            for (int j = 0; j < DMAX; ++j) {
                const double v = group_read<G>(x[j / G], j % G);
                b[j] = (!DISP || j < Dc) ? v : 0.0;
            }
            // ---- 2. this lane's observations lg, lg + G, ..
            double acc[DMAX];
#pragma unroll
            for (int j = 0; j < DMAX; ++j) acc[j] = 0.0;
            const int S = (n + G - 1) / G;
#pragma unroll 1
            for (int kk = 0; kk < S; ++kk) {
                const int i = lg + G * kk;
                const d2* const row = (const d2*)(T + (int64_t)i * RS);
                double e = 0.0;
#pragma unroll
                for (int j2 = 0; j2 < DMAX / 2; ++j2) {
                    if (2 * j2 < DP) {                    // (DP wave-uniform)
                        const d2 v = row[j2];
                        e = fma(b[2 * j2], v.x, e);
                        e = fma(b[2 * j2 + 1], v.y, e);
                    }
                }
                const d2 yl = row[DP >> 1];
                if constexpr (OW) e += ow(row).x;
                double term, d, g;
                obs(k, e, yl, term, d, g);
                const bool live = OW ? ow(row).y != 0.0 : i < n;
                ll += share(live, row, term);
                if constexpr (DISP) gt += share(live, row, g);
                d = share(live, row, d);
                // (the row again, from the cache: holding it across the residual costs 2 DMAX registers)
#pragma unroll
                for (int j2 = 0; j2 < DMAX / 2; ++j2) {
                    if (2 * j2 < DP) {
                        const d2 v = row[j2];
                        acc[2 * j2] = fma(d, v.x, acc[2 * j2]);
                        acc[2 * j2 + 1] = fma(d, v.y, acc[2 * j2 + 1]);
                    }
                }
            }
            // ---- 3. reduce-scatter of the gradient partials: lane c % G ends with the sum of column c; (DISP) tau's sum
            //         to the lane that owns coordinate Dc
            const int nsum = DISP ? Dc : DP;
#pragma unroll
            for (int j = 0; j < DMAX; ++j) acc[j] = j < nsum ? group_sum<G>(acc[j]) : 0.0;
            double GT = 0.0;
            if constexpr (DISP) GT = group_sum<G>(gt);
#pragma unroll
            for (int i = 0; i < DL; ++i) {
                double v = 0.0;
#pragma unroll
                for (int j = i * G; j < (i + 1) * G; ++j) v = (j - i * G == lg) ? acc[j] : v;
                const int c = lg + G * i;
                gl[i] = c < Dc ? v : ((DISP && c == Dc) ? GT : 0.0);
            }
            llik = (DISP && k.bad) ? -kInf : group_sum<G>(ll);
            lpri = group_sum<G>(lp);
        }
    }
};

// ---------------------------------------------------------------------------
// Varying-intercept (hierarchical) GLM, non-centred (SMCN_MODEL_HGLM): Dc = p + intercept fixed coefficients b, J groups,
// group index g_i of observation i,
//   eta_i = [b_0 +] X_i b + e^lt z_{g_i},   y_i ~ family(eta_i [, e^ld])   (the four SMCN_MODEL_GLM families, same terms)
//   b_c ~ N(0, s_c^2), z_j ~ N(0, 1), tau = e^lt ~ half-normal(s_tau) with its Jacobian, ld ~ N(m_d, s_d^2) (families 2, 3).
// x = (b_1..b_Dc, z_1..z_J, lt [, ld]), D = Dc + J + 1 (+ 1) <= 64; one wavefront per particle, coordinate c on lane c.
// The table reg_repack lays behind the caller's block: a row per observation, [1 (intercept), X_i1 .. X_ip,
// 0 (to an even count DP), y_i, lgamma(y_i + 1), g_i, 0], RS = DP + 4 doubles, at a 128-byte boundary, zero rows up to a
// multiple of 64.  Lane l takes row k0 + l of each 64-row chunk, as GlmModel<64, 1>:
//   eta: the fixed part with the coefficients read out as scalars, the group part with ONE cross-lane read (ds_bpermute)
//        of z from lane Dc + g_i;
//   the 64-step read-out of the chunk's residuals: lane c < Dc accumulates d_i X_ic, lane Dc + j accumulates d_i [g_i == j]
//        (the broadcast group index compared with its own j; no column load), multiplied by e^lt once at the end;
//   d / d lt = sum_i d_i alpha_{g_i} (a per-lane term) and the dispersion sum go through wave_sum4 with llik and lpri.
// The per-observation terms are the flat GLM's (smcn_glm_family.hpp).  Non-finite: the GLM rules, and -inf (lpri and
// llik) when e^(2 lt) overflows.
// ---------------------------------------------------------------------------
template <int G_, int DL_>
struct GlmHierModel {
    static_assert(G_ == 64 && DL_ == 1, "GlmHierModel: one wavefront per particle, one coordinate per lane");
    static constexpr int G = G_, DL = DL_, SHARED = 0, MIN_WAVES = 2, LDS_LEVELS = 2;
    static constexpr bool DIST = true;
    using d2 = double __attribute__((ext_vector_type(2)));
    bool poisson, nb;             // family 1 among the canonical pair 0 / 1, family 3 among the dispersion pair 2 / 3
    int lg, D, Dc, J, DP, RS, n;
    int role;                     // this lane's coordinate: 0 coefficient, 1 group z_j, 2 lt, 3 ld, 4 none
    bool hasd;
    const double* T;              // the repacked table
    double mc, inv_s2, lc;        // prior of the lane's coordinate: mean, 1 / s^2, constant

    __device__ int dim() const { return D; }
    __device__ void init(const double* md, int lg_, double*) {
        lg = lg_;
        const double fam = md[0];
        hasd = fam >= 2.0;
        poisson = fam == 1.0;
        nb = fam == 3.0;
        n = (int)md[1];
        const int p = (int)md[2];
        Dc = p + (int)md[3];
        J = (int)md[4];
        D = Dc + J + 1 + (hasd ? 1 : 0);
        DP = (Dc + 1) & ~1;
        RS = hglm_row_doubles(Dc);
        T = md + hglm_table_offset(hglm_head(Dc, hasd), n, p);
        role = lg < Dc ? 0 : (lg < Dc + J ? 1 : (lg == Dc + J ? 2 : (lg < D ? 3 : 4)));
        double s = 1.0;
        mc = 0.0;
        if (role == 0) s = md[5 + lg];
        else if (role == 2) s = md[5 + Dc];
        else if (role == 3) { mc = md[6 + Dc]; s = md[7 + Dc]; }
        inv_s2 = role < 4 ? 1.0 / (s * s) : 0.0;
        // half-normal on tau with the Jacobian of lt = log tau: log 2 - log s_tau - log(2 pi) / 2 (+ lt - e^2lt / 2 s_tau^2)
        lc = role == 2 ? (0.69314718055994530942 - log(s)) - 0.5 * kLog2Pi : (role < 4 ? -log(s) - 0.5 * kLog2Pi : 0.0);
    }
    __device__ void eval(const double (&x)[DL], double& lpri, double& llik, double (&gp)[DL], double (&gl)[DL]) const {
        // ---- everything that depends on lt or ld alone, once
        const double lt = group_read<64>(x[0], Dc + J);
        const double tau = exp_fast(lt), e2 = tau * tau;
        const bool bad = !(e2 < kInf);                     // e^(2 lt) overflows
        const auto k = glm_tau_const(nb, hasd ? group_read<64>(x[0], Dc + J + 1) : 0.0);
        // ---- prior of the lane's coordinate
        double lp, g0;
        if (role == 2) {
            lp = (lc + lt) - 0.5 * e2 * inv_s2;
            g0 = fma(-e2, inv_s2, 1.0);
        } else {
            const double v = x[0] - mc;
            g0 = -v * inv_s2;
            lp = fma(-0.5 * v, v * inv_s2, lc);
        }
        // ---- observations, 64 a chunk
        double acc[4] = {0.0, 0.0, 0.0, 0.0}, ll = 0.0, gt = 0.0, ga = 0.0;
        const int col = lg < DP ? lg : 0;
        const bool grp = role == 1;
        const int jl = lg - Dc;                            // (group lanes) this lane's j
        const double xb = lg < Dc ? x[0] : 0.0;            // (0 on the pad column)
        for (int k0 = 0; k0 < n; k0 += 64) {
            const d2* const row = (const d2*)(T + (int64_t)(k0 + lg) * RS);
            double e0 = 0.0, e1 = 0.0;
            for (int j = 0; j < DP; j += 2) {              // (j wave-uniform: the coefficients are scalar operands)
                const d2 v = row[j >> 1];
                e0 = fma(group_read<64>(xb, j), v.x, e0);
                e1 = fma(group_read<64>(xb, j + 1), v.y, e1);
            }
            const d2 yl = row[DP >> 1];
            const int gi = (int)row[(DP >> 1) + 1].x;
            const double a = tau * __shfl(x[0], Dc + gi, 64);   // alpha_{g_i}
            const double e = (e0 + e1) + a;
            double term, d, g = 0.0;
            if (hasd) {
                glm_disp_obs(nb, k, e, yl.x, yl.y, term, d, g);
            } else {
                double mean;
                glm_canon_obs(poisson, e, yl.x, yl.y, term, mean);
                d = yl.x - mean;
            }
            const bool live = k0 + lg < n;
            ll += live ? term : 0.0;
            gt += live ? g : 0.0;
            d = live ? d : 0.0;
            ga = fma(d, a, ga);
            // the chunk's 64 residuals read out as scalars: column `lg` of their rows, or their group indicator
            const double* const colp = T + (int64_t)k0 * RS + col;
#pragma unroll 16
            for (int i = 0; i < 64; ++i) {
                const double w = grp ? (__builtin_amdgcn_readlane(gi, i) == jl ? 1.0 : 0.0) : colp[(int64_t)i * RS];
                acc[i & 3] = fma(lane_value(d, i), w, acc[i & 3]);
            }
        }
        double L, P, GT, GA;
        wave_sum4(ll, lp, gt, ga, L, P, GT, GA);
        const double cs = (acc[0] + acc[1]) + (acc[2] + acc[3]);
        gl[0] = role == 0 ? cs : (role == 1 ? tau * cs : (role == 2 ? GA : (role == 3 ? GT : 0.0)));
        gp[0] = g0;
        llik = (bad || k.bad) ? -kInf : L;
        lpri = bad ? -kInf : P;
    }
};

// ---------------------------------------------------------------------------
// Multilevel GLM, non-centred (SMCN_MODEL_MLGLM): Dc = p + intercept fixed coefficients b and R <= 4 independent varying
// terms; term r has J_r levels, a level g_ir and a multiplier z_ir per observation (1: varying intercept, a covariate:
// varying slope; two terms may share a factor),
//   eta_i = [b_0 +] X_i b + sum_r z_ir e^lt_r u_{r,g_ir},   y_i ~ family(eta_i [, e^ld])   (the SMCN_MODEL_GLM families)
//   b_c ~ N(0, s_c^2), u_rj ~ N(0, 1), e^lt_r ~ half-normal(s_tau_r) with its Jacobian, ld ~ N(m_d, s_d^2) (families 2, 3).
// x = (b_1..b_Dc, u_1,1..u_1,J1, .., u_R,1..u_R,JR, lt_1..lt_R [, ld]), D = Dc + sum J_r + R (+ 1) <= 64; one wavefront
// per particle, coordinate c on lane c.  With R = 1 and z = 1 this is GlmHierModel's density, term for term.
// The table: a row per observation, [1 (intercept), X_i1 .. X_ip, 0 (to an even count DP), y_i, lgamma(y_i + 1), g_1i, z_1i,
// .., g_Ri, z_Ri], RS = DP + 2 + 2R doubles, at a 128-byte boundary, zero rows up to a multiple of 64.  The shape is
// GlmHierModel's -- lane l takes row k0 + l of each 64-row chunk:
//   eta: the fixed part with the coefficients as scalars, then per term one cross-lane read (ds_bpermute) of u from its
//        owner, lane off_r + g_ir, times e^lt_r, times z_ir;
//   the 64-step read-out: in the first pass lane c < Dc accumulates d_i X_ic while the owners of term 1's u compare the
//        broadcast key off_1 + g_1i with their own lane index and accumulate d_i z_1i; terms 2..R take a pass each over
//        the broadcast (key, d_i z_ri) -- no lane has to find out which term it belongs to first.  e^lt_r multiplies the
//        sum at the end;
//   d / d lt_r = sum_i d_i z_ir e^lt_r u_{r,g_ir} is a per-lane term: with llik, lpri and the dispersion sum up to seven
//        wave-wide sums, one wave_sum4 for R = 1 (GlmHierModel's) and a second one for terms 2..R.
// The terms' registers are arrays with compile-time indices under guards on the wave-uniform R (a private array indexed
// at run time would be placed in scratch).  Non-finite: -inf (lpri and llik) when any e^(2 lt_r) overflows, then the GLM
// rules.
// ---------------------------------------------------------------------------
template <int G_, int DL_>
struct GlmMultiModel {
    static_assert(G_ == 64 && DL_ == 1, "GlmMultiModel: one wavefront per particle, one coordinate per lane");
    static constexpr int G = G_, DL = DL_, SHARED = 0, MIN_WAVES = 2, LDS_LEVELS = 2;
    static constexpr bool DIST = true;
    static constexpr int RM = kMlMaxTerms;
    using d2 = double __attribute__((ext_vector_type(2)));
    bool poisson, nb;             // family 1 among the canonical pair 0 / 1, family 3 among the dispersion pair 2 / 3
    int lg, D, Dc, R, LT0, DP, RS, n;
    int off[RM];                  // first lane of term r's u (wave-uniform)
    int role;                     // this lane's coordinate: 0 coefficient, 1 a level's u, 2 an lt, 3 ld, 4 none
    int tr;                       // (roles 1, 2) the lane's term
    bool hasd;
    const double* T;              // the repacked table
    double mc, inv_s2, lc;        // prior of the lane's coordinate: mean, 1 / s^2, constant

    __device__ int dim() const { return D; }
    __device__ void init(const double* md, int lg_, double*) {
        lg = lg_;
        const double fam = md[0];
        hasd = fam >= 2.0;
        poisson = fam == 1.0;
        nb = fam == 3.0;
        n = (int)md[1];
        const int p = (int)md[2];
        Dc = p + (int)md[3];
        R = (int)md[4];
        int o = Dc;
        tr = 0;
#pragma unroll
        for (int r = 0; r < RM; ++r) {
            off[r] = o;
            o += r < R ? (int)md[5 + r] : 0;
            tr = (r < R && lg >= off[r]) ? r : tr;             // (u lanes: the last term that starts at or before lg)
        }
        LT0 = o;
        D = LT0 + R + (hasd ? 1 : 0);
        DP = (Dc + 1) & ~1;
        RS = mlglm_row_doubles(Dc, R);
        T = md + mlglm_table_offset(mlglm_head(Dc, R, hasd), R, n, p);
        role = lg < Dc ? 0 : (lg < LT0 ? 1 : (lg < LT0 + R ? 2 : (lg < D ? 3 : 4)));
        tr = role == 2 ? lg - LT0 : tr;
        double s = 1.0;
        mc = 0.0;
        if (role == 0) s = md[9 + lg];
        else if (role == 2) s = md[9 + Dc + tr];
        else if (role == 3) { mc = md[9 + Dc + R]; s = md[10 + Dc + R]; }
        inv_s2 = role < 4 ? 1.0 / (s * s) : 0.0;
        // half-normal on e^lt_r with the Jacobian of lt_r: log 2 - log s_tau_r - log(2 pi) / 2 (+ lt - e^2lt / 2 s_tau_r^2)
        lc = role == 2 ? (0.69314718055994530942 - log(s)) - 0.5 * kLog2Pi : (role < 4 ? -log(s) - 0.5 * kLog2Pi : 0.0);
    }
    __device__ void eval(const double (&x)[DL], double& lpri, double& llik, double (&gp)[DL], double (&gl)[DL]) const {
        // ---- everything that depends on the lt_r or ld alone, once
        double tau[RM], e2o = 0.0, tauo = 0.0;                 // (e2o, tauo: the lane's own term's)
        bool bad = false;
#pragma unroll
        for (int r = 0; r < RM; ++r) {
            tau[r] = 0.0;
            if (r < R) {
                tau[r] = exp_fast(group_read<64>(x[0], LT0 + r));
                const double e2 = tau[r] * tau[r];
                bad = bad || !(e2 < kInf);                     // e^(2 lt_r) overflows
                e2o = tr == r ? e2 : e2o;
                tauo = tr == r ? tau[r] : tauo;
            }
        }
        const auto k = glm_tau_const(nb, hasd ? group_read<64>(x[0], LT0 + R) : 0.0);
        // ---- prior of the lane's coordinate
        double lp, g0;
        if (role == 2) {
            lp = (lc + x[0]) - 0.5 * e2o * inv_s2;
            g0 = fma(-e2o, inv_s2, 1.0);
        } else {
            const double v = x[0] - mc;
            g0 = -v * inv_s2;
            lp = fma(-0.5 * v, v * inv_s2, lc);
        }
        // ---- observations, 64 a chunk
        double acc[4] = {0.0, 0.0, 0.0, 0.0}, ll = 0.0, gt = 0.0, ga[RM] = {0.0, 0.0, 0.0, 0.0};
        const int col = lg < DP ? lg : 0;
        const bool grp = role == 1;
        const double xb = lg < Dc ? x[0] : 0.0;            // (0 on the pad column)
        for (int k0 = 0; k0 < n; k0 += 64) {
            const d2* const row = (const d2*)(T + (int64_t)(k0 + lg) * RS);
            double e0 = 0.0, e1 = 0.0;
            for (int j = 0; j < DP; j += 2) {              // (j wave-uniform: the coefficients are scalar operands)
                const d2 v = row[j >> 1];
                e0 = fma(group_read<64>(xb, j), v.x, e0);
                e1 = fma(group_read<64>(xb, j + 1), v.y, e1);
            }
            const d2 yl = row[DP >> 1];
            int key[RM];                                   // the lane that owns u_{r, g_ir}
            double z[RM], a[RM], as = 0.0;
#pragma unroll
            for (int r = 0; r < RM; ++r) {
                key[r] = 0, z[r] = 0.0, a[r] = 0.0;
                if (r < R) {
                    const d2 gz = row[(DP >> 1) + 1 + r];
                    key[r] = off[r] + (int)gz.x;
                    z[r] = gz.y;
                    a[r] = (tau[r] * __shfl(x[0], key[r], 64)) * z[r];
                    as = r == 0 ? a[0] : as + a[r];
                }
            }
            const double e = (e0 + e1) + as;
            double term, d, g = 0.0;
            if (hasd) {
                glm_disp_obs(nb, k, e, yl.x, yl.y, term, d, g);
            } else {
                double mean;
                glm_canon_obs(poisson, e, yl.x, yl.y, term, mean);
                d = yl.x - mean;
            }
            const bool live = k0 + lg < n;
            ll += live ? term : 0.0;
            gt += live ? g : 0.0;
            d = live ? d : 0.0;
#pragma unroll
            for (int r = 0; r < RM; ++r)
                if (r < R) ga[r] = fma(d, a[r], ga[r]);
            // the chunk's 64 residuals read out as scalars: column `lg` of their rows, or term 1's z where its key is
            // this lane
            const double* const colp = T + (int64_t)k0 * RS + col;
#pragma unroll 16
            for (int i = 0; i < 64; ++i) {
                const double w = grp ? (__builtin_amdgcn_readlane(key[0], i) == lg ? lane_value(z[0], i) : 0.0)
                                     : colp[(int64_t)i * RS];
                acc[i & 3] = fma(lane_value(d, i), w, acc[i & 3]);
            }
            // terms 2..R: d_i z_ri to the lane its key names (a lane of another term or role matches no key)
#pragma unroll
            for (int r = 1; r < RM; ++r) {
                if (r < R) {
                    const double dz = d * z[r];
#pragma unroll 16
                    for (int i = 0; i < 64; ++i)
                        acc[i & 3] += __builtin_amdgcn_readlane(key[r], i) == lg ? lane_value(dz, i) : 0.0;
                }
            }
        }
        double L, P, GT, GA[RM];
        wave_sum4(ll, lp, gt, ga[0], L, P, GT, GA[0]);
        GA[1] = GA[2] = GA[3] = 0.0;
        if (R > 1) {
            double u0;
            wave_sum4(ga[1], ga[2], ga[3], 0.0, GA[1], GA[2], GA[3], u0);
        }
        double GAo = GA[0];
#pragma unroll
        for (int r = 1; r < RM; ++r) GAo = tr == r ? GA[r] : GAo;
        const double cs = (acc[0] + acc[1]) + (acc[2] + acc[3]);
        gl[0] = role == 0 ? cs : (role == 1 ? tauo * cs : (role == 2 ? GAo : (role == 3 ? GT : 0.0)));
        gp[0] = g0;
        llik = (bad || k.bad) ? -kInf : L;
        lpri = bad ? -kInf : P;
    }
};

// ---------------------------------------------------------------------------
// Wide GLM (SMCN_MODEL_WGLM): SMCN_MODEL_GLM's density -- the four families, the same data block, the same table -- for
// 65 <= D <= 256 coordinates.  One wavefront per particle, coordinate c = lane + 64 k in slot k of lane `lane`
// (DL = 2: D <= 128, DL = 4: D <= 256); x = (b_1..b_Dc [, tau]), tau on lane Dc % 64, slot Dc / 64.  Not a shape of
// GlmModel: the walk differs in substance (slots, two passes).  The per-observation terms are the flat GLM's
// (smcn_glm_family.hpp), the family a wave-uniform runtime branch as in GlmHierModel.  One evaluation walks the observations in chunks of 64, one
// row per lane, in two passes over the chunk:
//   eta: slot by slot, the coefficient of column 64 k + j read out of lane j as a scalar operand, the lane's own row read
//        with 16-byte loads, two accumulators;
//   column sums: the chunk's 64 residuals read out as scalars; lane l accumulates d_i T[(k0 + i) RS + l + 64 k] for
//        every slot k that has columns -- DL independent chains per lane (two accumulators each), every read a coalesced
//        512-byte line, and the sums land on the owning lane and slot with no butterfly.
// The dispersion sum, llik and lpri go through one wave_sum4.  No atomics, no LDS: a result depends on its inputs alone.
// Slots without columns (D <= 64 (k + 1) - 64) are skipped under wave-uniform bounds kept out of lane masks (`uniform`).
// ---------------------------------------------------------------------------
template <int G_, int DL_>
struct GlmWideModel {
    static_assert(G_ == 64 && (DL_ == 2 || DL_ == 4), "GlmWideModel: one wavefront per particle, two or four coordinates per lane");
    // (four coordinates per lane: the NUTS kernel holds 15 vectors of them -- 120 registers -- beside the evaluation; with
    //  two wavefronts per SIMD (256 registers) it spilled 340 B per lane, with one it needs no scratch.  DESIGN.md 4.4)
    static constexpr int G = G_, DL = DL_, SHARED = 0, MIN_WAVES = DL_ == 2 ? 2 : 1, LDS_LEVELS = 2;
    static constexpr bool DIST = true;
    using d2 = double __attribute__((ext_vector_type(2)));
    bool poisson, nb;             // family 1 among the canonical pair 0 / 1, family 3 among the dispersion pair 2 / 3
    int lg, D, Dc, DP, RS, n;
    bool hasd;
    const double* T;              // the repacked table
    double mc[DL], inv_s2[DL], lc[DL];   // prior mean, 1 / s^2 and -log s - log(2 pi) / 2 of the lane's coordinates

    // a wave-uniform bound the compiler may not hoist into a lane mask per unrolled slot (smcn_predict.hpp: pr_opaque)
    static __device__ __forceinline__ int uniform(int v) {
        asm volatile("" : "+s"(v));
        return v;
    }
    __device__ int dim() const { return D; }
    __device__ void init(const double* md, int lg_, double*) {
        lg = lg_;
        const double fam = md[0];
        hasd = fam >= 2.0;
        poisson = fam == 1.0;
        nb = fam == 3.0;
        n = (int)md[1];
        const int p = (int)md[2];
        Dc = p + (int)md[3];
        D = Dc + (hasd ? 1 : 0);
        DP = (Dc + 1) & ~1;
        RS = glm_row_doubles(Dc);
        T = md + glm_table_offset(Dc + (hasd ? 2 : 0), n, p);
#pragma unroll
        for (int i = 0; i < DL; ++i) {
            const int c = lg + G * i;
            const bool isd = hasd && c == Dc;
            const double s = c < Dc ? md[4 + c] : (isd ? md[5 + Dc] : 1.0);
            mc[i] = isd ? md[4 + Dc] : 0.0;
            inv_s2[i] = c < D ? 1.0 / (s * s) : 0.0;
            lc[i] = c < D ? -log(s) - 0.5 * kLog2Pi : 0.0;
        }
    }
    __device__ void eval(const double (&x)[DL], double& lpri, double& llik, double (&gp)[DL], double (&gl)[DL]) const {
        double ll = 0.0, lp = 0.0, gt = 0.0;
        double xb[DL];                                     // the coefficients (0 for tau, the pad column and beyond)
        int col[DL];                                       // the lane's column of slot k (0 where the slot's column is past DP)
#pragma unroll
        for (int k = 0; k < DL; ++k) {
            const double v = x[k] - mc[k];
            gp[k] = -v * inv_s2[k];
            lp += fma(-0.5 * v, v * inv_s2[k], lc[k]);
            xb[k] = lg + G * k < Dc ? x[k] : 0.0;
            col[k] = lg + G * k < DP ? lg + G * k : 0;
        }
        double xt = x[0];
#pragma unroll
        for (int k = 1; k < DL; ++k) xt = (Dc >> 6) == k ? x[k] : xt;
        const auto tc = glm_tau_const(nb, hasd ? group_read<64>(xt, Dc & 63) : 0.0);
        double acc[DL][2];
#pragma unroll
        for (int k = 0; k < DL; ++k) acc[k][0] = acc[k][1] = 0.0;
        for (int k0 = 0; k0 < n; k0 += 64) {
            const int dp = uniform(DP);
            // ---- eta of row k0 + lg
            const d2* const row = (const d2*)(T + (int64_t)(k0 + lg) * RS);
            double e0 = 0.0, e1 = 0.0;
#pragma unroll
            for (int k = 0; k < DL; ++k) {
                const int jn = dp - 64 * k < 64 ? dp - 64 * k : 64;   // (wave-uniform; <= 0: the slot has no columns)
#pragma unroll 4
                for (int j = 0; j < jn; j += 2) {          // (j wave-uniform: the coefficients are scalar operands)
                    const d2 v = row[(64 * k + j) >> 1];
                    e0 = fma(group_read<64>(xb[k], j), v.x, e0);
                    e1 = fma(group_read<64>(xb[k], j + 1), v.y, e1);
                }
            }
            const double e = e0 + e1;
            const d2 yl = row[dp >> 1];
            double term, d, g = 0.0;
            if (hasd) {
                glm_disp_obs(nb, tc, e, yl.x, yl.y, term, d, g);
            } else {
                double mean;
                glm_canon_obs(poisson, e, yl.x, yl.y, term, mean);
                d = yl.x - mean;
            }
            const bool live = k0 + lg < n;
            ll += live ? term : 0.0;
            gt += live ? g : 0.0;
            d = live ? d : 0.0;
            // ---- the chunk's 64 residuals read out as scalars: the lane's column of every slot, weighted by them
            const double* const base = T + (int64_t)k0 * RS;
#pragma unroll 4
            for (int i = 0; i < 64; ++i) {
                const double di = lane_value(d, i);
                const double* const ri = base + (int64_t)i * RS;
#pragma unroll
                for (int k = 0; k < DL; ++k)
                    if (64 * k < dp) acc[k][i & 1] = fma(di, ri[col[k]], acc[k][i & 1]);
            }
        }
        double L, P, GT, u1;
        wave_sum4(ll, lp, gt, 0.0, L, P, GT, u1);
#pragma unroll
        for (int k = 0; k < DL; ++k) {
            const int c = lg + G * k;
            gl[k] = c < Dc ? acc[k][0] + acc[k][1] : ((hasd && c == Dc) ? GT : 0.0);
        }
        llik = (hasd && tc.bad) ? -kInf : L;
        lpri = P;
    }
};

// ---------------------------------------------------------------------------
// Categorical (multinomial logistic) regression, class 0 the reference (SMCN_MODEL_CATEGORICAL): K classes, Dc = p +
// intercept columns,
//   eta_i0 = 0, eta_ik = [b_k0 +] X_i b_k (k = 1..K-1),   log p(y_i) = eta_{i,y_i} - logsumexp(0, eta_i1, .., eta_i,K-1)
//   b_kj ~ N(0, s_c^2) with c = (k - 1) Dc + j;  x = (b_1,1..b_1,Dc, .., b_K-1,Dc) class-major, D = (K - 1) Dc <= 64.
// The table is GlmModel's (glm_table_offset(D, ..), row width from Dc) with the label in the y slot.  Per observation:
//   m = max(0, eta_ik), S = sum of e^(eta_ik - m) over every class but the (first) one that attains m -- it contributes
//   exactly 1 and stays out of S, so nothing cancels -- lse = m + log1p(S), term = (eta_{i,y_i} - m) - log1p(S), and
//   the residuals d_ik = [y_i = k] - e^(eta_ik - m) / (1 + S).  Non-finite: -inf once a logit is not finite.
// The K - 1 logits and residuals of a row are arrays with compile-time indices (guards and selects; c -> (k, j) depends
// on the runtime Dc, and a private array indexed at run time would be placed in scratch).
//   G = 8 (D <= 8): coordinate c on lane c; lane lg evaluates observations lg, lg + 8, ..  (K - 1) Dc <= 8 leaves 20
//                   (k, j) pairs that can ever be a coordinate (j < 8 / (k + 1)): the coefficients and the gradient
//                   partials are held by pair, and reduce-scattered over the group at the end.
//   G = 64 (D <= 64): one wavefront per particle, coordinate c on lane c, lane l on row k0 + l of each 64-row chunk as
//                   GlmModel<64, 1>.  Lane c needs the residual of ITS class k(c) for every row of the chunk: the chunk's
//                   residuals are staged in LDS, [row][class] at a stride of 15 doubles (odd: the writes of one class
//                   by the 64 lanes fall in distinct banks), and lane c reads d_{i,k(c)} beside X_{i,j(c)} -- one LDS
//                   read per row, where reading the K - 1 residuals out as scalars and selecting costs K - 1 (DESIGN.md
//                   4.4).  A wavefront's area is 64 x 15 doubles (7.5 KB); SHARED holds the four of a 256-lane block.
// ---------------------------------------------------------------------------
template <int G_, int DL_>
struct GlmCatModel {
    static_assert((G_ == 8 || G_ == 64) && DL_ == 1, "GlmCatModel: 8 or 64 lanes per particle, one coordinate per lane");
    static constexpr int KM = G_ == 64 ? kCatMaxClasses - 1 : 8;   // non-reference classes the shape holds
    static constexpr int STRIDE = kCatMaxClasses - 1;              // (G = 64) LDS doubles per staged row
    static constexpr int WAVE_AREA = 64 * STRIDE;
    static constexpr int G = G_, DL = DL_, SHARED = G_ == 64 ? 4 * WAVE_AREA : 0, MIN_WAVES = 2, LDS_LEVELS = 2;
    static constexpr bool DIST = true;
    static constexpr int NPAIR = 20;                               // (G = 8) the (k, j) pairs with j < 8 / (k + 1)
    using d2 = double __attribute__((ext_vector_type(2)));
    using ldsp = __attribute__((address_space(3))) double*;
    int lg, D, Dc, Km1, DP, RS, n;
    int kc, jc;                   // the lane's coordinate: class block (0-based) and column
    const double* T;              // the repacked table
    ldsp stage;                   // (G = 64) this wavefront's residual area
    double inv_s2, lc;            // 1 / s_c^2 and -log s_c - log(2 pi) / 2 of the lane's coordinate (0 beyond D)

    // first pair of class block k in the G = 8 pair arrays: 0, 8, 12, 14, 16, 17, 18, 19
    static constexpr int pair0(int k) { return k == 0 ? 0 : pair0(k - 1) + 8 / k; }

    __device__ int dim() const { return D; }
    __device__ void init(const double* md, int lg_, double* shared) {
        lg = lg_;
        Km1 = (int)md[0] - 1;
        n = (int)md[1];
        const int p = (int)md[2];
        Dc = p + (int)md[3];
        D = Km1 * Dc;
        DP = (Dc + 1) & ~1;
        RS = glm_row_doubles(Dc);
        T = md + glm_table_offset(D, n, p);
        kc = lg < D ? lg / Dc : 0;
        jc = lg < D ? lg - kc * Dc : 0;
        const double s = lg < D ? md[4 + lg] : 1.0;
        inv_s2 = lg < D ? 1.0 / (s * s) : 0.0;
        lc = lg < D ? -log(s) - 0.5 * kLog2Pi : 0.0;
        stage = G_ == 64 ? (ldsp)shared + (threadIdx.x >> 6) * WAVE_AREA : (ldsp)shared;
    }
    // one row's softmax from its K - 1 logits: log-likelihood term, and e^(eta_k - m) / (1 + S) in place of the logits
    __device__ __forceinline__ double softmax(double (&e)[KM], int y) const {
        double m = 0.0, ey = 0.0;
        int ks = 0;
#pragma unroll
        for (int k = 0; k < KM; ++k) {
            if (k < Km1) {
                const bool gt = e[k] > m;
                m = gt ? e[k] : m;
                ks = gt ? k + 1 : ks;
                ey = y == k + 1 ? e[k] : ey;
            }
        }
        // (exp_fast is exact at 0 -- the maximum's own 1 -- and flushes below -800; a NaN stays NaN)
        auto ex = [](double a) { return exp_fast(a < -800.0 ? -800.0 : a); };
        double S = ks == 0 ? 0.0 : ex(-m);
#pragma unroll
        for (int k = 0; k < KM; ++k) {
            if (k < Km1) {
                e[k] = ex(e[k] - m);
                S += ks == k + 1 ? 0.0 : e[k];
            }
        }
        double inv;
        const double l1 = log1p_pos(S, inv);
#pragma unroll
        for (int k = 0; k < KM; ++k)
            if (k < Km1) e[k] *= inv;
        return (ey - m) - l1;
    }
    __device__ void eval(const double (&x)[DL], double& lpri, double& llik, double (&gp)[DL], double (&gl)[DL]) const {
        gp[0] = -x[0] * inv_s2;
        const double lp = fma(-0.5 * x[0], x[0] * inv_s2, lc);
        double ll = 0.0;
        if constexpr (G_ == 64) {
            double acc[4] = {0.0, 0.0, 0.0, 0.0};
            const double xb = lg < D ? x[0] : 0.0;
            for (int k0 = 0; k0 < n; k0 += 64) {
                const d2* const row = (const d2*)(T + (int64_t)(k0 + lg) * RS);
                double e[KM];
#pragma unroll
                for (int k = 0; k < KM; ++k) e[k] = 0.0;
                for (int j = 0; j < DP; j += 2) {              // (j wave-uniform: the coefficients are scalar operands)
                    const d2 v = row[j >> 1];
                    const bool pad = j + 1 >= Dc;              // (the pad column's 0 times the next class's coefficient)
#pragma unroll
                    for (int k = 0; k < KM; ++k) {
                        if (k < Km1) {
                            const double b1 = group_read<64>(xb, k * Dc + j + 1);
                            e[k] = fma(group_read<64>(xb, k * Dc + j), v.x, e[k]);
                            e[k] = fma(pad ? 0.0 : b1, v.y, e[k]);
                        }
                    }
                }
                const int y = (int)row[DP >> 1].x;
                const double term = softmax(e, y);
                const bool live = k0 + lg < n;
                ll += live ? term : 0.0;
                // the chunk's residuals to LDS, [row][class]; lane c then reads its class's for each of the 64 rows
#pragma unroll
                for (int k = 0; k < KM; ++k)
                    if (k < Km1) stage[lg * STRIDE + k] = live ? (y == k + 1 ? 1.0 : 0.0) - e[k] : 0.0;
                wave_exchange_fence();
                const double* const colp = T + (int64_t)k0 * RS + jc;
                const ldsp dp = stage + kc;
#pragma unroll 16
                for (int i = 0; i < 64; ++i) acc[i & 3] = fma(dp[i * STRIDE], colp[(int64_t)i * RS], acc[i & 3]);
                wave_exchange_fence();                         // (the next chunk's writes after these reads)
            }
            gl[0] = lg < D ? (acc[0] + acc[1]) + (acc[2] + acc[3]) : 0.0;
            double L, P, u0, u1;
            wave_sum4(ll, lp, 0.0, 0.0, L, P, u0, u1);
            llik = finite_d(L) ? L : -kInf;
            lpri = P;
        } else {
            // ---- 1. the coefficients to every lane of the group, by (class block, column) pair
            double b[NPAIR], acc[NPAIR];
#pragma unroll
            for (int k = 0; k < KM; ++k) {
#pragma unroll
                for (int j = 0; j < 8 / (k + 1); ++j) {
                    b[pair0(k) + j] = (k < Km1 && j < Dc) ? group_read<G>(x[0], k * Dc + j) : 0.0;
                    acc[pair0(k) + j] = 0.0;
                }
            }
            // ---- 2. this lane's observations lg, lg + G, ..
            const int S = (n + G - 1) / G;
#pragma unroll 1
            for (int s = 0; s < S; ++s) {
                const int i = lg + G * s;
                const double* const row = T + (int64_t)i * RS;
                double e[KM];
#pragma unroll
                for (int k = 0; k < KM; ++k) {
                    e[k] = 0.0;
                    if (k < Km1) {
#pragma unroll
                        for (int j = 0; j < 8 / (k + 1); ++j)
                            if (j < Dc) e[k] = fma(b[pair0(k) + j], row[j], e[k]);
                    }
                }
                const int y = (int)row[DP];
                const double term = softmax(e, y);
                const bool live = i < n;
                ll += live ? term : 0.0;
                // (the row again, from the cache)
#pragma unroll
                for (int k = 0; k < KM; ++k) {
                    if (k < Km1) {
                        const double d = live ? (y == k + 1 ? 1.0 : 0.0) - e[k] : 0.0;
#pragma unroll
                        for (int j = 0; j < 8 / (k + 1); ++j)
                            if (j < Dc) acc[pair0(k) + j] = fma(d, row[j], acc[pair0(k) + j]);
                    }
                }
            }
            // ---- 3. reduce-scatter of the gradient partials: lane (k Dc + j) ends with the sum of its pair
            double v = 0.0;
#pragma unroll
            for (int k = 0; k < KM; ++k) {
#pragma unroll
                for (int j = 0; j < 8 / (k + 1); ++j) {
                    if (k < Km1 && j < Dc) {
                        const double t = group_sum<G>(acc[pair0(k) + j]);
                        v = lg == k * Dc + j ? t : v;
                    }
                }
            }
            gl[0] = lg < D ? v : 0.0;
            const double L = group_sum<G>(ll);
            llik = finite_d(L) ? L : -kInf;
            lpri = group_sum<G>(lp);
        }
    }
};

// ---------------------------------------------------------------------------
// Ordinal (ordered-logistic) regression (SMCN_MODEL_ORDINAL): K >= 2 classes, p >= 0 columns, no intercept, eta_i = X_i b,
// cutpoints c_1 < .. < c_{K-1} from Stan's `ordered` transform of u: c_1 = u_1, c_k = c_{k-1} + e^u_k,
//   P(y_i = k) = logit^-1(eta_i - c_k) - logit^-1(eta_i - c_{k+1})   (c_0 = -inf, c_K = +inf),
//   b_j ~ N(0, s_j^2), c_k ~ N(0, t_k^2), with the log-Jacobian sum_{k>=2} u_k;  x = (b_1..b_p, u_1..u_{K-1}), D <= 64.
// In the stable form, with delta_k = c_{k+1} - c_k = e^u_{k+1} (sigma(a) - sigma(b) = sigma(a) sigma(-b) (1 - e^-(a-b))),
//   log P(y_i = k) = -softplus(c_k - eta_i) [k >= 1] - softplus(eta_i - c_{k+1}) [k <= K-2] + log(1 - e^-delta_k) [middle k].
// The last term depends on the parameters only: its sum over observations is n_k log(1 - e^-delta_k), with the class
// counts n_k that smcn_ctx_create stores behind the table, formed from u on the cutpoint lane of u_{k+1} (= u there for
// u < -36, where e^u is below the rounding of 1; finite for every finite u), gradient n_k delta_k / expm1(delta_k).
// The two softplus terms are GlmModel's logistic pattern (exp_fast(-|a|), log1p_pos, the sigmoid from the same
// exponential).  Gradients: d/d eta = sigma(c_k - eta) - sigma(eta - c_{k+1}); -sigma(c_k - eta) to the lower cutpoint,
// +sigma(eta - c_{k+1}) to the upper one; the chain to u takes suffix sums over the cutpoint lanes, g_u1 = sum_j g_cj and
// g_um = e^u_m sum_{j>=m} g_cj, for the likelihood and for the cutpoint prior alike (the Jacobian adds 1 to g_um, m >= 2).
// The table is GlmModel's with the row width from p and the label in the y slot, [X_i1 .. X_ip, 0 (to an even count),
// y_i, 0]; the K class counts follow it (ord_counts_offset).  Non-finite: lpri = llik = -inf once a cutpoint is not finite
// (e^u_m overflows), llik = -inf once an eta_i is not finite.  The cutpoints are the sequential running sum, as
// `constrain` forms them.
//   G = 8 (D <= 8): coordinate c on lane c; every lane gathers the coefficients and the increments and forms the
//                   cutpoints itself, and picks c_y and c_{y+1} of its rows by compile-time selects; the gradient partials
//                   are held by coordinate slot (column j < p, cutpoint p + m - 1), reduce-scattered over the group.
//   G = 64 (D <= 64): one wavefront per particle, coordinate c on lane c, lane l on row k0 + l of each 64-row chunk as
//                   GlmModel<64, 1>.  The row owner fetches c_y and c_{y+1} with cross-lane reads (as GlmHierModel
//                   fetches z_{g_i}).  In the read-out a cutpoint lane compares the row's label, read out as a scalar,
//                   with its own index (GlmHierModel's group indicator) and takes the row's lower or upper partial:
//                   GlmCatModel's LDS staging would need a K-slot row per observation (up to 65 doubles) to let a lane
//                   read its own slot, where the compare costs a few VALU operations and no LDS.
// ---------------------------------------------------------------------------
// sum of v over lanes lg .. G - 1 of the group (Kogge-Stone)
template <int G>
__device__ __forceinline__ double group_suffix_sum(double v, int lg) {
    v += group_shift_down<G, 1>(v, lg);
    v += group_shift_down<G, 2>(v, lg);
    v += group_shift_down<G, 4>(v, lg);
    if constexpr (G >= 16) v += group_shift_down<G, 8>(v, lg);
    if constexpr (G >= 32) v += group_shift_down<G, 16>(v, lg);
    if constexpr (G >= 64) v += group_shift_down<G, 32>(v, lg);
    return v;
}

template <int G_, int DL_>
struct GlmOrdModel {
    static_assert((G_ == 8 || G_ == 64) && DL_ == 1, "GlmOrdModel: 8 or 64 lanes per particle, one coordinate per lane");
    static constexpr int G = G_, DL = DL_, SHARED = 0, MIN_WAVES = 2, LDS_LEVELS = 2;
    static constexpr bool DIST = true;
    using d2 = double __attribute__((ext_vector_type(2)));
    int lg, D, p, Km1, DP, RS, n;
    int mc;                       // the lane's cutpoint index m (coordinate p + m - 1), -1 on the other lanes
    const double* T;              // the repacked table
    double inv_s2, lc;            // 1 / s^2 and -log s - log(2 pi) / 2 of the lane's coordinate's prior (0 beyond D)
    double cnt;                   // (lanes of u_m, m >= 2) n_{m-1}, the count of the middle class below c_m

    __device__ int dim() const { return D; }
    __device__ void init(const double* md, int lg_, double*) {
        lg = lg_;
        Km1 = (int)md[0] - 1;
        n = (int)md[1];
        p = (int)md[2];
        D = p + Km1;
        DP = (p + 1) & ~1;
        RS = glm_row_doubles(p);
        T = md + glm_table_offset(D, n, p);
        mc = (lg >= p && lg < D) ? lg - p + 1 : -1;
        const double s = lg < D ? md[3 + lg] : 1.0;
        inv_s2 = lg < D ? 1.0 / (s * s) : 0.0;
        lc = lg < D ? -log(s) - 0.5 * kLog2Pi : 0.0;
        cnt = mc >= 2 ? md[ord_counts_offset(D, n, p) + mc - 1] : 0.0;
    }
    __device__ void eval(const double (&x)[DL], double& lpri, double& llik, double (&gp)[DL], double (&gl)[DL]) const {
        const double u = x[0];
        const bool isc = mc >= 1;
        const double ev = mc >= 2 ? exp(u) : u;            // (cutpoint lanes) c_m - c_{m-1}, or c_1
        // ---- the cutpoints: c_m on the lane of u_m, c_{K-1} everywhere
        double cut = 0.0, cK = 0.0;
        double ll = 0.0, gx, gc;
        if constexpr (G_ == 64) {
#pragma unroll 1
            for (int j = 0; j < Km1; ++j) {
                cK += group_read<64>(ev, p + j);
                cut = lg == p + j ? cK : cut;
            }
            // ---- observations, 64 a chunk
            double ax[4] = {0.0, 0.0, 0.0, 0.0}, ac[2] = {0.0, 0.0};
            const int col = lg < p ? lg : 0;
            const double xb = lg < p ? u : 0.0;            // (0 on the pad column)
            for (int k0 = 0; k0 < n; k0 += 64) {
                const d2* const row = (const d2*)(T + (int64_t)(k0 + lg) * RS);
                double e0 = 0.0, e1 = 0.0;
                for (int j = 0; j < DP; j += 2) {          // (j wave-uniform: the coefficients are scalar operands)
                    const d2 v = row[j >> 1];
                    e0 = fma(group_read<64>(xb, j), v.x, e0);
                    e1 = fma(group_read<64>(xb, j + 1), v.y, e1);
                }
                const int y = (int)row[DP >> 1].x;
                const double lo = __shfl(cut, p + (y >= 1 ? y - 1 : 0), 64);
                const double hi = __shfl(cut, p + (y < Km1 ? y : Km1 - 1), 64);
                double term, de, glo, ghi;
                glm_ord_obs(Km1, e0 + e1, y, lo, hi, term, de, glo, ghi);
                const bool live = k0 + lg < n;
                ll += live ? term : 0.0;
                de = live ? de : 0.0;
                glo = live ? glo : 0.0;
                ghi = live ? ghi : 0.0;
                // the chunk's 64 rows read out as scalars: column `lg` weighted by d / d eta, or the row's cutpoint partial
                // when its label puts this lane's cutpoint below (y = m) or above (y = m - 1) it
                const double* const colp = T + (int64_t)k0 * RS + col;
#pragma unroll 16
                for (int i = 0; i < 64; ++i) {
                    const int yi = __builtin_amdgcn_readlane(y, i);
                    ax[i & 3] = fma(lane_value(de, i), colp[(int64_t)i * RS], ax[i & 3]);
                    ac[i & 1] += mc == yi ? lane_value(glo, i) : (mc == yi + 1 ? lane_value(ghi, i) : 0.0);
                }
            }
            gx = (ax[0] + ax[1]) + (ax[2] + ax[3]);
            gc = ac[0] + ac[1];
        } else {
            // ---- 1. the coefficients and the increments to every lane of the group; the cutpoints, by coordinate slot
            double b[8], cs[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const double w = j < D ? group_read<G>(ev, j) : 0.0;
                b[j] = j < p ? w : 0.0;
                cK += (j >= p && j < D) ? w : 0.0;
                cs[j] = cK;
                cut = lg == j ? cK : cut;
            }
            // ---- 2. this lane's observations lg, lg + G, ..: gradient partials by slot, column j < p or cutpoint p + m - 1
            double acc[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] = 0.0;
            const int S = (n + G - 1) / G;
#pragma unroll 1
            for (int s = 0; s < S; ++s) {
                const int i = lg + G * s;
                const double* const row = T + (int64_t)i * RS;
                double e = 0.0;
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (j < p) e = fma(b[j], row[j], e);   // (p wave-uniform)
                const int y = (int)row[DP];
                double lo = 0.0, hi = 0.0;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    lo = j == p + y - 1 ? cs[j] : lo;
                    hi = j == p + y ? cs[j] : hi;
                }
                double term, de, glo, ghi;
                glm_ord_obs(Km1, e, y, lo, hi, term, de, glo, ghi);
                const bool live = i < n;
                ll += live ? term : 0.0;
                de = live ? de : 0.0;
                glo = live ? glo : 0.0;
                ghi = live ? ghi : 0.0;
                // (the row again, from the cache)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    if (j < p) acc[j] = fma(de, row[j], acc[j]);
                    else if (j < D) acc[j] += j == p + y - 1 ? glo : (j == p + y ? ghi : 0.0);
                }
            }
            // ---- 3. reduce-scatter of the partials: lane c ends with the sum of slot c
            double v = 0.0;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (j < D) {
                    const double t = group_sum<G>(acc[j]);
                    v = lg == j ? t : v;
                }
            }
            gx = v;
            gc = v;
        }
        // ---- priors: b_j, or c_m with the log-Jacobian u_m (m >= 2)
        const double pv = isc ? cut : u;
        const double pg = -pv * inv_s2;                    // d lpri / d b_j, or d lpri / d c_m
        const double lp = fma(-0.5 * pv, pv * inv_s2, lc) + (mc >= 2 ? u : 0.0);
        // ---- the middle classes' n_k log(1 - e^-delta_k), delta_k = e^u_{k+1}, on the lane of u_{k+1}
        double cg = 0.0;
        if (cnt > 0.0) {
            const bool tiny = u < -36.0;                   // e^u < 2.4e-16: log(1 - e^-e^u) = u, e^u / expm1(e^u) = 1
            ll += cnt * (tiny ? u : log(-expm1(-ev)));
            cg = cnt * (tiny ? 1.0 : ev / expm1(ev));
        }
        // ---- the chain to u: suffix sums over the cutpoint lanes, times dc_j / du_m (1 for m = 1, e^u_m above)
        const double sl = group_suffix_sum<G>(isc ? gc : 0.0, lg);
        const double sp = group_suffix_sum<G>(isc ? pg : 0.0, lg);
        const double dm = mc >= 2 ? ev : 1.0;
        gl[0] = lg < p ? gx : (isc ? fma(dm, sl, cg) : 0.0);
        gp[0] = lg < p ? pg : (isc ? fma(dm, sp, mc >= 2 ? 1.0 : 0.0) : 0.0);
        double L, P;
        if constexpr (G_ == 64) {
            double u0, u1;
            wave_sum4(ll, lp, 0.0, 0.0, L, P, u0, u1);
        } else {
            L = group_sum<G>(ll);
            P = group_sum<G>(lp);
        }
        const bool bad = !finite_d(cK);                    // a cutpoint is not finite
        llik = bad ? -kInf : (finite_d(L) ? L : -kInf);
        lpri = bad ? -kInf : P;
    }
};

}  // namespace smcn

#include "smcn_glm_cont.hpp"   // SMCN_MODEL_CGLM: the continuous-response families and their functor
