// Continuous-response GLM (SMCN_MODEL_CGLM): the per-observation terms of its two families and its density functor.
//   0 gamma_log:  y ~ Gamma(shape a = e^tau, rate a / mu), mu = e^eta.  With c = log y, u = c - eta, r = e^u = y / mu:
//                   term = a (tau + u - r) - lgamma(a) - c,   d term / d eta = a (r - 1),
//                   d term / d tau = a (tau + 1 - psi(a) + u - r)
//   1 student_t:  y ~ t_df(eta, sigma = e^tau), df fixed.  With z = (y - eta) e^-tau:
//                   term = C(df) - tau - (df + 1) / 2 log1p(z^2 / df),   C = lgamma((df + 1) / 2) - lgamma(df / 2) - log(df pi) / 2,
//                   d term / d eta = (df + 1) z e^-tau / (df + z^2),   d term / d tau = (df + 1) z^2 / (df + z^2) - 1
// Three tiers of constants, so that the observation loop holds one exponential (gamma), or one reciprocal and one
// logarithm (student_t), and no lgamma (inlined there it made the flat GLM's kernels spill, smcn_glm_family.hpp):
//   ContDf     what depends on df alone, formed once per kernel (init) and kept wave-uniform -- scalar registers;
//   ContConst  what depends on tau (and df), formed once per evaluation:
//                gamma, a < kGammaAsym:  k0 = a tau - lgamma(a), k1 = tau + 1 - psi(a) from lgamma_digamma_pos;
//                gamma, a >= kGammaAsym: Stirling, lgamma(a) = (a - 1/2) tau - a + log(2 pi) / 2 + stirling_tail(1 / a) and
//                                        psi(a) = tau - 1 / (2a) - digamma_tail(1 / a), so
//                                        k0 = tau / 2 + a - log(2 pi) / 2 - stirling_tail(1 / a),  k1 = 1 + 1 / (2a) + digamma_tail(1 / a)
//                                        -- no a tau-sized intermediate, and tau - psi(a) without its cancellation;
//                student_t:              k0 = C - tau, k1 = e^-tau;
//   the observation body.
// Far outliers (student_t): beyond |z| > T = 1e150 min(1, sqrt(df)) -- below it neither z^2 nor z^2 / df overflows --
// log1p(z^2 / df) is 2 log|z| - log df, d is (df + 1) / z e^-tau and gt is df: what they differ from the full forms by is
// df / z^2 < 1e-300 max(df, 1) of their size, nothing in double for df < 1e280.  The logarithm and the reciprocal are the
// same two calls either side of T, on |z| or on 1 + z^2 / df.  Above |z| of about 4.5e307 the reciprocal of |z| is
// subnormal, so d -- about 1e-308 (df + 1) e^-tau there -- loses digits or flushes to 0; the term and gt do not use it.
// Non-finite: llik = -inf when e^tau (gamma) or e^-tau (student_t) leaves the normal range -- the rest of the evaluation
// then runs with tau = 0, so every gradient stays a number --, when e^-eta overflows (gamma; e^u = inf gives it by
// itself), and when z itself overflows (student_t).
#pragma once
#include "smcn_device.hpp"
#include "smcn_glm_family.hpp"
#include "smcn_regdata.hpp"

namespace smcn {

// a value every lane of the wavefront holds alike, as a scalar
__device__ __forceinline__ double wave_uniform(double v) {
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
}

// what student_t derives from df alone (all 0 for gamma_log, which reads none of it)
struct ContDf {
    double df, idf, dfp1, hp, q;    // df, 1 / df, df + 1, (df + 1) / 2, (df + 1) / df
    double c, ldf, T;               // C(df), log df, the far-outlier threshold on |z|
};

// C(df) with x = df / 2: for x >= kGammaAsym from Stirling's series, where the two (x - 1/2) log x-sized terms and
// log(df pi) / 2 cancel in closed form, C = x log1p(1 / (2x)) - 1/2 - log(2 pi) / 2 + tail(x + 1/2) - tail(x) (-> the
// normal's -log(2 pi) / 2); below, as the difference of two lgamma
__device__ __forceinline__ ContDf glm_cont_df(bool student, double df) {
    ContDf f{};
    if (!student) return f;
    f.df = df;
    f.idf = 1.0 / df;
    f.dfp1 = df + 1.0;
    f.hp = 0.5 * f.dfp1;
    f.q = f.dfp1 * f.idf;
    f.ldf = log(df);
    f.T = 1e150 * fmin(1.0, sqrt(df));
    const double x = 0.5 * df;
    if (x >= kGammaAsym) {
        double inv;
        const double l1 = log1p_pos(0.5 / x, inv);
        f.c = (fma(x, l1, -0.5) - 0.5 * kLog2Pi) + (stirling_tail(1.0 / (x + 0.5)) - stirling_tail(1.0 / x));
    } else {
        double la, lb, ps;
        lgamma_digamma_pos(x + 0.5, la, ps);
        lgamma_digamma_pos(x, lb, ps);
        f.c = (la - lb) - 0.5 * (f.ldf + kLogPi);
    }
    return f;
}

// what one evaluation derives from tau (the two families share the registers)
struct ContConst {
    double a;                     // gamma: e^tau
    double k0, k1;                // gamma: a tau - lgamma(a), tau + 1 - psi(a);  student_t: C - tau, e^-tau
    bool bad;
    ContDf f;
};

__device__ __forceinline__ ContConst glm_cont_const(bool student, double tau, const ContDf& f) {
    ContConst k;
    k.f = f;
    const double s = student ? -tau : tau;                     // the exponent whose exponential the family needs
    k.bad = !(s <= kLogDblMax && s >= kLogDblMinNormal);
    tau = k.bad ? 0.0 : tau;
    if (student) {
        k.a = 0.0;
        k.k0 = f.c - tau;
        k.k1 = exp_fast(-tau);
    } else {
        k.a = exp_fast(tau);
        if (k.a >= kGammaAsym) {
            const double ia = 1.0 / k.a;
            k.k0 = (fma(0.5, tau, k.a) - 0.5 * kLog2Pi) - stirling_tail(ia);
            k.k1 = 1.0 + fma(0.5, ia, digamma_tail(ia));
        } else {
            double lg, ps;
            lgamma_digamma_pos(k.a, lg, ps);
            k.k0 = fma(k.a, tau, -lg);
            k.k1 = (tau + 1.0) - ps;
        }
    }
    return k;
}
__device__ __forceinline__ ContConst glm_cont_const(bool student, double tau, double df) {
    return glm_cont_const(student, tau, glm_cont_df(student, df));
}

// one observation: log-likelihood term, d term / d eta and d term / d tau; c is the row's slot behind y (log y: gamma)
__device__ __forceinline__ void glm_cont_obs(bool student, const ContConst& k, double eta, double y, double c, double& term,
                                             double& d, double& gt) {
    if (!student) {
        const double u = c - eta;
        // (exp_fast is for |u| <= 800: e^800 = inf, e^-800 = 0; a NaN stays a NaN)
        const double r = exp_fast(u < -800.0 ? -800.0 : (u > 800.0 ? 800.0 : u));
        term = fma(k.a, u - r, k.k0) - c;
        term = -eta <= kLogDblMax ? term : -kInf;          // e^-eta overflows
        d = k.a * (r - 1.0);
        gt = k.a * ((k.k1 + u) - r);
    } else {
        const ContDf& f = k.f;
        const double ze = (y - eta) * k.k1;                // z = (y - eta) e^-tau
        const double za = fabs(ze);
        const bool far = za > f.T;
        const double w = (ze * ze) * f.idf;                // (far: unused, and possibly inf)
        const double u1 = far ? za : 1.0 + w;
        const double inv = rcp_nr(u1), lg = log_ge1(u1);
        // log1p(w): log(1 + w) with the rounding of 1 + w put back (log1p_pos), or 2 log|z| - log df
        const double l = far ? fma(2.0, lg, -f.ldf) : fma(w - (u1 - 1.0), inv, lg);
        term = fma(-f.hp, l, k.k0);
        term = za < kInf ? term : -kInf;                   // z overflows (or eta is a NaN)
        d = far ? (f.dfp1 * k.k1) * copysign(inv, ze) : (f.q * inv) * (ze * k.k1);
        gt = far ? f.df : fma(f.dfp1, w * inv, -1.0);
    }
}

// ---------------------------------------------------------------------------
// The density functor: GlmModel<G, DL, true>'s sibling (smcn_models.hpp) -- the same table walk, the same reduce-scatter
// (G = 8) or column-sum scheme (G = 64), tau's gradient on the lane that owns coordinate Dc -- over the data block
//   [family (0 gamma_log, 1 student_t), n, p, intercept, df, s_1..s_Dc, m_tau, s_tau, y_1..y_n, X (n x p, row-major)]
// and the table reg_repack lays behind it (cglm_table_offset): a row per observation, [1 (intercept only), X_i1 .. X_ip,
// 0 (to an even column count DP), y_i, c_i], c_i = log y_i (gamma_log) or 0, RS = DP + 2 doubles, at a 128-byte boundary,
// zero rows up to a multiple of 64.  x = (b_1..b_Dc, tau), D = Dc + 1.
//   G = 8:  one coordinate per lane, D <= 8 (kGlmDispG8, as the flat dispersion families);
//   G = 64: one particle per wavefront, coordinate c on lane c, D <= 64.
// A padding row (y = 0, c = 0) is evaluated like any other and selected out: its term may be anything.
// ---------------------------------------------------------------------------
template <int G_, int DL_>
struct GlmContModel {
    static constexpr int G = G_, DL = DL_, SHARED = 0, MIN_WAVES = 2, LDS_LEVELS = 2;
    static constexpr bool DIST = true;
    static constexpr int DMAX = G_ * DL_;
    static_assert(G_ == 64 ? DL_ == 1 : (DMAX % 2) == 0, "GlmContModel: 64 lanes with one coordinate each, or an even capacity");
    static constexpr int HEAD = 5;            // doubles of the data block in front of the priors
    using d2 = double __attribute__((ext_vector_type(2)));
    int lg, D, Dc, DP, RS, n;
    bool student;
    ContDf f;             // (wave-uniform)
    const double* T;      // the repacked table
    double mc[DL], inv_s2[DL], lc[DL];   // prior mean; 1 / s^2 and -log s - log(2 pi) / 2 of the lane's coordinates (0 beyond D)

    __device__ int dim() const { return D; }
    __device__ void init(const double* md, int lg_, double*) {
        lg = lg_;
        student = md[0] != 0.0;
        n = (int)md[1];
        const int p = (int)md[2];
        Dc = p + (int)md[3];
        D = Dc + 1;
        DP = (Dc + 1) & ~1;
        RS = glm_row_doubles(Dc);
        T = md + cglm_table_offset(Dc + 2, n, p);
        const ContDf v = glm_cont_df(student, md[4]);
        f.df = wave_uniform(v.df), f.idf = wave_uniform(v.idf), f.dfp1 = wave_uniform(v.dfp1), f.hp = wave_uniform(v.hp);
        f.q = wave_uniform(v.q), f.c = wave_uniform(v.c), f.ldf = wave_uniform(v.ldf), f.T = wave_uniform(v.T);
#pragma unroll
        for (int i = 0; i < DL; ++i) {
            const int c = lg + G * i;
            const double s = c < Dc ? md[HEAD + c] : (c == Dc ? md[HEAD + 1 + Dc] : 1.0);
            mc[i] = c == Dc ? md[HEAD + Dc] : 0.0;
            inv_s2[i] = c < D ? 1.0 / (s * s) : 0.0;
            lc[i] = c < D ? -log(s) - 0.5 * kLog2Pi : 0.0;
        }
    }
    __device__ void eval(const double (&x)[DL], double& lpri, double& llik, double (&gp)[DL], double (&gl)[DL]) const {
        double ll = 0.0, lp = 0.0, gt = 0.0;
#pragma unroll
        for (int i = 0; i < DL; ++i) {
            const double v = x[i] - mc[i];
            gp[i] = -v * inv_s2[i];
            lp += fma(-0.5 * v, v * inv_s2[i], lc[i]);
        }
        double xt = x[0];
#pragma unroll
        for (int i = 1; i < DL; ++i) xt = Dc / G == i ? x[i] : xt;
        const ContConst k = glm_cont_const(student, group_read<G>(xt, Dc % G), f);
        if constexpr (G_ == 64) {
            // (four accumulators for the column sums and two for eta, as GlmModel<64, 1>)
            double acc[4] = {0.0, 0.0, 0.0, 0.0};
            const int col = lg < DP ? lg : 0;
            const double xb = lg < Dc ? x[0] : 0.0;            // (tau is not a coefficient: 0 on the pad column)
            for (int k0 = 0; k0 < n; k0 += 64) {
                const d2* const row = (const d2*)(T + (int64_t)(k0 + lg) * RS);
                double e0 = 0.0, e1 = 0.0;
                for (int j = 0; j < DP; j += 2) {          // (j wave-uniform: the coefficients are scalar operands)
                    const d2 v = row[j >> 1];
                    e0 = fma(group_read<64>(xb, j), v.x, e0);
                    e1 = fma(group_read<64>(xb, j + 1), v.y, e1);
                }
                const d2 yc = row[DP >> 1];
                double term, d, g;
                glm_cont_obs(student, k, e0 + e1, yc.x, yc.y, term, d, g);
                const bool live = k0 + lg < n;
                ll += live ? term : 0.0;
                gt += live ? g : 0.0;
                d = live ? d : 0.0;
                // column `lg` of the chunk's 64 rows, weighted by their residuals (read out as scalars)
                const double* const colp = T + (int64_t)k0 * RS + col;
#pragma unroll 16
                for (int i = 0; i < 64; ++i) acc[i & 3] = fma(lane_value(d, i), colp[(int64_t)i * RS], acc[i & 3]);
            }
            double L, P, GT, u1;
            wave_sum4(ll, lp, gt, 0.0, L, P, GT, u1);
            gl[0] = lg < Dc ? (acc[0] + acc[1]) + (acc[2] + acc[3]) : (lg == Dc ? GT : 0.0);
            llik = k.bad ? -kInf : L;
            lpri = P;
        } else {
            // ---- 1. the Dc coefficients to every lane of the group (0 in tau's slot and beyond)
            double b[DMAX];
#pragma unroll
            for (int j = 0; j < DMAX; ++j) {
                const double v = group_read<G>(x[j / G], j % G);
                b[j] = j < Dc ? v : 0.0;
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
                const d2 yc = row[DP >> 1];
                double term, d, g;
                glm_cont_obs(student, k, e, yc.x, yc.y, term, d, g);
                const bool live = i < n;
                ll += live ? term : 0.0;
                gt += live ? g : 0.0;
                d = live ? d : 0.0;
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
            // ---- 3. reduce-scatter of the gradient partials: lane c % G ends with the sum of column c; tau's sum to the
            //         lane that owns coordinate Dc
#pragma unroll
            for (int j = 0; j < DMAX; ++j) acc[j] = j < Dc ? group_sum<G>(acc[j]) : 0.0;
            const double GT = group_sum<G>(gt);
#pragma unroll
            for (int i = 0; i < DL; ++i) {
                double v = 0.0;
#pragma unroll
                for (int j = i * G; j < (i + 1) * G; ++j) v = (j - i * G == lg) ? acc[j] : v;
                const int c = lg + G * i;
                gl[i] = c < Dc ? v : (c == Dc ? GT : 0.0);
            }
            llik = k.bad ? -kInf : group_sum<G>(ll);
            lpri = group_sum<G>(lp);
        }
    }
};

}  // namespace smcn
