// GLM with per-observation offsets and weights (SMCN_MODEL_OGLM): SMCN_MODEL_GLM's four families, priors, coordinates
// and both shapes, with
//   eta_i = [b_0 +] X_i b + o_i,   llik = sum_i w_i l(y_i | eta_i [, tau]),   grad = sum_i w_i d_i X_i  (tau: sum_i w_i gt_i).
// The table reg_repack (smcn_regdata.hpp) lays behind the caller's block (oglm_table_offset: the same place whatever the
// flags): a row per observation, [1 (intercept only), X_i1 .. X_ip, 0 (to an even count DP), y_i, lgamma(y_i + 1), o_i,
// w_i], RS = DP + 4 doubles; o_i = 0 and w_i = 1 where the caller gave none, and the kernels always read both.  A
// padding row is all zero, so its weight is 0: `w != 0` is the one test for "this row counts", and a row that does not
// count adds exactly 0 to every sum whatever its term is (-inf or NaN included: e^eta may overflow there).
// Siblings of GlmModel / GlmDispModel rather than a switch on them, so that their instruction streams and register
// allocation stay as they are; the per-observation terms are their own obs() (and tau_const()), called on members of
// which only the family flag is set (as GlmHierModel does).
#pragma once
#include "smcn_models.hpp"

namespace smcn {

// 8 lanes per particle up to these D (D counts tau), one wavefront per particle above (Offsets and weights)
constexpr int kOglmG8 = 16, kOglmDispG8 = 8;

// families 0 (bernoulli_logit) and 1 (poisson_log)
template <int G_, int DL_>
struct GlmOffModel {
    static constexpr int G = G_, DL = DL_, SHARED = 0, MIN_WAVES = 2, LDS_LEVELS = 2;
    static constexpr bool DIST = true;
    static constexpr int DMAX = G_ * DL_;
    static_assert(G_ == 64 ? DL_ == 1 : (DMAX % 2) == 0, "GlmOffModel: 64 lanes with one coordinate each, or an even capacity");
    using d2 = double __attribute__((ext_vector_type(2)));
    int lg, D, DP, RS, n;
    GlmModel<64, 1> glm;          // obs() (only `poisson` is set)
    const double* T;              // the repacked table
    double inv_s2[DL], lc[DL];    // 1 / s_c^2 and -log s_c - log(2 pi) / 2 of the lane's coordinates (0 beyond D)

    __device__ int dim() const { return D; }
    __device__ void init(const double* md, int lg_, double*) {
        lg = lg_;
        glm.poisson = md[0] != 0.0;
        n = (int)md[1];
        const int p = (int)md[2];
        D = p + (int)md[3];
        DP = (D + 1) & ~1;
        RS = oglm_row_doubles(D);
        T = md + oglm_table_offset(D, n, p);
#pragma unroll
        for (int i = 0; i < DL; ++i) {
            const int c = lg + G * i;
            const double s = c < D ? md[5 + c] : 1.0;
            inv_s2[i] = c < D ? 1.0 / (s * s) : 0.0;
            lc[i] = c < D ? -log(s) - 0.5 * kLog2Pi : 0.0;
        }
    }
    __device__ void eval(const double (&x)[DL], double& lpri, double& llik, double (&gp)[DL], double (&gl)[DL]) const {
        double ll = 0.0, lp = 0.0;
#pragma unroll
        for (int i = 0; i < DL; ++i) {
            gp[i] = -x[i] * inv_s2[i];
            lp += fma(-0.5 * x[i], x[i] * inv_s2[i], lc[i]);
        }
        if constexpr (G_ == 64) {
            double acc[4] = {0.0, 0.0, 0.0, 0.0};
            const int col = lg < DP ? lg : 0;
            for (int k0 = 0; k0 < n; k0 += 64) {
                const d2* const row = (const d2*)(T + (int64_t)(k0 + lg) * RS);
                double e0 = 0.0, e1 = 0.0;
                for (int j = 0; j < DP; j += 2) {          // (j wave-uniform: the coefficients are scalar operands)
                    const d2 v = row[j >> 1];
                    e0 = fma(group_read<64>(x[0], j), v.x, e0);
                    e1 = fma(group_read<64>(x[0], j + 1), v.y, e1);
                }
                const d2 yl = row[DP >> 1], ow = row[(DP >> 1) + 1];
                const double e = (e0 + e1) + ow.x;
                double term, d;
                glm.obs(e, yl.x, yl.y, term, d);
                const bool live = ow.y != 0.0;             // (a padding row's weight is 0)
                ll += live ? ow.y * term : 0.0;
                d = live ? ow.y * d : 0.0;
                const double* const colp = T + (int64_t)k0 * RS + col;
#pragma unroll 16
                for (int i = 0; i < 64; ++i) acc[i & 3] = fma(lane_value(d, i), colp[(int64_t)i * RS], acc[i & 3]);
            }
            gl[0] = lg < D ? (acc[0] + acc[1]) + (acc[2] + acc[3]) : 0.0;
            double L, P, u0, u1;
            wave_sum4(ll, lp, 0.0, 0.0, L, P, u0, u1);
            llik = L;
            lpri = P;
        } else {
            // ---- 1. the D coefficients to every lane of the group
            double b[DMAX];
#pragma unroll
            for (int j = 0; j < DMAX; ++j) b[j] = group_read<G>(x[j / G], j % G);
            // ---- 2. this lane's observations lg, lg + G, ..
            double acc[DMAX];
#pragma unroll
            for (int j = 0; j < DMAX; ++j) acc[j] = 0.0;
            const int S = (n + G - 1) / G;
#pragma unroll 1
            for (int k = 0; k < S; ++k) {
                const int i = lg + G * k;
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
                const d2 yl = row[DP >> 1], ow = row[(DP >> 1) + 1];
                e += ow.x;
                double term, d;
                glm.obs(e, yl.x, yl.y, term, d);
                const bool live = ow.y != 0.0;
                ll += live ? ow.y * term : 0.0;
                d = live ? ow.y * d : 0.0;
#pragma unroll
                for (int j2 = 0; j2 < DMAX / 2; ++j2) {
                    if (2 * j2 < DP) {
                        const d2 v = row[j2];
                        acc[2 * j2] = fma(d, v.x, acc[2 * j2]);
                        acc[2 * j2 + 1] = fma(d, v.y, acc[2 * j2 + 1]);
                    }
                }
            }
            // ---- 3. reduce-scatter of the gradient partials: lane c % G ends with the sum of column c
#pragma unroll
            for (int j = 0; j < DMAX; ++j) acc[j] = j < DP ? group_sum<G>(acc[j]) : 0.0;
#pragma unroll
            for (int i = 0; i < DL; ++i) {
                double v = 0.0;
#pragma unroll
                for (int j = i * G; j < (i + 1) * G; ++j) v = (j - i * G == lg) ? acc[j] : v;
                gl[i] = (lg + G * i) < D ? v : 0.0;
            }
            llik = group_sum<G>(ll);
            lpri = group_sum<G>(lp);
        }
    }
};

// families 2 (normal) and 3 (neg_binomial_2_log): x = (b_1..b_Dc, tau), as GlmDispModel
template <int G_, int DL_>
struct GlmOffDispModel {
    static constexpr int G = G_, DL = DL_, SHARED = 0, MIN_WAVES = 2, LDS_LEVELS = 2;
    static constexpr bool DIST = true;
    static constexpr int DMAX = G_ * DL_;
    static_assert(G_ == 64 ? DL_ == 1 : (DMAX % 2) == 0, "GlmOffDispModel: 64 lanes with one coordinate each, or an even capacity");
    using d2 = double __attribute__((ext_vector_type(2)));
    using TauConst = typename GlmDispModel<64, 1>::TauConst;
    int lg, D, Dc, DP, RS, n;
    GlmDispModel<64, 1> disp;     // tau_const() and obs() (only `nb` is set)
    const double* T;              // the repacked table
    double mc[DL], inv_s2[DL], lc[DL];   // prior mean, 1 / s^2 and -log s - log(2 pi) / 2 of the lane's coordinates

    __device__ int dim() const { return D; }
    __device__ void init(const double* md, int lg_, double*) {
        lg = lg_;
        disp.nb = md[0] == 3.0;
        n = (int)md[1];
        const int p = (int)md[2];
        Dc = p + (int)md[3];
        D = Dc + 1;
        DP = (Dc + 1) & ~1;
        RS = oglm_row_doubles(Dc);
        T = md + oglm_table_offset(Dc + 2, n, p);
#pragma unroll
        for (int i = 0; i < DL; ++i) {
            const int c = lg + G * i;
            const double s = c < Dc ? md[5 + c] : (c == Dc ? md[6 + Dc] : 1.0);
            mc[i] = c == Dc ? md[5 + Dc] : 0.0;
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
        const TauConst k = disp.tau_const(group_read<G>(xt, Dc % G));
        if constexpr (G_ == 64) {
            double acc[4] = {0.0, 0.0, 0.0, 0.0};
            const int col = lg < DP ? lg : 0;
            const double xb = lg < Dc ? x[0] : 0.0;           // (tau is not a coefficient: 0 on the pad column)
            for (int k0 = 0; k0 < n; k0 += 64) {
                const d2* const row = (const d2*)(T + (int64_t)(k0 + lg) * RS);
                double e0 = 0.0, e1 = 0.0;
                for (int j = 0; j < DP; j += 2) {
                    const d2 v = row[j >> 1];
                    e0 = fma(group_read<64>(xb, j), v.x, e0);
                    e1 = fma(group_read<64>(xb, j + 1), v.y, e1);
                }
                const d2 yl = row[DP >> 1], ow = row[(DP >> 1) + 1];
                const double e = (e0 + e1) + ow.x;
                double term, d, g;
                disp.obs(k, e, yl.x, yl.y, term, d, g);
                const bool live = ow.y != 0.0;                // (a padding row's weight is 0)
                ll += live ? ow.y * term : 0.0;
                gt += live ? ow.y * g : 0.0;
                d = live ? ow.y * d : 0.0;
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
                    if (2 * j2 < DP) {
                        const d2 v = row[j2];
                        e = fma(b[2 * j2], v.x, e);
                        e = fma(b[2 * j2 + 1], v.y, e);
                    }
                }
                const d2 yl = row[DP >> 1], ow = row[(DP >> 1) + 1];
                e += ow.x;
                double term, d, g;
                disp.obs(k, e, yl.x, yl.y, term, d, g);
                const bool live = ow.y != 0.0;
                ll += live ? ow.y * term : 0.0;
                gt += live ? ow.y * g : 0.0;
                d = live ? ow.y * d : 0.0;
#pragma unroll
                for (int j2 = 0; j2 < DMAX / 2; ++j2) {
                    if (2 * j2 < DP) {
                        const d2 v = row[j2];
                        acc[2 * j2] = fma(d, v.x, acc[2 * j2]);
                        acc[2 * j2 + 1] = fma(d, v.y, acc[2 * j2 + 1]);
                    }
                }
            }
            // ---- 3. reduce-scatter of the gradient partials; tau's sum to the lane that owns coordinate Dc
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
