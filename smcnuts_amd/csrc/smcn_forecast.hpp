// Forecasts of the arma target: the h-step conditional laws of y_{T+1..T+H} per particle, their weighted mixture over the
// particles (moments, cdf at thresholds, log predictive densities of a held-out continuation) as mergeable partials, and
// simulated paths.  Owned by smcn_forecast.hip.
//
// Definitions.  Per point x = (mu, beta, theta, s), sigma = exp(s) (the device library's exp), s2 = sigma * sigma, and
// the series y_1..y_T of the context (arma.stan: y_0 := mu, err_0 := 0):
//   in-sample innovation   err_1 = fma(-beta, mu, y_1 - mu)
//                          err_t = fma(-theta, err_{t-1}, fma(-beta, y_{t-1}, y_t - mu))
//                          (ArmaLaneModel::recur's expressions: err_T has the density's bits)
//   h-step law             y_{T+h} | y_{1:T}, x ~ N(m_h, v_h)
//                          m_1 = fma(theta, err_T, fma(beta, y_T, mu)),  m_h = fma(beta, m_{h-1}, mu)
//                          psi_0 = 1, psi_1 = beta + theta, psi_j = beta * psi_{j-1};  C_1 = 1, C_h = fma(psi_{h-1}, psi_{h-1}, C_{h-1})
//                          v_h = s2 * C_h        (iterative: no 1 / (1 - beta), no stationarity assumed)
//   bad at h               sigma, m_h or v_h non-finite, or v_h <= 0
//   marginal term          a_h = -0.5 (log(2 pi) + log v_h) - 0.5 (yf_h - m_h)^2 / v_h              (NaN when bad at h)
//   joint term             the recurrence continued through the held-out values, yf_0 := y_T, e_0 := err_T:
//                          e_j = fma(-theta, e_{j-1}, fma(-beta, yf_{j-1}, yf_j - mu)),  r_j = e_j / sigma
//                          l_j = (-0.5 log(2 pi) - s) - 0.5 r_j^2,   J_h = J_{h-1} + l_h  (J_0 = 0)
//                          J_h is llik(y_{1:T}, yf_{1:h}) - llik(y_{1:T}) of the arma density
//   cdf                    Phi((at_hk - m_h) / sqrt(v_h)) = 0.5 erfc(-z / sqrt 2)
//
// Mixture over the contributing particles (finite lw), lw' = lw - mw, w = exp(lw'): the partials row of horizon h
// (column layout: include/smcnuts_hip.h, smcn_forecast_partials).  A particle that is bad at h is counted in nbad_h and
// adds nothing to row h; a term a_h or J_h that is not finite adds nothing to its log-sum-exp.  The moments are summed
// about a shift c: per wavefront its own weighted mean of m_h (formed about the m_h of its first such particle with
// w > 0); merged blocks keep the first block's.
//
// Paths.  Slot s takes the particle a_s; z_{s,h} = the Box-Muller cosine (box_muller_lean) of the uniforms q = 0, 1 of
// philox_uniform(seed, iter = s, particle = h, stream 21), h = 1..H; e_h = sigma * z_{s,h};
//   y_{T+1} = m_1 + e_1,   y_{T+h} = fma(theta, e_{h-1}, fma(beta, y_{T+h-1}, mu)) + e_h.
// From the first non-finite value on a path is NaN.  A value depends on (seed, s, h) and its ancestor alone.
//
// Shape.  One LANE per particle (per slot): the T-step chain is two dependent fma per step, y_t is wave-uniform and comes
// from scalar loads.  forecast_partials_kernel then walks h = 1..H: every lane advances its law by one step, the
// wavefront reduces the row's Q values (group_sum<64>'s butterfly; maxima first for the two log-sum-exps), the block's
// four wavefronts meet in LDS (two buffers in turn: one barrier per horizon) and the first Q threads merge them in
// wavefront order and write the slice's row.  A slice is a block's 256 particles: the slice count is a function of M
// alone.  forecast_merge_kernel merges the slices in slice order, groups of kFcGroup first, one thread per (h, column).
// No atomics anywhere: a repeated call returns identical bits.
#pragma once
#include "smcn_device.hpp"

namespace smcn {

constexpr int kFcBlock = 256;            // particles of a slice
constexpr int kFcGroup = 16;             // slices a thread of stage 1 merges
constexpr int kFcMaxH = 512, kFcMaxAt = 16;
constexpr int kFcCols = 10, kFcMaxQ = kFcCols + kFcMaxAt;
enum : int { FC_MA = 0, FC_SA, FC_MJ, FC_SJ, FC_NBAD, FC_C, FC_SW, FC_S1, FC_S2, FC_V };
enum : uint32_t { kStreamFcAnc = 20, kStreamFcNoise = 21 };
constexpr double kFcSqrtHalf = 0.70710678118654752440;

using fc_cptr = const __attribute__((address_space(4))) double*;

__device__ __forceinline__ double fc_exp_neg(double d) { return exp_fast(fmax(-fabs(d), -800.0)); }

// One particle's laws, advanced a horizon at a time
struct FcLane {
    double mu, beta, theta, s, sigma, s2, err;      // err: err_T
    double m, P, C, v;                              // the law of the current horizon
    double e, yp, J;                                // the continued recurrence: e_{h}, yf_{h}, J_h
    bool sig_ok, bad;

    // md = [T, y_1..y_T]; the chain
    __device__ __forceinline__ void init(const double* md, double x0, double x1, double x2, double x3) {
        const fc_cptr y = (fc_cptr)md + 1;
        const int T = __builtin_amdgcn_readfirstlane((int)((fc_cptr)md)[0]);
        mu = x0; beta = x1; theta = x2; s = x3;
        const double nth = -theta, nbeta = -beta;
        double yq = y[0];
        err = fma(nbeta, mu, yq - mu);
#pragma unroll 8
        for (int t = 1; t < T; ++t) {
            const double yt = y[t];
            err = fma(nth, err, fma(nbeta, yq, yt - mu));
            yq = yt;
        }
        sigma = exp(s);
        s2 = sigma * sigma;
        sig_ok = finite_d(sigma);
        m = fma(beta, yq, mu);          // (m_1 less its theta err_T: step(1) adds it)
        P = 1.0; C = 1.0; v = s2;
        e = err; yp = yq; J = 0.0;
        bad = true;
    }
    // to horizon h (1-based, called in turn)
    __device__ __forceinline__ void step(int h) {
        if (h == 1) {
            m = fma(theta, err, m);
        } else {
            m = fma(beta, m, mu);
            P = h == 2 ? beta + theta : beta * P;
            C = fma(P, P, C);
            v = s2 * C;
        }
        bad = !(sig_ok && finite_d(m) && finite_d(v) && v > 0.0);
    }
    __device__ __forceinline__ double marginal(double yf) const {
        const double d = yf - m;
        return bad ? __builtin_nan("") : -0.5 * (kLog2Pi + log(v)) - 0.5 * (d * d) / v;
    }
    // J_h, the held-out value yf of this horizon taken into the recurrence
    __device__ __forceinline__ double joint(double yf) {
        e = fma(-theta, e, fma(-beta, yp, yf - mu));
        yp = yf;
        const double r = e / sigma;
        J += (-0.5 * kLog2Pi - s) - 0.5 * (r * r);
        return J;
    }
    __device__ __forceinline__ double cdf(double at) const {
        return 0.5 * erfc(-((at - m) / sqrt(v)) * kFcSqrtHalf);
    }
};

// ---- the plain form: out[t][1 + 2H (+ 2H)] = err_T, m_1..m_H, v_1..v_H (, a_1..a_H, J_1..J_H) ---------------------------
__global__ void __launch_bounds__(kFcBlock) forecast_points_kernel(const double* __restrict__ md, const double* __restrict__ x,
                                                                   int64_t M, int H, const double* __restrict__ yf,
                                                                   double* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * kFcBlock + threadIdx.x;
    const bool live = t < M;
    const int64_t tq = live ? t : M - 1;
    const double* const xp = x + tq * 4;
    const double x0 = xp[0], x1 = xp[1], x2 = xp[2], x3 = xp[3];
    FcLane L;
    L.init(md, x0, x1, x2, x3);
    const bool fin = finite_d(x0) && finite_d(x1) && finite_d(x2) && finite_d(x3);
    const double nan = __builtin_nan("");
    const int W = 1 + (yf ? 4 : 2) * H;
    double* const o = out + tq * W;
    if (live) o[0] = fin ? L.err : nan;
    const fc_cptr yfc = (fc_cptr)yf;
    for (int h = 1; h <= H; ++h) {
        L.step(h);
        double a = nan, J = nan;
        if (yf) {
            const double yv = yfc[h - 1];
            a = L.marginal(yv);
            J = L.joint(yv);
        }
        if (live) {
            o[h] = fin ? L.m : nan;
            o[H + h] = fin ? L.v : nan;
            if (yf) {
                o[2 * H + h] = fin ? a : nan;
                o[3 * H + h] = fin ? J : nan;
            }
        }
    }
}

// ---- merging blocks of one weight scale, in order: column q of the merge of blocks 0..n-1, g(s, col) block s's value -----
// (ma, Sa), (mj, Sj): max-shifted sums; (c, SW, S1, S2): re-centred on the first block that has a c; the rest: plain sums
template <class G>
__device__ __forceinline__ double fc_merge(int q, int64_t n, G&& g) {
    if (q <= FC_SJ) {
        const int cm = q <= FC_SA ? FC_MA : FC_MJ;
        double ma = -kInf, Sa = 0.0;
        for (int64_t s = 0; s < n; ++s) {
            const double m2 = g(s, cm), s2 = g(s, cm + 1);
            if (s2 > 0.0) {
                const double e = fc_exp_neg(m2 - ma);
                if (m2 > ma) {
                    Sa = fma(Sa, e, s2);
                    ma = m2;
                } else {
                    Sa = fma(s2, e, Sa);
                }
            }
        }
        return q == cm ? ma : Sa;
    }
    if (q >= FC_C && q <= FC_S2) {
        double c = __builtin_nan(""), SW = 0.0, S1 = 0.0, S2 = 0.0;
        for (int64_t s = 0; s < n; ++s) {
            const double sws = g(s, FC_SW), c2 = g(s, FC_C);
            if (c2 == c2) {
                if (c != c) {
                    c = c2;
                    S1 = g(s, FC_S1);
                    S2 = g(s, FC_S2);
                } else {
                    const double dl = c2 - c, t1 = g(s, FC_S1);
                    S2 += g(s, FC_S2) + dl * (2.0 * t1 + dl * sws);
                    S1 += t1 + dl * sws;
                }
            }
            SW += sws;
        }
        return q == FC_C ? c : (q == FC_SW ? SW : (q == FC_S1 ? S1 : S2));
    }
    double v = 0.0;
    for (int64_t s = 0; s < n; ++s) v += g(s, q);
    return v;
}

__device__ __forceinline__ double fc_wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}
// the wavefront's (max, sum exp(. - max)) of the lanes' terms; a lane without a finite term passes -inf
__device__ __forceinline__ void fc_wave_lse(double term, double& mx, double& S) {
    mx = fc_wave_max(term);
    const double e = term > -kInf ? fc_exp_neg(term - mx) : 0.0;
    S = group_sum<64>(e);
}

// ---- the slices' partials: part[(slice * Q + col) * H + (h - 1)], slice = blockIdx.x (particles t0 + 256 slice ..) ------
template <bool HASY>
__global__ void __launch_bounds__(kFcBlock) forecast_partials_kernel(const double* __restrict__ md, const double* __restrict__ x,
                                                                     int64_t rs, int64_t cs, const double* __restrict__ lw,
                                                                     const double* __restrict__ head, int64_t M, int64_t t0,
                                                                     int H, int Tn, const double* __restrict__ yf,
                                                                     const double* __restrict__ at, double* __restrict__ part) {
    __shared__ double sh[2][4][kFcMaxQ];
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int Q = kFcCols + Tn;
    const int64_t t = t0 + (int64_t)blockIdx.x * kFcBlock + tid;
    const bool live = t < M;
    const int64_t tq = live ? t : M - 1;
    const double* const xp = x + tq * rs;
    FcLane L;
    L.init(md, xp[0], xp[cs], xp[2 * cs], xp[3 * cs]);
    const double lwq = lw[tq];
    const bool contrib = live && finite_d(lwq);
    const double lwp = contrib ? lwq - head[0] : 0.0;
    const double w = contrib ? fc_exp_neg(lwp) : 0.0;
    const fc_cptr yfc = (fc_cptr)yf, atc = (fc_cptr)at;
    double* const slab = part + (int64_t)blockIdx.x * Q * H;
    for (int h = 1; h <= H; ++h) {
        L.step(h);
        const bool ok = contrib && !L.bad;
        double* const mine = sh[h & 1][wv];
        if constexpr (HASY) {
            const double yv = yfc[h - 1];
            const double a = lwp + L.marginal(yv), J = lwp + L.joint(yv);
            double mx, S;
            fc_wave_lse((ok && finite_d(a)) ? a : -kInf, mx, S);
            if (lane == 0) { mine[FC_MA] = mx; mine[FC_SA] = S; }
            fc_wave_lse((ok && finite_d(J)) ? J : -kInf, mx, S);
            if (lane == 0) { mine[FC_MJ] = mx; mine[FC_SJ] = S; }
        } else if (lane == 0) {
            mine[FC_MA] = -kInf; mine[FC_SA] = 0.0; mine[FC_MJ] = -kInf; mine[FC_SJ] = 0.0;
        }
        // the shift of the moments.  First the m_h of the first lane that counts and has a weight above 0 (a particle whose
        // weight has underflowed adds exactly 0 to every sum, and its m_h may be far from where the mass is); the
        // wavefront's weighted mean about that shift is then the shift the sums are taken about: a single particle's m_h
        // may lie many spreads from the mean (|beta| > 1), and S2 / SW - (S1 / SW)^2 would cancel by as much
        const unsigned long long okm = __ballot(ok && w > 0.0);
        const int first = okm ? (int)__builtin_ctzll(okm) : 0;
        const double c0 = okm ? group_read<64>(L.m, first) : __builtin_nan("");
        const double wk = ok ? w : 0.0;
        const double nb = group_sum<64>((contrib && L.bad) ? 1.0 : 0.0);
        const double SW = group_sum<64>(wk);
        const double mbar = c0 + group_sum<64>(wk * (ok ? L.m - c0 : 0.0)) / SW;
        const double c = finite_d(mbar) ? mbar : c0;
        const double dl = ok ? L.m - c : 0.0, wd = wk * dl;
        const double S1 = group_sum<64>(wd), S2 = group_sum<64>(wd * dl);
        const double V = group_sum<64>(ok ? wk * L.v : 0.0);
        if (lane == 0) {
            mine[FC_NBAD] = nb; mine[FC_C] = c; mine[FC_SW] = SW; mine[FC_S1] = S1; mine[FC_S2] = S2; mine[FC_V] = V;
        }
        for (int k = 0; k < Tn; ++k) {
            const double p = group_sum<64>(ok ? wk * L.cdf(atc[(int64_t)(h - 1) * Tn + k]) : 0.0);
            if (lane == 0) mine[kFcCols + k] = p;
        }
        __syncthreads();
        if (tid < Q) {
            const double (*blk)[kFcMaxQ] = sh[h & 1];
            slab[(int64_t)tid * H + (h - 1)] = fc_merge(tid, 4, [&](int64_t s, int col) { return blk[s][col]; });
        }
    }
}

// Stage 1 (FINAL = false): out[(group * Q + col) * H + h] = the merge of the group's slices; stage 2: res[(1 + h) * Q + col]
// = the merge of all n blocks of `in`, and res's row 0 the header.  One thread per (h, col).
template <bool FINAL>
__global__ void forecast_merge_kernel(const double* __restrict__ in, const double* __restrict__ head, int64_t n, int H, int Q,
                                      double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (FINAL && i < Q) out[i] = i < 4 ? head[i] : 0.0;
    if (i >= (int64_t)H * Q) return;
    const int h = (int)(i % H), q = (int)(i / H);
    const int64_t s0 = FINAL ? 0 : (int64_t)blockIdx.y * kFcGroup;
    const int64_t cnt = FINAL ? n : (s0 + kFcGroup < n ? kFcGroup : n - s0);
    const double* const base = in + s0 * Q * H + h;
    const double r = fc_merge(q, cnt, [&](int64_t s, int col) { return base[(s * Q + col) * H]; });
    if (FINAL) out[(int64_t)(1 + h) * Q + q] = r;
    else out[((int64_t)blockIdx.y * Q + q) * H + h] = r;
}

// ---- paths: y[j][h - 1] of slot s_first + j from particle anc[j] -------------------------------------------------------
__global__ void __launch_bounds__(kFcBlock) forecast_draws_kernel(const double* __restrict__ md, const double* __restrict__ x,
                                                                  int64_t rs, int64_t cs, const int64_t* __restrict__ anc,
                                                                  int64_t n, int64_t s_first, uint64_t seed, int H,
                                                                  double* __restrict__ y) {
    const int64_t j = (int64_t)blockIdx.x * kFcBlock + threadIdx.x;
    const bool live = j < n;
    const int64_t jq = live ? j : n - 1;
    const double* const xp = x + anc[jq] * rs;
    FcLane L;
    L.init(md, xp[0], xp[cs], xp[2 * cs], xp[3 * cs]);
    L.step(1);
    const uint32_t s = (uint32_t)(s_first + jq);
    double yv = L.m, ep = 0.0;
    bool dead = false;
    for (int h = 1; h <= H; ++h) {
        const u32x4 o = philox4x32_10({0u, (uint32_t)h, s, kStreamFcNoise}, (uint32_t)seed, (uint32_t)(seed >> 32));
        double z0, z1;
        box_muller_lean(u53(o.a, o.b), u53(o.c, o.d), z0, z1);
        const double e = L.sigma * z0;
        yv = (h == 1 ? L.m : fma(L.theta, ep, fma(L.beta, yv, L.mu))) + e;
        ep = e;
        dead = dead || !finite_d(yv);
        if (live) y[jq * H + (h - 1)] = dead ? __builtin_nan("") : yv;
    }
}

}  // namespace smcn
