// One-step residual checks of the arma target: per particle the in-sample one-step means, standardised residuals, their
// autocorrelations and the Ljung-Box statistic, and their weighted mixture over the particles as mergeable partials.
// Included by smcn_forecast.hip (after smcn_forecast.hpp, whose wavefront helpers it uses); owns smcn_ctx's rs.
//
// Definitions, in this operation order.  Per point x = (mu, beta, theta, s), sigma = exp(s) (the device library's exp, as
// FcLane::init), and the series y_1..y_T of the context (y_0 := mu, err_0 := 0):
//   innovation       err_1 = fma(-beta, mu, y_1 - mu),  err_t = fma(-theta, err_{t-1}, fma(-beta, y_{t-1}, y_t - mu))
//                    (FcLane::init's expressions, ArmaLaneModel::recur's: err_T has the bits smcn_forecast_points reports)
//   one-step mean    nu_t = y_t - err_t
//   residual         r_t = err_t / sigma
//   one-step term    l_t = (-0.5 log(2 pi) - s) - 0.5 (r_t r_t)          (forecast's l_j; sum_t l_t is the arma log-likelihood)
//   PIT              Phi(r_t) = 0.5 erfc(-r_t sqrt(1/2))
//   bad at t         sigma not finite or not > 0, or err_t or r_t not finite
//                    (a particle whose err_t or r_t is finite but whose SQUARE is not -- beyond about 1e154, on its way to
//                    overflowing -- is not bad at t: its row's second moments, S2 and Z2, are then inf or NaN while nbad_t
//                    is still 0, its first moments are what fp64 gives, and its l_t = -inf adds nothing to the row's pair)
// With L lags (0 <= L <= 32, L <= T - 1), A_0 = A_1 = .. = 0 before t = 1 and r_t := 0 for t < 1:
//   A_0 = fma(r_t, r_t, A_0),  A_k = fma(r_t, r_{t-k}, A_k), k = 1..L, in ascending t
//   rho_k = A_k / A_0          (uncentred: the innovations have mean 0 under the model)
//   Q = (T (T + 2)) q_L,  q_0 = 0, q_k = q_{k-1} + (rho_k rho_k) / (T - k)     (ascending k; T, T + 2, T - k as doubles)
//   bad for the lag rows: bad at any t, or A_0 not finite or not > 0, or Q not finite
//
// Mixture over the contributing particles (finite lw), lw' = lw - mw, w = exp(lw'): a block is [1 + T + (L > 0 ? L + 1 : 0)]
// rows of kRsCols = 20 columns (include/smcnuts_hip.h, smcn_residuals_partials).  Row 0: the header of
// smcn_pointwise_partials.  Time row t over the contributing particles that are not bad at t; lag row k (k = 1..L) and
// the Q row over those not bad for the lag rows.  The shifted moments of nu_t, r_t, rho_k and Q follow forecast's rule:
// a wavefront's weighted mean, formed about the value of its first particle with w > 0; merged blocks keep the first
// block's shift.
//
// Shape.  One LANE per particle; y_t is wave-uniform and comes from scalar loads.  residuals_partials_kernel walks
// t = 1..T: every lane advances its chain by one step and its lag sums by one product per lag, the wavefront reduces the
// row's 12 values (group_sum<64>'s butterfly; the maximum first for the log-sum-exp; the bad count from a ballot), the
// block's four wavefronts meet in LDS (two buffers in turn: one barrier per row) and the first kRsCols threads merge
// them in wavefront order and write the slice's row.  The lag rows and the Q row follow in the same way.  The lag window
// (the L previous r_t) and the L + 1 sums are private arrays that only ever see compile-time indices (a register shift
// under the wave-uniform guard k <= L): they stay in registers.  The kernel is compiled for windows of 0, 16 and 32 lags.
// A slice is a block's 256 particles: the slice count is a function of M alone.  residuals_merge_kernel merges the
// slices in slice order, groups of kFcGroup first, one thread per (row, column).  No atomics: a repeated call returns
// identical bits.
#pragma once
#include "smcn_forecast.hpp"

namespace smcn {

constexpr int kRsMaxL = 32, kRsMaxAt = 8;
constexpr int kRsCols = 20;
enum : int { RS_ML = 0, RS_SL, RS_NBAD, RS_C, RS_SW, RS_S1, RS_S2, RS_V, RS_CZ, RS_Z1, RS_Z2, RS_U, RS_P0 };

// One particle's chain, advanced a step at a time
struct RsLane {
    double mu, nbeta, nth, s, sigma, lc, err, yq;
    double nu, r;                                   // of the current step
    bool sig_ok, bad, bad_any;

    __device__ __forceinline__ void init(double x0, double x1, double x2, double x3) {
        mu = x0; nbeta = -x1; nth = -x2; s = x3;
        sigma = exp(s);
        sig_ok = finite_d(sigma) && sigma > 0.0;
        lc = -0.5 * kLog2Pi - s;
        err = 0.0; yq = 0.0; nu = 0.0; r = 0.0;
        bad = true; bad_any = false;
    }
    // to step t (1-based, called in turn) with yt = y_t
    __device__ __forceinline__ void step(int t, double yt) {
        err = t == 1 ? fma(nbeta, mu, yt - mu) : fma(nth, err, fma(nbeta, yq, yt - mu));
        yq = yt;
        nu = yt - err;
        r = err / sigma;
        bad = !(sig_ok && finite_d(err) && finite_d(r));
        bad_any = bad_any || bad;
    }
    __device__ __forceinline__ double term() const { return lc - 0.5 * (r * r); }
    __device__ __forceinline__ double pit() const { return 0.5 * erfc(-r * kFcSqrtHalf); }
};

// The lag window and the lag sums of one particle, for at most LM lags.  Every index is a compile-time constant once
// the loops are unrolled; which lags are live is the wave-uniform L
template <int LM>
struct RsLags {
    static constexpr int N = LM > 0 ? LM : 1;
    double win[N];           // win[j] = r_{t-1-j}
    double A[N + 1];

    __device__ __forceinline__ void init() {
#pragma unroll
        for (int k = 0; k < N; ++k) win[k] = 0.0;
#pragma unroll
        for (int k = 0; k <= N; ++k) A[k] = 0.0;
    }
    __device__ __forceinline__ void push(double r, int L) {
        A[0] = fma(r, r, A[0]);
#pragma unroll
        for (int k = LM; k >= 1; --k) {
            if (k <= L) {
                A[k] = fma(r, win[k - 1], A[k]);
                win[k - 1] = k >= 2 ? win[k - 2] : r;
            }
        }
    }
    // rho_k of a run-time k in 1..L
    __device__ __forceinline__ double rho(int k) const {
        double a = 0.0;
#pragma unroll
        for (int j = 1; j <= LM; ++j) a = j == k ? A[j] : a;
        return a / A[0];
    }
    __device__ __forceinline__ double ljung_box(int T, int L) const {
        double q = 0.0;
#pragma unroll
        for (int k = 1; k <= LM; ++k) {
            if (k <= L) {
                const double rk = A[k] / A[0];
                q = q + (rk * rk) / (double)(T - k);
            }
        }
        return ((double)T * (double)(T + 2)) * q;
    }
    // bad for the lag rows, given the chain's bad_any
    __device__ __forceinline__ bool bad(bool bad_any, double Q) const {
        return bad_any || !(finite_d(A[0]) && A[0] > 0.0) || !finite_d(Q);
    }
};

// ---- the plain form: out[t][W] = nu_1..nu_T, r_1..r_T (, rho_1..rho_L, Q), W = 2T + (L > 0 ? L + 1 : 0) ------------------
__global__ void __launch_bounds__(kFcBlock) residuals_points_kernel(const double* __restrict__ md, const double* __restrict__ x,
                                                                    int64_t M, int L, double* __restrict__ out) {
    const fc_cptr y = (fc_cptr)md + 1;
    const int T = __builtin_amdgcn_readfirstlane((int)((fc_cptr)md)[0]);
    const int64_t p = (int64_t)blockIdx.x * kFcBlock + threadIdx.x;
    const bool live = p < M;
    const int64_t pq = live ? p : M - 1;
    const double* const xp = x + pq * 4;
    const double x0 = xp[0], x1 = xp[1], x2 = xp[2], x3 = xp[3];
    const bool fin = finite_d(x0) && finite_d(x1) && finite_d(x2) && finite_d(x3);
    const double nan = __builtin_nan("");
    RsLane ln;
    ln.init(x0, x1, x2, x3);
    RsLags<kRsMaxL> lg;
    lg.init();
    const int64_t W = 2 * (int64_t)T + (L > 0 ? L + 1 : 0);
    double* const o = out + pq * W;
    for (int t = 1; t <= T; ++t) {
        ln.step(t, y[t - 1]);
        lg.push(ln.r, L);
        if (live) {
            o[t - 1] = fin ? ln.nu : nan;
            o[T + t - 1] = fin ? ln.r : nan;
        }
    }
    if (L > 0 && live) {
        for (int k = 1; k <= L; ++k) o[2 * (int64_t)T + k - 1] = fin ? lg.rho(k) : nan;
        o[2 * (int64_t)T + L] = fin ? lg.ljung_box(T, L) : nan;
    }
}

// ---- merging blocks of one weight scale, in order: column q of the merge of blocks 0..n-1, g(s, col) block s's value -----
// (ml, Sl): a max-shifted sum; (c, SW, S1, S2) and (cz, SW, Z1, Z2): re-centred on the first block that has a shift; the
// rest: plain sums
template <class G>
__device__ __forceinline__ double rs_merge(int q, int64_t n, G&& g) {
    if (q <= RS_SL) {
        double ma = -kInf, Sa = 0.0;
        for (int64_t s = 0; s < n; ++s) {
            const double m2 = g(s, RS_ML), s2 = g(s, RS_SL);
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
        return q == RS_ML ? ma : Sa;
    }
    const bool mom = q >= RS_C && q <= RS_S2, zed = q >= RS_CZ && q <= RS_Z2;
    if (mom || zed) {
        const int qc = mom ? RS_C : RS_CZ, q1 = mom ? RS_S1 : RS_Z1, q2 = mom ? RS_S2 : RS_Z2;
        double c = __builtin_nan(""), SW = 0.0, S1 = 0.0, S2 = 0.0;
        for (int64_t s = 0; s < n; ++s) {
            const double sws = g(s, RS_SW), c2 = g(s, qc);
            if (c2 == c2) {
                if (c != c) {
                    c = c2;
                    S1 = g(s, q1);
                    S2 = g(s, q2);
                } else {
                    const double dl = c2 - c, t1 = g(s, q1);
                    S2 += g(s, q2) + dl * (2.0 * t1 + dl * sws);
                    S1 += t1 + dl * sws;
                }
            }
            SW += sws;
        }
        return q == qc ? c : (q == RS_SW ? SW : (q == q1 ? S1 : S2));
    }
    double v = 0.0;
    for (int64_t s = 0; s < n; ++s) v += g(s, q);
    return v;
}

// the wavefront's shifted sums of v over its lanes `ok` (wk: their weights, 0 on the others; SW: the sum of wk)
__device__ __forceinline__ void rs_wave_moments(bool ok, double wk, double SW, double v, double& c, double& S1, double& S2) {
    // the shift: first the v of the first lane that counts and has a weight above 0, then the wavefront's weighted mean
    // about it (smcn_forecast.hpp: a particle whose weight has underflowed adds exactly 0, and its v may be far away)
    const unsigned long long okm = __ballot(ok && wk > 0.0);
    const int first = okm ? (int)__builtin_ctzll(okm) : 0;
    const double c0 = okm ? group_read<64>(v, first) : __builtin_nan("");
    const double mbar = c0 + group_sum<64>(wk * (ok ? v - c0 : 0.0)) / SW;
    c = finite_d(mbar) ? mbar : c0;
    const double dl = ok ? v - c : 0.0, wd = wk * dl;
    S1 = group_sum<64>(wd);
    S2 = group_sum<64>(wd * dl);
}

// ---- the slices' partials: part[(slice * kRsCols + col) * R + (row - 1)], slice = blockIdx.x (particles t0 + 256 slice ..),
// R = T + (L > 0 ? L + 1 : 0) rows: the time rows, the lag rows, the Q row -------------------------------------------------
template <int LM>
__global__ void __launch_bounds__(kFcBlock) residuals_partials_kernel(const double* __restrict__ md, const double* __restrict__ x,
                                                                      int64_t rs, int64_t cs, const double* __restrict__ lw,
                                                                      const double* __restrict__ head, int64_t M, int64_t t0,
                                                                      int L, int Tn, const double* __restrict__ q_at,
                                                                      double* __restrict__ part) {
    __shared__ double sh[2][4][kRsCols];
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const fc_cptr y = (fc_cptr)md + 1;
    const int T = __builtin_amdgcn_readfirstlane((int)((fc_cptr)md)[0]);
    const int R = T + (L > 0 ? L + 1 : 0);
    const int64_t p = t0 + (int64_t)blockIdx.x * kFcBlock + tid;
    const bool live = p < M;
    const int64_t pq = live ? p : M - 1;
    const double* const xp = x + pq * rs;
    RsLane ln;
    ln.init(xp[0], xp[cs], xp[2 * cs], xp[3 * cs]);
    RsLags<LM> lg;
    lg.init();
    const double s2 = ln.sigma * ln.sigma;
    const double lwq = lw[pq];
    const bool contrib = live && finite_d(lwq);
    const double lwp = contrib ? lwq - head[0] : 0.0;
    const double w = contrib ? fc_exp_neg(lwp) : 0.0;
    double* const slab = part + (int64_t)blockIdx.x * kRsCols * R;
    const double nan = __builtin_nan("");
    if (tid < 2 * 4 * kRsCols) (&sh[0][0][0])[tid] = 0.0;       // (the columns from RS_P0 on stay 0 up to the Q row)
    __syncthreads();
    // the merge of the block's four wavefronts of a row
    auto flush = [&](int row) {
        __syncthreads();
        if (tid < kRsCols) {
            const double (*blk)[kRsCols] = sh[row & 1];
            slab[(int64_t)tid * R + (row - 1)] = rs_merge(tid, 4, [&](int64_t s, int col) { return blk[s][col]; });
        }
    };
    for (int t = 1; t <= T; ++t) {
        ln.step(t, y[t - 1]);
        if constexpr (LM > 0) lg.push(ln.r, L);
        const bool ok = contrib && !ln.bad;
        double* const mine = sh[t & 1][wv];
        const double term = lwp + ln.term();
        double ml, Sl;
        fc_wave_lse((ok && finite_d(term)) ? term : -kInf, ml, Sl);
        const double nb = (double)__popcll(__ballot(contrib && ln.bad));
        const double wk = ok ? w : 0.0;
        const double SW = group_sum<64>(wk);
        double c, S1, S2, cz, Z1, Z2;
        rs_wave_moments(ok, wk, SW, ln.nu, c, S1, S2);
        rs_wave_moments(ok, wk, SW, ln.r, cz, Z1, Z2);
        const double V = group_sum<64>(ok ? wk * s2 : 0.0);
        const double U = group_sum<64>(ok ? wk * ln.pit() : 0.0);
        if (lane == 0) {
            mine[RS_ML] = ml; mine[RS_SL] = Sl; mine[RS_NBAD] = nb; mine[RS_C] = c; mine[RS_SW] = SW; mine[RS_S1] = S1;
            mine[RS_S2] = S2; mine[RS_V] = V; mine[RS_CZ] = cz; mine[RS_Z1] = Z1; mine[RS_Z2] = Z2; mine[RS_U] = U;
        }
        flush(t);
    }
    if constexpr (LM > 0) {
        if (L > 0) {
            const double Q = lg.ljung_box(T, L);
            const bool pbad = lg.bad(ln.bad_any, Q), ok = contrib && !pbad;
            const double nb = (double)__popcll(__ballot(contrib && pbad));
            const double wk = ok ? w : 0.0;
            const double SW = group_sum<64>(wk);
            const fc_cptr qc = (fc_cptr)q_at;
            for (int k = 1; k <= L + 1; ++k) {
                const int row = T + k;
                const bool last = k == L + 1;
                double* const mine = sh[row & 1][wv];
                double c, S1, S2;
                rs_wave_moments(ok, wk, SW, last ? Q : lg.rho(k), c, S1, S2);
                if (lane == 0) {
                    mine[RS_ML] = -kInf; mine[RS_SL] = 0.0; mine[RS_NBAD] = nb; mine[RS_C] = c; mine[RS_SW] = SW; mine[RS_S1] = S1;
                    mine[RS_S2] = S2; mine[RS_V] = 0.0; mine[RS_CZ] = nan; mine[RS_Z1] = 0.0; mine[RS_Z2] = 0.0; mine[RS_U] = 0.0;
                }
                if (last) {
                    for (int j = 0; j < Tn; ++j) {
                        const double e = group_sum<64>((ok && Q > qc[j]) ? wk : 0.0);
                        if (lane == 0) mine[RS_P0 + j] = e;
                    }
                }
                flush(row);
            }
        }
    }
}

// Stage 1 (FINAL = false): out[(group * kRsCols + col) * R + row] = the merge of the group's slices; stage 2:
// res[(1 + row) * kRsCols + col] = the merge of all n blocks of `in`, and res's row 0 the header.  One thread per (row, col).
template <bool FINAL>
__global__ void residuals_merge_kernel(const double* __restrict__ in, const double* __restrict__ head, int64_t n, int R,
                                       double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (FINAL && i < kRsCols) out[i] = i < 4 ? head[i] : 0.0;
    if (i >= (int64_t)R * kRsCols) return;
    const int row = (int)(i % R), q = (int)(i / R);
    const int64_t s0 = FINAL ? 0 : (int64_t)blockIdx.y * kFcGroup;
    const int64_t cnt = FINAL ? n : (s0 + kFcGroup < n ? kFcGroup : n - s0);
    const double* const base = in + s0 * kRsCols * R + row;
    const double r = rs_merge(q, cnt, [&](int64_t s, int col) { return base[(s * kRsCols + col) * R]; });
    if (FINAL) out[(int64_t)(1 + row) * kRsCols + q] = r;
    else out[((int64_t)blockIdx.y * kRsCols + q) * R + row] = r;
}

}  // namespace smcn
