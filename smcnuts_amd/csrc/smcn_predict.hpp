// Held-out prediction for the five regression targets: at NEW rows (X_new [, y_new, g_new]) the posterior predictive
// mean and variance (GLM families, hierarchical), the class probabilities (categorical, ordinal), the expected class
// index (ordinal) and log p(y_new_i | x_p) with its weighted log-sum-exp over particles (lpd), without forming a matrix.
//
// Shape: pw_walk's (smcn_pointwise.hpp).  A LANE owns a new row and keeps it in registers, a wavefront owns a tile of 64
// rows and walks a slice of the particles in chunks of 64; coordinate j of the chunk's particles is one coalesced load
// from the [D][N] state; what depends on a particle alone is formed once per chunk, one particle per lane; every
// statistic accumulates in the lane's own registers (no atomics); predict_combine_kernel merges the slices' partials in
// slice order, groups of kPwGroup first (the slice count is pointwise_slices(M, m)).  The new rows are a table of their
// own in the model's row layout (smcn_predict_set_data repacks them with the routine that repacks the training design).
//
// The GLM families ARE pw_walk, given the new rows' table.  The three other models have coordinates that pw_walk's
// read-out cannot address -- the register that holds coordinate c is fixed at compile time, and these models pick c at
// run time (z_{g_i}, c_{y_i}, b_{k, j} with c = k Dc + j) -- so the chunk's values of those coordinates go through a
// per-wavefront LDS area V[r][64 particles]:
//   hierarchical  the z block, r = group.  Row i reads z_{g_i} of particle q: one ds_read_b64 per (row, particle), where a
//                 gather from the state would be one 64-address vector load per (row, particle) for the same 8 bytes
//                 (Prediction).  e^lt and the dispersion constants: once per particle.
//   ordinal       the cutpoints (the sequential running sum, ord_constrain_kernel's order), log(1 - e^-delta_k) from u and,
//                 for the class probabilities, 1 - e^-delta_k from u: each formed ONCE per particle by the lane that
//                 holds it; row i reads c_{y_i}, c_{y_i + 1} and its middle term, and every cutpoint for the expected
//                 class index sum_k sigma(eta - c_k) (the reads of one k are one address: a broadcast).
//   categorical   all D coordinates: for particle q lane c reads coordinate c back -- GlmCatModel<64, 1>'s layout, a
//                 coordinate per lane -- and coefficient (k, j) is read out of lane k Dc + j as a scalar.  The row index
//                 j and the class k are compile-time (unrolled to the instantiation's capacity, guarded by the wave-uniform
//                 Dc and K), so neither the row nor the K logits / probabilities is indexed at run time.
// Element (r, q) lives at r * 64 + ((q + r) & 63), whose 8 bytes sit in the bank pair 2 ((q + r) mod 32) of the 64 banks.
// The chunk's writes (lane = particle, one r) and the categorical read (lane = coordinate r at one q) give each 32-lane
// group 32 distinct pairs.  The per-row reads (hierarchical r = g_i, ordinal r = y_i) are free of conflicts for r
// distinct modulo 32, and equal r is a broadcast; two lanes of a group whose r differ by exactly 32 (reachable: J up
// to 62, K up to 65) share a pair at different addresses, a 2-way conflict.  No padding is used.
//
// Partials (column layout: include/smcnuts_hip.h, smcn_predict_partials).  lw' = lw - mw, w = exp(lw'); over the
// contributing particles (finite lw):
//   ma, Sa        running maximum of lw' + ll and sum exp(lw' + ll - ma) over finite terms                    (lpd)
//   ninf          how many have ll = -inf;  nbad: how many have a non-finite mean / variance / probability
//   c, SW, S1, S2 the first mean E[y | x_p], sum w, sum w (mean - c), sum w (mean - c)^2   (mean, between-particle variance)
//   V             sum w Var(y | x_p)
//   EM, P_k       sum w sum_k sigma(eta - c_k);  sum w P(y = k | x_p)
#pragma once
#include "smcn_pw_walk.hpp"

namespace smcn {

constexpr int kPrColsGlm = 9;
enum : int { PR_MA = 0, PR_SA, PR_NINF, PR_NBAD, PR_C, PR_SW, PR_S1, PR_S2, PR_V };
constexpr int kPrCatP0 = 4;                 // categorical: P_0 .. P_{K-1} from here
constexpr int kPrOrdEM = 4, kPrOrdP0 = 5;   // ordinal: EM, then P_0 .. P_{K-1} (K <= kPrMaxProb only)
constexpr int kPrMaxProb = kCatMaxClasses;

struct PrArgs {
    const double* T;      // the new rows' table (the model's row layout, rows padded to a multiple of 64)
    const double* x;      // particle t's coordinate j at x[t * rs + j * cs]
    int64_t rs, cs, M;
    int64_t cps;          // chunks of 64 particles per slice
    int fam, m, Dc, J, K, D;   // family (hierarchical), new rows, columns of a row, groups, classes, coordinates
};

__device__ __forceinline__ double* pr_area() {
    extern __shared__ double pr_lds_[];
    return pr_lds_;
}
__device__ __forceinline__ int pr_slot(int r, int q) { return r * 64 + ((q + r) & 63); }
// A wave-uniform bound the compiler may not treat as loop-invariant.  The unrolled loops below guard step j by j < bound;
// hoisted out of the particle loop, each of those comparisons is kept as a 64-bit lane mask -- two SGPRs per j and loop,
// over 300 at capacity 64, spilled to VGPR lanes and read back every step.  Behind this the comparison is one s_cmp in
// place.
__device__ __forceinline__ int pr_opaque(int v) {
    asm volatile("" : "+s"(v));
    return v;
}

// what Var(y | x_p) takes from the dispersion coordinate alone: sigma^2 = e^2tau (normal), 1 / phi = e^-tau (NB2)
__device__ __forceinline__ double pr_var_const(int fam, double tau) {
    const double a = fam == 2 ? 2.0 * tau : -tau;
    return fam >= 2 ? exp_fast(fmin(fmax(a, -800.0), 800.0)) : 0.0;
}
// Var(y | x_p): Bernoulli p (1 - p), Poisson mu, normal sigma^2, NB2 mu + mu^2 / phi
__device__ __forceinline__ double pr_var(int fam, double mean, double vc) {
    return fam == 0 ? mean * (1.0 - mean) : (fam == 1 ? mean : (fam == 2 ? vc : fma(mean * mean, vc, mean)));
}

// lpd: log-sum-exp of lw' + ll around its running maximum (pointwise_stats_kernel's update)
struct PrLpd {
    double ma = -kInf, Sa = 0.0, ninf = 0.0;
    __device__ __forceinline__ void add(double lwq, double term) {
        const bool fin = term > -kInf;
        ninf += fin ? 0.0 : 1.0;
        const double v = lwq + (fin ? term : 0.0), d = v - ma, e = pw_exp_neg(d);
        const bool up = d > 0.0;
        const double Sn = up ? fma(Sa, e, 1.0) : Sa + e;
        Sa = fin ? Sn : Sa;
        ma = (fin && up) ? v : ma;
    }
};
// weighted moments of E[y | x_p] around the first one, and sum w Var(y | x_p)
struct PrMom {
    double c = __builtin_nan(""), SW = 0.0, S1 = 0.0, S2 = 0.0, V = 0.0, nbad = 0.0;
    __device__ __forceinline__ void add(double wq, double mean, double var) {
        const bool ok = finite_d(mean) && finite_d(var);
        nbad += ok ? 0.0 : 1.0;
        c = (ok && c != c) ? mean : c;
        const double dl = ok ? mean - c : 0.0, w = ok ? wq : 0.0, wd = w * dl;
        SW += w;
        S1 += wd;
        S2 = fma(wd, dl, S2);
        V = ok ? fma(w, var, V) : V;
    }
};
__device__ __forceinline__ void pr_store_glm(double* o, int64_t mpad, const PrLpd& L, const PrMom& Mo) {
    o[PR_MA * mpad] = L.ma;
    o[PR_SA * mpad] = L.Sa;
    o[PR_NINF * mpad] = L.ninf;
    o[PR_NBAD * mpad] = Mo.nbad;
    o[PR_C * mpad] = Mo.c;
    o[PR_SW * mpad] = Mo.SW;
    o[PR_S1 * mpad] = Mo.S1;
    o[PR_S2 * mpad] = Mo.S2;
    o[PR_V * mpad] = Mo.V;
}

// ---- GLM families: pw_walk on the new rows' table ----------------------------------------------------------------------
// (a.md is laid out as the context's model data, so pw_walk finds the table where it looks for it; the matrix form is
// pointwise_loglik_kernel itself)
template <int DPMAX, bool DISP, bool OW = false>
__global__ void __launch_bounds__(64) predict_glm_stats_kernel(PwArgs a, int64_t tiles, const double* __restrict__ lw,
                                                               const double* __restrict__ head, double* __restrict__ part) {
    const int64_t tile = blockIdx.x % tiles, slice = blockIdx.x / tiles;
    const int64_t i = tile * 64 + (threadIdx.x & 63u), mpad = tiles * 64;
    const double mw = head[0];
    const double nbmax = exp_fast(kLogDblMax);      // what pw_walk's NB2 mean is clamped to: e^eta overflows
    double vcv = 0.0;                               // (per lane: one particle of the chunk)
    int tbad = 0;
    PrLpd L;
    PrMom Mo;
    pw_walk<DPMAX, DISP, OW>(
        a, tile, slice,
        [&](int64_t t, bool have) {
            if constexpr (DISP) {
                const double tau = have ? a.x[t * a.rs + a.Dc * a.cs] : 0.0;
                vcv = pr_var_const(a.fam, tau);
                tbad = a.fam == 3 && !(tau <= kLogDblMax && tau >= kLogDblMinNormal);
            }
            return have ? lw[t] - mw : -kInf;
        },
        [&](int64_t t, double lwq, double wq, double term, double mean) {
            const int q = (int)(t & 63);
            if constexpr (DISP) {
                const bool over = a.fam == 3 && mean >= nbmax && group_read_i<64>(tbad, q) == 0;
                mean = over ? kInf : mean;
            }
            L.add(lwq, term);
            Mo.add(wq, mean, pr_var(a.fam, mean, DISP ? group_read<64>(vcv, q) : 0.0));
        });
    if (i < a.n) pr_store_glm(part + slice * kPrColsGlm * mpad + i, mpad, L, Mo);
}

// ---- hierarchical ------------------------------------------------------------------------------------------------------
// f(t, lwq, wq, term, mean, var): one (row, particle) pair, t, lwq, wq wave-uniform; alpha(t, tau, z_{g_i}) gives the
// row's intercept (pr_walk_hier: tau z_{g_i}, the fitted group's)
template <int DPMAX, bool DISP, class Chunk, class Term, class Alpha>
__device__ __forceinline__ void pr_walk_hier_alpha(const PrArgs& a, int64_t tile, int64_t slice, Chunk&& chunk, Term&& f,
                                                   Alpha&& alpha) {
    using d2 = double __attribute__((ext_vector_type(2)));
    double* const zb = pr_area();                  // z[j][particle]
    const int lane = (int)(threadIdx.x & 63u);
    const int Dc = a.Dc, J = a.J, DP = (Dc + 1) & ~1, RS = hglm_row_doubles(Dc);
    const d2* const rowp = (const d2*)(a.T + (tile * 64 + lane) * RS);
    double row[DPMAX];
#pragma unroll
    for (int j = 0; j < DPMAX; j += 2) {
        const d2 v = j < DP ? rowp[j >> 1] : d2{0.0, 0.0};
        row[j] = v.x;
        row[j + 1] = v.y;
    }
    const d2 yl = rowp[DP >> 1];
    const double y = yl.x, lgy = yl.y;
    const int gi = (int)rowp[(DP >> 1) + 1].x;     // (0 on the pad rows)
    const bool poisson = a.fam == 1, nb = a.fam == 3;

    const int64_t p_end = a.M < (slice + 1) * a.cps * 64 ? a.M : (slice + 1) * a.cps * 64;
    for (int64_t p0 = slice * a.cps * 64; p0 < p_end; p0 += 64) {
        const int64_t t = p0 + lane;
        const bool have = t < a.M;
        const double* const xp = a.x + (have ? t : 0) * a.rs;
        double xc[DPMAX];
        const int ncol = pr_opaque(Dc);
#pragma unroll
        for (int j = 0; j < DPMAX; ++j) xc[j] = (j < ncol && have) ? xp[j * a.cs] : 0.0;
        for (int j = 0; j < J; ++j) zb[pr_slot(j, lane)] = have ? xp[(Dc + j) * a.cs] : 0.0;
        const double tauv = exp_fast(have ? xp[(Dc + J) * a.cs] : 0.0);      // GlmHierModel: tau = e^lt
        const double ld = (DISP && have) ? xp[(Dc + J + 1) * a.cs] : 0.0;
        TauConst kc{};
        if constexpr (DISP) kc = glm_tau_const(nb, ld);
        const double vcv = pr_var_const(a.fam, ld);
        const int flv = (kc.big ? 1 : 0) | (kc.bad ? 2 : 0) | (tauv * tauv < kInf ? 0 : 4);   // (4: e^(2 lt) overflows)
        const double lwv = chunk(t, have);
        const double wv = finite_d(lwv) ? exp_fast(fmax(lwv, -800.0)) : 0.0;
        wave_exchange_fence();
        const int cnt = p_end - p0 < 64 ? (int)(p_end - p0) : 64;
#pragma unroll 1
        for (int q = 0; q < cnt; ++q) {
            const double lwq = group_read<64>(lwv, q);
            if (!finite_d(lwq)) continue;                  // (wave-uniform)
            double e0 = 0.0, e1 = 0.0;
            const int dpq = pr_opaque(DP);
#pragma unroll
            for (int j = 0; j < DPMAX; j += 2) {
                if (j < dpq) {                             // (wave-uniform)
                    e0 = fma(group_read<64>(xc[j], q), row[j], e0);
                    e1 = fma(group_read<64>(xc[j + 1], q), row[j + 1], e1);
                }
            }
            const double zq = zb[pr_slot(gi, q)];
            const double al = alpha(p0 + q, group_read<64>(tauv, q), zq);   // alpha_{g_i}
            const double eta = (e0 + e1) + al;
            const int fl = group_read_i<64>(flv, q);
            double term, mean;
            if constexpr (DISP) {
                TauConst k;
                k.tau = group_read<64>(kc.tau, q);
                k.phi = group_read<64>(kc.phi, q);
                k.iphi = group_read<64>(kc.iphi, q);
                k.c1 = group_read<64>(kc.c1, q);
                k.c2 = group_read<64>(kc.c2, q);
                k.big = (fl & 1) != 0;
                k.bad = (fl & 2) != 0;
                double d, gt;
                glm_disp_obs(nb, k, eta, y, lgy, term, d, gt);
                mean = nb ? (eta <= kLogDblMax ? exp_fast(eta) : kInf) : eta;
            } else {
                glm_canon_obs(poisson, eta, y, lgy, term, mean);
            }
            term = (fl & 6) ? -kInf : term;                // the particle's llik is -inf: every term
            f(p0 + q, lwq, group_read<64>(wv, q), term, mean, pr_var(a.fam, mean, group_read<64>(vcv, q)));
        }
        wave_exchange_fence();                             // (the next chunk's writes after these reads)
    }
}

template <int DPMAX, bool DISP, class Chunk, class Term>
__device__ __forceinline__ void pr_walk_hier(const PrArgs& a, int64_t tile, int64_t slice, Chunk&& chunk, Term&& f) {
    pr_walk_hier_alpha<DPMAX, DISP>(a, tile, slice, chunk, f, [](int64_t, double tauq, double zq) { return tauq * zq; });
}

template <int DPMAX, bool DISP>
__global__ void __launch_bounds__(64) predict_hier_loglik_kernel(PrArgs a, int64_t tiles, double* __restrict__ out) {
    const int64_t tile = blockIdx.x % tiles, slice = blockIdx.x / tiles;
    const int64_t i = tile * 64 + (threadIdx.x & 63u);
    pr_walk_hier<DPMAX, DISP>(
        a, tile, slice, [](int64_t, bool) { return 0.0; },
        [&](int64_t t, double, double, double term, double, double) {
            if (i < a.m) out[t * a.m + i] = term;
        });
}
template <int DPMAX, bool DISP>
__global__ void __launch_bounds__(64) predict_hier_stats_kernel(PrArgs a, int64_t tiles, const double* __restrict__ lw,
                                                                const double* __restrict__ head, double* __restrict__ part) {
    const int64_t tile = blockIdx.x % tiles, slice = blockIdx.x / tiles;
    const int64_t i = tile * 64 + (threadIdx.x & 63u), mpad = tiles * 64;
    const double mw = head[0];
    PrLpd L;
    PrMom Mo;
    pr_walk_hier<DPMAX, DISP>(
        a, tile, slice, [&](int64_t t, bool have) { return have ? lw[t] - mw : -kInf; },
        [&](int64_t, double lwq, double wq, double term, double mean, double var) {
            L.add(lwq, term);
            Mo.add(wq, mean, var);
        });
    if (i < a.m) pr_store_glm(part + slice * kPrColsGlm * mpad + i, mpad, L, Mo);
}

// ---- ordinal -----------------------------------------------------------------------------------------------------------
// sigma(a) and sigma(-a) from one exponential (GlmModel's logistic pattern)
__device__ __forceinline__ void pr_sigmoid(double a, double& s, double& sc) {
    const double t = exp_fast(fmax(-fabs(a), -800.0));
    const double inv = rcp_nr(1.0 + t), ti = t * inv;
    s = a >= 0.0 ? inv : ti;
    sc = a >= 0.0 ? ti : inv;
}
// f(t, lwq, wq, term, em, P, ok, eta): em = sum_k sigma(eta - c_k), P[k] = P(y = k | x_p) (PROB), ok: all of them finite
template <int DPMAX, bool PROB, bool STATS, class Chunk, class Term>
__device__ __forceinline__ void pr_walk_ord(const PrArgs& a, int64_t tile, int64_t slice, Chunk&& chunk, Term&& f) {
    using d2 = double __attribute__((ext_vector_type(2)));
    constexpr int KP = PROB ? kPrMaxProb : 1;
    const int lane = (int)(threadIdx.x & 63u);
    const int p = a.Dc, Km1 = a.K - 1, DP = (p + 1) & ~1, RS = glm_row_doubles(p);
    double* const cut = pr_area();                 // c_{j+1}[particle], j = 0 .. K-2
    double* const lmid = cut + Km1 * 64;           // log(1 - e^-delta_j), delta_j = e^u_{j+1}: the middle class j's term
    double* const omid = lmid + Km1 * 64;          // (PROB) 1 - e^-delta_j
    const d2* const rowp = (const d2*)(a.T + (tile * 64 + lane) * RS);
    double row[DPMAX];
#pragma unroll
    for (int j = 0; j < DPMAX; j += 2) {
        const d2 v = j < DP ? rowp[j >> 1] : d2{0.0, 0.0};
        row[j] = v.x;
        row[j + 1] = v.y;
    }
    const int y = (int)rowp[DP >> 1].x;
    const bool mid = y >= 1 && y < Km1;

    const int64_t p_end = a.M < (slice + 1) * a.cps * 64 ? a.M : (slice + 1) * a.cps * 64;
    for (int64_t p0 = slice * a.cps * 64; p0 < p_end; p0 += 64) {
        const int64_t t = p0 + lane;
        const bool have = t < a.M;
        const double* const xp = a.x + (have ? t : 0) * a.rs;
        double xc[DPMAX];
        const int ncol = pr_opaque(p);
#pragma unroll
        for (int j = 0; j < DPMAX; ++j) xc[j] = (j < ncol && have) ? xp[j * a.cs] : 0.0;
        // the particle's cutpoints, the sequential running sum; the middle classes' terms from u
        double cK = 0.0;
#pragma unroll 1
        for (int j = 0; j < Km1; ++j) {
            const double u = have ? xp[(p + j) * a.cs] : 0.0;
            const double ev = j >= 1 ? exp(u) : u;
            cK += ev;
            cut[pr_slot(j, lane)] = cK;
            if (j >= 1) {
                const double o = -expm1(-ev);
                lmid[pr_slot(j, lane)] = u < -36.0 ? u : log(o);   // (GlmOrdModel: e^u is below the rounding of 1)
                if constexpr (PROB && STATS) omid[pr_slot(j, lane)] = o;
            }
        }
        const int badv = finite_d(cK) ? 0 : 1;             // a cutpoint is not finite: llik = -inf
        const double lwv = chunk(t, have);
        const double wv = finite_d(lwv) ? exp_fast(fmax(lwv, -800.0)) : 0.0;
        wave_exchange_fence();
        const int cnt = p_end - p0 < 64 ? (int)(p_end - p0) : 64;
#pragma unroll 1
        for (int q = 0; q < cnt; ++q) {
            const double lwq = group_read<64>(lwv, q);
            if (!finite_d(lwq)) continue;                  // (wave-uniform)
            double e0 = 0.0, e1 = 0.0;
            const int dpq = pr_opaque(DP);
#pragma unroll
            for (int j = 0; j < DPMAX; j += 2) {
                if (j < dpq) {                             // (wave-uniform)
                    e0 = fma(group_read<64>(xc[j], q), row[j], e0);
                    e1 = fma(group_read<64>(xc[j + 1], q), row[j + 1], e1);
                }
            }
            const double eta = e0 + e1;
            const double lo = cut[pr_slot(y >= 1 ? y - 1 : 0, q)];
            const double hi = cut[pr_slot(y < Km1 ? y : Km1 - 1, q)];
            double term, de, glo, ghi;
            glm_ord_obs(Km1, eta, y, lo, hi, term, de, glo, ghi);
            term += mid ? lmid[pr_slot(mid ? y : 1, q)] : 0.0;
            term = group_read_i<64>(badv, q) ? -kInf : term;
            double em = 0.0, P[KP];
#pragma unroll
            for (int k = 0; k < KP; ++k) P[k] = 0.0;
            if constexpr (STATS && PROB) {
                double sprev = 1.0;                        // sigma(eta - c_0), c_0 = -inf
#pragma unroll
                for (int k = 0; k < kPrMaxProb; ++k) {
                    if (k < Km1) {                         // class k: sigma(eta - c_k) sigma(c_{k+1} - eta) (1 - e^-delta_k)
                        double s, sc;
                        pr_sigmoid(eta - cut[pr_slot(k, q)], s, sc);
                        em += s;
                        const double pk = sprev * sc;
                        P[k] = k >= 1 ? pk * omid[pr_slot(k, q)] : pk;
                        sprev = s;
                    } else if (k == Km1) {
                        P[k] = sprev;
                    }
                }
            } else if constexpr (STATS) {
#pragma unroll 1
                for (int k = 0; k < Km1; ++k) {
                    double s, sc;
                    pr_sigmoid(eta - cut[pr_slot(k, q)], s, sc);
                    em += s;
                }
            }
            f(p0 + q, lwq, group_read<64>(wv, q), term, em, P, finite_d(em), eta);
        }
        wave_exchange_fence();                             // (the next chunk's writes after these reads)
    }
}

template <int DPMAX>
__global__ void __launch_bounds__(64) predict_ord_loglik_kernel(PrArgs a, int64_t tiles, double* __restrict__ out) {
    const int64_t tile = blockIdx.x % tiles, slice = blockIdx.x / tiles;
    const int64_t i = tile * 64 + (threadIdx.x & 63u);
    pr_walk_ord<DPMAX, false, false>(
        a, tile, slice, [](int64_t, bool) { return 0.0; },
        [&](int64_t t, double, double, double term, double, const double (&)[1], bool, double) {
            if (i < a.m) out[t * a.m + i] = term;
        });
}
template <int DPMAX, bool PROB>
__global__ void __launch_bounds__(64) predict_ord_stats_kernel(PrArgs a, int64_t tiles, const double* __restrict__ lw,
                                                               const double* __restrict__ head, double* __restrict__ part) {
    constexpr int KP = PROB ? kPrMaxProb : 1;
    const int64_t tile = blockIdx.x % tiles, slice = blockIdx.x / tiles;
    const int64_t i = tile * 64 + (threadIdx.x & 63u), mpad = tiles * 64;
    const int Q = kPrOrdP0 + (PROB ? a.K : 0);
    const double mw = head[0];
    PrLpd L;
    double nbad = 0.0, EM = 0.0, PS[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) PS[k] = 0.0;
    pr_walk_ord<DPMAX, PROB, true>(
        a, tile, slice, [&](int64_t t, bool have) { return have ? lw[t] - mw : -kInf; },
        [&](int64_t, double lwq, double wq, double term, double em, const double (&P)[KP], bool ok, double) {
            L.add(lwq, term);
            nbad += ok ? 0.0 : 1.0;
            const double w = ok ? wq : 0.0;
            EM = ok ? fma(w, em, EM) : EM;
            if constexpr (PROB) {
#pragma unroll
                for (int k = 0; k < KP; ++k) PS[k] = ok ? fma(w, P[k], PS[k]) : PS[k];
            }
        });
    if (i < a.m) {
        double* const o = part + slice * Q * mpad + i;
        o[PR_MA * mpad] = L.ma;
        o[PR_SA * mpad] = L.Sa;
        o[PR_NINF * mpad] = L.ninf;
        o[PR_NBAD * mpad] = nbad;
        o[kPrOrdEM * mpad] = EM;
        if constexpr (PROB) {
#pragma unroll
            for (int k = 0; k < KP; ++k)
                if (k < a.K) o[(kPrOrdP0 + k) * mpad] = PS[k];
        }
    }
}

// ---- categorical -------------------------------------------------------------------------------------------------------
// GlmCatModel::softmax with the probabilities kept: e[k] becomes P(y = k + 1), p0 = P(y = 0); returns the term
template <int KM>
__device__ __forceinline__ double pr_cat_softmax(double (&e)[KM], int y, int Km1, double& p0, bool& ok) {
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
    auto ex = [](double a) { return exp_fast(a < -800.0 ? -800.0 : a); };
    const double e0 = ks == 0 ? 1.0 : ex(-m);
    double S = ks == 0 ? 0.0 : e0;
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
    p0 = e0 * inv;
    const double term = (ey - m) - l1;
    ok = finite_d(term) && finite_d(inv);
    return ok ? term : -kInf;                      // (GlmCatModel: -inf once a logit is not finite)
}
// f(t, lwq, wq, term, p0, P, ok): P[k] = P(y = k + 1 | x_p).  LFIN: f takes one more argument, whether
// every logit is finite (a -inf logit leaves the softmax, and so `ok`, finite)
template <int DCMAX, int KM, bool LFIN = false, class Chunk, class Term>
__device__ __forceinline__ void pr_walk_cat(const PrArgs& a, int64_t tile, int64_t slice, Chunk&& chunk, Term&& f) {
    using d2 = double __attribute__((ext_vector_type(2)));
    double* const xb = pr_area();                  // x[c][particle]
    const int lane = (int)(threadIdx.x & 63u);
    const int Dc = a.Dc, Km1 = a.K - 1, D = a.D, DP = (Dc + 1) & ~1, RS = glm_row_doubles(Dc);
    const d2* const rowp = (const d2*)(a.T + (tile * 64 + lane) * RS);
    double row[DCMAX];
#pragma unroll
    for (int j = 0; j < DCMAX; j += 2) {
        const d2 v = j < DP ? rowp[j >> 1] : d2{0.0, 0.0};
        row[j] = v.x;
        row[j + 1] = v.y;
    }
    const int y = (int)rowp[DP >> 1].x;

    const int64_t p_end = a.M < (slice + 1) * a.cps * 64 ? a.M : (slice + 1) * a.cps * 64;
    for (int64_t p0 = slice * a.cps * 64; p0 < p_end; p0 += 64) {
        const int64_t t = p0 + lane;
        const bool have = t < a.M;
        const double* const xp = a.x + (have ? t : 0) * a.rs;
#pragma unroll 4
        for (int c = 0; c < D; ++c) xb[pr_slot(c, lane)] = have ? xp[c * a.cs] : 0.0;
        const double lwv = chunk(t, have);
        const double wv = finite_d(lwv) ? exp_fast(fmax(lwv, -800.0)) : 0.0;
        wave_exchange_fence();
        const int cnt = p_end - p0 < 64 ? (int)(p_end - p0) : 64;
#pragma unroll 1
        for (int q = 0; q < cnt; ++q) {
            const double lwq = group_read<64>(lwv, q);
            if (!finite_d(lwq)) continue;                  // (wave-uniform)
            const double xq = lane < D ? xb[pr_slot(lane, q)] : 0.0;   // particle q: coordinate c on lane c
            double e[KM];
#pragma unroll
            for (int k = 0; k < KM; ++k) e[k] = 0.0;
#pragma unroll
            for (int j = 0; j < DCMAX; ++j) {
                if (j < Dc) {                              // (wave-uniform, as k < Km1)
#pragma unroll
                    for (int k = 0; k < KM; ++k)
                        if (k < Km1) e[k] = fma(group_read<64>(xq, k * Dc + j), row[j], e[k]);
                }
            }
            [[maybe_unused]] bool lfin = true;
            if constexpr (LFIN) {
#pragma unroll
                for (int k = 0; k < KM; ++k)
                    if (k < Km1) lfin = lfin && finite_d(e[k]);
            }
            double pz;
            bool ok;
            const double term = pr_cat_softmax<KM>(e, y, Km1, pz, ok);
            if constexpr (LFIN) f(p0 + q, lwq, group_read<64>(wv, q), term, pz, e, ok, lfin);
            else f(p0 + q, lwq, group_read<64>(wv, q), term, pz, e, ok);
        }
        wave_exchange_fence();                             // (the next chunk's writes after these reads)
    }
}

template <int DCMAX, int KM>
__global__ void __launch_bounds__(64) predict_cat_loglik_kernel(PrArgs a, int64_t tiles, double* __restrict__ out) {
    const int64_t tile = blockIdx.x % tiles, slice = blockIdx.x / tiles;
    const int64_t i = tile * 64 + (threadIdx.x & 63u);
    pr_walk_cat<DCMAX, KM>(
        a, tile, slice, [](int64_t, bool) { return 0.0; },
        [&](int64_t t, double, double, double term, double, const double (&)[KM], bool) {
            if (i < a.m) out[t * a.m + i] = term;
        });
}
template <int DCMAX, int KM>
__global__ void __launch_bounds__(64) predict_cat_stats_kernel(PrArgs a, int64_t tiles, const double* __restrict__ lw,
                                                               const double* __restrict__ head, double* __restrict__ part) {
    const int64_t tile = blockIdx.x % tiles, slice = blockIdx.x / tiles;
    const int64_t i = tile * 64 + (threadIdx.x & 63u), mpad = tiles * 64;
    const int Q = kPrCatP0 + a.K;
    const double mw = head[0];
    PrLpd L;
    double nbad = 0.0, P0 = 0.0, PS[KM];
#pragma unroll
    for (int k = 0; k < KM; ++k) PS[k] = 0.0;
    pr_walk_cat<DCMAX, KM>(
        a, tile, slice, [&](int64_t t, bool have) { return have ? lw[t] - mw : -kInf; },
        [&](int64_t, double lwq, double wq, double term, double pz, const double (&P)[KM], bool ok) {
            L.add(lwq, term);
            nbad += ok ? 0.0 : 1.0;
            const double w = ok ? wq : 0.0;
            P0 = ok ? fma(w, pz, P0) : P0;
#pragma unroll
            for (int k = 0; k < KM; ++k) PS[k] = ok ? fma(w, P[k], PS[k]) : PS[k];
        });
    if (i < a.m) {
        double* const o = part + slice * Q * mpad + i;
        o[PR_MA * mpad] = L.ma;
        o[PR_SA * mpad] = L.Sa;
        o[PR_NINF * mpad] = L.ninf;
        o[PR_NBAD * mpad] = nbad;
        o[kPrCatP0 * mpad] = P0;
#pragma unroll
        for (int k = 0; k < KM; ++k)
            if (k + 1 < a.K) o[(kPrCatP0 + 1 + k) * mpad] = PS[k];
    }
}

// ---- merging the slices' partials --------------------------------------------------------------------------------------
// pointwise_combine_kernel's two stages for a block of Q columns: the (ma, Sa) pair is a max-shifted sum, (c, SW, S1, S2)
// -- MOM, the GLM layout -- are merged by re-centring on the first slice's shift, every other column is a plain sum (one
// call has one weight scale).  Slice order throughout.
template <bool FINAL>
__global__ void predict_combine_kernel(const double* __restrict__ part, const double* __restrict__ head, int64_t slices,
                                       int64_t m, int64_t mpad, int Q, int mom, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (FINAL && i == 0) {
        for (int q = 0; q < Q; ++q) out[q] = q < 4 ? head[q] : 0.0;
    }
    if (i >= m) return;
    const int64_t s0 = FINAL ? 0 : (int64_t)blockIdx.y * kPwGroup;
    const int64_t s1 = FINAL ? slices : (s0 + kPwGroup < slices ? s0 + kPwGroup : slices);
    double* const r = FINAL ? out + (1 + i) * Q : out + (int64_t)blockIdx.y * Q * mpad + i;
    const int64_t st = FINAL ? 1 : mpad;
    double ma = -kInf, Sa = 0.0;
    double c = __builtin_nan(""), SW = 0.0, S1 = 0.0, S2 = 0.0;
    for (int64_t s = s0; s < s1; ++s) {
        const double* const o = part + s * Q * mpad + i;
        const double m2 = o[PR_MA * mpad], s2 = o[PR_SA * mpad];
        if (s2 > 0.0) {
            const double e = pw_exp_neg(m2 - ma);
            if (m2 > ma) {
                Sa = fma(Sa, e, s2);
                ma = m2;
            } else {
                Sa = fma(s2, e, Sa);
            }
        }
        if (mom) {
            const double sws = o[PR_SW * mpad], c2 = o[PR_C * mpad];
            if (c2 == c2) {
                if (c != c) {
                    c = c2;
                    S1 = o[PR_S1 * mpad];
                    S2 = o[PR_S2 * mpad];
                } else {
                    const double dl = c2 - c, t1 = o[PR_S1 * mpad];
                    S2 += o[PR_S2 * mpad] + dl * (2.0 * t1 + dl * sws);
                    S1 += t1 + dl * sws;
                }
            }
            SW += sws;
        }
    }
    r[PR_MA * st] = ma;
    r[PR_SA * st] = Sa;
    if (mom) {
        r[PR_C * st] = c;
        r[PR_SW * st] = SW;
        r[PR_S1 * st] = S1;
        r[PR_S2 * st] = S2;
    }
    for (int col = PR_NINF; col < Q; ++col) {
        if (mom && col >= PR_C && col <= PR_S2) continue;
        double v = 0.0;
        for (int64_t s = s0; s < s1; ++s) v += part[(s * Q + col) * mpad + i];
        r[col * st] = v;
    }
}

}  // namespace smcn
