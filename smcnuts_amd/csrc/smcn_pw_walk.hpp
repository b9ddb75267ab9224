// The GLM walk over (observation tile) x (particle slice) that the pointwise, PSIS, prediction and draw kernels share
// (its shape: smcn_pointwise.hpp), its arguments, and the host-side choice of its instantiation.  No kernel lives here,
// so any unit may include it.
#pragma once
#include <type_traits>

#include "smcn_models.hpp"

namespace smcn {

constexpr int kPwCols = 11;
constexpr int kPwGroup = 16;   // slices a thread of the combine kernels merges in stage 1 (pointwise_combine_kernel)
enum : int { PW_MA = 0, PW_SA, PW_MB, PW_SB, PW_SB2, PW_C, PW_SW, PW_S1, PW_S2, PW_F, PW_NINF };

// particle slices of a call: enough wavefronts to fill the chip at small n (about 4096), whole chunks of 64 particles;
// a function of M and n only
__host__ __device__ inline int64_t pointwise_slices(int64_t M, int64_t n, int64_t* chunks_per_slice) {
    const int64_t tiles = (n + 63) / 64, chunks = (M + 63) / 64;
    int64_t want = (4096 + tiles - 1) / tiles;
    want = want < 1 ? 1 : (want > chunks ? chunks : want);
    const int64_t cps = (chunks + want - 1) / want;
    *chunks_per_slice = cps;
    return (chunks + cps - 1) / cps;
}

// e^-|d| for the running log-sum-exp updates; 0 below e^-800 (exp_fast wants a finite argument)
__device__ __forceinline__ double pw_exp_neg(double d) { return exp_fast(fmax(-fabs(d), -800.0)); }

struct PwArgs {
    const double* md;     // the context's model data (header, then the repacked table)
    const double* x;      // particle t's coordinate j at x[t * rs + j * cs]
    int64_t rs, cs, M;
    int64_t cps;          // chunks of 64 particles per slice
    int fam, n, p, Dc;
};

// Walks the slice's particles for the tile's 64 observations.  `chunk(lane's particle index, live)` returns the
// particle's log-weight term (per lane: one particle each); f(t, lwq, wq, term, mean) takes one term of the lane's
// observation, with t, lwq and wq = exp(lwq) wave-uniform; a functor that takes (t, lwq, wq, term, mean, eta, y, k) is
// handed the linear predictor, the lane's response and the particle's dispersion constants (zeros unless DISP) as well.
// Particles for which chunk() returns a non-finite value are passed over.
// OW: SMCN_MODEL_OGLM's table -- a row carries o_i and w_i behind lgamma(y_i + 1), the table lies at oglm_table_offset, and
// eta_i takes o_i.  A parameter, off by default, so that the walks of SMCN_MODEL_GLM keep their instruction streams.
template <int DPMAX, bool DISP, bool OW = false, class Chunk, class Term>
__device__ __forceinline__ void pw_walk(const PwArgs& a, int64_t tile, int64_t slice, Chunk&& chunk, Term&& f) {
    using d2 = double __attribute__((ext_vector_type(2)));
    const int lane = (int)(threadIdx.x & 63u);
    const int Dc = a.Dc, DP = (Dc + 1) & ~1, RS = OW ? oglm_row_doubles(Dc) : glm_row_doubles(Dc);
    const int npri = DISP ? Dc + 2 : Dc;
    const double* const T = a.md + (OW ? oglm_table_offset(npri, a.n, a.p) : glm_table_offset(npri, a.n, a.p));
    // the lane's row (rows are padded to a multiple of 64 with zeros: unmasked)
    const d2* const rowp = (const d2*)(T + (tile * 64 + lane) * RS);
    double row[DPMAX];
#pragma unroll
    for (int j = 0; j < DPMAX; j += 2) {
        const d2 v = j < DP ? rowp[j >> 1] : d2{0.0, 0.0};
        row[j] = v.x;
        row[j + 1] = v.y;
    }
    const d2 yl = rowp[DP >> 1];
    const double y = yl.x, lgy = yl.y;
    // (the weight slot is not read: a term is log p(y_i | x); weights belong to the training likelihood's sum)
    double off = 0.0;
    if constexpr (OW) off = rowp[(DP >> 1) + 1].x;
    const bool poisson = a.fam == 1, nb = a.fam == 3;

    const int64_t p_end = a.M < (slice + 1) * a.cps * 64 ? a.M : (slice + 1) * a.cps * 64;
    for (int64_t p0 = slice * a.cps * 64; p0 < p_end; p0 += 64) {
        const int64_t t = p0 + lane;
        const bool have = t < a.M;
        const double* const xp = a.x + (have ? t : 0) * a.rs;
        double xc[DPMAX];
#pragma unroll
        for (int j = 0; j < DPMAX; ++j) xc[j] = (j < Dc && have) ? xp[j * a.cs] : 0.0;
        const double lwv = chunk(t, have);
        const double wv = finite_d(lwv) ? exp_fast(fmax(lwv, -800.0)) : 0.0;
        TauConst kc{};
        if constexpr (DISP) kc = glm_tau_const(nb, have ? xp[Dc * a.cs] : 0.0);
        const int cnt = p_end - p0 < 64 ? (int)(p_end - p0) : 64;
#pragma unroll 1
        for (int q = 0; q < cnt; ++q) {
            const double lwq = group_read<64>(lwv, q);
            if (!finite_d(lwq)) continue;                  // (wave-uniform)
            double e0 = 0.0, e1 = 0.0;
#pragma unroll
            for (int j = 0; j < DPMAX; j += 2) {
                if (j < DP) {                              // (wave-uniform)
                    e0 = fma(group_read<64>(xc[j], q), row[j], e0);
                    e1 = fma(group_read<64>(xc[j + 1], q), row[j + 1], e1);
                }
            }
            double eta = e0 + e1;
            if constexpr (OW) eta += off;
            double term, mean;
            TauConst k{};
            if constexpr (DISP) {
                k.tau = group_read<64>(kc.tau, q);
                k.phi = group_read<64>(kc.phi, q);
                k.iphi = group_read<64>(kc.iphi, q);
                k.c1 = group_read<64>(kc.c1, q);
                k.c2 = group_read<64>(kc.c2, q);
                const int fl = group_read_i<64>((kc.big ? 1 : 0) | (kc.bad ? 2 : 0), q);
                k.big = (fl & 1) != 0;
                k.bad = (fl & 2) != 0;
                double d, gt;
                glm_disp_obs(nb, k, eta, y, lgy, term, d, gt);
                term = k.bad ? -kInf : term;               // the dispersion coordinate is out of range: every term
                mean = nb ? exp_fast(fmin(eta, kLogDblMax)) : eta;
            } else {
                glm_canon_obs(poisson, eta, y, lgy, term, mean);
            }
            if constexpr (std::is_invocable_v<Term&, int64_t, double, double, double, double, double, double, const TauConst&>)
                f(p0 + q, lwq, group_read<64>(wv, q), term, mean, eta, y, k);     // (smcn_calibration.hpp: the tails want these)
            else
                f(p0 + q, lwq, group_read<64>(wv, q), term, mean);
        }
    }
}

// ---- host side (static: a copy per unit, none in the library's symbol table) ---------------------------------------
// the GLM walk's arguments over the image `md` of the block L describes (the training data, or the new rows)
static inline PwArgs pw_args(const RegLayout& L, const double* md, const double* x, int64_t rs, int64_t cs, int64_t M, int64_t cps) {
    PwArgs a;
    a.md = md;
    a.x = x;
    a.rs = rs;
    a.cs = cs;
    a.M = M;
    a.cps = cps;
    a.fam = L.fam;
    a.n = (int)L.n;
    a.p = (int)L.p;
    a.Dc = L.Dc;
    return a;
}
// f(row capacity) for table rows of Dc columns: DP <= 16 / 32 / 64 doubles
template <class F>
static void row_cap(int Dc, F&& f) {
    const int DP = (Dc + 1) & ~1;
    if (DP <= 16) f(std::integral_constant<int, 16>{});
    else if (DP <= 32) f(std::integral_constant<int, 32>{});
    else f(std::integral_constant<int, 64>{});
}
// f(row capacity, dispersion family)
template <class F>
static void row_cap_disp(int Dc, int fam, F&& f) {
    row_cap(Dc, [&](auto dp) { fam >= 2 ? f(dp, std::true_type{}) : f(dp, std::false_type{}); });
}
// f(row capacity, dispersion family, offset table): the GLM walk's instantiation for the block L describes
template <class F>
static void row_cap_glm(const RegLayout& L, F&& f) {
    row_cap_disp(L.Dc, L.fam, [&](auto dp, auto disp) {
        L.model == SMCN_MODEL_OGLM ? f(dp, disp, std::true_type{}) : f(dp, disp, std::false_type{});
    });
}

}  // namespace smcn
