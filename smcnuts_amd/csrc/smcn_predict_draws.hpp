// Posterior predictive DRAWS for the five regression targets: y[s][i] ~ p(. | x_{a_s}, new row i), S replicated data
// sets of the m new rows, each from ONE ancestor particle a_s (systematic resampling of the weights with S slots).
//
// Shape: the walks of smcn_predict.hpp (pw_walk, pr_walk_hier, pr_walk_ord, pr_walk_cat) with the gathered ancestors as
// "the particles": draws_ancestors_kernel searches the blocked cumulative sum (scan_tile_kernel, scan_offsets_kernel,
// cdf_search of smcn_weights.hpp), draws_gather_kernel copies the ancestors' coordinates into a [D][slots] array in the
// layout the walks read, and the model's draw kernel samples inside the walk's Term callback and stores y coalesced as
// out[slot * m + i] (lane = row).  FUSED = false (GLM families, hierarchical) is the two-pass form: the walk stores the
// law's mean (NaN once the law is undefined) and draws_sample_kernel samples it in place, one element per lane.
//
// Uniforms: philox_uniform(seed, iter = s, particle = i (the row), stream, q); streams 16 ancestor offset, 17 outcome,
// 18 gamma, 19 new-group intercept (particle = the group's label).  A draw depends on (seed, s, i) and its ancestor
// alone: not on tiles, slices, the slot range of the call or S.
//
// Bad draws are NaN (the host counts them): a non-finite eta, mean or cutpoint, mu > 2^53, a dispersion coordinate
// outside the range the density accepts, e^eta or e^(2 lt) overflowing, an attempt cap reached.
#pragma once
#include "smcn_predict.hpp"

namespace smcn {

enum : uint32_t { kStreamDrawAnc = 16, kStreamDrawOut = 17, kStreamDrawGamma = 18, kStreamDrawGroup = 19 };
constexpr double kDrawMaxMu = 9007199254740992.0;   // 2^53: above, the integers are no longer all representable
constexpr int kDrawAttempts = 64;                   // rejection samplers: attempts before the draw is given up (NaN)
constexpr int kDrawInvSteps = 1000;                 // Poisson inversion: steps
constexpr uint32_t kDrawBoostQ = 192;               // gamma stream: the uniform of the phi < 1 boost (3 * kDrawAttempts)

struct DrawKey {
    uint64_t seed;
    uint32_t s, i;
};
struct DrawArgs {
    uint64_t seed;
    int64_t s_first;          // the global slot of gathered particle 0
    const int64_t* newg;      // hierarchical: per row, the label of a NEW group (>= J), anything below J otherwise; or null
};

__device__ __forceinline__ double draw_nan() { return __builtin_nan(""); }
__device__ __forceinline__ double draw_u(const DrawKey& k, uint32_t stream, uint32_t q) {
    return philox_uniform(k.seed, k.s, k.i, stream, q);
}
// uniforms q and q + 1 of one Philox block (q even)
__device__ __forceinline__ void draw_u2(const DrawKey& k, uint32_t stream, uint32_t q, double& ua, double& ub) {
    const u32x4 o = philox4x32_10({q >> 1, k.i, k.s, stream}, (uint32_t)k.seed, (uint32_t)(k.seed >> 32));
    ua = u53(o.a, o.b);
    ub = u53(o.c, o.d);
}
// the library's Box-Muller, cosine branch
__device__ __forceinline__ double draw_normal(double u1, double u2) {
    double z0, z1;
    box_muller_lean(u1, u2, z0, z1);
    return z0;
}

// Poisson(mu): inversion below 10, Hoermann's PTRS from 10 (outcome stream).  NaN for mu outside [0, 2^53].
__device__ __forceinline__ double draw_poisson(double mu, const DrawKey& key) {
    if (!(mu >= 0.0 && mu <= kDrawMaxMu)) return draw_nan();
    if (mu < 10.0) {
        const double u = draw_u(key, kStreamDrawOut, 0u);
        double p = exp(-mu), F = p;
        int k = 0;
#pragma unroll 1
        while (u > F && k < kDrawInvSteps) {
            ++k;
            p *= mu / (double)k;
            F += p;
        }
        return u > F ? draw_nan() : (double)k;
    }
    const double b = 0.931 + 2.53 * sqrt(mu), a = -0.059 + 0.02483 * b;
    const double lial = log(1.1239 + 1.1328 / (b - 3.4)), vr = 0.9277 - 3.6224 / (b - 2.0), lmu = log(mu);
    double y = draw_nan();
#pragma unroll 1
    for (int t = 0; t < kDrawAttempts; ++t) {
        double ua, V;
        draw_u2(key, kStreamDrawOut, 2u * (uint32_t)t, ua, V);
        const double U = ua - 0.5, w = 0.5 - fabs(U);
        const double k = floor((2.0 * a / w + b) * U + mu + 0.43);
        if (w >= 0.07 && V <= vr) {
            y = k;
            break;
        }
        if (k < 0.0 || (w < 0.013 && V > w)) continue;
        double lg, psi;
        lgamma_digamma_pos(k + 1.0, lg, psi);
        if (log(V) + lial - log(a / (w * w) + b) <= -mu + k * lmu - lg) {
            y = k;
            break;
        }
    }
    return y;
}

// Gamma(phi, 1) by Marsaglia-Tsang (gamma stream); below 1 the shape phi + 1 and the boost u^(1 / phi).  NaN at the cap.
__device__ __forceinline__ double draw_gamma(double phi, const DrawKey& key) {
    const bool small = phi < 1.0;
    const double ap = small ? phi + 1.0 : phi;
    const double d = ap - 1.0 / 3.0, c = 1.0 / sqrt(9.0 * d);
    double G = draw_nan();
#pragma unroll 1
    for (int t = 0; t < kDrawAttempts; ++t) {
        const uint32_t q = 3u * (uint32_t)t;
        const double z = draw_normal(draw_u(key, kStreamDrawGamma, q), draw_u(key, kStreamDrawGamma, q + 1u));
        const double v1 = 1.0 + c * z, v = v1 * v1 * v1;
        if (v <= 0.0) continue;
        if (log1p(-draw_u(key, kStreamDrawGamma, q + 2u)) < 0.5 * z * z + d - d * v + d * log(v)) {
            G = d * v;
            break;
        }
    }
    if (small) G *= exp(log(draw_u(key, kStreamDrawGamma, kDrawBoostQ)) / phi);
    return G;
}

// What the sampler takes from the dispersion coordinate: sigma = e^tau (normal), phi = e^tau (NB2); `bad` under the
// density's own range rules (glm_tau_const) or once e^tau is not finite
__device__ __forceinline__ double draw_disp(int fam, double tau, int& bad) {
    const bool ok = fam == 2 ? (-2.0 * tau <= kLogDblMax && tau <= kLogDblMax)
                             : (fam == 3 ? (tau <= kLogDblMax && tau >= kLogDblMinNormal) : true);
    bad = ok ? 0 : 1;
    return (ok && fam >= 2) ? exp(tau) : 1.0;
}

// One outcome of a GLM family given the law's mean (p, mu, eta, mu) and the dispersion constant; a NaN mean is a bad draw
__device__ __forceinline__ double draw_family(int fam, double mean, double disp, const DrawKey& key) {
    if (!finite_d(mean)) return draw_nan();
    if (fam == 0) return draw_u(key, kStreamDrawOut, 0u) < mean ? 1.0 : 0.0;
    if (fam == 2) {
        double u1, u2;
        draw_u2(key, kStreamDrawOut, 0u, u1, u2);
        return mean + disp * draw_normal(u1, u2);
    }
    if (!(mean <= kDrawMaxMu)) return draw_nan();     // (NB2: the law's own mean, whatever the gamma factor makes of it)
    double mu = mean;
    if (fam == 3) mu = mean * (draw_gamma(disp, key) / disp);
    return draw_poisson(mu, key);
}

// ---- ancestors -------------------------------------------------------------------------------------------------------
// w = exp(lw - max finite lw), 0 for a non-finite log-weight (head: pointwise_header_kernel)
__global__ void draws_weights_kernel(const double* __restrict__ lw, const double* __restrict__ head, int64_t M,
                                     double* __restrict__ w) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= M) return;
    const double v = lw[t];
    w[t] = finite_d(v) ? pw_exp_neg(v - head[0]) : 0.0;
}
// a_s = min{p : C_p > (s + u0) / S}, u0 on Philox stream `stream`, on C = (tile offset + blocked scan) / total, clamped to the last contributing particle
__global__ void draws_ancestors_kernel(const double* __restrict__ local, const double* __restrict__ toff, int nt, int64_t M,
                                       const double* __restrict__ lw, int64_t S, int64_t s_first, int64_t s_count,
                                       uint64_t seed, uint32_t stream, int64_t* __restrict__ anc) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= s_count) return;
    const double total = toff[(M - 1) / kScanTile] + local[M - 1];
    const double u0 = philox_uniform(seed, 0u, 0u, stream, 0u);
    const double key = ((double)(s_first + j) + u0) / (double)S;
    int64_t lo = cdf_search(key, total, toff, local, nt, M, false);
    if (lo >= M) {
        lo = M - 1;
        while (lo > 0 && !finite_d(lw[lo])) --lo;
    }
    anc[j] = lo;
}
// xg[c][j] = coordinate c of particle anc[j] (the walks then read it with rs = 1, cs = n)
__global__ void draws_gather_kernel(const double* __restrict__ x, int64_t rs, int64_t cs, const int64_t* __restrict__ anc,
                                    int64_t n, int D, double* __restrict__ xg) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const double* const xp = x + anc[j] * rs;
    for (int c = 0; c < D; ++c) xg[(int64_t)c * n + j] = xp[c * cs];
}

// ---- GLM families ----------------------------------------------------------------------------------------------------
template <int DPMAX, bool DISP, bool FUSED, bool OW = false>
__global__ void __launch_bounds__(64) draws_glm_kernel(PwArgs a, int64_t tiles, DrawArgs d, double* __restrict__ out) {
    const int64_t tile = blockIdx.x % tiles, slice = blockIdx.x / tiles;
    const int64_t i = tile * 64 + (threadIdx.x & 63u);
    const double nbmax = exp_fast(kLogDblMax);      // what pw_walk's NB2 mean is clamped to: e^eta overflows
    double dv = 1.0;                                // (per lane: one particle of the chunk)
    int bv = 0;
    pw_walk<DPMAX, DISP, OW>(
        a, tile, slice,
        [&](int64_t t, bool have) {
            if constexpr (DISP) dv = draw_disp(a.fam, have ? a.x[t * a.rs + a.Dc * a.cs] : 0.0, bv);
            return 0.0;
        },
        [&](int64_t t, double, double, double, double mean) {
            const int q = (int)(t & 63);
            double disp = 1.0;
            if constexpr (DISP) {
                disp = group_read<64>(dv, q);
                const bool bad = group_read_i<64>(bv, q) != 0 || (a.fam == 3 && mean >= nbmax);
                mean = bad ? draw_nan() : mean;
            }
            if (i < a.n) {
                if constexpr (FUSED) {
                    const DrawKey key{d.seed, (uint32_t)(d.s_first + t), (uint32_t)i};
                    out[t * a.n + i] = draw_family(a.fam, mean, disp, key);
                } else {
                    out[t * a.n + i] = mean;
                }
            }
        });
}

// the second pass of the two-pass form: out[t][i] holds the law's mean; tau_row: the gathered dispersion coordinate or null
__global__ void __launch_bounds__(256) draws_sample_kernel(int fam, int64_t m, int64_t n, DrawArgs d,
                                                           const double* __restrict__ tau_row, double* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * m) return;
    const int64_t t = e / m, i = e - t * m;
    int bad = 0;
    const double disp = tau_row ? draw_disp(fam, tau_row[t], bad) : 1.0;
    const DrawKey key{d.seed, (uint32_t)(d.s_first + t), (uint32_t)i};
    out[e] = draw_family(fam, out[e], disp, key);
}

// ---- hierarchical ----------------------------------------------------------------------------------------------------
template <int DPMAX, bool DISP, bool FUSED>
__global__ void __launch_bounds__(64) draws_hier_kernel(PrArgs a, int64_t tiles, DrawArgs d, double* __restrict__ out) {
    const int64_t tile = blockIdx.x % tiles, slice = blockIdx.x / tiles;
    const int64_t i = tile * 64 + (threadIdx.x & 63u);
    const int64_t label = (d.newg && i < a.m) ? d.newg[i] : -1;
    const bool isnew = label >= a.J;
    double dv = 1.0;
    int bv = 0;
    pr_walk_hier_alpha<DPMAX, DISP>(
        a, tile, slice,
        [&](int64_t t, bool have) {
            const double* const xp = a.x + (have ? t : 0) * a.rs;
            const double tv = exp_fast(have ? xp[(a.Dc + a.J) * a.cs] : 0.0);
            int db = 0;
            if constexpr (DISP) dv = draw_disp(a.fam, have ? xp[(a.Dc + a.J + 1) * a.cs] : 0.0, db);
            bv = db | (tv * tv < kInf ? 0 : 1);          // (e^(2 lt) overflows: the particle's density is -inf)
            return 0.0;
        },
        [&](int64_t t, double, double, double, double mean, double) {
            const int q = (int)(t & 63);
            mean = group_read_i<64>(bv, q) != 0 ? draw_nan() : mean;
            const double disp = DISP ? group_read<64>(dv, q) : 1.0;
            if (i < a.m) {
                if constexpr (FUSED) {
                    const DrawKey key{d.seed, (uint32_t)(d.s_first + t), (uint32_t)i};
                    out[t * a.m + i] = draw_family(a.fam, mean, disp, key);
                } else {
                    out[t * a.m + i] = mean;
                }
            }
        },
        [&](int64_t t, double tauq, double zq) {
            if (isnew) {                                 // a fresh group: alpha = tau z, z keyed by (s, label)
                const DrawKey key{d.seed, (uint32_t)(d.s_first + t), (uint32_t)label};
                double u1, u2;
                draw_u2(key, kStreamDrawGroup, 0u, u1, u2);
                zq = draw_normal(u1, u2);
            }
            return tauq * zq;
        });
}

// ---- ordinal ---------------------------------------------------------------------------------------------------------
// y = #{k : c_k < eta + logit(u)}: the logistic latent variable against the cutpoints the walk keeps in LDS
template <int DPMAX>
__global__ void __launch_bounds__(64) draws_ord_kernel(PrArgs a, int64_t tiles, DrawArgs d, double* __restrict__ out) {
    const int64_t tile = blockIdx.x % tiles, slice = blockIdx.x / tiles;
    const int64_t i = tile * 64 + (threadIdx.x & 63u);
    const int Km1 = a.K - 1;
    const double* const cut = pr_area();
    pr_walk_ord<DPMAX, false, false>(
        a, tile, slice, [](int64_t, bool) { return 0.0; },
        [&](int64_t t, double, double, double, double, const double (&)[1], bool, double eta) {
            if (i >= a.m) return;
            const int q = (int)(t & 63);
            double y = draw_nan();
            if (finite_d(eta) && finite_d(cut[pr_slot(Km1 - 1, q)])) {   // (the running sum: the last one carries any non-finite cutpoint)
                const DrawKey key{d.seed, (uint32_t)(d.s_first + t), (uint32_t)i};
                const double u = draw_u(key, kStreamDrawOut, 0u);
                const double lat = eta + (log(u) - log1p(-u));
                int cnt = 0;
#pragma unroll 1
                for (int k = 0; k < Km1; ++k) cnt += cut[pr_slot(k, q)] < lat ? 1 : 0;
                y = (double)cnt;
            }
            out[t * a.m + i] = y;
        });
}

// ---- categorical -----------------------------------------------------------------------------------------------------
// y = min{k : P_0 + .. + P_k > u}, summed in class order, else K - 1
template <int DCMAX, int KM>
__global__ void __launch_bounds__(64) draws_cat_kernel(PrArgs a, int64_t tiles, DrawArgs d, double* __restrict__ out) {
    const int64_t tile = blockIdx.x % tiles, slice = blockIdx.x / tiles;
    const int64_t i = tile * 64 + (threadIdx.x & 63u);
    const int Km1 = a.K - 1;
    pr_walk_cat<DCMAX, KM, true>(
        a, tile, slice, [](int64_t, bool) { return 0.0; },
        [&](int64_t t, double, double, double, double pz, const double (&P)[KM], bool ok, bool lfin) {
            if (i >= a.m) return;
            double y = draw_nan();
            if (ok && lfin) {                              // (a non-finite logit, -inf included: no draw)
                const DrawKey key{d.seed, (uint32_t)(d.s_first + t), (uint32_t)i};
                const double u = draw_u(key, kStreamDrawOut, 0u);
                double F = pz;
                bool found = F > u;
                int cls = found ? 0 : Km1;
#pragma unroll
                for (int k = 0; k < KM; ++k) {
                    if (k < Km1) {
                        F += P[k];
                        const bool hit = !found && F > u;
                        cls = hit ? k + 1 : cls;
                        found = found || hit;
                    }
                }
                y = (double)cls;
            }
            out[t * a.m + i] = y;
        });
}

}  // namespace smcn
