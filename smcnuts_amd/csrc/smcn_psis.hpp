// Pareto-smoothed importance-sampling LOO of the SMCN_MODEL_GLM families (definition: DESIGN.md 4.4, "Pareto-smoothed
// LOO"; column layouts: include/smcnuts_hip.h, smcn_psis_*).  Per observation i and contributing particle p (finite
// log-weight): lw' = lw - mw, ll = log p(y_i | x_p), lr = lw' - ll -- the term the stats kernel of smcn_pointwise.hpp
// forms.  S contributing particles over all shards give M = min(S / 5, ceil(3 sqrt S)) tail candidates.
//
// Three stages, each a function of (mw, S) and its inputs alone, so that shards can run them with the global mw and S:
//   candidates  the rank's T_cap = M + 1 largest lr with their ll per observation, descending, ties by particle index,
//               padded with -inf.  psis_stage_kernel walks a slab of observation tiles with pw_walk (the terms have the
//               bits of pointwise_loglik_kernel) and writes ll as [observation][particle]; psis_select_kernel, one block
//               per observation, radix-selects the T_cap-th largest lr by COUNT on the sm_key map (8 passes of 8 bits, a
//               256-bin LDS histogram; a thread adds a run of equal digits once, because a concentrated column lands in
//               one bin), compacts the entries above it and the lowest-indexed ties at it into LDS in particle order (a
//               ballot scan: no atomics), and sorts them there (bitonic, on (key, particle index): a total order, so the
//               result depends on the values alone).
//   body        the max-shifted sums (mb, Sb, Sb2) of lr and sum e^{lw'} over the particles with lr <= cutoff_i: a second
//               pw_walk with the stats kernel's update, slices merged in slice order (groups of kPwGroup, then the groups)
//               as pointwise_combine_kernel does.  The body is summed as a body, never as total minus tail.
//   fit         one block per observation on its candidates alone: cutoff, tail, Zhang-Stephens fit, smoothing, finish.
// The cutoff on the lr scale is the largest candidate whose z = lr - mx does not exceed c (z of the T_cap-th largest):
// "z > c" is then the same set as "lr > cutoff" even where the subtraction of mx rounds two lr onto one z.
#pragma once
#include "smcn_pointwise.hpp"

namespace smcn {

constexpr int kPsBlock = 256;
constexpr int kPsMaxCap = 4096;       // candidates per observation the selection sorts in LDS (T_cap = M + 1)
constexpr int kPsMaxTail = 4096;      // tail entries the fit sorts in LDS (M: the fit takes T_cap <= 4097)
constexpr int kPsBodyCols = 4;        // mb, Sb, Sb2, Sw
constexpr int kPsOutCols = 6;         // pareto_k, elpd_psis, psis_ess, tail_len, cutoff, sigma
constexpr int kPsMaxGrid = 96;        // 30 + floor(sqrt(4096)) = 94 grid points of the fit
enum : int { PS_MB = 0, PS_SB, PS_SB2, PS_SW };

// M = min(floor(S / 5), ceil(3 sqrt(S))), the ceiling in integers (ceil(sqrt(9 S)))
__host__ __device__ inline int64_t psis_tail_len(int64_t S) {
    if (S < 1) return 0;
    int64_t r = (int64_t)sqrt((double)(9 * S));
    while (r * r < 9 * S) ++r;
    while (r > 0 && (r - 1) * (r - 1) >= 9 * S) --r;
    const int64_t a = S / 5;
    return a < r ? a : r;
}

// T_cap = M + 1 of the call's header (head[3] = S), at most `cap`
__device__ __forceinline__ int psis_cap(const double* head, int cap) {
    const int64_t t = psis_tail_len((int64_t)head[3]) + 1;
    return t < cap ? (int)t : cap;
}

// ll of a slab of `slab_tiles` observation tiles from tile0 on: stage[(local observation) * Mpad + particle].  Particles
// with a non-finite log-weight are passed over (their slots are never read).
template <int DPMAX, bool DISP, bool OW = false>
__global__ void __launch_bounds__(64) psis_stage_kernel(PwArgs a, int64_t tile0, int64_t slab_tiles,
                                                        const double* __restrict__ lw,
                                                        const double* __restrict__ head, int64_t Mpad,
                                                        double* __restrict__ stage) {
    const int64_t lt = blockIdx.x % slab_tiles, slice = blockIdx.x / slab_tiles;
    const double mw = head[0];
    double* const row = stage + (lt * 64 + (int64_t)(threadIdx.x & 63u)) * Mpad;
    pw_walk<DPMAX, DISP, OW>(
        a, tile0 + lt, slice, [&](int64_t t, bool have) { return have ? lw[t] - mw : -kInf; },
        [&](int64_t t, double, double, double term, double) { row[t] = term; });
}

// descending bitonic sort of P (a power of two) entries on (key, then ascending index); all threads of the block
__device__ __forceinline__ void psis_sort_desc(u64* skey, unsigned* sidx, unsigned P) {
    for (unsigned k = 2; k <= P; k <<= 1) {
        for (unsigned j = k >> 1; j > 0; j >>= 1) {
            for (unsigned i = threadIdx.x; i < P; i += kPsBlock) {
                const unsigned l = i ^ j;
                if (l > i) {
                    const u64 ka = skey[i], kb = skey[l];
                    const unsigned ia = sidx[i], ib = sidx[l];
                    const bool a_first = ka > kb || (ka == kb && ia < ib);
                    const bool b_first = kb > ka || (ka == kb && ib < ia);
                    if ((i & k) == 0 ? b_first : a_first) {
                        skey[i] = kb;
                        skey[l] = ka;
                        sidx[i] = ib;
                        sidx[l] = ia;
                    }
                }
            }
            __syncthreads();
        }
    }
}

// ballot scan of a flag over the block in thread order: the thread's offset among the flagged, and their number
__device__ __forceinline__ unsigned psis_scan(bool flag, unsigned* wcnt /*4*/, unsigned* total) {
    const int lane = (int)(threadIdx.x & 63u), w = (int)(threadIdx.x >> 6);
    const u64 b = __ballot(flag);
    __syncthreads();
    if (lane == 0) wcnt[w] = (unsigned)__popcll(b);
    __syncthreads();
    unsigned off = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < kPsBlock / 64; ++k) {
        off += k < w ? wcnt[k] : 0u;
        tot += wcnt[k];
    }
    *total = tot;
    return off + (unsigned)__popcll(b & ((1ull << lane) - 1ull));
}

// The K = min(T_cap, M) largest lr of observation obs0 + blockIdx.x among the rank's M particles (non-contributing ones
// count as -inf, below every contributing one) -> cand_lr / cand_ll [n][Tcap], and the rank's own cutoff (NaN when the
// rank holds fewer than Tcap particles: the merged candidates of all ranks decide then).
__global__ void __launch_bounds__(kPsBlock) psis_select_kernel(const double* __restrict__ stage, int64_t Mpad,
                                                               const double* __restrict__ lw,
                                                               const double* __restrict__ head, int64_t M, int64_t obs0,
                                                               int64_t n, int stride, double* __restrict__ cand_lr,
                                                               double* __restrict__ cand_ll, double* __restrict__ cutoff) {
    __shared__ u64 skey[kPsMaxCap];
    __shared__ unsigned sidx[kPsMaxCap];
    __shared__ unsigned bins[256];
    __shared__ unsigned wcnt[kPsBlock / 64];
    __shared__ u64 s_prefix;
    __shared__ unsigned s_need;
    const int64_t i = obs0 + blockIdx.x;
    if (i >= n) return;
    const int tid = (int)threadIdx.x;
    const double mw = head[0];
    const int Tcap = psis_cap(head, stride < kPsMaxCap ? stride : kPsMaxCap);
    const int K = (int64_t)Tcap < M ? Tcap : (int)M;
    const double* const row = stage + (int64_t)blockIdx.x * Mpad;
    auto key_of = [&](int64_t t) {
        const double l = lw[t] - mw;
        return sm_key(finite_d(l) ? l - row[t] : -kInf);
    };
    u64 prefix = 0;
    unsigned need = (unsigned)K;
    for (int pass = 0; pass < 8; ++pass) {
        bins[tid] = 0;
        __syncthreads();
        const int dshift = 56 - 8 * pass;
        int cb = 0;
        unsigned cc = 0;
        for (int64_t t = tid; t < M; t += kPsBlock) {
            const u64 key = key_of(t);
            if (pass == 0 || (key >> (dshift + 8)) == prefix) {
                const int b = (int)((key >> dshift) & 255u);
                if (b == cb) {
                    ++cc;
                } else {
                    if (cc) atomicAdd(&bins[cb], cc);
                    cb = b;
                    cc = 1;
                }
            }
        }
        if (cc) atomicAdd(&bins[cb], cc);
        __syncthreads();
        if (tid == 0) {       // from the top digit down: the digit that holds the need-th largest
            unsigned cum = 0;
            int d = 255;
            for (; d > 0; --d) {
                const unsigned h = bins[d];
                if (cum + h >= need) break;
                cum += h;
            }
            s_prefix = (prefix << 8) | (u64)d;
            s_need = need - cum;
        }
        __syncthreads();
        prefix = s_prefix;
        need = s_need;
    }
    // prefix is the key of the K-th largest; `need` of its copies belong to the K, G = K - need keys lie above it
    const u64 ckey = prefix;
    const unsigned G = (unsigned)K - need;
    unsigned baseG = 0, baseE = 0;
    for (int64_t t0 = 0; t0 < M; t0 += kPsBlock) {
        const int64_t t = t0 + tid;
        const u64 key = t < M ? key_of(t) : 0ull;
        const bool g = t < M && key > ckey, e = t < M && key == ckey;
        unsigned tg, te;
        const unsigned pg = baseG + psis_scan(g, wcnt, &tg);
        const unsigned pe = baseE + psis_scan(e, wcnt, &te);
        if (g && pg < G) {
            skey[pg] = key;
            sidx[pg] = (unsigned)t;
        }
        if (e && pe < need) {
            skey[G + pe] = key;
            sidx[G + pe] = (unsigned)t;
        }
        baseG += tg;
        baseE += te;
    }
    unsigned P = 1;
    while (P < (unsigned)K) P <<= 1;
    for (unsigned d = (unsigned)K + tid; d < P; d += kPsBlock) {
        skey[d] = 0ull;
        sidx[d] = 0xffffffffu;
    }
    __syncthreads();
    psis_sort_desc(skey, sidx, P);
    for (int d = tid; d < stride; d += kPsBlock) {
        double vr = -kInf, vl = -kInf;
        if (d < K) {
            vr = sm_unkey(skey[d]);
            vl = vr > -kInf ? row[sidx[d]] : -kInf;
        }
        cand_lr[i * stride + d] = vr;
        cand_ll[i * stride + d] = vl;
    }
    if (tid == 0) {
        double cut = __builtin_nan("");
        if (K == Tcap) {
            const double mx = sm_unkey(skey[0]);
            if (!(mx < kInf)) {
                cut = mx;                            // (some term is -inf: everything is body; or a NaN)
            } else {
                const double c = sm_unkey(skey[K - 1]) - mx;
                int d = K - 1;
                while (d > 0 && sm_unkey(skey[d - 1]) - mx <= c) --d;
                cut = sm_unkey(skey[d]);
            }
        }
        cutoff[i] = cut;
    }
}

// the slices' body partials of a tile: part[(slice * kPsBodyCols + col) * npad + i]
template <int DPMAX, bool DISP, bool OW = false>
__global__ void __launch_bounds__(64) psis_body_kernel(PwArgs a, int64_t tiles, const double* __restrict__ lw,
                                                       const double* __restrict__ head,
                                                       const double* __restrict__ cutoff, double* __restrict__ part) {
    const int64_t tile = blockIdx.x % tiles, slice = blockIdx.x / tiles;
    const double mw = head[0];
    const int64_t i = tile * 64 + (threadIdx.x & 63u), npad = tiles * 64;
    const double cut = i < a.n ? cutoff[i] : -kInf;
    double mb = -kInf, Sb = 0.0, Sb2 = 0.0, Sw = 0.0;
    pw_walk<DPMAX, DISP, OW>(
        a, tile, slice, [&](int64_t t, bool have) { return have ? lw[t] - mw : -kInf; },
        [&](int64_t, double lwq, double wq, double term, double) {
            const bool fin = term > -kInf;
            const double v = lwq - (fin ? term : 0.0);
            const bool in = fin && v <= cut;
            const double d = v - mb, e = pw_exp_neg(d), e2 = e * e;
            const bool up = d > 0.0;
            const double Sn = up ? fma(Sb, e, 1.0) : Sb + e, Qn = up ? fma(Sb2, e2, 1.0) : Sb2 + e2;
            Sb = in ? Sn : Sb;
            Sb2 = in ? Qn : Sb2;
            mb = (in && up) ? v : mb;
            Sw += in ? wq : 0.0;
        });
    if (i < a.n) {
        double* const o = part + slice * kPsBodyCols * npad + i;
        o[PS_MB * npad] = mb;
        o[PS_SB * npad] = Sb;
        o[PS_SB2 * npad] = Sb2;
        o[PS_SW * npad] = Sw;
    }
}

// pointwise_combine_kernel for the body partials: stage 1 merges the slices of group blockIdx.y in slice order into the
// slices' layout, stage 2 (FINAL) the groups into out[i * kPsBodyCols + col]
template <bool FINAL>
__global__ void psis_body_combine_kernel(const double* __restrict__ part, int64_t slices, int64_t n, int64_t npad,
                                         double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t s0 = FINAL ? 0 : (int64_t)blockIdx.y * kPwGroup;
    const int64_t s1 = FINAL ? slices : (s0 + kPwGroup < slices ? s0 + kPwGroup : slices);
    double mb = -kInf, Sb = 0.0, Sb2 = 0.0, Sw = 0.0;
    for (int64_t s = s0; s < s1; ++s) {
        const double* const o = part + s * kPsBodyCols * npad + i;
        const double m2 = o[PS_MB * npad], s2 = o[PS_SB * npad], q2 = o[PS_SB2 * npad];
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
        Sw += o[PS_SW * npad];
    }
    double* const r = FINAL ? out + i * kPsBodyCols : out + (int64_t)blockIdx.y * kPsBodyCols * npad + i;
    const int64_t st = FINAL ? 1 : npad;
    r[PS_MB * st] = mb;
    r[PS_SB * st] = Sb;
    r[PS_SB2 * st] = Sb2;
    r[PS_SW * st] = Sw;
}

// One block per observation: its Tcap candidates (any order; stage 1 and the host merge deliver them descending) and body
// partials -> out[i][kPsOutCols].  Everything in fp64 with the device library's exp / log / log1p / expm1.
__global__ void __launch_bounds__(kPsBlock) psis_fit_kernel(const double* __restrict__ cand_lr,
                                                            const double* __restrict__ cand_ll,
                                                            const double* __restrict__ body,
                                                            const double* __restrict__ head, int stride,
                                                            double* __restrict__ out) {
    __shared__ u64 skey[kPsMaxTail];          // keys of the tail, then x_j, then the smoothed z~_j
    __shared__ unsigned sidx[kPsMaxTail];
    __shared__ double sh[4];
    __shared__ unsigned wcnt[kPsBlock / 64];
    __shared__ double gb[kPsMaxGrid], gk[kPsMaxGrid], gL[kPsMaxGrid], gw[kPsMaxGrid];
    __shared__ double s_b;
    const int64_t i = blockIdx.x;
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int Tcap = psis_cap(head, stride < kPsMaxTail + 1 ? stride : kPsMaxTail + 1);
    const double* const lr = cand_lr + (int64_t)i * stride;
    const double* const ll = cand_ll + (int64_t)i * stride;
    double* const o = out + i * kPsOutCols;
    const double nan = __builtin_nan("");
    double* const sx = (double*)skey;

    double m = -kInf, mn = kInf;
    bool anynan = false;
    for (int d = tid; d < Tcap; d += kPsBlock) {
        const double v = lr[d];
        anynan = anynan || v != v;
        m = fmax(m, v);
        mn = fmin(mn, v);
    }
    const double mx = block_max(m, sh);
    const double cmin = -block_max(-mn, sh);
    const bool bad = block_max(anynan ? 1.0 : 0.0, sh) != 0.0;
    if (bad || mx == -kInf) {      // a NaN term, or no contributing particle
        if (tid < kPsOutCols) o[tid] = nan;
        return;
    }
    if (!(mx < kInf)) {       // rule 1: a contributing particle with ll = -inf
        if (tid == 0) {
            o[0] = kInf;
            o[1] = -kInf;
            o[2] = 0.0;
            o[3] = 0.0;
            o[4] = kInf;
            o[5] = nan;
        }
        return;
    }
    const double c = cmin - mx;
    double cem = -kInf;
    for (int d = tid; d < Tcap; d += kPsBlock) {
        const double v = lr[d];
        cem = (v - mx <= c) ? fmax(cem, v) : cem;
    }
    const double cut = block_max(cem, sh);

    // the tail, z > c, in candidate order, then sorted descending
    unsigned T = 0;
    for (int d0 = 0; d0 < Tcap; d0 += kPsBlock) {
        const int d = d0 + tid;
        const bool g = d < Tcap && (lr[d] - mx > c);
        unsigned tg;
        const unsigned pos = T + psis_scan(g, wcnt, &tg);
        if (g && pos < (unsigned)kPsMaxTail) {
            skey[pos] = sm_key(lr[d]);
            sidx[pos] = (unsigned)d;
        }
        T += tg;
    }
    T = T < (unsigned)kPsMaxTail ? T : (unsigned)kPsMaxTail;      // (T <= Tcap - 1 <= kPsMaxTail: the host checks Tcap)
    unsigned P = 1;
    while (P < T) P <<= 1;
    for (unsigned d = T + tid; d < P; d += kPsBlock) {
        skey[d] = 0ull;
        sidx[d] = 0xffffffffu;
    }
    __syncthreads();
    if (T > 1) psis_sort_desc(skey, sidx, P);

    // descending position d holds ascending rank j = T - d (1-based)
    const double Td = (double)T;
    double kk = kInf, sigma = nan;
    if (T >= 5) {
        const double ec = exp(c);
        for (unsigned d = tid; d < T; d += kPsBlock) {
            const double z = sm_unkey(skey[d]) - mx;
            sx[d] = ec * expm1(z - c);
        }
        __syncthreads();
        const int mg = 30 + (int)floor(sqrt(Td));
        const unsigned q = (unsigned)floor(Td / 4.0 + 0.5);
        const double xq = sx[T - q], xT = sx[0];
        for (int l = wv; l < mg; l += kPsBlock / 64) {
            const double bl = (1.0 - sqrt((double)mg / ((double)(l + 1) - 0.5))) / (3.0 * xq) + 1.0 / xT;
            double s = 0.0;
            for (unsigned d = lane; d < T; d += 64) s += log1p(-bl * sx[d]);
            s = wave_sum(s);
            if (lane == 0) {
                const double kl = s / Td;
                gb[l] = bl;
                gk[l] = kl;
                gL[l] = Td * (log(-bl / kl) - kl - 1.0);
            }
        }
        __syncthreads();
        if (tid < mg) {
            double s = 0.0;
            const double Ll = gL[tid];
            for (int l2 = 0; l2 < mg; ++l2) s += exp(gL[l2] - Ll);
            gw[tid] = 1.0 / s;
        }
        __syncthreads();
        if (tid == 0) {
            const double thr = 10.0 * 2.220446049250313e-16;
            double sw = 0.0, b = 0.0;
            for (int l = 0; l < mg; ++l) sw += gw[l] >= thr ? gw[l] : 0.0;
            for (int l = 0; l < mg; ++l) b += gw[l] >= thr ? gb[l] * (gw[l] / sw) : 0.0;
            s_b = b;
        }
        __syncthreads();
        const double b = s_b;
        double s = 0.0;
        for (unsigned d = tid; d < T; d += kPsBlock) s += log1p(-b * sx[d]);
        const double kp = block_sum(s, sh) / Td;
        sigma = -kp / b;
        kk = (Td * kp + 5.0) / (Td + 10.0);
        __syncthreads();
        const bool smooth = finite_d(kk);
        for (unsigned d = tid; d < T; d += kPsBlock) {
            double zt;
            if (smooth) {
                const double p = ((double)(T - d) - 0.5) / Td, l1 = log1p(-p);
                const double qj = kk == 0.0 ? -sigma * l1 : sigma * expm1(-kk * l1) / kk;
                zt = fmin(log(qj + ec), 0.0);
            } else {
                zt = lr[sidx[d]] - mx;
            }
            sx[d] = zt;
        }
    } else {
        for (unsigned d = tid; d < T; d += kPsBlock) sx[d] = lr[sidx[d]] - mx;
    }
    __syncthreads();

    // finish: the tail's max-shifted sums, then merged with the body's
    double ma = -kInf, mr = -kInf;
    for (unsigned d = tid; d < T; d += kPsBlock) {
        const double r = sx[d] + mx;
        mr = fmax(mr, r);
        ma = fmax(ma, r + ll[sidx[d]]);
    }
    ma = block_max(ma, sh);
    mr = block_max(mr, sh);
    double sa = 0.0, sr = 0.0, sr2 = 0.0;
    for (unsigned d = tid; d < T; d += kPsBlock) {
        const double r = sx[d] + mx;
        const double e = exp(r - mr);
        sa += exp(r + ll[sidx[d]] - ma);
        sr += e;
        sr2 += e * e;
    }
    sa = block_sum(sa, sh);
    sr = block_sum(sr, sh);
    sr2 = block_sum(sr2, sh);
    if (tid == 0) {
        const double mb = body[i * kPsBodyCols + PS_MB], Sb = body[i * kPsBodyCols + PS_SB];
        const double Sb2 = body[i * kPsBodyCols + PS_SB2], Sw = body[i * kPsBodyCols + PS_SW];
        double lognum, mD, eb, et;
        if (T == 0) {
            lognum = log(Sw);
            mD = mb;
            eb = 1.0;
            et = 0.0;
            sr = 0.0;
            sr2 = 0.0;
        } else {
            const double mN = Sw > 0.0 ? fmax(ma, 0.0) : ma;
            lognum = mN + log((Sw > 0.0 ? Sw * exp(-mN) : 0.0) + sa * exp(ma - mN));
            mD = Sb > 0.0 ? fmax(mr, mb) : mr;
            eb = Sb > 0.0 ? exp(mb - mD) : 0.0;
            et = exp(mr - mD);
        }
        const double sum = Sb * eb + sr * et, sum2 = Sb2 * eb * eb + sr2 * et * et;
        o[0] = kk;
        o[1] = lognum - (mD + log(sum));
        o[2] = sum * sum / sum2;
        o[3] = Td;
        o[4] = cut;
        o[5] = sigma;
    }
}

}  // namespace smcn
