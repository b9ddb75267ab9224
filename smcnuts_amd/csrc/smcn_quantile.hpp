// Posterior summaries: weighted quantiles (inverse of the weighted empirical CDF, NumPy's "inverted_cdf") and tail masses
// of every constrained coordinate of a population, without a sort.
//
// Staging: the constrained values coordinate-major, vals[c * M + t], and one fixed-point weight per particle,
// fw[t] = max(rint(w_t / W * 2^52), 1) for w_t > 0 and 0 otherwise (sm_fixed_kernel).  Every mass below is a sum of these
// unsigned 64-bit integers: exact in any order, so LDS and global INTEGER atomics are used freely and a result depends
// on the multiset of (value, weight) pairs alone -- not on the order of the particles or the launch geometry (the
// total W is an integer sum too: sm_total_kernel; over shards it is the rank-order sum of the shards' totals).  The unit is 2^-52 of the total mass: a population of N particles sums to 2^52 +- N, below 2^53, so every
// histogram bin and every total is also an exact double (what the shard exchange moves).
//
// Selection: MSB-first radix select on the order-preserving key of a double (sm_key), 8 passes of 8 bits.  Pass k builds,
// per (coordinate, probability), the weighted 256-bin histogram of digit k over the elements whose k higher digits equal
// that probability's prefix (sm_hist_kernel); sm_pick_kernel scans it, takes the first digit whose cumulative mass reaches
// the probability's remaining threshold, appends it to the prefix and subtracts the mass below it.  After 8 passes the
// prefix IS the key of the selected value.  Probabilities arrive sorted, so equal prefixes are neighbours: only the first
// of a run (its "leader") is counted, the others read the leader's histogram -- pass 0 (no prefix) counts once per
// coordinate.
//
// Contention: the top digit of a double is its sign and 7 exponent bits, and for a concentrated posterior the next one
// (4 exponent bits, 4 mantissa bits) is no better: a whole column lands in one or two bins.  Each thread therefore keeps
// two (bin, mass) slots in registers over its 8 elements and adds a mass to LDS only when a third bin turns up; the two
// slots are then flushed wave-wide: lanes holding the same bin sum their masses across the wavefront and ONE lane adds
// (sm_wave_add).  A block then adds its non-empty bins to the global histogram.
#pragma once
#include "smcn_pw_walk.hpp"   // (pw_exp_neg)

namespace smcn {

constexpr int kSmMaxQ = 16;            // probabilities / thresholds per call
constexpr int kSmBlock = 256;
constexpr int kSmElems = 8;            // elements per thread of the counting kernels
constexpr double kSmUnit = 4503599627370496.0;   // 2^52 units of fixed-point mass make the whole

// (u64 and the order-preserving key sm_key / sm_unkey: smcn_device.hpp, PSIS selects on the same key)

__device__ __forceinline__ u64 sm_wave_sum(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the resident population of a coordinate-wise model through constrain_coord: [D][N] -> [D][N]
__global__ void sm_stage_kernel(const double* __restrict__ x, double* __restrict__ out, int64_t N, int D, int model_id) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= N * D) return;
    out[t] = constrain_coord(model_id, (int)(t / N), D, x[t]);
}

// fixed-point weights of log-weights lw against the (global) maximum gmax and total gsum = sum exp(lw - gmax); their local
// total is added to *tot
__global__ void __launch_bounds__(kSmBlock) sm_fixed_kernel(const double* __restrict__ lw, int64_t M, double gmax,
                                                            double gsum, u64* __restrict__ fw, u64* __restrict__ tot) {
    __shared__ u64 sh[kSmBlock / 64];
    const int64_t t = (int64_t)blockIdx.x * kSmBlock + threadIdx.x;
    u64 f = 0;
    if (t < M) {
        const double v = lw[t];
        const double w = finite_d(v) ? pw_exp_neg(v - gmax) : 0.0;
        if (w > 0.0) {
            const double q = rint(w / gsum * kSmUnit);
            f = q >= 1.0 ? (u64)q : 1ull;
        }
        fw[t] = f;
    }
    f = sm_wave_sum(f);
    if ((threadIdx.x & 63u) == 0) sh[threadIdx.x >> 6] = f;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 s = 0;
        for (int i = 0; i < kSmBlock / 64; ++i) s += sh[i];
        if (s) atomicAdd(tot, s);
    }
}

// The total sum exp(lw - max) of a shard, independent of the order of the particles: each weight w in [0, 1] is split as
// w 2^32 = hi + lo 2^-40 (hi its integer part, lo the rest rounded to 40 bits) and both parts are summed as integers;
// sm_total_final_kernel puts (HI + LO 2^-40) 2^-32 in the header's sum.  (The header kernel's own sum is a float sum in
// thread order: its last bits move with the order of the particles, and with them every fixed-point weight.)
__global__ void __launch_bounds__(kSmBlock) sm_total_kernel(const double* __restrict__ lw, int64_t M,
                                                            const double* __restrict__ head, u64* __restrict__ tot) {
    __shared__ u64 sh[2 * (kSmBlock / 64)];
    const int64_t t = (int64_t)blockIdx.x * kSmBlock + threadIdx.x;
    const double gmax = head[0];
    u64 hi = 0, lo = 0;
    if (t < M) {
        const double v = lw[t];
        const double w = finite_d(v) ? pw_exp_neg(v - gmax) : 0.0;
        const double a = w * 4294967296.0, fl = floor(a);
        hi = (u64)fl;
        lo = (u64)rint((a - fl) * 1099511627776.0);
    }
    hi = sm_wave_sum(hi);
    lo = sm_wave_sum(lo);
    if ((threadIdx.x & 63u) == 0) {
        sh[threadIdx.x >> 6] = hi;
        sh[kSmBlock / 64 + (threadIdx.x >> 6)] = lo;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 a = 0, b = 0;
        for (int i = 0; i < kSmBlock / 64; ++i) {
            a += sh[i];
            b += sh[kSmBlock / 64 + i];
        }
        if (a) atomicAdd(&tot[0], a);
        if (b) atomicAdd(&tot[1], b);
    }
}
__global__ void sm_total_final_kernel(const u64* __restrict__ tot, double* __restrict__ head) {
    if (threadIdx.x == 0 && blockIdx.x == 0 && head[3] > 0.0)
        head[1] = ((double)tot[0] + (double)tot[1] * (1.0 / 1099511627776.0)) * (1.0 / 4294967296.0);
}

// Adds mass f to bins[d] for every lane with f != 0; lanes that hold the same bin are summed across the wavefront first
// and one of them adds.  Called by all lanes of a wavefront together.  After four distinct bins the remaining lanes add
// for themselves (a wavefront that spreads over many bins does not contend).
__device__ __forceinline__ void sm_wave_add(u64* bins, int d, u64 f) {
    const int lane = (int)(threadIdx.x & 63u);
    bool todo = f != 0;
#pragma unroll 1
    for (int it = 0; it < 4; ++it) {
        const u64 pending = __ballot(todo);
        if (!pending) return;
        const int lead = __ffsll((long long)pending) - 1;
        const int d0 = __shfl(d, lead, 64);
        const bool mine = todo && d == d0;
        const u64 s = sm_wave_sum(mine ? f : 0ull);
        if (lane == lead) atomicAdd(&bins[d0], s);
        todo = todo && !mine;
    }
    if (todo) atomicAdd(&bins[d], f);
}

// One histogram pass (see the head of the file).  Grid (chunks of kSmBlock * kSmElems particles, coordinates); dynamic
// LDS: nq * 256 bins.  prefix[c * nq + q]: the `pass` digits chosen so far (unused in pass 0).  hist[(c * nq + q) * 256 + d]
// is added to for the leaders q only; *nanflag[c] is set when a particle of positive weight holds a NaN.
__global__ void __launch_bounds__(kSmBlock) sm_hist_kernel(const double* __restrict__ vals, int64_t M,
                                                           const u64* __restrict__ fw, const u64* __restrict__ prefix,
                                                           int nq, int pass, u64* __restrict__ hist,
                                                           int* __restrict__ nanflag) {
    extern __shared__ u64 sm_bins[];
    __shared__ u64 lp[kSmMaxQ];
    __shared__ int lq[kSmMaxQ];
    __shared__ int nlead;
    const int c = blockIdx.y, tid = threadIdx.x;
    if (tid == 0) {
        int n = 0;
        if (pass == 0) {
            lp[0] = 0;
            lq[0] = 0;
            n = 1;
        } else {
            for (int q = 0; q < nq; ++q) {
                const u64 p = prefix[c * nq + q];
                if (q == 0 || p != lp[n - 1]) {
                    lp[n] = p;
                    lq[n] = q;
                    ++n;
                }
            }
        }
        nlead = n;
    }
    for (int i = tid; i < nq * 256; i += kSmBlock) sm_bins[i] = 0;
    __syncthreads();
    const int nl = nlead;
    const int dshift = 56 - 8 * pass;
    const double* const col = vals + (int64_t)c * M;
    const int64_t base = (int64_t)blockIdx.x * (kSmBlock * kSmElems);
    int da = -1, db = -1;
    u64 fa = 0, fb = 0;
    bool nan = false;
#pragma unroll
    for (int e = 0; e < kSmElems; ++e) {
        const int64_t t = base + e * kSmBlock + tid;
        if (t >= M) continue;
        const u64 f = fw[t];
        if (!f) continue;
        const double v = col[t];
        nan = nan || v != v;
        const u64 key = sm_key(v);
        int bin = -1;
        if (pass == 0) {
            bin = (int)(key >> 56);
        } else {
            const u64 hi = key >> (dshift + 8);
            for (int l = 0; l < nl; ++l)
                if (hi == lp[l]) bin = l * 256 + (int)((key >> dshift) & 255u);
        }
        if (bin < 0) continue;
        if (bin == da) {
            fa += f;
        } else if (bin == db) {
            fb += f;
        } else if (da < 0) {
            da = bin;
            fa = f;
        } else if (db < 0) {
            db = bin;
            fb = f;
        } else {
            atomicAdd(&sm_bins[bin], f);
        }
    }
    sm_wave_add(sm_bins, da, fa);
    sm_wave_add(sm_bins, db, fb);
    if (nan) nanflag[c] = 1;
    __syncthreads();
    for (int i = tid; i < nl * 256; i += kSmBlock) {
        const u64 s = sm_bins[i];
        if (s) atomicAdd(&hist[((int64_t)c * nq + lq[i >> 8]) * 256 + (i & 255)], s);
    }
}

// the probability's leader: the first q of the run of equal prefixes (pass 0: q = 0)
__device__ __forceinline__ int sm_leader(const u64* prefix, int c, int nq, int q, int pass) {
    if (pass == 0) return 0;
    const u64 p = prefix[c * nq + q];
    while (q > 0 && prefix[c * nq + q - 1] == p) --q;
    return q;
}

// One block per (coordinate, probability): the first digit whose cumulative mass reaches the remaining threshold.
// pass 0 reads the thresholds thr0[q] (the same for every coordinate).  State in -> state out (two sets: other blocks
// still read the prefixes of this pass).
__global__ void __launch_bounds__(256) sm_pick_kernel(const u64* __restrict__ hist, const u64* __restrict__ pin,
                                                      const u64* __restrict__ tin, const u64* __restrict__ thr0,
                                                      u64* __restrict__ pout, u64* __restrict__ tout, int nq, int pass) {
    __shared__ u64 cum[256];
    const int c = blockIdx.x / nq, q = blockIdx.x % nq, tid = threadIdx.x;
    const int ql = sm_leader(pin, c, nq, q, pass);
    const u64 h = hist[((int64_t)c * nq + ql) * 256 + tid];
    const u64 thr = pass == 0 ? thr0[q] : tin[c * nq + q];
    const u64 pfx = pass == 0 ? 0ull : pin[c * nq + q];
    cum[tid] = h;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const u64 a = tid >= o ? cum[tid - o] : 0ull;
        __syncthreads();
        cum[tid] += a;
        __syncthreads();
    }
    const u64 incl = cum[tid], excl = incl - h;
    const bool hit = excl < thr && incl >= thr;
    // (a threshold above the total mass cannot come from a probability in (0, 1]; the last digit then, so that the state
    //  is always written)
    const bool over = tid == 255 && incl < thr;
    if (hit || over) {
        pout[c * nq + q] = (pfx << 8) | (u64)tid;
        tout[c * nq + q] = hit ? thr - excl : 1ull;
    }
}

// selected values from the final prefixes
__global__ void sm_values_kernel(const u64* __restrict__ prefix, int n, double* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = sm_unkey(prefix[i]);
}

// histograms as doubles for the host, [Dc][nl][256] with nl = 1 in pass 0 and nq after (followers read their leader's
// bins), then the Dc NaN flags
__global__ void sm_export_kernel(const u64* __restrict__ hist, const u64* __restrict__ prefix,
                                 const int* __restrict__ nanflag, int Dc, int nq, int pass, double* __restrict__ out) {
    const int nl = pass == 0 ? 1 : nq;
    const int64_t n = (int64_t)Dc * nl * 256, i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const int d = (int)(i & 255), q = (int)((i >> 8) % nl), c = (int)((i >> 8) / nl);
        const int ql = sm_leader(prefix, c, nq, q, pass);
        out[i] = (double)hist[((int64_t)c * nq + ql) * 256 + d];
    } else if (i < n + Dc) {
        out[i] = (double)nanflag[i - n];
    }
}

// Tail masses: cnt[c * T + j] += sum of fw over the particles with vals[c][t] <= at[c * T + j].  Grid as sm_hist_kernel's.
__global__ void __launch_bounds__(kSmBlock) sm_cdf_kernel(const double* __restrict__ vals, int64_t M,
                                                          const u64* __restrict__ fw, const double* __restrict__ at,
                                                          int T, u64* __restrict__ cnt, int* __restrict__ nanflag) {
    __shared__ u64 part[kSmMaxQ];
    const int c = blockIdx.y, tid = threadIdx.x;
    if (tid < kSmMaxQ) part[tid] = 0;
    __syncthreads();
    double thr[kSmMaxQ];
    u64 acc[kSmMaxQ];
#pragma unroll
    for (int j = 0; j < kSmMaxQ; ++j) {
        thr[j] = j < T ? at[c * T + j] : -kInf;
        acc[j] = 0;
    }
    const double* const col = vals + (int64_t)c * M;
    const int64_t base = (int64_t)blockIdx.x * (kSmBlock * kSmElems);
    bool nan = false;
#pragma unroll 1
    for (int e = 0; e < kSmElems; ++e) {
        const int64_t t = base + e * kSmBlock + tid;
        if (t >= M) continue;
        const u64 f = fw[t];
        if (!f) continue;
        const double v = col[t];
        nan = nan || v != v;
#pragma unroll
        for (int j = 0; j < kSmMaxQ; ++j) acc[j] += (j < T && v <= thr[j]) ? f : 0ull;
    }
    if (nan) nanflag[c] = 1;
#pragma unroll
    for (int j = 0; j < kSmMaxQ; ++j) {
        if (j < T) {                                   // (block-uniform)
            const u64 s = sm_wave_sum(acc[j]);
            if ((tid & 63) == 0 && s) atomicAdd(&part[j], s);
        }
    }
    __syncthreads();
    if (tid < T && part[tid]) atomicAdd(&cnt[c * T + tid], part[tid]);
}

// counts as doubles, then the Dc NaN flags
__global__ void sm_counts_kernel(const u64* __restrict__ cnt, const int* __restrict__ nanflag, int n, int Dc,
                                 double* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (double)cnt[i];
    else if (i < n + Dc) out[i] = (double)nanflag[i - n];
}

}  // namespace smcn
