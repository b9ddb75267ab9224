// A fused block's device work between the NUTS launch and the host's wait, in two launches (smcn_set_block_post 1):
//
//   block_stream_kernel   nuts2_post_kernel (smcn_nuts2.hpp) + gen_partials_kernel (smcn_step.hpp) for the block's B
//                         generations in ONE pass over the lane kernel's pair-major records: unpack, re-weight, write the
//                         generations and the last transition's arrays, and form the block partials of every generation
//                         from the values in registers -- the generations are not read back;
//   block_tail_kernel     gen_reduce_blocks_kernel + store_counts_kernel + the lpB -> gathB copy + (one shard)
//                         combine_ranks_gens_kernel: one thread block per generation.
//
// Every output keeps the bits of the separate launches, which stay in the library (smcn_set_block_post 0) as the
// reference the tests compare against.  The sums keep their order: a thread block here is ONE (block, generation) cell of
// gen_partials_kernel's grid -- same particles first + k * stride per thread, accumulated in k, then the same block
// reductions.  With compact records (B > 1) a generation's log-weights are in its own records -- the lane kernel walked
// the weight chain --, so the cells are independent; only the block's last transition adds its increment, to the weight
// its predecessor's record holds (B == 1: to the weight before the block), by the expression of nuts2_post_kernel.
// The leapfrog / moved counts (integers: exact in any order) go per cell to cntpart and are summed by the tail kernel:
// no counters to clear in front of the NUTS launch, no atomics.
#pragma once
#include "smcn_nuts2.hpp"
#include "smcn_step.hpp"

namespace smcn {

// grid (nb, B), kRedBlock threads; KR >= ceil(N / (nb * kRedBlock)) particles per thread, held in registers.
// cntpart[(2 * b + q) * nb + block]: q = 0 leapfrogs, 1 moved particles of generation b in this block's cell.
template <int D, int KR>
__global__ void __launch_bounds__(kRedBlock) block_stream_kernel(
    const double* __restrict__ out, const double* __restrict__ in, const double* __restrict__ x0,
    const double* __restrict__ logw, double* __restrict__ x_new, double* __restrict__ r_new, double* __restrict__ lpri0,
    double* __restrict__ llik0, double* __restrict__ lpri1, double* __restrict__ llik1, int32_t* __restrict__ nleap,
    int32_t* __restrict__ depth, int32_t* __restrict__ ndraws, int32_t* __restrict__ flags, double* __restrict__ logw_new,
    double* __restrict__ x_next /* may be null */, double* __restrict__ logw_next /* may be null */,
    double* __restrict__ gen_x, double* __restrict__ gen_logw, int64_t N, int B, int model_id, double* __restrict__ part0,
    double* __restrict__ cntpart) {
    using d2 = double __attribute__((ext_vector_type(2)));
    // pairs per record: full output [x'(VH), r'(VH), (lpri1, llik1), (lpri0, llik0), (stats0, stats1)], compact output
    // [x'(VH), (logw_b, stats0)], input [x0(VH), r0(VH), (e0, pad)]; pair j of record t, particle p at
    // [(t * pairs + j) * N + p]
    constexpr int VP = n2_vp(D), VH = VP / 2, OP = n2_out_doubles(D) / 2, IP = n2_in_doubles(D) / 2, CP = VH + 1;
    __shared__ double sh[4 * (5 + 2 * D)];      // the widest batch of block reductions below
    __shared__ double shref[D];
    const int b = (int)blockIdx.y, nb = (int)gridDim.x, NQ = gen_block_nq(D);
    const int64_t first = (int64_t)blockIdx.x * kRedBlock + threadIdx.x, stride = (int64_t)nb * kRedBlock;
    const d2* const full = reinterpret_cast<const d2*>(out);   // the one full record per particle: the last transition's
    const d2* const comp = full + N * OP;                      // compact records of the transitions before it
    const d2* const inp = reinterpret_cast<const d2*>(in);
    const bool last = b == B - 1;
    const double cst = 0.5 * D * kLog2Pi;
    double xk[KR][VP], lwk[KR];
    bool live[KR];
    double leaps = 0.0, moved = 0.0;
    // The transitions before the last (B - 1 of the grid's B rows): ALL loads of the thread's particles first, nothing
    // between them that they could wait for -- one round trip to memory instead of one per particle.  (A slot beyond the
    // population reads particle N - 1: in bounds, not used.)
    double xp[KR][VP];                 // the samples before this transition
    d2 cur[KR][CP];
    if (!last) {
#pragma unroll
        for (int k = 0; k < KR; ++k) {
            const int64_t i = first + k * stride, ii = i < N ? i : N - 1;
            if (b == 0) {
#pragma unroll
                for (int c = 0; c < D; ++c) xp[k][c] = x0[(int64_t)c * N + ii];
            } else {
#pragma unroll
                for (int j = 0; j < VH; ++j) {
                    const d2 v = comp[((int64_t)(b - 1) * CP + j) * N + ii];
                    xp[k][2 * j] = v.x;
                    xp[k][2 * j + 1] = v.y;
                }
            }
#pragma unroll
            for (int j = 0; j < CP; ++j) cur[k][j] = comp[((int64_t)b * CP + j) * N + ii];
        }
    }
#pragma unroll
    for (int k = 0; k < KR; ++k) {
        const int64_t i = first + k * stride;
        live[k] = i < N;
        lwk[k] = -kInf;
#pragma unroll
        for (int c = 0; c < VP; ++c) xk[k][c] = 0.0;
        if (!live[k]) continue;
        bool all = true;
        unsigned long long s0;
        if (!last) {
#pragma unroll
            for (int j = 0; j < VH; ++j) {
                xk[k][2 * j] = cur[k][j].x;
                xk[k][2 * j + 1] = cur[k][j].y;
            }
            lwk[k] = cur[k][VH].x;         // the kernel already folded this transition into the weight
            s0 = (unsigned long long)__double_as_longlong(cur[k][VH].y);
#pragma unroll
            for (int c = 0; c < D; ++c) all = all && (xk[k][c] != xp[k][c]);
        } else {
            if (b == 0) {
#pragma unroll
                for (int c = 0; c < D; ++c) xp[k][c] = x0[(int64_t)c * N + i];
            } else {
#pragma unroll
                for (int j = 0; j < VH; ++j) {
                    const d2 v = comp[((int64_t)(b - 1) * CP + j) * N + i];
                    xp[k][2 * j] = v.x;
                    xp[k][2 * j + 1] = v.y;
                }
            }
            double rv[VP], r0[VP];
#pragma unroll
            for (int j = 0; j < VH; ++j) {
                const d2 v = full[(int64_t)j * N + i], w = full[(int64_t)(VH + j) * N + i];
                const d2 z = inp[((int64_t)b * IP + VH + j) * N + i];
                xk[k][2 * j] = v.x; xk[k][2 * j + 1] = v.y;
                rv[2 * j] = w.x; rv[2 * j + 1] = w.y;
                r0[2 * j] = z.x; r0[2 * j + 1] = z.y;
            }
            double k0 = 0.0, k1 = 0.0;
#pragma unroll
            for (int c = 0; c < D; ++c) {
                all = all && (xk[k][c] != xp[k][c]);
                k0 = fma(r0[c], r0[c], k0);
                k1 = fma(rv[c], rv[c], k1);
                x_new[(int64_t)c * N + i] = xk[k][c];
                r_new[(int64_t)c * N + i] = rv[c];
                if (x_next) x_next[(int64_t)c * N + i] = xk[k][c];
            }
            const d2 p1 = full[(int64_t)VP * N + i], p0 = full[(int64_t)(VP + 1) * N + i];
            const d2 st = full[(int64_t)(VP + 2) * N + i];
            const double a1 = p1.x, b1 = p1.y, a0 = p0.x, bb0 = p0.y;
            s0 = (unsigned long long)__double_as_longlong(st.x);
            const unsigned long long s1 = (unsigned long long)__double_as_longlong(st.y);
            lpri1[i] = a1; llik1[i] = b1; lpri0[i] = a0; llik0[i] = bb0;
            nleap[i] = (int32_t)(s0 & 0xffffffffu);
            depth[i] = (int32_t)(s0 >> 32);
            ndraws[i] = (int32_t)(s1 & 0xffffffffu);
            flags[i] = (int32_t)(s1 >> 32);
            const double qk = -0.5 * k0 - cst;
            const double Lk = -0.5 * k1 - cst;
            const double c1 = combine_lp(a1, b1, 1.0);
            const double c0 = combine_lp(a0, bb0, 1.0);
            double lw = b == 0 ? logw[i] : comp[((int64_t)(b - 1) * CP + VH) * N + i].x;
            lw = lw + c1 - c0 + Lk - qk;
            lwk[k] = lw;
            logw_new[i] = lw;
            if (logw_next) logw_next[i] = lw;
        }
#pragma unroll
        for (int c = 0; c < D; ++c) gen_x[((int64_t)b * D + c) * N + i] = xk[k][c];
        gen_logw[(int64_t)b * N + i] = lwk[k];
        leaps += (double)(s0 & 0xffffffffu);
        moved += all ? 1.0 : 0.0;
    }
    // ---- gen_partials_kernel's cell (blockIdx.x, generation b), from the registers ----
    double* const part = part0 + (int64_t)b * NQ * nb;
    double m = -kInf, nanflag = 0.0;
    int64_t am = -1;                    // this thread's first index of its maximum
#pragma unroll
    for (int k = 0; k < KR; ++k) {
        if (!live[k]) continue;
        const double v = lwk[k];
        if (v != v) nanflag = 1.0;
        if (v > m) { m = v; am = first + k * stride; }
    }
    const double mt = m;
    {
        double mm[2] = {m, nanflag};
        block_max_n(mm, sh);
        m = mm[0];
        nanflag = mm[1];
    }
    const double mx = nanflag != 0.0 ? __builtin_nan("") : m;
    // the block's first index of the maximum (indices < 2^53 are exact in a double); none when every weight is -inf
    const double neg_first = block_max((am >= 0 && mt == m) ? -(double)am : -kInf, sh);
    const int64_t iref = neg_first == -kInf ? -1 : (int64_t)(-neg_first);
    // the reference point is c(x) of particle iref: its owner hands the coordinates over
    if (iref >= 0 && am == iref) {
#pragma unroll
        for (int k = 0; k < KR; ++k)
            if (first + k * stride == iref) {
#pragma unroll
                for (int c = 0; c < D; ++c) shref[c] = xk[k][c];
            }
    }
    __syncthreads();
    double sc[D];
#pragma unroll
    for (int c = 0; c < D; ++c) {
        const double r = iref < 0 ? 0.0 : constrain_coord(model_id, c, D, shref[c]);
        sc[c] = finite_d(r) ? r : 0.0;
    }
    const double sft = finite_d(mx) ? mx : 0.0;
    // red: leapfrogs, moved, cnt, s1, s2, then sum e d and sum e d^2 per coordinate -- each the sum gen_partials_kernel
    // forms (k ascending in the thread, then block_sum's tree), all behind one pair of barriers
    double red[5 + 2 * D];
#pragma unroll
    for (int q = 0; q < 5 + 2 * D; ++q) red[q] = 0.0;
    red[0] = leaps;
    red[1] = moved;
#pragma unroll
    for (int k = 0; k < KR; ++k) {
        const double v = lwk[k];
        if (!(live[k] && v != -kInf)) continue;
        const double e = exp(v - sft);
        if (v == mx) red[2] += 1.0;
        else red[3] += e;
        red[4] = fma(e, e, red[4]);
#pragma unroll
        for (int c = 0; c < D; ++c) {
            const double xv = constrain_coord(model_id, c, D, xk[k][c]);
            const double d = xv - sc[c];
            red[5 + c] = fma(e, d, red[5 + c]);
            red[5 + D + c] = fma(e * d, d, red[5 + D + c]);
        }
    }
    block_sum_n(red, sh);
    if (threadIdx.x == 0) {
        cntpart[(int64_t)(2 * b) * nb + blockIdx.x] = red[0];
        cntpart[(int64_t)(2 * b + 1) * nb + blockIdx.x] = red[1];
        part[blockIdx.x] = mx;
        part[nb + blockIdx.x] = red[2];
        part[2 * nb + blockIdx.x] = red[3];
        part[3 * nb + blockIdx.x] = red[4];
#pragma unroll
        for (int c = 0; c < D; ++c) {
            part[(int64_t)(4 + c) * nb + blockIdx.x] = red[5 + c];
            part[(int64_t)(4 + D + c) * nb + blockIdx.x] = red[5 + D + c];
            part[(int64_t)(4 + 2 * D + c) * nb + blockIdx.x] = sc[c];
        }
    }
}

// One thread block per generation g of the fused block: the shard partials of generation k0 + 1 + g (lpB row g, copied
// to gathB row g when gathB is given) -- gen_reduce_blocks_kernel's sums: a thread takes the block partials b = its index
// + 256 k, ascending, then block_sum's tree; the coordinates' reductions batched --, the leapfrog / moved counts of
// transition g (history row k0 + g, and cnt), and, combine != 0 (one shard), history row k0 + 1 + g and the step
// scalars as combine_ranks_gens_kernel leaves them.  nb <= kTailPerThread * kRedBlock block partials per generation,
// read once, into registers.
constexpr int kTailPerThread = 4;
template <int DC>
__global__ void __launch_bounds__(kRedBlock) block_tail_kernel(const double* part0, int nb, const double* cntpart,
                                                               double* cnt, const double* shift, double* lpB,
                                                               double* gathB, double* hist0 /* row k0 */,
                                                               int hist_stride, int combine, double n_total,
                                                               double log_n_local, double phi, double* ss,
                                                               double* ss_scratch, int ss_stride) {
    constexpr int NQ = 4 + 2 * DC, NQB = gen_block_nq(DC), KB = kTailPerThread;
    __shared__ double sh[4 * (6 + DC)];
    const int g = (int)blockIdx.x, B = (int)gridDim.x;
    const double* const part = part0 + (int64_t)g * NQB * nb;
    double* const out = lpB + (int64_t)g * NQ;
    double pv[KB][NQB], nl = 0.0, nm = 0.0, sc[DC];
    bool has[KB];
#pragma unroll
    for (int k = 0; k < KB; ++k) {
        const int b = (int)threadIdx.x + k * kRedBlock;
        has[k] = b < nb;
#pragma unroll
        for (int q = 0; q < NQB; ++q) pv[k][q] = has[k] ? part[(int64_t)q * nb + b] : 0.0;
        if (has[k]) {       // integers: exact in any order
            nl += cntpart[(int64_t)(2 * g) * nb + b];
            nm += cntpart[(int64_t)(2 * g + 1) * nb + b];
        }
    }
#pragma unroll
    for (int c = 0; c < DC; ++c) sc[c] = shift[c];
    double M = -kInf, nanflag = 0.0;
#pragma unroll
    for (int k = 0; k < KB; ++k) {
        if (!has[k]) continue;
        const double v = pv[k][0];
        if (v != v) nanflag = 1.0;
        M = fmax(M, v);
    }
    {
        double mm[2] = {M, nanflag};
        block_max_n(mm, sh);
        M = mm[0];
        nanflag = mm[1];
    }
    if (nanflag != 0.0) M = __builtin_nan("");
    const double sM = finite_d(M) ? M : 0.0;
    double scale[KB];
    bool use[KB];
    double red[6] = {0.0, 0.0, 0.0, 0.0, nl, nm};    // cnt, s1, s2, W, leapfrogs, moved
#pragma unroll
    for (int k = 0; k < KB; ++k) {
        const double mb = pv[k][0];
        use[k] = has[k] && !(mb == -kInf || mb != mb);
        scale[k] = 0.0;
        if (!use[k]) continue;
        scale[k] = exp((finite_d(mb) ? mb : 0.0) - sM);
        const double cb = pv[k][1], s1b = pv[k][2];
        if (mb == M) { red[0] += cb; red[1] += s1b * scale[k]; }
        else red[1] += (s1b + cb) * scale[k];
        red[2] += pv[k][3] * scale[k] * scale[k];
        red[3] += (s1b + cb) * scale[k];
    }
    block_sum_n(red, sh);
    const double W = red[3];
    if (threadIdx.x == 0) {
        out[0] = M; out[1] = red[0]; out[2] = red[1]; out[3] = red[2];
        cnt[2 * g] = red[4];
        cnt[2 * g + 1] = red[5];
        hist0[(int64_t)g * hist_stride + H_LEAPS] = red[4];
        hist0[(int64_t)g * hist_stride + H_MOVED] = red[5];
    }
    double a[DC], bq[DC];
#pragma unroll
    for (int c = 0; c < DC; ++c) {
        a[c] = 0.0;
#pragma unroll
        for (int k = 0; k < KB; ++k) {
            if (!use[k]) continue;
            const double Wb = pv[k][1] + pv[k][2];
            const double r = pv[k][4 + 2 * DC + c];
            a[c] += (pv[k][4 + c] + (r - sc[c]) * Wb) * scale[k];
        }
    }
    block_sum_n(a, sh);
#pragma unroll
    for (int c = 0; c < DC; ++c) {
        const double dm = W > 0.0 ? a[c] / W : 0.0;   // this shard's mean - shift
        bq[c] = 0.0;
#pragma unroll
        for (int k = 0; k < KB; ++k) {
            if (!use[k]) continue;
            const double Wb = pv[k][1] + pv[k][2];
            const double d = (pv[k][4 + 2 * DC + c] - sc[c]) - dm;   // reference point - shard mean
            bq[c] += (pv[k][4 + DC + c] + d * fma(d, Wb, 2.0 * pv[k][4 + c])) * scale[k];
        }
    }
    block_sum_n(bq, sh);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < DC; ++c) { out[4 + c] = a[c]; out[4 + DC + c] = bq[c]; }
    }
    __syncthreads();    // the row written above is read below
    if (gathB)
        for (int q = threadIdx.x; q < NQ; q += kRedBlock) gathB[(int64_t)g * NQ + q] = out[q];
    if (combine)
        combine_ranks_body(out, 1, 0, DC, n_total, log_n_local, shift, phi, hist0 + (int64_t)(g + 1) * hist_stride,
                           g == B - 1 ? ss : ss_scratch + (int64_t)g * ss_stride, B * NQ);
}

}  // namespace smcn
