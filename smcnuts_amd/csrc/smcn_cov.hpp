// Posterior covariance: the weighted second moments of the constrained coordinates of a staged population
// (smcn_summary_begin's image, vals[c * M + t]) as ONE symmetric matrix product on the fp64 matrix cores.
//
// With a = v - c (c: a centre near the mean) and one appended constant coordinate "1" (centre 0) the augmented
// (Dc + 1) x (Dc + 1) matrix  sum_p w_p [a_p; 1][a_p; 1]^T = [[G, S1], [S1^T, W]]  holds every sum the covariance needs:
// G_ij = sum w a_i a_j, S1_i = sum w a_i, W = sum w.  The host finishes with d = S1 / W, C = G / W - d d^T, m = c + d
// (covariance.py); sum w v v^T - m m^T is never formed.
//
// Product.  v_mfma_f64_16x16x4_f64 (__builtin_amdgcn_mfma_f64_16x16x4f64): lane l holds A[row l & 15][k l >> 4] and
// B[k l >> 4][col l & 15], one double each; result register r of lane l is C[row (l >> 4) + 4 r][col l & 15] (NOT the f32
// map).  A = w (v - c), B = (v - c); the k index is the particle.  The image is coordinate-major, so lane l loads a run
// of 4 consecutive particles (32 bytes) of its row, particles p0 + 4 (l >> 4) + t, t = 0..3, of a chunk of 16; step t of
// the chunk's 4 MFMAs consumes element t of every lane's run -- the same permutation of k in A and in B, which a sum over
// k allows.  Padding coordinates (the augmented dimension rounded up to 16) and padding particles enter as exact zeros;
// so does every particle of weight 0, in A AND in B (0 * NaN is NaN on the matrix cores too).  A non-finite value of a
// particle of positive weight reaches exactly the dot products of its row and its column.
//
// Shape.  One wavefront owns a B x B block of 16 x 16 output tiles (B = kCovBlock) of the upper triangle and a slice of
// the particles: per chunk it loads B row runs for A, B for B (a diagonal block: the same loads), and issues up to
// 4 B^2 MFMAs into B^2 accumulators that never leave the registers.  The grid is (blocks of the upper triangle) x
// (particle slices); a slice's partial is stored once, cov_combine_kernel merges the slices per entry in slice order
// (groups of 16, then the groups: pointwise_combine_kernel's scheme) and mirrors the upper triangle.  No LDS, no
// atomics, no scratch; a result depends on (inputs, slices) alone.
#pragma once
#include "smcn_pw_walk.hpp"

namespace smcn {

constexpr int kCovMaxDc = 1023;        // augmented dimension <= 1024: 64 tile rows
constexpr int kCovGroup = 16;          // slices merged per stage-1 thread
#ifndef SMCN_COV_BLOCK
#define SMCN_COV_BLOCK 2
#endif
constexpr int kCovBlock = SMCN_COV_BLOCK;   // tiles per wavefront along each side (the shapes built and why this one)
constexpr int64_t kCovMaxSlices = 1024;
constexpr int64_t kCovMaxPartWords = (int64_t)1 << 23;   // the slices' partials stay below 64 MiB

using cov_d4 = __attribute__((ext_vector_type(4))) double;

__host__ __device__ inline int cov_tiles(int Dc) { return (Dc + 1 + 15) / 16; }
__host__ __device__ inline int64_t cov_tile_pairs(int Dc) { const int64_t T = cov_tiles(Dc); return T * (T + 1) / 2; }
// index of upper-triangle tile (I <= J) of a T x T tile grid, row by row
__host__ __device__ inline int64_t cov_pair_index(int I, int J, int T) { return (int64_t)I * T - (int64_t)I * (I - 1) / 2 + (J - I); }
// the most slices a call may use: the partials, slices * tile pairs * 256 doubles, stay below 64 MiB; never above 1024
__host__ __device__ inline int64_t cov_slice_cap(int Dc) {
    const int64_t cap = kCovMaxPartWords / (cov_tile_pairs(Dc) * 256);
    return cap < 1 ? 1 : (cap > kCovMaxSlices ? kCovMaxSlices : cap);
}
// slices of a call, a function of M and Dc alone: about 4096 wavefronts (four per SIMD, what the partials kernel's
// registers admit) over the blocks of the upper triangle, at least 4 chunks of 16 particles each, at most cov_slice_cap
__host__ __device__ inline int64_t cov_slices(int64_t M, int Dc) {
    const int64_t NB = (cov_tiles(Dc) + kCovBlock - 1) / kCovBlock, blocks = NB * (NB + 1) / 2;
    const int64_t chunks = (M + 15) / 16, most = (chunks + 3) / 4, cap = cov_slice_cap(Dc);
    int64_t want = (4096 + blocks - 1) / blocks;
    want = want > most ? most : want;
    want = want > cap ? cap : want;
    return want < 1 ? 1 : want;
}

// w[t] = exp(lw[t] - mw) for a finite log-weight, 0 otherwise (pointwise_header_kernel's and sm_fixed_kernel's exponential)
__global__ void cov_weight_kernel(const double* __restrict__ lw, int64_t M, double mw, double* __restrict__ w) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= M) return;
    const double v = lw[t];
    w[t] = finite_d(v) ? pw_exp_neg(v - mw) : 0.0;
}

// The shard's own weighted mean over the particles of positive weight, in two stages of fixed order and no atomics.
// Stage 1, grid (chunks of kCovCentreChunk particles, Dc): the chunk's sum w v and sum w of coordinate blockIdx.y
// (block_sum's fixed tree) to part[(c * nch + chunk) * 2 + {0, 1}].  Stage 2, one block per coordinate: the chunks'
// sums thread-strided in chunk order, then the tree; 0 where the shard has no weight.
constexpr int kCovCentreElems = 8;
constexpr int kCovCentreChunk = kRedBlock * kCovCentreElems;
__global__ void __launch_bounds__(kRedBlock) cov_centre_partial_kernel(const double* __restrict__ vals,
                                                                       const double* __restrict__ w, int64_t M,
                                                                       int64_t nch, double* __restrict__ part) {
    __shared__ double sh[4];
    const double* const col = vals + (int64_t)blockIdx.y * M;
    const int64_t base = (int64_t)blockIdx.x * kCovCentreChunk;
    double s = 0.0, sw = 0.0;
#pragma unroll
    for (int e = 0; e < kCovCentreElems; ++e) {
        const int64_t t = base + e * kRedBlock + threadIdx.x;
        if (t < M) {
            const double wt = w[t], x = col[t];
            const bool on = wt > 0.0;                   // (a value without weight is never multiplied)
            s = on ? fma(wt, x, s) : s;
            sw = on ? sw + wt : sw;
        }
    }
    s = block_sum(s, sh);
    sw = block_sum(sw, sh);
    if (threadIdx.x == 0) {
        double* const o = part + ((int64_t)blockIdx.y * nch + blockIdx.x) * 2;
        o[0] = s;
        o[1] = sw;
    }
}
__global__ void __launch_bounds__(kRedBlock) cov_centre_final_kernel(const double* __restrict__ part, int64_t nch,
                                                                     double* __restrict__ centre) {
    __shared__ double sh[4];
    const double* const p = part + (int64_t)blockIdx.x * nch * 2;
    double s = 0.0, sw = 0.0;
    for (int64_t k = threadIdx.x; k < nch; k += kRedBlock) {
        s += p[2 * k];
        sw += p[2 * k + 1];
    }
    s = block_sum(s, sh);
    sw = block_sum(sw, sh);
    if (threadIdx.x == 0) centre[blockIdx.x] = sw > 0.0 ? s / sw : 0.0;
}

// a lane's run of 4 consecutive doubles row[p .. p + 3], zeros past M; two 16-byte loads where the run is aligned
__device__ __forceinline__ void cov_load4(const double* __restrict__ row, int64_t p, int64_t M, bool vec, double (&o)[4]) {
    if (p + 4 <= M) {
        if (vec) {
            const double2 a = *reinterpret_cast<const double2*>(row + p), b = *reinterpret_cast<const double2*>(row + p + 2);
            o[0] = a.x; o[1] = a.y; o[2] = b.x; o[3] = b.y;
        } else {
#pragma unroll
            for (int t = 0; t < 4; ++t) o[t] = row[p + t];
        }
    } else {
#pragma unroll
        for (int t = 0; t < 4; ++t) o[t] = p + t < M ? row[p + t] : 0.0;
    }
}

// the masked differences d[t] = v - c of coordinate ci for the run's particles: 0 where the weight is 0, for a padding
// coordinate (ci > Dc) and past M; the constant coordinate ci == Dc is 1 (centre 0)
__device__ __forceinline__ void cov_diff4(const double* __restrict__ vals, const double* __restrict__ centre, int ci, int Dc,
                                          int64_t p, int64_t M, bool vec, const double (&wv)[4], double (&d)[4]) {
    double x[4] = {0.0, 0.0, 0.0, 0.0};
    double c = 0.0;
    if (ci < Dc) {
        cov_load4(vals + (int64_t)ci * M, p, M, vec, x);
        c = centre[ci];
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const double v = ci < Dc ? x[t] - c : (ci == Dc ? 1.0 : 0.0);
        d[t] = wv[t] > 0.0 ? v : 0.0;
    }
}

// Partials of one block of the upper triangle over one slice: part[(slice * pairs + pair(I, J)) * 256 + row * 16 + col].
// Grid (NB (NB + 1) / 2 blocks, slices), NB = ceil(T / B); 64 threads.  cps: chunks of 16 particles per slice.
template <int B>
__global__ void __launch_bounds__(64) cov_partials_kernel(const double* __restrict__ vals, const double* __restrict__ w,
                                                          const double* __restrict__ centre, int64_t M, int Dc, int T,
                                                          int NB, int64_t cps, double* __restrict__ part) {
    const int lane = (int)(threadIdx.x & 63u), r = lane & 15, g = lane >> 4;
    int bi = 0, rem = (int)blockIdx.x;
    while (rem >= NB - bi) {
        rem -= NB - bi;
        ++bi;
    }
    const int bj = bi + rem;
    const bool diag = bi == bj;
    const int64_t slice = blockIdx.y, chunks = (M + 15) / 16;
    const int64_t c0 = slice * cps, c1 = c0 + cps < chunks ? c0 + cps : chunks;
    const bool vec = (M & 1) == 0;                     // rows start 16-byte aligned and a run starts at a multiple of 4
    cov_d4 acc[B][B];
#pragma unroll
    for (int i = 0; i < B; ++i)
#pragma unroll
        for (int j = 0; j < B; ++j) acc[i][j] = cov_d4{0.0, 0.0, 0.0, 0.0};
    for (int64_t ch = c0; ch < c1; ++ch) {
        const int64_t p = ch * 16 + 4 * g;
        double wv[4];
        cov_load4(w, p, M, true, wv);                  // (the weights' buffer is 16-byte aligned for every M)
        double a[B][4], b[B][4];
#pragma unroll
        for (int i = 0; i < B; ++i) {
            if (bi * B + i < T) {                      // (wave-uniform)
                double d[4];
                cov_diff4(vals, centre, (bi * B + i) * 16 + r, Dc, p, M, vec, wv, d);
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    a[i][t] = wv[t] * d[t];
                    if (diag) b[i][t] = d[t];
                }
            }
        }
        if (!diag) {
#pragma unroll
            for (int j = 0; j < B; ++j)
                if (bj * B + j < T) cov_diff4(vals, centre, (bj * B + j) * 16 + r, Dc, p, M, vec, wv, b[j]);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int i = 0; i < B; ++i)
#pragma unroll
                for (int j = 0; j < B; ++j)
                    if (bi * B + i < T && bj * B + j < T && (!diag || i <= j))
                        acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i][t], b[j][t], acc[i][j], 0, 0, 0);
    }
    const int64_t pairs = (int64_t)T * (T + 1) / 2;
#pragma unroll
    for (int i = 0; i < B; ++i)
#pragma unroll
        for (int j = 0; j < B; ++j) {
            const int I = bi * B + i, J = bj * B + j;
            if (I < T && J < T && (!diag || i <= j)) {
                double* const o = part + (slice * pairs + cov_pair_index(I, J, T)) * 256;
#pragma unroll
                for (int q = 0; q < 4; ++q) o[(g + 4 * q) * 16 + r] = acc[i][j][q];
            }
        }
}

// Merges the slices' partials per entry in slice order.  Stage 1 (FINAL = false): group blockIdx.y's slices
// [g kCovGroup, (g + 1) kCovGroup) into grp[g][entry]; stage 2 (FINAL = true): the groups in order, written to
// out[i][j] and out[j][i] of the (Dc + 1)^2 matrix for i <= j (a diagonal tile's lower half is dropped).
template <bool FINAL>
__global__ void cov_combine_kernel(const double* __restrict__ part, int64_t n, int64_t entries, int T, int Da,
                                   double* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= entries) return;
    const int64_t s0 = FINAL ? 0 : (int64_t)blockIdx.y * kCovGroup;
    const int64_t s1 = FINAL ? n : (s0 + kCovGroup < n ? s0 + kCovGroup : n);
    double s = 0.0;
    for (int64_t k = s0; k < s1; ++k) s += part[k * entries + e];
    if (!FINAL) {
        out[(int64_t)blockIdx.y * entries + e] = s;
        return;
    }
    int64_t pair = e >> 8;
    int I = 0;
    while (pair >= T - I) {
        pair -= T - I;
        ++I;
    }
    const int J = I + (int)pair, i = I * 16 + (int)((e >> 4) & 15), j = J * 16 + (int)(e & 15);
    if (i <= j && j < Da) {
        out[(int64_t)i * Da + j] = s;
        out[(int64_t)j * Da + i] = s;
    }
}

}  // namespace smcn
