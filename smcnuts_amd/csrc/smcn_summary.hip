// libsmcnuts_hip.so, the summary unit: weighted quantiles and tail masses (smcn_summary_*) and the posterior covariance
// (smcn_cov_*) of the population smcn_summary_begin stages.  Owns the kernels of smcn_quantile.hpp and smcn_cov.hpp, and
// smcn_ctx's sm and cov.
#include <cmath>

#include "smcn_ctx.hpp"
#include "smcn_quantile.hpp"
#include "smcn_cov.hpp"

// ---- posterior summaries: weighted quantiles and tail masses (smcn_quantile.hpp) -------------------------------------------
namespace {
struct SmLayout {
    double *vals, *lw, *head, *thr_at, *out, *cdf_out;
    u64 *fw, *tot, *pfx[2], *thr[2], *thr0, *cnt;
    int *nan, *nan_cdf;
};
int64_t sm_words(int64_t M, int Dc) { return (int64_t)Dc * M + 2 * M + 48 + (int64_t)Dc * (4 + 8 * kSmMaxQ); }
SmLayout sm_layout(const smcn_ctx* c) {
    const int64_t M = c->sm.M, S = (int64_t)c->sm.Dc * kSmMaxQ;
    const int Dc = c->sm.Dc;
    SmLayout L;
    double* p = c->sm.buf;
    L.vals = p; p += (int64_t)Dc * M;
    L.fw = (u64*)p; p += M;
    L.lw = p; p += M;
    L.head = p; p += 16;
    L.tot = (u64*)p; p += 16;
    L.thr0 = (u64*)p; p += 16;
    L.nan = (int*)p; p += Dc;
    for (int i = 0; i < 2; ++i) { L.pfx[i] = (u64*)p; p += S; }
    for (int i = 0; i < 2; ++i) { L.thr[i] = (u64*)p; p += S; }
    L.thr_at = p; p += S;
    L.cnt = (u64*)p; p += S;
    L.out = p; p += S + Dc;
    L.nan_cdf = (int*)p; p += Dc;
    L.cdf_out = p;                  // S + Dc
    return L;
}
}  // namespace
// waits for the stream and adds the time between sm.ev[0] and sm.ev[last] to the call's device time
static int sm_finish(smcn_ctx* c, int last) {
    HIPC(c, stream_wait(c->stream));
    double ms = 0.0;
    HIPC(c, c->sm.ev[last].since(c->sm.ev[0], &ms));
    c->sm.ms += ms;
    return 0;
}
static int sm_hist_ensure(smcn_ctx* c) { return grow(c, c->sm.hist, (int64_t)c->sm.Dc * kSmMaxQ * 256 * 2 + c->sm.Dc); }
static dim3 sm_grid(const smcn_ctx* c) {
    return dim3((unsigned)grid_for(c->sm.M, kSmBlock * kSmElems), (unsigned)c->sm.Dc);
}
// one histogram pass over the staged population with the prefixes of state set c->sm.cur
static int sm_launch_hist(smcn_ctx* c, const SmLayout& L, int nq, int pass) {
    const int64_t bins = (int64_t)c->sm.Dc * nq * 256;
    HIPC(c, hipMemsetAsync(c->sm.hist, 0, sizeof(u64) * bins, c->stream));
    sm_hist_kernel<<<sm_grid(c), kSmBlock, sizeof(u64) * nq * 256, c->stream>>>(L.vals, c->sm.M, L.fw, L.pfx[c->sm.cur], nq,
                                                                                 pass, c->sm.hist, L.nan);
    HIPC(c, hipGetLastError());
    return 0;
}

extern "C" {

int smcn_summary_begin(smcn_ctx* c, const double* x, const double* logw, const double* v, int64_t M, int Dv, double* head) {
    CHECK_CTX(c);
    if (!head || M < 1) FAIL(c, "smcn_summary_begin: bad arguments");
    if (x && v) FAIL(c, "smcn_summary_begin: pass x (unconstrained) or v (constrained), not both");
    if (!x && !v && (M != c->N || logw))
        FAIL(c, "smcn_summary_begin: the resident particles come with their resident log-weights (x = v = NULL: logw = NULL, M = N)");
    if (v && (Dv < 1 || Dv > 65535)) FAIL(c, "smcn_summary_begin: v needs its number of columns (1 .. 65535)");
    if (M > (int64_t)1 << 40) FAIL(c, "smcn_summary_begin: too many particles");
    const int Dc = v ? Dv : c->Dc;
    c->sm.stage_state = 0;
    if (int rc = grow(c, c->sm.buf, sm_words(M, Dc))) return rc;
    c->sm.M = M;
    c->sm.Dc = Dc;
    int rc = 0;
    const SmLayout L = sm_layout(c);
    const int64_t n = M * Dc;
    if (x || v) {
        if ((rc = ensure_stage(c, n))) return rc;
        if (x && (rc = ensure_stage2(c, n))) return rc;
        HIPC(c, hipMemcpyAsync(c->stage, x ? x : v, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
        if (logw) HIPC(c, hipMemcpyAsync(L.lw, logw, sizeof(double) * M, hipMemcpyHostToDevice, c->stream));
        else HIPC(c, hipMemsetAsync(L.lw, 0, sizeof(double) * M, c->stream));
    }
    HIPC(c, c->sm.ev[0].record(c->stream));
    if (x) {                    // [M][D] through the model's constrain path, then coordinate-major
        launch_constrain_rows(c, c->stage, c->stage2, M);
        launch_transpose(c, c->stage2, L.vals, M, Dc);
    } else if (v) {
        launch_transpose(c, c->stage, L.vals, M, Dc);
    } else {                    // the resident generation, already [D][N]
        if (has_constrain_pass(c))
            launch_constrain_pass(c, c->x, L.vals, M, M, 1, M);
        else
            sm_stage_kernel<<<grid_for(n, 256), 256, 0, c->stream>>>(c->x, L.vals, M, c->D, c->cmodel);
        HIPC(c, hipMemcpyAsync(L.lw, c->logw, sizeof(double) * M, hipMemcpyDeviceToDevice, c->stream));
    }
    launch_pointwise_header(c, L.lw, M, L.head);
    // the header's sum once more, as an integer sum: the same bits for every order of the particles
    HIPC(c, hipMemsetAsync(L.tot, 0, sizeof(u64) * 4, c->stream));
    sm_total_kernel<<<grid_for(M, kSmBlock), kSmBlock, 0, c->stream>>>(L.lw, M, L.head, L.tot + 2);
    sm_total_final_kernel<<<1, 64, 0, c->stream>>>(L.tot + 2, L.head);
    HIPC(c, hipGetLastError());
    HIPC(c, c->sm.ev[1].record(c->stream));
    HIPC(c, hipMemcpyAsync(head, L.head, sizeof(double) * 4, hipMemcpyDeviceToHost, c->stream));
    c->sm.ms = 0.0;
    for (double& p : c->sm.pass_ms) p = 0.0;
    if ((rc = sm_finish(c, 1))) return rc;
    c->sm.stage_state = 1;
    return 0;
}

int smcn_summary_weights(smcn_ctx* c, double lw_max, double lw_sum, double* mass) {
    CHECK_CTX(c);
    if (c->sm.stage_state < 1) FAIL(c, "smcn_summary_weights: call smcn_summary_begin first");
    if (!mass || !std::isfinite(lw_max) || !(lw_sum > 0.0) || !std::isfinite(lw_sum))
        FAIL(c, "smcn_summary_weights: bad arguments (no particle with positive weight?)");
    const SmLayout L = sm_layout(c);
    HIPC(c, hipMemsetAsync(L.tot, 0, sizeof(u64) * 2, c->stream));
    HIPC(c, c->sm.ev[0].record(c->stream));
    sm_fixed_kernel<<<grid_for(c->sm.M, kSmBlock), kSmBlock, 0, c->stream>>>(L.lw, c->sm.M, lw_max, lw_sum, L.fw, L.tot);
    HIPC(c, hipGetLastError());
    HIPC(c, c->sm.ev[1].record(c->stream));
    u64 tot = 0;
    HIPC(c, hipMemcpyAsync(&tot, L.tot, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    int rc = sm_finish(c, 1);
    if (rc) return rc;
    *mass = (double)tot;
    c->sm.stage_state = 2;
    return 0;
}

static int sm_check_nq(smcn_ctx* c, const char* who, int nq) {
    if (c->sm.stage_state < 2) FAIL(c, std::string(who) + ": call smcn_summary_begin and smcn_summary_weights first");
    if (nq < 1 || nq > kSmMaxQ) FAIL(c, std::string(who) + ": 1 .. 16 probabilities");
    return sm_hist_ensure(c);
}

int smcn_summary_select(smcn_ctx* c, int nq, const double* thr) {
    CHECK_CTX(c);
    int rc = sm_check_nq(c, "smcn_summary_select", nq);
    if (rc) return rc;
    if (!thr) FAIL(c, "smcn_summary_select: bad arguments");
    c->sm.thr_h.assign(kSmMaxQ, 0);
    for (int q = 0; q < nq; ++q) {
        if (!(thr[q] >= 1.0 && thr[q] <= 9007199254740992.0) || (q && thr[q] < thr[q - 1]))
            FAIL(c, "smcn_summary_select: thresholds are masses in 1 .. 2^53, in ascending order");
        c->sm.thr_h[q] = (u64)thr[q];
    }
    const SmLayout L = sm_layout(c);
    HIPC(c, hipMemcpyAsync(L.thr0, c->sm.thr_h.data(), sizeof(u64) * kSmMaxQ, hipMemcpyHostToDevice, c->stream));
    HIPC(c, hipMemsetAsync(L.nan, 0, sizeof(int) * c->sm.Dc, c->stream));
    c->sm.cur = 0;
    HIPC(c, c->sm.ev[0].record(c->stream));
    for (int pass = 0; pass < 8; ++pass) {
        if ((rc = sm_launch_hist(c, L, nq, pass))) return rc;
        sm_pick_kernel<<<c->sm.Dc * nq, 256, 0, c->stream>>>(c->sm.hist, L.pfx[c->sm.cur], L.thr[c->sm.cur], L.thr0,
                                                             L.pfx[c->sm.cur ^ 1], L.thr[c->sm.cur ^ 1], nq, pass);
        HIPC(c, hipGetLastError());
        c->sm.cur ^= 1;
        HIPC(c, c->sm.ev[pass + 1].record(c->stream));
    }
    if ((rc = sm_finish(c, 8))) return rc;
    for (int pass = 0; pass < 8; ++pass) HIPC(c, c->sm.ev[pass + 1].since(c->sm.ev[pass], &c->sm.pass_ms[pass]));
    return 0;
}

int smcn_summary_hist(smcn_ctx* c, int pass, int nq, double* out) {
    CHECK_CTX(c);
    int rc = sm_check_nq(c, "smcn_summary_hist", nq);
    if (rc) return rc;
    if (!out || pass < 0 || pass > 7) FAIL(c, "smcn_summary_hist: bad arguments");
    const SmLayout L = sm_layout(c);
    if (pass == 0) {
        HIPC(c, hipMemsetAsync(L.nan, 0, sizeof(int) * c->sm.Dc, c->stream));
        c->sm.cur = 0;
        c->sm.pfx_h.assign((size_t)c->sm.Dc * nq, 0);
    } else if (c->sm.pfx_h.size() != (size_t)c->sm.Dc * nq) {
        FAIL(c, "smcn_summary_hist: passes 1 .. 7 follow smcn_summary_descend of the pass before, with the same probabilities");
    }
    const int64_t n = (int64_t)c->sm.Dc * (pass == 0 ? 1 : nq) * 256 + c->sm.Dc;
    double* const dout = (double*)(c->sm.hist + (int64_t)c->sm.Dc * kSmMaxQ * 256);
    HIPC(c, c->sm.ev[0].record(c->stream));
    if ((rc = sm_launch_hist(c, L, nq, pass))) return rc;
    sm_export_kernel<<<grid_for(n, 256), 256, 0, c->stream>>>(c->sm.hist, L.pfx[c->sm.cur], L.nan, c->sm.Dc, nq, pass, dout);
    HIPC(c, hipGetLastError());
    HIPC(c, c->sm.ev[1].record(c->stream));
    HIPC(c, hipMemcpyAsync(out, dout, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    if ((rc = sm_finish(c, 1))) return rc;
    HIPC(c, c->sm.ev[1].since(c->sm.ev[0], &c->sm.pass_ms[pass]));
    return 0;
}

int smcn_summary_descend(smcn_ctx* c, int pass, int nq, const int32_t* digits, const double* residual) {
    CHECK_CTX(c);
    int rc = sm_check_nq(c, "smcn_summary_descend", nq);
    if (rc) return rc;
    const size_t S = (size_t)c->sm.Dc * nq;
    if (!digits || !residual || pass < 0 || pass > 7 || c->sm.pfx_h.size() != S)
        FAIL(c, "smcn_summary_descend: follows smcn_summary_hist of the same pass");
    c->sm.thr_h.assign(S, 0);
    for (size_t i = 0; i < S; ++i) {
        if (digits[i] < 0 || digits[i] > 255 || !(residual[i] >= 0.0 && residual[i] <= 9007199254740992.0))
            FAIL(c, "smcn_summary_descend: digits are 0 .. 255, residual masses 0 .. 2^53");
        c->sm.pfx_h[i] = (pass == 0 ? 0ull : c->sm.pfx_h[i] << 8) | (u64)digits[i];
        c->sm.thr_h[i] = (u64)residual[i];
    }
    const SmLayout L = sm_layout(c);
    HIPC(c, hipMemcpyAsync(L.pfx[c->sm.cur], c->sm.pfx_h.data(), sizeof(u64) * S, hipMemcpyHostToDevice, c->stream));
    HIPC(c, hipMemcpyAsync(L.thr[c->sm.cur], c->sm.thr_h.data(), sizeof(u64) * S, hipMemcpyHostToDevice, c->stream));
    HIPC(c, stream_wait(c->stream));
    return 0;
}

int smcn_summary_values(smcn_ctx* c, int nq, double* out, double* nan_flags) {
    CHECK_CTX(c);
    int rc = sm_check_nq(c, "smcn_summary_values", nq);
    if (rc) return rc;
    if (!out || !nan_flags) FAIL(c, "smcn_summary_values: bad arguments");
    const SmLayout L = sm_layout(c);
    const int S = c->sm.Dc * nq;
    sm_values_kernel<<<grid_for(S, 256), 256, 0, c->stream>>>(L.pfx[c->sm.cur], S, L.out);
    sm_counts_kernel<<<grid_for(c->sm.Dc, 256), 256, 0, c->stream>>>(L.cnt, L.nan, 0, c->sm.Dc, L.out + S);
    HIPC(c, hipGetLastError());
    HIPC(c, hipMemcpyAsync(out, L.out, sizeof(double) * S, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipMemcpyAsync(nan_flags, L.out + S, sizeof(double) * c->sm.Dc, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, stream_wait(c->stream));
    return 0;
}

int smcn_summary_cdf(smcn_ctx* c, int T, const double* at, double* out) {
    CHECK_CTX(c);
    if (c->sm.stage_state < 2) FAIL(c, "smcn_summary_cdf: call smcn_summary_begin and smcn_summary_weights first");
    if (T < 1 || T > kSmMaxQ || !at || !out) FAIL(c, "smcn_summary_cdf: 1 .. 16 thresholds per coordinate");
    const SmLayout L = sm_layout(c);
    const int S = c->sm.Dc * T;
    int* const nan = L.nan_cdf;      // (its own NaN flags: the call does not depend on a selection before it)
    HIPC(c, hipMemcpyAsync(L.thr_at, at, sizeof(double) * S, hipMemcpyHostToDevice, c->stream));
    HIPC(c, hipMemsetAsync(L.cnt, 0, sizeof(u64) * S, c->stream));
    HIPC(c, hipMemsetAsync(nan, 0, sizeof(int) * c->sm.Dc, c->stream));
    HIPC(c, c->sm.ev[0].record(c->stream));
    sm_cdf_kernel<<<sm_grid(c), kSmBlock, 0, c->stream>>>(L.vals, c->sm.M, L.fw, L.thr_at, T, L.cnt, nan);
    double* const dout = L.cdf_out;
    sm_counts_kernel<<<grid_for(S + c->sm.Dc, 256), 256, 0, c->stream>>>(L.cnt, nan, S, c->sm.Dc, dout);
    HIPC(c, hipGetLastError());
    HIPC(c, c->sm.ev[1].record(c->stream));
    HIPC(c, hipMemcpyAsync(out, dout, sizeof(double) * (S + c->sm.Dc), hipMemcpyDeviceToHost, c->stream));
    return sm_finish(c, 1);
}

int smcn_summary_last_ms(const smcn_ctx* c, double* ms) {
    if (!c || !ms) return -1;
    *ms = c->sm.ms;
    return 0;
}

int smcn_summary_pass_ms(const smcn_ctx* c, double* ms) {
    if (!c || !ms) return -1;
    for (int i = 0; i < 8; ++i) ms[i] = c->sm.pass_ms[i];
    return 0;
}

// ---- posterior covariance (smcn_cov.hpp) ---------------------------------------------------------------------------------
int smcn_cov_dims(const smcn_ctx* c, int64_t* out) {
    if (!c || !out) return -1;
    if (c->sm.stage_state < 1) return -3;
    out[0] = c->sm.M;
    out[1] = c->sm.Dc;
    out[2] = c->sm.Dc <= kCovMaxDc ? cov_slices(c->sm.M, c->sm.Dc) : 0;
    out[3] = c->sm.Dc <= kCovMaxDc ? cov_slice_cap(c->sm.Dc) : 0;
    return 0;
}

int smcn_cov_partials(smcn_ctx* c, double lw_max, const double* centre, int64_t slices, double* out, double* centre_out) {
    CHECK_CTX(c);
    if (c->sm.stage_state < 1) FAIL(c, "smcn_cov_partials: call smcn_summary_begin first");
    if (!out && !centre_out) FAIL(c, "smcn_cov_partials: bad arguments");
    if (!std::isfinite(lw_max)) FAIL(c, "smcn_cov_partials: lw_max must be finite (no particle with positive weight?)");
    const int Dc = c->sm.Dc;
    const int64_t M = c->sm.M;
    if (Dc > kCovMaxDc)
        FAIL(c, "smcn_cov_partials: at most 1023 constrained coordinates, not " + std::to_string(Dc));
    const int64_t cap = cov_slice_cap(Dc);
    if (slices < 0 || slices > cap)
        FAIL(c, "smcn_cov_partials: slices must be 0 (the rule's own count) or 1 .. " + std::to_string(cap) +
                    " for " + std::to_string(Dc) + " coordinates");
    if (slices == 0) slices = cov_slices(M, Dc);
    const int T = cov_tiles(Dc), Da = Dc + 1, NB = (T + kCovBlock - 1) / kCovBlock;
    const int64_t entries = cov_tile_pairs(Dc) * 256, groups = (slices + kCovGroup - 1) / kCovGroup;
    const int64_t chunks = (M + 15) / 16, cps = (chunks + slices - 1) / slices;
    // cov.buf: [w M | centre 16 T | slice partials | group partials | result Da Da | the centre's chunk sums 2 Dc nch]
    const int64_t nch = (M + kCovCentreChunk - 1) / kCovCentreChunk;
    const int64_t o_c = (M + 15) / 16 * 16, o_part = o_c + 16 * T, o_grp = o_part + slices * entries;
    const int64_t o_out = o_grp + groups * entries, o_cp = o_out + (int64_t)Da * Da, words = o_cp + 2 * Dc * nch;
    if (int rc = grow(c, c->cov.buf, words)) return rc;
    const SmLayout L = sm_layout(c);
    double *const w = c->cov.buf, *const cen = c->cov.buf + o_c, *const part = c->cov.buf + o_part;
    double *const grp = c->cov.buf + o_grp, *const res = c->cov.buf + o_out;
    if (centre) HIPC(c, hipMemcpyAsync(cen, centre, sizeof(double) * Dc, hipMemcpyHostToDevice, c->stream));
    HIPC(c, c->cov.ev[0].record(c->stream));
    cov_weight_kernel<<<grid_for(M, 256), 256, 0, c->stream>>>(L.lw, M, lw_max, w);
    if (!centre) {
        double* const cp = c->cov.buf + o_cp;
        cov_centre_partial_kernel<<<dim3((unsigned)nch, (unsigned)Dc), kRedBlock, 0, c->stream>>>(L.vals, w, M, nch, cp);
        cov_centre_final_kernel<<<Dc, kRedBlock, 0, c->stream>>>(cp, nch, cen);
    }
    if (out) {
        cov_partials_kernel<kCovBlock><<<dim3((unsigned)(NB * (NB + 1) / 2), (unsigned)slices), 64, 0, c->stream>>>(
            L.vals, w, cen, M, Dc, T, NB, cps, part);
        cov_combine_kernel<false><<<dim3((unsigned)grid_for(entries, 256), (unsigned)groups), 256, 0, c->stream>>>(
            part, slices, entries, T, Da, grp);
        cov_combine_kernel<true><<<grid_for(entries, 256), 256, 0, c->stream>>>(grp, groups, entries, T, Da, res);
    }
    HIPC(c, hipGetLastError());
    HIPC(c, c->cov.ev[1].record(c->stream));
    if (out) HIPC(c, hipMemcpyAsync(out, res, sizeof(double) * Da * Da, hipMemcpyDeviceToHost, c->stream));
    if (centre_out) HIPC(c, hipMemcpyAsync(centre_out, cen, sizeof(double) * Dc, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, stream_wait(c->stream));
    HIPC(c, c->cov.ev[1].since(c->cov.ev[0], &c->cov.ms));
    return 0;
}

int smcn_cov_last_ms(const smcn_ctx* c, double* ms) {
    if (!c || !ms) return -1;
    *ms = c->cov.ms;
    return 0;
}

}  // extern "C"
