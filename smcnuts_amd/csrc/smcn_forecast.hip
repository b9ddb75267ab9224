// libsmcnuts_hip.so, the forecast unit: the arma target's h-step laws, their mixture's partials and simulated paths
// (smcn_forecast_*), and its in-sample one-step residual checks (smcn_residuals_*).  Owns the kernels of
// smcn_forecast.hpp and smcn_residuals.hpp and smcn_ctx's fc and rs.
#include <cmath>

#include "smcn_ctx.hpp"
#include "smcn_forecast.hpp"
#include "smcn_residuals.hpp"

// The one check of the unit's entry points: a context, and an arma one (`scope` names what the caller asked for)
#define ARMA_CHECK(c, who, scope)                                                              \
    CHECK_CTX(c);                                                                              \
    if ((c)->model != SMCN_MODEL_ARMA) FAIL(c, std::string(who) + ": " + scope);
static const char* kFcScope = "forecasts cover SMCN_MODEL_ARMA contexts only";
static const char* kRsScope = "one-step residual checks cover SMCN_MODEL_ARMA contexts only";
#define FC_CHECK(c, who) ARMA_CHECK(c, who, kFcScope)
#define RS_CHECK(c, who) ARMA_CHECK(c, who, kRsScope)
#define FC_CHECK_SET(c, who) \
    if ((c)->fc.H < 1) FAIL(c, std::string(who) + ": no horizon (smcn_forecast_set first)")

static int64_t fc_slices(int64_t M) { return (M + kFcBlock - 1) / kFcBlock; }
// slices whose partials the slab holds at once: whole groups, at most 4096 slices and about 2^22 doubles
static int64_t fc_window(int64_t H, int Q) {
    int64_t w = ((int64_t)1 << 22) / (H * Q);
    w = w > 4096 ? 4096 : w;
    w = w / kFcGroup * kFcGroup;
    return w < kFcGroup ? kFcGroup : w;
}
static const double* fc_yf(const smcn_ctx* c) { return c->fc.has_y ? (const double*)c->fc.set : nullptr; }
static const double* fc_at(const smcn_ctx* c) { return c->fc.Tn ? (const double*)c->fc.set + c->fc.H : nullptr; }

extern "C" {

int smcn_forecast_set(smcn_ctx* c, int64_t H, const double* y_future, const double* at, int Tn) {
    FC_CHECK(c, "smcn_forecast_set");
    if (H < 1 || H > kFcMaxH) FAIL(c, "smcn_forecast_set: the horizon H must be in 1..512");
    if (Tn < 0 || Tn > kFcMaxAt) FAIL(c, "smcn_forecast_set: the number of thresholds per horizon Tn must be in 0..16");
    if ((Tn > 0) != (at != nullptr)) FAIL(c, "smcn_forecast_set: `at` holds [H][Tn] thresholds (NULL with Tn = 0 only)");
    std::vector<double> h((size_t)(H * (1 + Tn)), 0.0);
    for (int64_t i = 0; y_future && i < H; ++i) {
        if (!std::isfinite(y_future[i])) FAIL(c, "smcn_forecast_set: y_future[" + std::to_string(i) + "] is not finite");
        h[i] = y_future[i];
    }
    for (int64_t i = 0; i < H * Tn; ++i) {
        if (!std::isfinite(at[i])) FAIL(c, "smcn_forecast_set: at[" + std::to_string(i) + "] is not finite");
        h[H + i] = at[i];
    }
    c->fc.H = 0;
    const int rc = grow(c, c->fc.set, (int64_t)h.size());
    if (rc) return rc;
    HIPC(c, stream_wait(c->stream));                             // (a kernel of an earlier call may still read the setting)
    HIPC(c, hipMemcpyAsync(c->fc.set, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, c->stream));
    HIPC(c, stream_wait(c->stream));                             // (h is a local)
    c->fc.H = H;
    c->fc.Tn = Tn;
    c->fc.has_y = y_future ? 1 : 0;
    return 0;
}

int smcn_forecast_dims(smcn_ctx* c, int64_t* H, int* Q, int* has_y, int* Tn) {
    FC_CHECK(c, "smcn_forecast_dims");
    FC_CHECK_SET(c, "smcn_forecast_dims");
    if (H) *H = c->fc.H;
    if (Q) *Q = kFcCols + c->fc.Tn;
    if (has_y) *has_y = c->fc.has_y;
    if (Tn) *Tn = c->fc.Tn;
    return 0;
}

int smcn_forecast_slices(smcn_ctx* c, int64_t M, int64_t* slices) {
    FC_CHECK(c, "smcn_forecast_slices");
    FC_CHECK_SET(c, "smcn_forecast_slices");
    if (M < 1 || !slices) FAIL(c, "smcn_forecast_slices: bad arguments");
    *slices = fc_slices(M);
    return 0;
}

int smcn_forecast_points(smcn_ctx* c, const double* x, int64_t M, double* out) {
    FC_CHECK(c, "smcn_forecast_points");
    FC_CHECK_SET(c, "smcn_forecast_points");
    if (!x || !out || M < 1) FAIL(c, "smcn_forecast_points: bad arguments");
    const int64_t H = c->fc.H, W = 1 + (c->fc.has_y ? 4 : 2) * H;
    if (fc_slices(M) > 2147483647LL) FAIL(c, "smcn_forecast_points: too many points");
    int rc = ensure_stage(c, M * c->D);
    if (rc) return rc;
    if ((rc = grow(c, c->fc.buf, M * W))) return rc;
    HIPC(c, hipMemcpyAsync(c->stage, x, sizeof(double) * M * c->D, hipMemcpyHostToDevice, c->stream));
    forecast_points_kernel<<<(int)fc_slices(M), kFcBlock, 0, c->stream>>>(c->mdata, c->stage, M, (int)H, fc_yf(c), c->fc.buf);
    HIPC(c, hipGetLastError());
    HIPC(c, hipMemcpyAsync(out, c->fc.buf, sizeof(double) * M * W, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, stream_wait(c->stream));
    return 0;
}

int smcn_forecast_partials(smcn_ctx* c, const double* x, const double* logw, int64_t M, double* out) {
    FC_CHECK(c, "smcn_forecast_partials");
    FC_CHECK_SET(c, "smcn_forecast_partials");
    if (!out || M < 1) FAIL(c, "smcn_forecast_partials: bad arguments");
    const int H = (int)c->fc.H, Tn = c->fc.Tn, Q = kFcCols + Tn;
    const int64_t slices = fc_slices(M), groups = (slices + kFcGroup - 1) / kFcGroup, win = fc_window(H, Q);
    const int64_t row = (int64_t)H * Q;
    if (groups > 65535) FAIL(c, "smcn_forecast_partials: too many particles (M <= 268431360)");
    // fc.buf: [header 16 | lw M | slab (a window of slices) | group partials | result (1 + H) Q]
    const int64_t o_lw = 16, o_slab = o_lw + (M + 15) / 16 * 16, o_grp = o_slab + (slices < win ? slices : win) * row;
    const int64_t o_out = o_grp + groups * row;
    int rc = grow(c, c->fc.buf, o_out + (1 + H) * Q);
    if (rc) return rc;
    double* const B = c->fc.buf;
    Particles P;
    if ((rc = stage_particles(c, "smcn_forecast_partials", x, logw, M, B + o_lw, &P))) return rc;
    HIPC(c, c->fc.ev0.record(c->stream));
    launch_pointwise_header(c, P.lw, M, B);
    for (int64_t s0 = 0; s0 < slices; s0 += win) {
        const int64_t ns = slices - s0 < win ? slices - s0 : win, ng = (ns + kFcGroup - 1) / kFcGroup;
        if (c->fc.has_y)
            forecast_partials_kernel<true><<<(int)ns, kFcBlock, 0, c->stream>>>(c->mdata, P.xd, P.rs, P.cs, P.lw, B, M, s0 * kFcBlock, H,
                                                                                 Tn, fc_yf(c), fc_at(c), B + o_slab);
        else
            forecast_partials_kernel<false><<<(int)ns, kFcBlock, 0, c->stream>>>(c->mdata, P.xd, P.rs, P.cs, P.lw, B, M, s0 * kFcBlock, H,
                                                                                  Tn, nullptr, fc_at(c), B + o_slab);
        forecast_merge_kernel<false><<<dim3((unsigned)grid_for(row, 256), (unsigned)ng), 256, 0, c->stream>>>(
            B + o_slab, B, ns, H, Q, B + o_grp + s0 / kFcGroup * row);
    }
    forecast_merge_kernel<true><<<grid_for(row, 256), 256, 0, c->stream>>>(B + o_grp, B, groups, H, Q, B + o_out);
    HIPC(c, hipGetLastError());
    HIPC(c, c->fc.ev1.record(c->stream));
    HIPC(c, hipMemcpyAsync(out, B + o_out, sizeof(double) * (1 + H) * Q, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, stream_wait(c->stream));
    HIPC(c, c->fc.ev1.since(c->fc.ev0, &c->fc.ms[0]));
    return 0;
}

int smcn_forecast_draws(smcn_ctx* c, const double* x, const double* logw, int64_t M, int64_t S, uint64_t seed,
                        const int64_t* ancestors, int64_t s_first, int64_t s_count, double* y_out, int64_t* ancestors_out,
                        int64_t* n_bad_out) {
    FC_CHECK(c, "smcn_forecast_draws");
    FC_CHECK_SET(c, "smcn_forecast_draws");
    const std::string why = draw_refusal("smcn_forecast_draws", "paths", M, S, s_first, s_count, y_out, ancestors);
    if (!why.empty()) FAIL(c, why);
    const int64_t H = c->fc.H, n = s_count;
    // fc.dbuf: [the plan's front | y n H]
    const DrawPlan p(M, n, kScanTile);
    const int64_t o_y = p.o_tail;
    int rc = grow(c, c->fc.dbuf, o_y + n * H);
    if (rc) return rc;
    double* const B = c->fc.dbuf;
    const int64_t* const anc = (const int64_t*)(B + p.o_anc);
    Particles P;
    if ((rc = stage_particles(c, "smcn_forecast_draws", x, logw, M, B + p.o_lw, &P))) return rc;
    if ((rc = draw_ancestors(c, "smcn_forecast_draws", c->fc.ev0, p, B, P.lw, M, S, s_first, n, seed, kStreamFcAnc, ancestors, true)))
        return rc;
    forecast_draws_kernel<<<grid_for(n, kFcBlock), kFcBlock, 0, c->stream>>>(c->mdata, P.xd, P.rs, P.cs, anc, n, s_first, seed, (int)H,
                                                                            B + o_y);
    return draw_finish(c, "smcn_forecast_draws", c->fc.ev0, c->fc.ev1, &c->fc.ms[1], nullptr, anc, n, B + o_y, n * H, y_out,
                       ancestors_out, n_bad_out);
}

int smcn_forecast_last_ms(const smcn_ctx* c, double* ms) {
    if (!c || !ms) return -1;
    ms[0] = c->fc.ms[0];
    ms[1] = c->fc.ms[1];
    return 0;
}

}  // extern "C"

// ---- one-step residual checks (smcn_residuals.hpp) ------------------------------------------------------------------------
#define RS_CHECK_SET(c, who) \
    if ((c)->rs.L < 0) FAIL(c, std::string(who) + ": no lags set (smcn_residuals_set first)")

static int64_t rs_rows(const smcn_ctx* c) { return c->arma_T + (c->rs.L > 0 ? c->rs.L + 1 : 0); }
// slices whose partials the slab holds at once, by forecast's rule: whole groups, about 2^22 doubles (a group always fits:
// smcn_residuals_set bounds the rows)
static int64_t rs_window(int64_t R) { return fc_window(R, kRsCols); }

template <int LM>
static void rs_launch(smcn_ctx* c, const Particles& P, double* B, int64_t M, int64_t s0, int64_t ns, double* slab) {
    residuals_partials_kernel<LM><<<(int)ns, kFcBlock, 0, c->stream>>>(c->mdata, P.xd, P.rs, P.cs, P.lw, B, M, s0 * kFcBlock, c->rs.L,
                                                                        c->rs.Tn, c->rs.set, slab);
}

extern "C" {

int smcn_residuals_set(smcn_ctx* c, int L, const double* q_at, int Tn) {
    RS_CHECK(c, "smcn_residuals_set");
    if (L < 0 || L > kRsMaxL) FAIL(c, "smcn_residuals_set: the number of lags L must be in 0..32");
    if ((int64_t)L > c->arma_T - 1)
        FAIL(c, "smcn_residuals_set: L = " + std::to_string(L) + " lags need a series of at least L + 1 values (T = " +
                    std::to_string(c->arma_T) + ")");
    if (Tn < 0 || Tn > kRsMaxAt) FAIL(c, "smcn_residuals_set: the number of thresholds of Q, Tn, must be in 0..8");
    if ((Tn > 0) != (q_at != nullptr)) FAIL(c, "smcn_residuals_set: `q_at` holds [Tn] thresholds (NULL with Tn = 0 only)");
    if (Tn > 0 && L == 0) FAIL(c, "smcn_residuals_set: thresholds of Q need L >= 1");
    if ((c->arma_T + L + 2) * kRsCols > ((int64_t)1 << 18))
        FAIL(c, "smcn_residuals_set: the series is too long: (T + L + 2) * 20 must not exceed 2^18 = 262144 (T + L <= 13105)");
    double h[kRsMaxAt] = {};
    for (int i = 0; i < Tn; ++i) {
        if (!std::isfinite(q_at[i])) FAIL(c, "smcn_residuals_set: q_at[" + std::to_string(i) + "] is not finite");
        h[i] = q_at[i];
    }
    c->rs.L = -1;
    const int rc = grow(c, c->rs.set, kRsMaxAt);
    if (rc) return rc;
    HIPC(c, stream_wait(c->stream));                             // (a kernel of an earlier call may still read the setting)
    HIPC(c, hipMemcpyAsync(c->rs.set, h, sizeof(h), hipMemcpyHostToDevice, c->stream));
    HIPC(c, stream_wait(c->stream));                             // (h is a local)
    c->rs.L = L;
    c->rs.Tn = Tn;
    return 0;
}

int smcn_residuals_dims(smcn_ctx* c, int64_t* T, int* L, int* Qc, int* Tn) {
    RS_CHECK(c, "smcn_residuals_dims");
    RS_CHECK_SET(c, "smcn_residuals_dims");
    if (T) *T = c->arma_T;
    if (L) *L = c->rs.L;
    if (Qc) *Qc = kRsCols;
    if (Tn) *Tn = c->rs.Tn;
    return 0;
}

int smcn_residuals_points(smcn_ctx* c, const double* x, int64_t M, double* out) {
    RS_CHECK(c, "smcn_residuals_points");
    RS_CHECK_SET(c, "smcn_residuals_points");
    if (!x || !out || M < 1) FAIL(c, "smcn_residuals_points: bad arguments");
    const int64_t W = 2 * c->arma_T + (c->rs.L > 0 ? c->rs.L + 1 : 0);
    if (fc_slices(M) > 2147483647LL) FAIL(c, "smcn_residuals_points: too many points");
    int rc = ensure_stage(c, M * c->D);
    if (rc) return rc;
    if ((rc = grow(c, c->rs.buf, M * W))) return rc;
    HIPC(c, hipMemcpyAsync(c->stage, x, sizeof(double) * M * c->D, hipMemcpyHostToDevice, c->stream));
    residuals_points_kernel<<<(int)fc_slices(M), kFcBlock, 0, c->stream>>>(c->mdata, c->stage, M, c->rs.L, c->rs.buf);
    HIPC(c, hipGetLastError());
    HIPC(c, hipMemcpyAsync(out, c->rs.buf, sizeof(double) * M * W, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, stream_wait(c->stream));
    return 0;
}

int smcn_residuals_partials(smcn_ctx* c, const double* x, const double* logw, int64_t M, double* out) {
    RS_CHECK(c, "smcn_residuals_partials");
    RS_CHECK_SET(c, "smcn_residuals_partials");
    if (!out || M < 1) FAIL(c, "smcn_residuals_partials: bad arguments");
    const int L = c->rs.L;
    const int64_t R = rs_rows(c), row = R * kRsCols;
    const int64_t slices = fc_slices(M), groups = (slices + kFcGroup - 1) / kFcGroup, win = rs_window(R);
    if (groups > 65535) FAIL(c, "smcn_residuals_partials: too many particles (M <= 268431360)");
    // rs.buf: [header 16 | lw M | slab (a window of slices) | group partials | result (1 + R) kRsCols]
    const int64_t o_lw = 16, o_slab = o_lw + (M + 15) / 16 * 16, o_grp = o_slab + (slices < win ? slices : win) * row;
    const int64_t o_out = o_grp + groups * row;
    int rc = grow(c, c->rs.buf, o_out + (1 + R) * kRsCols);
    if (rc) return rc;
    double* const B = c->rs.buf;
    Particles P;
    if ((rc = stage_particles(c, "smcn_residuals_partials", x, logw, M, B + o_lw, &P))) return rc;
    HIPC(c, c->rs.ev0.record(c->stream));
    launch_pointwise_header(c, P.lw, M, B);
    for (int64_t s0 = 0; s0 < slices; s0 += win) {
        const int64_t ns = slices - s0 < win ? slices - s0 : win, ng = (ns + kFcGroup - 1) / kFcGroup;
        if (L == 0) rs_launch<0>(c, P, B, M, s0, ns, B + o_slab);
        else if (L <= 16) rs_launch<16>(c, P, B, M, s0, ns, B + o_slab);
        else rs_launch<kRsMaxL>(c, P, B, M, s0, ns, B + o_slab);
        residuals_merge_kernel<false><<<dim3((unsigned)grid_for(row, 256), (unsigned)ng), 256, 0, c->stream>>>(
            B + o_slab, B, ns, (int)R, B + o_grp + s0 / kFcGroup * row);
    }
    residuals_merge_kernel<true><<<grid_for(row, 256), 256, 0, c->stream>>>(B + o_grp, B, groups, (int)R, B + o_out);
    HIPC(c, hipGetLastError());
    HIPC(c, c->rs.ev1.record(c->stream));
    HIPC(c, hipMemcpyAsync(out, B + o_out, sizeof(double) * (1 + R) * kRsCols, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, stream_wait(c->stream));
    HIPC(c, c->rs.ev1.since(c->rs.ev0, &c->rs.ms));
    return 0;
}

int smcn_residuals_last_ms(const smcn_ctx* c, double* ms) {
    if (!c || !ms) return -1;
    *ms = c->rs.ms;
    return 0;
}

}  // extern "C"
