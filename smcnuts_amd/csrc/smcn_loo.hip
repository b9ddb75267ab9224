// libsmcnuts_hip.so, the model-comparison unit: pointwise criteria (smcn_pointwise_*), calibration (smcn_calibration_*)
// and Pareto-smoothed LOO (smcn_psis_*).  Owns the kernels of smcn_pointwise.hpp, smcn_calibration.hpp and smcn_psis.hpp,
// and smcn_ctx's pw and ps.
#include "smcn_ctx.hpp"
#include "smcn_pointwise.hpp"
#include "smcn_calibration.hpp"
#include "smcn_psis.hpp"

// ---- pointwise log-likelihood and its reductions over particles (smcn_pointwise.hpp) ------------------------------------
void smcn_host::launch_pointwise_header(smcn_ctx* c, const double* lw, int64_t M, double* head) {
    pointwise_header_kernel<<<1, kRedBlock, 0, c->stream>>>(lw, M, head);
}
void smcn_host::launch_glm_loglik(smcn_ctx* c, const RegLayout& L, const PwArgs& a, int64_t tiles, int64_t blocks, double* out) {
    row_cap_glm(L, [&](auto dp, auto disp, auto ow) {
        pointwise_loglik_kernel<decltype(dp)::value, decltype(disp)::value, decltype(ow)::value>
            <<<(int)blocks, 64, 0, c->stream>>>(a, tiles, out);
    });
}

static const char* kPwScope =
    "pointwise criteria cover the SMCN_MODEL_GLM families (bernoulli_logit, poisson_log, normal, neg_binomial_2_log) "
    "only; hierarchical, categorical, ordinal, arma, PRMwCD, Gaussian and host-evaluated targets are not implemented";

static const char* kPwWeighted =
    "pointwise criteria and LOO of a fit with weights (SMCN_MODEL_OGLM, flags & 2) are not implemented: what a weighted "
    "row's leave-one-out term and the standard error of the sum should be is not settled here";
// "" or why the pointwise entry points do not serve this context
static std::string pw_refusal(const smcn_ctx* c) {
    if (c->model == SMCN_MODEL_OGLM) return (c->reg.flags & 2) ? kPwWeighted : "";
    return c->model == SMCN_MODEL_GLM ? "" : kPwScope;
}

extern "C" {

int smcn_pointwise_dims(const smcn_ctx* cc, int64_t* n_obs, int* n_cols) {
    smcn_ctx* c = const_cast<smcn_ctx*>(cc);
    if (!c) return -1;
    if (!pw_refusal(c).empty()) FAIL(c, "smcn_pointwise_dims: " + pw_refusal(c));
    if (n_obs) *n_obs = c->reg.n;
    if (n_cols) *n_cols = kPwCols;
    return 0;
}

int smcn_pointwise_loglik(smcn_ctx* c, const double* x, int64_t M, double* out) {
    CHECK_CTX(c);
    if (!pw_refusal(c).empty()) FAIL(c, "smcn_pointwise_loglik: " + pw_refusal(c));
    if (!x || !out || M < 1) FAIL(c, "smcn_pointwise_loglik: bad arguments");
    const int64_t n = c->reg.n, tiles = (n + 63) / 64;
    int64_t cps = 1;
    const int64_t slices = pointwise_slices(M, n, &cps);
    if (tiles * slices > 2147483647LL) FAIL(c, "smcn_pointwise_loglik: too many observations");
    int rc = ensure_stage(c, M * c->D);
    if (rc) return rc;
    if ((rc = grow(c, c->pw.buf, M * n))) return rc;
    HIPC(c, hipMemcpyAsync(c->stage, x, sizeof(double) * M * c->D, hipMemcpyHostToDevice, c->stream));
    const PwArgs a = pw_args(c->reg, c->mdata, c->stage, c->D, 1, M, cps);
    launch_glm_loglik(c, c->reg, a, tiles, tiles * slices, c->pw.buf);
    HIPC(c, hipGetLastError());
    HIPC(c, hipMemcpyAsync(out, c->pw.buf, sizeof(double) * M * n, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, stream_wait(c->stream));
    return 0;
}

int smcn_pointwise_partials(smcn_ctx* c, const double* x, const double* logw, int64_t M, double* out) {
    CHECK_CTX(c);
    if (!pw_refusal(c).empty()) FAIL(c, "smcn_pointwise_partials: " + pw_refusal(c));
    if (!out || M < 1) FAIL(c, "smcn_pointwise_partials: bad arguments");
    const int64_t n = c->reg.n, tiles = (n + 63) / 64, npad = tiles * 64;
    int64_t cps = 1;
    const int64_t slices = pointwise_slices(M, n, &cps);
    if (tiles * slices > 2147483647LL) FAIL(c, "smcn_pointwise_partials: too many observations");
    // pw.buf: [header 16 | lw M | slice partials | group partials | result (1 + n) Q]
    const int64_t groups = (slices + kPwGroup - 1) / kPwGroup;
    const int64_t o_lw = 16, o_part = o_lw + (M + 15) / 16 * 16, o_grp = o_part + slices * kPwCols * npad;
    const int64_t o_out = o_grp + groups * kPwCols * npad;
    int rc = grow(c, c->pw.buf, o_out + (1 + n) * kPwCols);
    if (rc) return rc;
    double* const head = c->pw.buf;
    double* const part = c->pw.buf + o_part;
    double* const grp = c->pw.buf + o_grp;
    double* const res = c->pw.buf + o_out;
    Particles P;
    if ((rc = stage_particles(c, "smcn_pointwise_partials", x, logw, M, c->pw.buf + o_lw, &P))) return rc;
    const double* const lw = P.lw;
    const PwArgs a = pw_args(c->reg, c->mdata, P.xd, P.rs, P.cs, M, cps);
    HIPC(c, c->pw.ev0.record(c->stream));
    launch_pointwise_header(c, lw, M, head);
    row_cap_glm(c->reg, [&](auto dp, auto disp, auto ow) {
        pointwise_stats_kernel<decltype(dp)::value, decltype(disp)::value, decltype(ow)::value>
            <<<(int)(tiles * slices), 64, 0, c->stream>>>(a, tiles, lw, head, part);
    });
    // (groups <= 256 blocks in y: pointwise_slices keeps the slices near 4096)
    pointwise_combine_kernel<false><<<dim3((unsigned)grid_for(n, 64), (unsigned)groups), 64, 0, c->stream>>>(part, head, slices, n, npad, grp);
    pointwise_combine_kernel<true><<<grid_for(n, 64), 64, 0, c->stream>>>(grp, head, groups, n, npad, res);
    HIPC(c, hipGetLastError());
    HIPC(c, c->pw.ev1.record(c->stream));
    HIPC(c, hipMemcpyAsync(out, res, sizeof(double) * (1 + n) * kPwCols, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, stream_wait(c->stream));
    HIPC(c, c->pw.ev1.since(c->pw.ev0, &c->pw.ms));
    return 0;
}

int smcn_pointwise_last_ms(const smcn_ctx* c, double* ms) {
    if (!c || !ms) return -1;
    *ms = c->pw.ms;
    return 0;
}

// ---- calibration: the predictive tails at the observations and their sums over particles (smcn_calibration.hpp) ---------
int smcn_calibration_dims(const smcn_ctx* cc, int64_t* n_obs, int* n_cols) {
    smcn_ctx* c = const_cast<smcn_ctx*>(cc);
    if (!c) return -1;
    if (!pw_refusal(c).empty()) FAIL(c, "smcn_calibration_dims: " + pw_refusal(c));
    if (n_obs) *n_obs = c->reg.n;
    if (n_cols) *n_cols = kCalCols;
    return 0;
}

int smcn_calibration_points(smcn_ctx* c, const double* x, int64_t M, double* out) {
    CHECK_CTX(c);
    if (!pw_refusal(c).empty()) FAIL(c, "smcn_calibration_points: " + pw_refusal(c));
    if (!x || !out || M < 1) FAIL(c, "smcn_calibration_points: bad arguments");
    const int64_t n = c->reg.n, tiles = (n + 63) / 64;
    int64_t cps = 1;
    const int64_t slices = pointwise_slices(M, n, &cps);
    if (tiles * slices > 2147483647LL) FAIL(c, "smcn_calibration_points: too many observations");
    int rc = ensure_stage(c, M * c->D);
    if (rc) return rc;
    if ((rc = grow(c, c->pw.buf, 2 * M * n))) return rc;
    HIPC(c, hipMemcpyAsync(c->stage, x, sizeof(double) * M * c->D, hipMemcpyHostToDevice, c->stream));
    const PwArgs a = pw_args(c->reg, c->mdata, c->stage, c->D, 1, M, cps);
    row_cap_glm(c->reg, [&](auto dp, auto disp, auto ow) {
        calibration_points_kernel<decltype(dp)::value, decltype(disp)::value, decltype(ow)::value>
            <<<(int)(tiles * slices), 64, 0, c->stream>>>(a, tiles, c->pw.buf);
    });
    HIPC(c, hipGetLastError());
    HIPC(c, hipMemcpyAsync(out, c->pw.buf, sizeof(double) * 2 * M * n, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, stream_wait(c->stream));
    return 0;
}

int smcn_calibration_partials(smcn_ctx* c, const double* x, const double* logw, int64_t M, double* out) {
    CHECK_CTX(c);
    if (!pw_refusal(c).empty()) FAIL(c, "smcn_calibration_partials: " + pw_refusal(c));
    if (!out || M < 1) FAIL(c, "smcn_calibration_partials: bad arguments");
    const int64_t n = c->reg.n, tiles = (n + 63) / 64, npad = tiles * 64;
    int64_t cps = 1;
    const int64_t slices = pointwise_slices(M, n, &cps);
    if (tiles * slices > 2147483647LL) FAIL(c, "smcn_calibration_partials: too many observations");
    // pw.buf: [header 16 | lw M | slice partials | group partials | result (1 + n) Qc]
    const int64_t groups = (slices + kPwGroup - 1) / kPwGroup;
    const int64_t o_lw = 16, o_part = o_lw + (M + 15) / 16 * 16, o_grp = o_part + slices * kCalCols * npad;
    const int64_t o_out = o_grp + groups * kCalCols * npad;
    int rc = grow(c, c->pw.buf, o_out + (1 + n) * kCalCols);
    if (rc) return rc;
    double* const head = c->pw.buf;
    double* const part = c->pw.buf + o_part;
    double* const grp = c->pw.buf + o_grp;
    double* const res = c->pw.buf + o_out;
    Particles P;
    if ((rc = stage_particles(c, "smcn_calibration_partials", x, logw, M, c->pw.buf + o_lw, &P))) return rc;
    const double* const lw = P.lw;
    const PwArgs a = pw_args(c->reg, c->mdata, P.xd, P.rs, P.cs, M, cps);
    HIPC(c, c->pw.ev0.record(c->stream));
    launch_pointwise_header(c, lw, M, head);
    row_cap_glm(c->reg, [&](auto dp, auto disp, auto ow) {
        calibration_stats_kernel<decltype(dp)::value, decltype(disp)::value, decltype(ow)::value>
            <<<(int)(tiles * slices), 64, 0, c->stream>>>(a, tiles, lw, head, part);
    });
    calibration_combine_kernel<false><<<dim3((unsigned)grid_for(n, 64), (unsigned)groups), 64, 0, c->stream>>>(part, head, slices, n, npad, grp);
    calibration_combine_kernel<true><<<grid_for(n, 64), 64, 0, c->stream>>>(grp, head, groups, n, npad, res);
    HIPC(c, hipGetLastError());
    HIPC(c, c->pw.ev1.record(c->stream));
    HIPC(c, hipMemcpyAsync(out, res, sizeof(double) * (1 + n) * kCalCols, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, stream_wait(c->stream));
    HIPC(c, c->pw.ev1.since(c->pw.ev0, &c->pw.cal_ms));
    return 0;
}

int smcn_calibration_last_ms(const smcn_ctx* c, double* ms) {
    if (!c || !ms) return -1;
    *ms = c->pw.cal_ms;
    return 0;
}

}  // extern "C"
// ---- Pareto-smoothed importance-sampling LOO (smcn_psis.hpp) ---------------------------------------------------------------
namespace {
// ps.buf of a call over particles: [header 16 | lw | slab of ll | candidates lr, ll [n][stride] | cutoff npad | slice
// partials | group partials | body [n][4] | out [n][6]]
struct PsLayout {
    int64_t n, tiles, npad, M, Mpad, cps, slices, groups, slab_tiles, stride;
    int64_t o_lw, o_stage, o_clr, o_cll, o_cut, o_part, o_grp, o_body, o_out, total;
};
constexpr int64_t kPsSlab = 1ll << 25;     // doubles of ll staged at once (256 MB), one observation tile at the least
}  // namespace

static int ps_layout(smcn_ctx* c, const char* who, int64_t M, int64_t S_bound, PsLayout* L) {
    if (!pw_refusal(c).empty()) FAIL(c, std::string(who) + ": " + pw_refusal(c));
    if (M < 1 || M > 2147483647LL) FAIL(c, std::string(who) + ": bad arguments");
    if (S_bound < 1) FAIL(c, std::string(who) + ": no contributing particle (S < 1)");
    L->stride = psis_tail_len(S_bound) + 1;
    if (L->stride > kPsMaxCap)
        FAIL(c, std::string(who) + ": the tail of " + std::to_string(L->stride - 1) + " candidates per observation exceeds " +
                    std::to_string(kPsMaxCap - 1) + " (more than 1863225 contributing particles are not implemented)");
    L->n = c->reg.n;
    L->tiles = (L->n + 63) / 64;
    L->npad = L->tiles * 64;
    L->M = M;
    L->Mpad = (M + 63) / 64 * 64;
    L->slices = pointwise_slices(M, L->n, &L->cps);
    L->groups = (L->slices + kPwGroup - 1) / kPwGroup;
    int64_t st = kPsSlab / (64 * L->Mpad);
    st = st < 1 ? 1 : (st > L->tiles ? L->tiles : st);
    while (st > 1 && st * L->slices > 2147483647LL) --st;
    L->slab_tiles = st;
    if (L->tiles * L->slices > 2147483647LL) FAIL(c, std::string(who) + ": too many observations");
    L->o_lw = 16;
    L->o_stage = L->o_lw + L->Mpad;
    L->o_clr = L->o_stage + st * 64 * L->Mpad;
    L->o_cll = L->o_clr + L->n * L->stride;
    L->o_cut = L->o_cll + L->n * L->stride;
    L->o_part = L->o_cut + L->npad;
    L->o_grp = L->o_part + L->slices * kPsBodyCols * L->npad;
    L->o_body = L->o_grp + L->groups * kPsBodyCols * L->npad;
    L->o_out = L->o_body + L->n * kPsBodyCols;
    L->total = L->o_out + L->n * kPsOutCols;
    return grow(c, c->ps.buf, L->total);
}
// header of a staged call from the caller's (mw, S)
static int ps_put_head(smcn_ctx* c, double mw, int64_t S) {
    const double h[16] = {mw, 0.0, 0.0, (double)S};
    HIPC(c, hipMemcpyAsync(c->ps.buf, h, sizeof(h), hipMemcpyHostToDevice, c->stream));
    HIPC(c, stream_wait(c->stream));      // (h is a local)
    return 0;
}
static void ps_run_candidates(smcn_ctx* c, const PsLayout& L, const PwArgs& a, const double* lw) {
    double* const B = c->ps.buf;
    for (int64_t t0 = 0; t0 < L.tiles; t0 += L.slab_tiles) {
        const int64_t nt = L.tiles - t0 < L.slab_tiles ? L.tiles - t0 : L.slab_tiles;
        row_cap_glm(c->reg, [&](auto dp, auto disp, auto ow) {
            psis_stage_kernel<decltype(dp)::value, decltype(disp)::value, decltype(ow)::value>
                <<<(int)(nt * L.slices), 64, 0, c->stream>>>(a, t0, nt, lw, B, L.Mpad, B + L.o_stage);
        });
        psis_select_kernel<<<(int)(nt * 64), kPsBlock, 0, c->stream>>>(B + L.o_stage, L.Mpad, lw, B, L.M, t0 * 64, L.n,
                                                                       (int)L.stride, B + L.o_clr, B + L.o_cll, B + L.o_cut);
    }
}
static void ps_run_body(smcn_ctx* c, const PsLayout& L, const PwArgs& a, const double* lw) {
    double* const B = c->ps.buf;
    row_cap_glm(c->reg, [&](auto dp, auto disp, auto ow) {
        psis_body_kernel<decltype(dp)::value, decltype(disp)::value, decltype(ow)::value>
            <<<(int)(L.tiles * L.slices), 64, 0, c->stream>>>(a, L.tiles, lw, B, B + L.o_cut, B + L.o_part);
    });
    psis_body_combine_kernel<false><<<dim3((unsigned)grid_for(L.n, 64), (unsigned)L.groups), 64, 0, c->stream>>>(
        B + L.o_part, L.slices, L.n, L.npad, B + L.o_grp);
    psis_body_combine_kernel<true><<<grid_for(L.n, 64), 64, 0, c->stream>>>(B + L.o_grp, L.groups, L.n, L.npad, B + L.o_body);
}
static int ps_elapsed(smcn_ctx* c, int slot, int e0, int e1) {
    HIPC(c, c->ps.ev[e1].since(c->ps.ev[e0], &c->ps.ms[slot]));
    return 0;
}

extern "C" {

int smcn_psis_candidates(smcn_ctx* c, const double* x, const double* logw, int64_t M, double mw, int64_t S, double* cand) {
    CHECK_CTX(c);
    if (!cand) FAIL(c, "smcn_psis_candidates: bad arguments");
    PsLayout L;
    int rc = ps_layout(c, "smcn_psis_candidates", M, S, &L);
    if (rc || (rc = ps_put_head(c, mw, S))) return rc;
    Particles P;
    if ((rc = stage_particles(c, "smcn_psis_candidates", x, logw, M, c->ps.buf + L.o_lw, &P))) return rc;
    const PwArgs a = pw_args(c->reg, c->mdata, P.xd, P.rs, P.cs, M, L.cps);
    HIPC(c, c->ps.ev[0].record(c->stream));
    ps_run_candidates(c, L, a, P.lw);
    HIPC(c, hipGetLastError());
    HIPC(c, c->ps.ev[1].record(c->stream));
    HIPC(c, hipMemcpyAsync(cand, c->ps.buf + L.o_clr, sizeof(double) * 2 * L.n * L.stride, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, stream_wait(c->stream));
    return ps_elapsed(c, 0, 0, 1);
}

int smcn_psis_body(smcn_ctx* c, const double* x, const double* logw, int64_t M, double mw, int64_t S, const double* cutoff,
                   double* body) {
    CHECK_CTX(c);
    if (!cutoff || !body) FAIL(c, "smcn_psis_body: bad arguments");
    PsLayout L;
    int rc = ps_layout(c, "smcn_psis_body", M, S, &L);
    if (rc || (rc = ps_put_head(c, mw, S))) return rc;
    Particles P;
    if ((rc = stage_particles(c, "smcn_psis_body", x, logw, M, c->ps.buf + L.o_lw, &P))) return rc;
    HIPC(c, hipMemcpyAsync(c->ps.buf + L.o_cut, cutoff, sizeof(double) * L.n, hipMemcpyHostToDevice, c->stream));
    const PwArgs a = pw_args(c->reg, c->mdata, P.xd, P.rs, P.cs, M, L.cps);
    HIPC(c, c->ps.ev[0].record(c->stream));
    ps_run_body(c, L, a, P.lw);
    HIPC(c, hipGetLastError());
    HIPC(c, c->ps.ev[1].record(c->stream));
    HIPC(c, hipMemcpyAsync(body, c->ps.buf + L.o_body, sizeof(double) * L.n * kPsBodyCols, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, stream_wait(c->stream));
    return ps_elapsed(c, 1, 0, 1);
}

int smcn_psis_fit(smcn_ctx* c, const double* cand, const double* body, int64_t n_obs, double mw, int64_t S, double* out) {
    CHECK_CTX(c);
    if (!cand || !body || !out || n_obs < 1 || n_obs > 2147483647LL) FAIL(c, "smcn_psis_fit: bad arguments");
    if (S < 1) FAIL(c, "smcn_psis_fit: no contributing particle (S < 1)");
    const int64_t stride = psis_tail_len(S) + 1;
    if (stride > kPsMaxTail + 1)
        FAIL(c, "smcn_psis_fit: the tail of " + std::to_string(stride - 1) + " candidates per observation exceeds " +
                    std::to_string(kPsMaxTail));
    // ps.buf: [header 16 | candidates lr, ll [n][stride] | body [n][4] | out [n][6]]
    const int64_t o_c = 16, o_b = o_c + 2 * n_obs * stride, o_o = o_b + n_obs * kPsBodyCols;
    int rc = grow(c, c->ps.buf, o_o + n_obs * kPsOutCols);
    if (rc || (rc = ps_put_head(c, mw, S))) return rc;
    double* const B = c->ps.buf;
    HIPC(c, hipMemcpyAsync(B + o_c, cand, sizeof(double) * 2 * n_obs * stride, hipMemcpyHostToDevice, c->stream));
    HIPC(c, hipMemcpyAsync(B + o_b, body, sizeof(double) * n_obs * kPsBodyCols, hipMemcpyHostToDevice, c->stream));
    HIPC(c, c->ps.ev[0].record(c->stream));
    psis_fit_kernel<<<(int)n_obs, kPsBlock, 0, c->stream>>>(B + o_c, B + o_c + n_obs * stride, B + o_b, B, (int)stride, B + o_o);
    HIPC(c, hipGetLastError());
    HIPC(c, c->ps.ev[1].record(c->stream));
    HIPC(c, hipMemcpyAsync(out, B + o_o, sizeof(double) * n_obs * kPsOutCols, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, stream_wait(c->stream));
    return ps_elapsed(c, 2, 0, 1);
}

int smcn_psis_loo(smcn_ctx* c, const double* x, const double* logw, int64_t M, double* out, double* head_out) {
    CHECK_CTX(c);
    if (!out) FAIL(c, "smcn_psis_loo: bad arguments");
    // S <= M is known on the device only: the candidate rows are laid out for S = M, the kernels read S from the header
    PsLayout L;
    int rc = ps_layout(c, "smcn_psis_loo", M, M, &L);
    if (rc) return rc;
    Particles P;
    if ((rc = stage_particles(c, "smcn_psis_loo", x, logw, M, c->ps.buf + L.o_lw, &P))) return rc;
    const PwArgs a = pw_args(c->reg, c->mdata, P.xd, P.rs, P.cs, M, L.cps);
    double* const B = c->ps.buf;
    HIPC(c, c->ps.ev[0].record(c->stream));
    launch_pointwise_header(c, P.lw, M, B);
    ps_run_candidates(c, L, a, P.lw);
    HIPC(c, c->ps.ev[1].record(c->stream));
    ps_run_body(c, L, a, P.lw);
    HIPC(c, c->ps.ev[2].record(c->stream));
    psis_fit_kernel<<<(int)L.n, kPsBlock, 0, c->stream>>>(B + L.o_clr, B + L.o_cll, B + L.o_body, B, (int)L.stride, B + L.o_out);
    HIPC(c, hipGetLastError());
    HIPC(c, c->ps.ev[3].record(c->stream));
    HIPC(c, hipMemcpyAsync(out, B + L.o_out, sizeof(double) * L.n * kPsOutCols, hipMemcpyDeviceToHost, c->stream));
    if (head_out) HIPC(c, hipMemcpyAsync(head_out, B, sizeof(double) * 4, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, stream_wait(c->stream));
    if ((rc = ps_elapsed(c, 0, 0, 1)) || (rc = ps_elapsed(c, 1, 1, 2)) || (rc = ps_elapsed(c, 2, 2, 3))) return rc;
    return ps_elapsed(c, 3, 0, 3);
}

int smcn_psis_last_ms(const smcn_ctx* c, double* ms) {
    if (!c || !ms) return -1;
    for (int k = 0; k < 4; ++k) ms[k] = c->ps.ms[k];
    return 0;
}

}  // extern "C"
