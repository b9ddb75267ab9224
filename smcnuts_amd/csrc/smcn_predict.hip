// libsmcnuts_hip.so, the prediction unit: held-out prediction at new rows (smcn_predict_*) and posterior predictive draws
// (smcn_predict_draws).  Owns the kernels of smcn_predict.hpp and smcn_predict_draws.hpp, and smcn_ctx's pr and dr.
#include "smcn_ctx.hpp"
#include "smcn_predict.hpp"
#include "smcn_predict_draws.hpp"

// ---- held-out prediction at new rows (smcn_predict.hpp) ----------------------------------------------------------------
static const char* kPrScope =
    "held-out prediction covers the regression targets (SMCN_MODEL_GLM, SMCN_MODEL_OGLM, SMCN_MODEL_HGLM, "
    "SMCN_MODEL_CATEGORICAL, SMCN_MODEL_ORDINAL); arma, PRMwCD, Gaussian and host-evaluated targets are not supported";
static bool pr_model(const smcn_ctx* c) {
    return c->model == SMCN_MODEL_GLM || c->model == SMCN_MODEL_OGLM || c->model == SMCN_MODEL_HGLM ||
           c->model == SMCN_MODEL_CATEGORICAL || c->model == SMCN_MODEL_ORDINAL;
}
static int pr_cols(const smcn_ctx* c) {
    const int K = c->reg.K;
    if (c->model == SMCN_MODEL_CATEGORICAL) return kPrCatP0 + K;
    if (c->model == SMCN_MODEL_ORDINAL) return kPrOrdP0 + (K <= kPrMaxProb ? K : 0);
    return kPrColsGlm;
}
// the arguments of the hierarchical, categorical and ordinal kernels over the new rows (c->pr.lay)
static PrArgs pr_args(const smcn_ctx* c, const double* x, int64_t rs, int64_t cs, int64_t M, int64_t cps) {
    PrArgs a;
    a.T = c->pr.md + c->pr.lay.t0;
    a.x = x;
    a.rs = rs;
    a.cs = cs;
    a.M = M;
    a.cps = cps;
    a.m = (int)c->pr.lay.n;
    a.D = c->D;
    a.fam = c->reg.fam;
    a.J = (int)c->reg.J;
    a.K = c->reg.K;
    a.Dc = c->reg.Dc;
    return a;
}
// categorical: f(row capacity, non-reference classes), the pairs that cover (K - 1) Dc <= 64
template <class F>
static void cat_cap(int Dc, F&& f) {
    using std::integral_constant;
    if (Dc <= 4) f(integral_constant<int, 4>{}, integral_constant<int, 15>{});
    else if (Dc <= 8) f(integral_constant<int, 8>{}, integral_constant<int, 12>{});
    else if (Dc <= 16) f(integral_constant<int, 16>{}, integral_constant<int, 7>{});
    else if (Dc <= 32) f(integral_constant<int, 32>{}, integral_constant<int, 3>{});
    else f(integral_constant<int, 64>{}, integral_constant<int, 1>{});
}
// Dynamic LDS of one wavefront's area V[r][64 particles] (smcn_predict.hpp): J rows (hierarchical), D (categorical),
// 2 (K - 1) or, with the class probabilities, 3 (K - 1) (ordinal); none for the GLM families.  The largest a model's
// limits allow is the ordinal model at p = 0, K = 65: 128 rows = kPrMaxLdsBytes exactly, what a launch may ask for
// without hipFuncSetAttribute.
constexpr size_t kPrMaxLdsBytes = 64 * 1024;
static size_t pr_lds_bytes(const smcn_ctx* c, bool stats) {
    const RegLayout& L = c->reg;
    size_t rows = 0;
    if (c->model == SMCN_MODEL_HGLM) rows = (size_t)L.J;
    else if (c->model == SMCN_MODEL_ORDINAL) rows = (size_t)(L.K - 1) * ((stats && L.K <= kPrMaxProb) ? 3 : 2);
    else if (c->model == SMCN_MODEL_CATEGORICAL) rows = (size_t)L.D;
    return sizeof(double) * 64 * rows;
}
#define PR_CHECK_LDS(c, stats, who)                                                                                     \
    if (pr_lds_bytes(c, stats) > kPrMaxLdsBytes)                                                                        \
        FAIL(c, std::string(who) + ": the model's per-wavefront LDS area (" + std::to_string(pr_lds_bytes(c, stats)) +  \
                    " B) is above the 65536 B a launch may ask for")
// Launches the model's matrix (STATS = false: out [M][m]) or statistics kernel over `blocks` wavefronts
template <bool STATS>
static void pr_launch(smcn_ctx* c, const double* x, int64_t rs, int64_t cs, int64_t M, int64_t cps, int64_t tiles,
                      int64_t blocks, const double* lw, const double* head, double* out) {
    const int g = (int)blocks;
    hipStream_t st = c->stream;
    if (c->model == SMCN_MODEL_GLM || c->model == SMCN_MODEL_OGLM) {
        const PwArgs a = pw_args(c->pr.lay, c->pr.md, x, rs, cs, M, cps);
        if constexpr (STATS) {
            row_cap_glm(c->pr.lay, [&](auto dp, auto disp, auto ow) {
                predict_glm_stats_kernel<decltype(dp)::value, decltype(disp)::value, decltype(ow)::value>
                    <<<g, 64, 0, st>>>(a, tiles, lw, head, out);
            });
        } else {
            launch_glm_loglik(c, c->pr.lay, a, tiles, blocks, out);     // (pointwise_loglik_kernel: smcn_loo.hip's)
        }
        return;
    }
    const PrArgs a = pr_args(c, x, rs, cs, M, cps);
    const size_t lds = pr_lds_bytes(c, STATS);
    if (c->model == SMCN_MODEL_HGLM) {
        row_cap_disp(a.Dc, a.fam, [&](auto dp, auto disp) {
            constexpr int DPM = decltype(dp)::value;
            constexpr bool DI = decltype(disp)::value;
            if constexpr (STATS) predict_hier_stats_kernel<DPM, DI><<<g, 64, lds, st>>>(a, tiles, lw, head, out);
            else predict_hier_loglik_kernel<DPM, DI><<<g, 64, lds, st>>>(a, tiles, out);
        });
    } else if (c->model == SMCN_MODEL_ORDINAL) {
        const bool prob = a.K <= kPrMaxProb;
        row_cap(a.Dc, [&](auto dp) {
            constexpr int DPM = decltype(dp)::value;
            if constexpr (STATS) {
                if (prob) predict_ord_stats_kernel<DPM, true><<<g, 64, lds, st>>>(a, tiles, lw, head, out);
                else predict_ord_stats_kernel<DPM, false><<<g, 64, lds, st>>>(a, tiles, lw, head, out);
            } else {
                predict_ord_loglik_kernel<DPM><<<g, 64, lds, st>>>(a, tiles, out);
            }
        });
    } else {
        cat_cap(a.Dc, [&](auto dc, auto km) {
            constexpr int DCM = decltype(dc)::value, KM = decltype(km)::value;
            if constexpr (STATS) predict_cat_stats_kernel<DCM, KM><<<g, 64, lds, st>>>(a, tiles, lw, head, out);
            else predict_cat_loglik_kernel<DCM, KM><<<g, 64, lds, st>>>(a, tiles, out);
        });
    }
}

extern "C" {

int smcn_predict_set_data(smcn_ctx* c, const double* block, int64_t len, int has_y) {
    CHECK_CTX(c);
    if (!pr_model(c)) FAIL(c, std::string("smcn_predict_set_data: ") + kPrScope);
    // the priors of the training block spliced in: the block smcn_ctx_create would take, checked by the same routine
    std::vector<double> full, mup;
    std::string why = reg_splice(c->reg, c->mdata_h.data(), block, len, full);
    if (!why.empty()) FAIL(c, why);
    RegLayout L;
    why = reg_check(c->model, full.data(), (int64_t)full.size(), &L);
    if (!why.empty()) FAIL(c, "smcn_predict_set_data (new rows, with the training priors spliced in): " + why);
    if (L.D != c->D) FAIL(c, "smcn_predict_set_data: the new rows give another dimension than the training data");
    reg_repack(L, full.data(), mup);
    c->pr.lay.n = 0;
    const int rc = grow(c, c->pr.md, L.rlen);
    if (rc) return rc;
    HIPC(c, hipMemcpyAsync(c->pr.md, mup.data(), sizeof(double) * L.rlen, hipMemcpyHostToDevice, c->stream));
    HIPC(c, stream_wait(c->stream));                             // (mup is a local)
    c->pr.lay = L;
    c->pr.has_y = has_y ? 1 : 0;
    return 0;
}

int smcn_predict_dims(smcn_ctx* c, int64_t* n_rows, int* n_cols, int* has_y) {
    CHECK_CTX(c);
    if (!pr_model(c)) FAIL(c, std::string("smcn_predict_dims: ") + kPrScope);
    if (c->pr.lay.n < 1) FAIL(c, "smcn_predict_dims: no new rows (smcn_predict_set_data first)");
    if (n_rows) *n_rows = c->pr.lay.n;
    if (n_cols) *n_cols = pr_cols(c);
    if (has_y) *has_y = c->pr.has_y;
    return 0;
}

int smcn_predict_loglik(smcn_ctx* c, const double* x, int64_t M, double* out) {
    CHECK_CTX(c);
    if (!pr_model(c)) FAIL(c, std::string("smcn_predict_loglik: ") + kPrScope);
    if (c->pr.lay.n < 1) FAIL(c, "smcn_predict_loglik: no new rows (smcn_predict_set_data first)");
    if (!c->pr.has_y) FAIL(c, "smcn_predict_loglik: the new rows were given without y");
    if (!x || !out || M < 1) FAIL(c, "smcn_predict_loglik: bad arguments");
    PR_CHECK_LDS(c, false, "smcn_predict_loglik");
    const int64_t m = c->pr.lay.n, tiles = (m + 63) / 64;
    int64_t cps = 1;
    const int64_t slices = pointwise_slices(M, m, &cps);
    if (tiles * slices > 2147483647LL) FAIL(c, "smcn_predict_loglik: too many rows");
    int rc = ensure_stage(c, M * c->D);
    if (rc) return rc;
    if ((rc = grow(c, c->pw.buf, M * m))) return rc;
    HIPC(c, hipMemcpyAsync(c->stage, x, sizeof(double) * M * c->D, hipMemcpyHostToDevice, c->stream));
    pr_launch<false>(c, c->stage, c->D, 1, M, cps, tiles, tiles * slices, nullptr, nullptr, c->pw.buf);
    HIPC(c, hipGetLastError());
    HIPC(c, hipMemcpyAsync(out, c->pw.buf, sizeof(double) * M * m, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, stream_wait(c->stream));
    return 0;
}

int smcn_predict_partials(smcn_ctx* c, const double* x, const double* logw, int64_t M, double* out) {
    CHECK_CTX(c);
    if (!pr_model(c)) FAIL(c, std::string("smcn_predict_partials: ") + kPrScope);
    if (c->pr.lay.n < 1) FAIL(c, "smcn_predict_partials: no new rows (smcn_predict_set_data first)");
    if (!out || M < 1) FAIL(c, "smcn_predict_partials: bad arguments");
    PR_CHECK_LDS(c, true, "smcn_predict_partials");
    const int64_t m = c->pr.lay.n, tiles = (m + 63) / 64, mpad = tiles * 64;
    const int Q = pr_cols(c), mom = (c->model == SMCN_MODEL_GLM || c->model == SMCN_MODEL_OGLM || c->model == SMCN_MODEL_HGLM) ? 1 : 0;
    int64_t cps = 1;
    const int64_t slices = pointwise_slices(M, m, &cps);
    if (tiles * slices > 2147483647LL) FAIL(c, "smcn_predict_partials: too many rows");
    // pw.buf: [header 16 | lw M | slice partials | group partials | result (1 + m) Q]
    const int64_t groups = (slices + kPwGroup - 1) / kPwGroup;
    const int64_t o_lw = 16, o_part = o_lw + (M + 15) / 16 * 16, o_grp = o_part + slices * Q * mpad;
    const int64_t o_out = o_grp + groups * Q * mpad;
    int rc = grow(c, c->pw.buf, o_out + (1 + m) * Q);
    if (rc) return rc;
    double* const head = c->pw.buf;
    double* const part = c->pw.buf + o_part;
    double* const grp = c->pw.buf + o_grp;
    double* const res = c->pw.buf + o_out;
    Particles P;
    if ((rc = stage_particles(c, "smcn_predict_partials", x, logw, M, c->pw.buf + o_lw, &P))) return rc;
    const double* const lw = P.lw;
    HIPC(c, c->pw.ev0.record(c->stream));
    launch_pointwise_header(c, lw, M, head);
    pr_launch<true>(c, P.xd, P.rs, P.cs, M, cps, tiles, tiles * slices, lw, head, part);
    predict_combine_kernel<false><<<dim3((unsigned)grid_for(m, 64), (unsigned)groups), 64, 0, c->stream>>>(part, head, slices, m, mpad, Q, mom, grp);
    predict_combine_kernel<true><<<grid_for(m, 64), 64, 0, c->stream>>>(grp, head, groups, m, mpad, Q, mom, res);
    HIPC(c, hipGetLastError());
    HIPC(c, c->pw.ev1.record(c->stream));
    HIPC(c, hipMemcpyAsync(out, res, sizeof(double) * (1 + m) * Q, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, stream_wait(c->stream));
    HIPC(c, c->pw.ev1.since(c->pw.ev0, &c->pr.ms));
    return 0;
}

int smcn_predict_last_ms(const smcn_ctx* c, double* ms) {
    if (!c || !ms) return -1;
    *ms = c->pr.ms;
    return 0;
}

}  // extern "C"
// ---- posterior predictive draws (smcn_predict_draws.hpp) ---------------------------------------------------------------
// Which (model, row capacity) instantiations sample inside the walk; the others store the law's mean and
// draws_sample_kernel samples it (Posterior predictive draws: the register counts behind the choice)
template <int DPMAX, bool DISP>
constexpr bool kDrawsFusedGlm = DPMAX <= 16;
template <int DPMAX, bool DISP>
constexpr bool kDrawsFusedHier = DPMAX <= 16;

// Launches the model's draw kernel over the n gathered particles xg [D][n] -> out [n][m]
static void dr_launch(smcn_ctx* c, const double* xg, int64_t n, const DrawArgs& d, double* out) {
    const int64_t m = c->pr.lay.n, tiles = (m + 63) / 64;
    int64_t cps = 1;
    const int64_t slices = pointwise_slices(n, m, &cps);
    const int g = (int)(tiles * slices);
    hipStream_t st = c->stream;
    const auto second = [&](int fam, bool disp, int tau_coord) {
        draws_sample_kernel<<<grid_for(n * m, 256), 256, 0, st>>>(fam, m, n, d, disp ? xg + (int64_t)tau_coord * n : nullptr, out);
    };
    if (c->model == SMCN_MODEL_GLM || c->model == SMCN_MODEL_OGLM) {
        const PwArgs a = pw_args(c->pr.lay, c->pr.md, xg, 1, n, n, cps);
        row_cap_glm(c->pr.lay, [&](auto dp, auto disp, auto ow) {
            constexpr int DP = decltype(dp)::value;
            constexpr bool DI = decltype(disp)::value;
            constexpr bool FU = kDrawsFusedGlm<DP, DI>;
            draws_glm_kernel<DP, DI, FU, decltype(ow)::value><<<g, 64, 0, st>>>(a, tiles, d, out);
            if (!FU) second(a.fam, DI, a.Dc);
        });
        return;
    }
    const PrArgs a = pr_args(c, xg, 1, n, n, cps);
    const size_t lds = pr_lds_bytes(c, false);
    if (c->model == SMCN_MODEL_HGLM) {
        row_cap_disp(a.Dc, a.fam, [&](auto dp, auto disp) {
            constexpr int DPM = decltype(dp)::value;
            constexpr bool DI = decltype(disp)::value;
            constexpr bool FU = kDrawsFusedHier<DPM, DI>;
            draws_hier_kernel<DPM, DI, FU><<<g, 64, lds, st>>>(a, tiles, d, out);
            if (!FU) second(a.fam, DI, a.Dc + a.J + 1);
        });
    } else if (c->model == SMCN_MODEL_ORDINAL) {
        row_cap(a.Dc, [&](auto dp) { draws_ord_kernel<decltype(dp)::value><<<g, 64, lds, st>>>(a, tiles, d, out); });
    } else {
        cat_cap(a.Dc, [&](auto dc, auto km) {
            draws_cat_kernel<decltype(dc)::value, decltype(km)::value><<<g, 64, lds, st>>>(a, tiles, d, out);
        });
    }
}

void smcn_host::launch_draw_ancestors(smcn_ctx* c, const double* lw, const double* head, int64_t M, int64_t S, int64_t s_first,
                                      int64_t n, uint64_t seed, uint32_t stream, double* w, double* local, double* ttot,
                                      double* toff, int64_t* anc) {
    const int nt = (int)((M + kScanTile - 1) / kScanTile);
    draws_weights_kernel<<<grid_for(M, 256), 256, 0, c->stream>>>(lw, head, M, w);
    launch_scan(c, w, M, nt, local, ttot, toff);
    draws_ancestors_kernel<<<grid_for(n, 256), 256, 0, c->stream>>>(local, toff, nt, M, lw, S, s_first, n, seed, stream, anc);
}

extern "C" {

int smcn_predict_draws(smcn_ctx* c, const double* x, const double* logw, int64_t M, int64_t S, uint64_t seed,
                       const int64_t* ancestors, const int64_t* new_group, int64_t s_first, int64_t s_count, double* y_out,
                       int64_t* ancestors_out, int64_t* n_bad_out) {
    CHECK_CTX(c);
    if (!pr_model(c)) FAIL(c, std::string("smcn_predict_draws: ") + kPrScope);
    if (c->pr.lay.n < 1) FAIL(c, "smcn_predict_draws: no new rows (smcn_predict_set_data first)");
    // (new_group is refused between y_out and the caller's ancestors: the plan's check runs without them first)
    std::string why = draw_refusal("smcn_predict_draws", "draws", M, S, s_first, s_count, y_out, nullptr);
    if (!why.empty()) FAIL(c, why);
    if (new_group && c->model != SMCN_MODEL_HGLM) FAIL(c, "smcn_predict_draws: new_group is for SMCN_MODEL_HGLM only");
    const int64_t m = c->pr.lay.n, tiles = (m + 63) / 64, n = s_count;
    if (new_group)
        for (int64_t i = 0; i < m; ++i)
            if (new_group[i] < 0 || new_group[i] > 4294967295LL)
                FAIL(c, "smcn_predict_draws: new_group[" + std::to_string(i) + "] is not a label in 0..2^32-1");
    why = draw_refusal("smcn_predict_draws", "draws", M, S, s_first, s_count, y_out, ancestors);
    if (!why.empty()) FAIL(c, why);
    PR_CHECK_LDS(c, false, "smcn_predict_draws");
    int64_t cps = 1;
    if (tiles * pointwise_slices(n, m, &cps) > 2147483647LL) FAIL(c, "smcn_predict_draws: too many rows");
    // dr.buf: [the plan's front | labels m | xg D n | y n m]
    const DrawPlan p(M, n, kScanTile);
    const int64_t o_ng = p.o_tail, o_xg = o_ng + p.pad(m), o_y = o_xg + p.pad(n * c->D);
    int rc = grow(c, c->dr.buf, o_y + n * m);
    if (rc) return rc;
    double* const B = c->dr.buf;
    const int64_t* const anc = (const int64_t*)(B + p.o_anc);
    int64_t* const ng = (int64_t*)(B + o_ng);
    Particles P;
    if ((rc = stage_particles(c, "smcn_predict_draws", x, logw, M, B + p.o_lw, &P))) return rc;
    if (new_group) HIPC(c, hipMemcpyAsync(ng, new_group, sizeof(int64_t) * m, hipMemcpyHostToDevice, c->stream));
    if ((rc = draw_ancestors(c, "smcn_predict_draws", c->pw.ev0, p, B, P.lw, M, S, s_first, n, seed, kStreamDrawAnc, ancestors, false)))
        return rc;
    draws_gather_kernel<<<grid_for(n, 256), 256, 0, c->stream>>>(P.xd, P.rs, P.cs, anc, n, c->D, B + o_xg);
    const DrawArgs d{seed, s_first, new_group ? ng : nullptr};
    dr_launch(c, B + o_xg, n, d, B + o_y);
    return draw_finish(c, "smcn_predict_draws", c->pw.ev0, c->pw.ev1, &c->dr.ms, ancestors ? nullptr : B + 3, anc, n, B + o_y, n * m,
                       y_out, ancestors_out, n_bad_out);
}

int smcn_predict_draws_last_ms(const smcn_ctx* c, double* ms) {
    if (!c || !ms) return -1;
    *ms = c->dr.ms;
    return 0;
}

}  // extern "C"
