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
    if (M < 1) FAIL(c, "smcn_predict_draws: M must be at least 1");
    if (S < 1 || S > 2147483647LL) FAIL(c, "smcn_predict_draws: the number of draws S must be in 1..2^31-1");
    if (s_first < 0 || s_count < 1 || s_first + s_count > S)
        FAIL(c, "smcn_predict_draws: the slot range [s_first, s_first + s_count) must be non-empty and lie in 0..S");
    if (!y_out) FAIL(c, "smcn_predict_draws: y_out is null");
    if (new_group && c->model != SMCN_MODEL_HGLM) FAIL(c, "smcn_predict_draws: new_group is for SMCN_MODEL_HGLM only");
    const int64_t m = c->pr.lay.n, tiles = (m + 63) / 64, n = s_count;
    if (new_group)
        for (int64_t i = 0; i < m; ++i)
            if (new_group[i] < 0 || new_group[i] > 4294967295LL)
                FAIL(c, "smcn_predict_draws: new_group[" + std::to_string(i) + "] is not a label in 0..2^32-1");
    if (ancestors)
        for (int64_t s = 0; s < S; ++s)
            if (ancestors[s] < 0 || ancestors[s] >= M)
                FAIL(c, "smcn_predict_draws: ancestors[" + std::to_string(s) + "] is not a particle in 0..M-1");
    PR_CHECK_LDS(c, false, "smcn_predict_draws");
    int64_t cps = 1;
    if (tiles * pointwise_slices(n, m, &cps) > 2147483647LL) FAIL(c, "smcn_predict_draws: too many rows");
    // dr.buf: [header 16 | lw M | w M | scan M | tile totals nt | tile offsets nt + 1 | ancestors n | labels m | xg D n | y n m]
    const int nt = (int)((M + kScanTile - 1) / kScanTile);
    const auto pad = [](int64_t v) { return (v + 15) / 16 * 16; };
    const int64_t o_lw = 16, o_w = o_lw + pad(M), o_loc = o_w + pad(M), o_tt = o_loc + pad(M), o_to = o_tt + pad(nt);
    const int64_t o_anc = o_to + pad(nt + 1), o_ng = o_anc + pad(n), o_xg = o_ng + pad(m), o_y = o_xg + pad(n * c->D);
    const int64_t need = o_y + n * m;
    int rc = grow(c, c->dr.buf, need);
    if (rc) return rc;
    double* const B = c->dr.buf;
    double* const head = B;
    int64_t* const anc = (int64_t*)(B + o_anc);
    int64_t* const ng = (int64_t*)(B + o_ng);
    Particles P;
    if ((rc = stage_particles(c, "smcn_predict_draws", x, logw, M, B + o_lw, &P))) return rc;
    const double* const lw = P.lw;
    if (new_group) HIPC(c, hipMemcpyAsync(ng, new_group, sizeof(int64_t) * m, hipMemcpyHostToDevice, c->stream));
    if (ancestors) HIPC(c, hipMemcpyAsync(anc, ancestors + s_first, sizeof(int64_t) * n, hipMemcpyHostToDevice, c->stream));
    HIPC(c, c->pw.ev0.record(c->stream));
    if (!ancestors) {
        launch_pointwise_header(c, lw, M, head);
        launch_draw_ancestors(c, lw, head, M, S, s_first, n, seed, kStreamDrawAnc, B + o_w, B + o_loc, B + o_tt, B + o_to, anc);
    }
    draws_gather_kernel<<<grid_for(n, 256), 256, 0, c->stream>>>(P.xd, P.rs, P.cs, anc, n, c->D, B + o_xg);
    const DrawArgs d{seed, s_first, new_group ? ng : nullptr};
    dr_launch(c, B + o_xg, n, d, B + o_y);
    HIPC(c, hipGetLastError());
    HIPC(c, c->pw.ev1.record(c->stream));
    double cnt = 1.0;
    if (!ancestors) HIPC(c, hipMemcpyAsync(&cnt, head + 3, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (ancestors_out) HIPC(c, hipMemcpyAsync(ancestors_out, anc, sizeof(int64_t) * n, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipMemcpyAsync(y_out, B + o_y, sizeof(double) * n * m, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, stream_wait(c->stream));
    HIPC(c, c->pw.ev1.since(c->pw.ev0, &c->dr.ms));
    if (cnt == 0.0) FAIL(c, "smcn_predict_draws: no particle has a finite log-weight");
    if (n_bad_out) {
        int64_t nb = 0;
        for (int64_t e = 0; e < n * m; ++e) nb += y_out[e] != y_out[e] ? 1 : 0;
        *n_bad_out = nb;
    }
    return 0;
}

int smcn_predict_draws_last_ms(const smcn_ctx* c, double* ms) {
    if (!c || !ms) return -1;
    *ms = c->dr.ms;
    return 0;
}

}  // extern "C"
