// The data block of a regression target (SMCN_MODEL_GLM, _HGLM, _CATEGORICAL, _ORDINAL, _MLGLM, _WGLM, _OGLM, _CGLM) on the host: where the
// header, the priors, y, g (and z) and X sit in the caller's block, which table the functors read behind it, the check
// of a caller's block and its repacking.  Plain C++17 with no HIP types: it compiles without a device compiler, so the code that
// indexes by caller-supplied lengths runs under the host sanitizers (tests/test_regdata_host.py).  The layout helpers
// are shared with the device functors (smcn_models.hpp), which find the table by the same arithmetic.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/smcnuts_hip.h"

#ifdef __HIPCC__
#define SMCN_HD __host__ __device__
#else
#define SMCN_HD
#endif

namespace smcn {

// GLM-type table: a row per observation at a 128-byte boundary behind the block, zero rows up to a multiple of 64
SMCN_HD inline int64_t glm_table_offset(int64_t D, int64_t n, int64_t p) {
    return (4 + D + n + n * p + 15) / 16 * 16;
}
SMCN_HD inline int glm_row_doubles(int D) { return ((D + 1) & ~1) + 2; }
SMCN_HD inline int64_t glm_table_rows(int64_t n) { return (n + 63) / 64 * 64; }
// GLM with offsets / weights (SMCN_MODEL_OGLM): five header slots; the table sits where it would for a block with both o
// and w, so that its place -- like everything else the functors read -- does not depend on the flags; a row carries o_i
// and w_i behind lgamma(y_i + 1)
SMCN_HD inline int64_t oglm_table_offset(int64_t npri, int64_t n, int64_t p) {
    return (5 + npri + 3 * n + n * p + 15) / 16 * 16;
}
SMCN_HD inline int oglm_row_doubles(int Dc) { return ((Dc + 1) & ~1) + 4; }
// continuous-response GLM (SMCN_MODEL_CGLM): five header slots (df behind the intercept flag); the flat GLM's rows, with
// log y_i (gamma_log) or 0 (student_t) in the slot behind y_i
SMCN_HD inline int64_t cglm_table_offset(int64_t npri, int64_t n, int64_t p) {
    return (5 + npri + n + n * p + 15) / 16 * 16;
}
// hierarchical GLM: the doubles before y, the table behind y, g and X, its row with the group slot
SMCN_HD inline int64_t hglm_head(int64_t Dc, bool disp) { return 5 + Dc + 1 + (disp ? 2 : 0); }
SMCN_HD inline int64_t hglm_table_offset(int64_t head, int64_t n, int64_t p) {
    return (head + 2 * n + n * p + 15) / 16 * 16;
}
SMCN_HD inline int hglm_row_doubles(int Dc) { return ((Dc + 1) & ~1) + 4; }
// multilevel GLM: up to kMlMaxTerms varying terms; the table starts at the first 128-byte boundary behind the block, a
// row holds a (g, z) pair per term behind y and lgamma(y + 1)
constexpr int kMlMaxTerms = 4;
SMCN_HD inline int64_t mlglm_head(int64_t Dc, int R, bool disp) { return 9 + Dc + R + (disp ? 2 : 0); }
SMCN_HD inline int64_t mlglm_table_offset(int64_t head, int R, int64_t n, int64_t p) {
    return (head + (1 + 2 * (int64_t)R) * n + n * p + 15) / 16 * 16;
}
SMCN_HD inline int mlglm_row_doubles(int Dc, int R) { return ((Dc + 1) & ~1) + 2 + 2 * R; }
constexpr int kCatMaxClasses = 16;
// ordinal: the K class counts behind the table
SMCN_HD inline int64_t ord_counts_offset(int64_t D, int64_t n, int64_t p) {
    return glm_table_offset(D, n, p) + glm_table_rows(n) * glm_row_doubles((int)p);
}

// One checked block: the caller's [header nh | priors npri | y n | g n (hierarchical) or g_r n, z_r n per term
// (multilevel) | X n x p], and its repacked image
// [block | padding | table rows x RS | class counts K (ordinal)].
struct RegLayout {
    int model = 0;
    int fam = 0, K = 0;         // the header's first slot: the family (GLM, hierarchical) or the classes (categorical, ordinal)
    int64_t n = 0, p = 0, J = 0;   // (multilevel: J is the sum of the terms' level counts)
    int R = 0;                  // multilevel: varying terms, and the levels of each (0 beyond R)
    int64_t Jr[kMlMaxTerms] = {0, 0, 0, 0};
    int ic = 0;                 // intercept flag
    int flags = 0;              // SMCN_MODEL_OGLM: 1 offsets, 2 weights
    double df = 0.0;            // SMCN_MODEL_CGLM: student_t's degrees of freedom (0: gamma_log)
    int Dc = 0, D = 0;          // columns of a table row (p for the ordinal model), coordinates
    int64_t nh = 0, npri = 0;   // header doubles, prior doubles
    int64_t y0 = 0, g0 = 0, X0 = 0, len = 0;      // offsets in the block (g0 = 0: no groups; multilevel: g_1), the block's length
    int64_t o0 = 0, w0 = 0;     // SMCN_MODEL_OGLM: offsets of o and w in the block (0: absent)
    int64_t t0 = 0, rows = 0;   // the table: offset, padded row count,
    int RS = 0, ys = 0;         // row width, y slot (lgamma(y + 1) and g, or the (g_r, z_r) pairs, follow it)
    int64_t c0 = 0;             // ordinal: offset of the class counts (0 otherwise)
    int64_t rlen = 0;           // length of the repacked image
    bool disp() const { return fam >= 2; }
};

namespace regdata {
// What differs between the models' checks apart from arithmetic: texts and bounds.
struct Spec {
    int nh;
    bool has_ic, has_J, has_R, need_cols;   // header slots 3 and 4 (J, or R with J_1..J_4 behind it); "no coefficients" refusal
    double kmax, pmax;
    const char *who, *layout, *slot0, *too_big, *sds;
    double dmin, dmax;                      // the coordinates the model's functors cover: dmin <= D <= dmax
    const char* too_small;                  // the refusal below dmin (none: dmin = 0)
    bool has_fl = false;                    // header slot 4 holds the flags (offsets, weights)
};
inline const Spec* spec(int model) {
    static const Spec glm = {
        4, true, false, false, true, 0.0, 1048576.0, "GLM target: ",
        "GLM target: data = [family, n, p, intercept, s_1..s_D, y_1..y_n, X (n x p, row-major)]",
        "GLM target: family must be 0 (bernoulli_logit) or 1 (poisson_log), or 2 (normal) or 3 (neg_binomial_2_log) "
        "with a dispersion prior",
        "GLM target: the device functor covers D <= 64 coefficients; larger models run host-evaluated "
        "(SMCN_MODEL_HOST + smcn_set_host_target: any object with logpdf / logpdfgrad through HostTarget)",
        "GLM target: prior sds must be finite and > 0", 0.0, 64.0, nullptr};
    static const Spec hglm = {
        5, true, true, false, false, 0.0, 1048576.0, "hierarchical GLM target: ",
        "hierarchical GLM target: data = [family, n, p, intercept, J, s_1..s_Dc, s_tau, (m_d, s_d: families "
        "2, 3), y_1..y_n, g_1..g_n, X (n x p, row-major)]",
        "hierarchical GLM target: family must be 0 (bernoulli_logit), 1 (poisson_log), 2 (normal) or 3 "
        "(neg_binomial_2_log)",
        "hierarchical GLM target: the device functor covers D = Dc + J + 1 (+ 1) <= 64 coordinates; larger models "
        "run host-evaluated (SMCN_MODEL_HOST + smcn_set_host_target: any object with logpdf / logpdfgrad through "
        "HostTarget)",
        "hierarchical GLM target: prior sds must be finite and > 0", 0.0, 64.0, nullptr};
    static const Spec cat = {
        4, true, false, false, true, (double)kCatMaxClasses, 1048576.0, "categorical target: ",
        "categorical target: data = [K, n, p, intercept, s_1..s_D, y_1..y_n, X (n x p, row-major)], "
        "D = (K - 1) (p + intercept)",
        "categorical target: K must be an integer in [2, 16] (the device functor holds up to 16 classes; more "
        "run host-evaluated: SMCN_MODEL_HOST + smcn_set_host_target, any object with logpdf / logpdfgrad "
        "through HostTarget)",
        "categorical target: the device functor covers D = (K - 1) (p + intercept) <= 64 coefficients; larger "
        "models run host-evaluated (SMCN_MODEL_HOST + smcn_set_host_target: any object with logpdf / logpdfgrad "
        "through HostTarget)",
        "categorical target: prior sds must be finite and > 0", 0.0, 64.0, nullptr};
    static const Spec ord = {
        3, false, false, false, false, HUGE_VAL, HUGE_VAL, "ordinal target: ",
        "ordinal target: data = [K, n, p, s_1..s_p, t_1..t_{K-1}, y_1..y_n, X (n x p, row-major)], "
        "D = p + K - 1",
        "ordinal target: K must be an integer >= 2",
        "ordinal target: the device functor covers D = p + K - 1 <= 64 coordinates; larger models run "
        "host-evaluated (SMCN_MODEL_HOST + smcn_set_host_target: any object with logpdf / logpdfgrad through "
        "HostTarget)",
        "ordinal target: prior sds (s for the coefficients, t for the cutpoints) must be finite and > 0", 0.0, 64.0, nullptr};
    static const Spec ml = {
        9, true, false, true, false, 0.0, 1048576.0, "multilevel GLM target: ",
        "multilevel GLM target: data = [family, n, p, intercept, R, J_1, J_2, J_3, J_4 (0 beyond R), s_1..s_Dc, "
        "s_tau_1..s_tau_R, (m_d, s_d: families 2, 3), y_1..y_n, then g_r (n) and z_r (n) for each of the R terms, "
        "X (n x p, row-major)]",
        "multilevel GLM target: family must be 0 (bernoulli_logit), 1 (poisson_log), 2 (normal) or 3 "
        "(neg_binomial_2_log)",
        "multilevel GLM target: the device functor covers D = Dc + J_1 + .. + J_R + R (+ 1) <= 64 coordinates; larger "
        "models run host-evaluated (SMCN_MODEL_HOST + smcn_set_host_target: any object with logpdf / logpdfgrad "
        "through HostTarget)",
        "multilevel GLM target: prior sds must be finite and > 0", 0.0, 64.0, nullptr};
    static const Spec wglm = {
        4, true, false, false, true, 0.0, 1048576.0, "wide GLM target: ",
        "wide GLM target: data = [family, n, p, intercept, s_1..s_D, y_1..y_n, X (n x p, row-major)] (SMCN_MODEL_GLM's block)",
        "wide GLM target: family must be 0 (bernoulli_logit) or 1 (poisson_log), or 2 (normal) or 3 (neg_binomial_2_log) "
        "with a dispersion prior",
        "wide GLM target: the device functor covers 65 <= D <= 256 coordinates; larger models run host-evaluated "
        "(SMCN_MODEL_HOST + smcn_set_host_target: any object with logpdf / logpdfgrad through HostTarget)",
        "wide GLM target: prior sds must be finite and > 0", 65.0, 256.0,
        "wide GLM target: the device functor covers 65 <= D <= 256 coordinates (D counts tau for families 2 and 3); "
        "D <= 64 is SMCN_MODEL_GLM's (GLMTarget)"};
    static const Spec oglm = {
        5, true, false, false, true, 0.0, 1048576.0, "offset GLM target: ",
        "offset GLM target: data = [family, n, p, intercept, flags, s_1..s_D, y_1..y_n, o_1..o_n (flags & 1), "
        "w_1..w_n (flags & 2), X (n x p, row-major)]",
        "offset GLM target: family must be 0 (bernoulli_logit) or 1 (poisson_log), or 2 (normal) or 3 (neg_binomial_2_log) "
        "with a dispersion prior",
        "offset GLM target: the device functor covers D <= 64 coefficients; larger models run host-evaluated "
        "(SMCN_MODEL_HOST + smcn_set_host_target: any object with logpdf / logpdfgrad through HostTarget)",
        "offset GLM target: prior sds must be finite and > 0", 0.0, 64.0, nullptr, true};
    static const Spec cglm = {
        5, true, false, false, true, 0.0, 1048576.0, "continuous GLM target: ",
        "continuous GLM target: data = [family, n, p, intercept, df, s_1..s_Dc, m_tau, s_tau, y_1..y_n, X (n x p, "
        "row-major)]",
        "continuous GLM target: family must be 0 (gamma_log) or 1 (student_t)",
        "continuous GLM target: the device functor covers D = Dc + 1 <= 64 coordinates (the coefficients and tau); larger "
        "models run host-evaluated (SMCN_MODEL_HOST + smcn_set_host_target: any object with logpdf / logpdfgrad through "
        "HostTarget)",
        "continuous GLM target: prior sds must be finite and > 0", 0.0, 64.0, nullptr};
    switch (model) {
        case SMCN_MODEL_CGLM: return &cglm;
        case SMCN_MODEL_OGLM: return &oglm;
        case SMCN_MODEL_GLM: return &glm;
        case SMCN_MODEL_WGLM: return &wglm;
        case SMCN_MODEL_HGLM: return &hglm;
        case SMCN_MODEL_CATEGORICAL: return &cat;
        case SMCN_MODEL_ORDINAL: return &ord;
        case SMCN_MODEL_MLGLM: return &ml;
    }
    return nullptr;
}
inline bool whole(double v, double lo, double hi) { return v >= lo && v <= hi && v == std::floor(v); }
}  // namespace regdata

// Checks the caller's data block of a regression model and fills *L: "", or what is wrong with the block.
inline std::string reg_check(int model, const double* md, int64_t len, RegLayout* L) {
    using regdata::whole;
    const regdata::Spec* const sp = regdata::spec(model);
    if (!sp) return "not a regression model";
    const auto say = [&](const char* what) { return std::string(sp->who) + what; };
    const bool og = model == SMCN_MODEL_OGLM;
    const bool glm = model == SMCN_MODEL_GLM || model == SMCN_MODEL_WGLM || og, hg = model == SMCN_MODEL_HGLM, cat = model == SMCN_MODEL_CATEGORICAL;
    const bool ml = model == SMCN_MODEL_MLGLM;
    const bool cg = model == SMCN_MODEL_CGLM;          // families of its own (0 gamma_log, 1 student_t), always with tau
    const bool fams = glm || hg || ml;                 // slot 0 is a family, not a class count
    if (len < sp->nh) return sp->layout;
    const double s0 = md[0], nd = md[1], pd = md[2], icd = sp->has_ic ? md[3] : 0.0, Jd = sp->has_J ? md[4] : 0.0;
    if (cg     ? !(s0 == 0.0 || s0 == 1.0)
        : fams ? !(s0 == 0.0 || s0 == 1.0 || s0 == 2.0 || s0 == 3.0)
               : !whole(s0, 2.0, sp->kmax))
        return sp->slot0;
    const bool disp = cg || (fams && s0 >= 2.0);
    if (!(icd == 0.0 || icd == 1.0)) return say("intercept must be 0 or 1");
    if (!whole(nd, 1.0, 2147483647.0)) return say("n must be an integer >= 1");
    if (!whole(pd, 0.0, sp->pmax)) return say("p must be an integer >= 0");
    const double fld = sp->has_fl ? md[4] : 0.0;
    if (sp->has_fl && fld == 0.0)
        return say("flags = 0 (neither offsets nor weights) is SMCN_MODEL_GLM's model: pass the block without the flags "
                   "slot as SMCN_MODEL_GLM");
    if (sp->has_fl && !whole(fld, 1.0, 3.0)) return say("flags must be 1 (offsets), 2 (weights) or 3 (both)");
    if (sp->has_J && !whole(Jd, 1.0, 1048576.0)) return say("J must be an integer >= 1 (the number of groups)");
    // multilevel: R terms, their level counts in the four slots behind R
    const double Rd = sp->has_R ? md[4] : 0.0;
    if (sp->has_R && !whole(Rd, 1.0, (double)kMlMaxTerms))
        return say("R must be an integer in [1, 4] (the number of varying terms)");
    double Jsum = 0.0;
    for (int r = 0; sp->has_R && r < kMlMaxTerms; ++r) {
        const double v = md[5 + r];
        if (r < (int)Rd ? !whole(v, 1.0, 1048576.0) : !(v == 0.0))
            return say("J_r must be an integer >= 1 (the levels of term r) for r <= R and 0 beyond R");
        Jsum += v;
    }
    const double Dcd = pd + icd;
    if (sp->need_cols && Dcd < 1.0) return say("no coefficients (p = 0 without an intercept)");
    // (in doubles: the ordinal model bounds neither p nor K before this)
    const double Dd = glm || cg ? Dcd + (disp ? 1 : 0)
                      : hg ? Dcd + Jd + 1 + (disp ? 1 : 0)
                      : ml ? Dcd + Jsum + Rd + (disp ? 1 : 0)
                      : cat ? (s0 - 1.0) * Dcd
                            : pd + s0 - 1.0;
    if (Dd > sp->dmax) return sp->too_big;
    if (Dd < sp->dmin) return sp->too_small;
    // continuous GLM: df belongs to student_t alone
    const double dfd = cg ? md[4] : 0.0;
    if (cg && s0 == 1.0 && !(dfd > 0.0 && std::isfinite(dfd))) return say("student_t needs df finite and > 0");
    if (cg && s0 == 0.0 && !(dfd == 0.0)) return say("gamma_log has no df: the slot must be 0");
    // the priors: sds, then the named ones -- a mean (finite) or an sd (finite and > 0)
    struct { const char* name; bool mean; } named[kMlMaxTerms + 2];
    int nn = 0;
    if (hg) named[nn++] = {"s_tau", false};
    for (int r = 0; r < (int)Rd; ++r) named[nn++] = {"s_tau", false};
    if (disp) {
        named[nn++] = {glm || cg ? "m_tau" : "m_d", true};
        named[nn++] = {glm || cg ? "s_tau" : "s_d", false};
    }
    RegLayout l;
    l.model = model;
    (fams || cg ? l.fam : l.K) = (int)s0;
    l.df = dfd;
    l.n = (int64_t)nd, l.p = (int64_t)pd, l.ic = (int)icd, l.J = (int64_t)Jd;
    l.Dc = (int)Dcd, l.D = (int)Dd;
    if (ml) {
        l.R = (int)Rd, l.J = (int64_t)Jsum;
        for (int r = 0; r < l.R; ++r) l.Jr[r] = (int64_t)md[5 + r];
    }
    const int64_t n = l.n, p = l.p, nsd = fams || cg ? l.Dc : l.D;
    l.nh = sp->nh;
    l.npri = nsd + nn;
    l.y0 = hg ? hglm_head(l.Dc, disp) : l.nh + l.npri;
    l.g0 = hg || ml ? l.y0 + n : 0;
    l.flags = (int)fld;
    l.o0 = (l.flags & 1) ? l.y0 + n : 0;
    l.w0 = (l.flags & 2) ? l.y0 + ((l.flags & 1) ? 2 : 1) * n : 0;
    l.X0 = l.y0 + (hg ? 2 : 1 + 2 * l.R + (l.o0 ? 1 : 0) + (l.w0 ? 1 : 0)) * n;
    l.len = l.X0 + n * p;
    if (len != l.len) {
        // a block laid out for families 0 / 1 but naming a dispersion family
        if (glm && disp && len == l.len - 2)
            return say("family must be 0 (bernoulli_logit) or 1 (poisson_log) for a block without m_tau, s_tau; "
                       "families 2 (normal) and 3 (neg_binomial_2_log) take data = [family, n, p, intercept, ") +
                   (og ? "flags, s_1..s_Dc, m_tau, s_tau, y_1..y_n, o, w, X]" : "s_1..s_Dc, m_tau, s_tau, y_1..y_n, X]");
        if (glm && disp)
            return say("data = [family, n, p, intercept, ") +
                   (og ? "flags, s_1..s_Dc, m_tau, s_tau, y_1..y_n, o_1..o_n (flags & 1), w_1..w_n (flags & 2), "
                       : "s_1..s_Dc, m_tau, s_tau, y_1..y_n, ") +
                   "X (n x p, row-major)] for families 2 (normal) and 3 (neg_binomial_2_log)";
        return sp->layout;
    }
    const auto positive = [](double v) { return v > 0.0 && std::isfinite(v); };
    for (int64_t c = 0; c < nsd; ++c)
        if (!positive(md[l.nh + c])) return sp->sds;
    for (int k = 0; k < nn; ++k) {
        const double v = md[l.nh + nsd + k];
        if (named[k].mean ? !std::isfinite(v) : !positive(v))
            return say(named[k].name) + (named[k].mean ? " must be finite" : " must be finite and > 0");
    }
    for (int64_t i = 0; i < n; ++i) {
        const double y = md[l.y0 + i];
        if (cg) {
            if (s0 == 0.0 ? !(y > 0.0 && std::isfinite(y)) : !std::isfinite(y))
                return say(s0 == 0.0 ? "gamma_log needs finite y > 0 (a zero has no gamma density: model zeros apart)"
                                     : "student_t needs finite y");
        } else if (!fams) {
            if (!(y >= 0.0 && y < s0 && y == std::floor(y))) return say("every label y must be an integer in [0, K)");
        } else if (s0 == 0.0) {
            if (!(y == 0.0 || y == 1.0)) return say("bernoulli_logit needs y in {0, 1}");
        } else if (s0 == 2.0) {
            if (!std::isfinite(y)) return say("normal needs finite y");
        } else if (!whole(y, 0.0, 9007199254740992.0)) {
            return say(s0 == 1.0 ? "poisson_log needs y in {0, 1, 2, ..}" : "neg_binomial_2_log needs y in {0, 1, 2, .., 2^53}");
        }
    }
    for (int64_t i = 0; hg && i < n; ++i) {
        const double g = md[l.g0 + i];
        if (!(g >= 0.0 && g < Jd && g == std::floor(g))) return say("every group index g must be an integer in [0, J)");
    }
    for (int r = 0; r < l.R; ++r) {                      // (multilevel) term r: g_r (n), z_r (n)
        const double* const gr = md + l.g0 + 2 * r * n;
        for (int64_t i = 0; i < n; ++i)
            if (!(gr[i] >= 0.0 && gr[i] < (double)l.Jr[r] && gr[i] == std::floor(gr[i])))
                return say("every group index g_r must be an integer in [0, J_r)");
        for (int64_t i = 0; i < n; ++i)
            if (!std::isfinite(gr[n + i])) return say("z must be finite");
    }
    for (int64_t i = 0; l.o0 && i < n; ++i)
        if (!std::isfinite(md[l.o0 + i])) return say("the offsets o must be finite");
    if (l.w0) {
        bool any = false;
        for (int64_t i = 0; i < n; ++i) {
            const double w = md[l.w0 + i];
            if (!(std::isfinite(w) && w >= 0.0)) return say("the weights w must be finite and >= 0");
            any = any || w > 0.0;
        }
        if (!any) return say("at least one weight w must be > 0");
    }
    for (int64_t t = 0; t < n * p; ++t)
        if (!std::isfinite(md[l.X0 + t])) return say("X must be finite");
    // the table, found as the functors find it (smcn_models.hpp)
    l.t0 = cg   ? cglm_table_offset(l.npri, n, p)
           : og ? oglm_table_offset(l.npri, n, p)
           : glm ? glm_table_offset(l.npri, n, p)
           : hg ? hglm_table_offset(l.y0, n, p)
           : ml ? mlglm_table_offset(l.y0, l.R, n, p)
                : glm_table_offset(l.D, n, p);
    l.RS = og ? oglm_row_doubles(l.Dc) : hg ? hglm_row_doubles(l.Dc) : ml ? mlglm_row_doubles(l.Dc, l.R) : glm_row_doubles(l.Dc);
    l.rows = glm_table_rows(n);
    l.ys = (l.Dc + 1) & ~1;
    l.rlen = l.t0 + l.rows * l.RS;
    if (model == SMCN_MODEL_ORDINAL) {
        l.c0 = ord_counts_offset(l.D, n, p);
        l.rlen = l.c0 + l.K;
    }
    *L = l;
    return "";
}

// The image the functors read, from a checked block: `mup` becomes [block | padding | table (| class counts)].  A row is
// [1 (intercept), X_i1 .. X_ip, 0 .. (to an even count), y_i, lgamma(y_i + 1) (families; 0 for the normal, whose y may
// be negative; continuous GLM: log y_i for gamma_log, 0 for student_t), g_i (hierarchical) or g_1i, z_1i, .., g_Ri, z_Ri (multilevel) or o_i (0 if absent), w_i (1 if absent)
// (offsets / weights: a padding row is all zero, so its weight is 0), 0 ..]; the ordinal model's K class counts n_0..n_{K-1} follow the table.
inline void reg_repack(const RegLayout& L, const double* md, std::vector<double>& mup) {
    const bool fams = L.model == SMCN_MODEL_GLM || L.model == SMCN_MODEL_HGLM || L.model == SMCN_MODEL_MLGLM ||
                      L.model == SMCN_MODEL_WGLM || L.model == SMCN_MODEL_OGLM;
    mup.assign(L.rlen, 0.0);
    std::copy(md, md + L.len, mup.begin());
    for (int64_t i = 0; i < L.n; ++i) {
        double* row = mup.data() + L.t0 + i * L.RS;
        if (L.ic) row[0] = 1.0;
        for (int64_t j = 0; j < L.p; ++j) row[L.ic + j] = md[L.X0 + i * L.p + j];
        const double y = md[L.y0 + i];
        row[L.ys] = y;
        if (fams) row[L.ys + 1] = L.fam == 2 ? 0.0 : std::lgamma(y + 1.0);
        if (L.model == SMCN_MODEL_CGLM) row[L.ys + 1] = L.fam == 0 ? std::log(y) : 0.0;
        if (L.g0 && !L.R) row[L.ys + 2] = md[L.g0 + i];
        if (L.model == SMCN_MODEL_OGLM) {
            row[L.ys + 2] = L.o0 ? md[L.o0 + i] : 0.0;
            row[L.ys + 3] = L.w0 ? md[L.w0 + i] : 1.0;
        }
        for (int r = 0; r < L.R; ++r) {
            row[L.ys + 2 + 2 * r] = md[L.g0 + 2 * r * L.n + i];
            row[L.ys + 3 + 2 * r] = md[L.g0 + (2 * r + 1) * L.n + i];
        }
        if (L.c0) mup[L.c0 + (int64_t)y] += 1.0;
    }
}

// New rows for a trained model: `block` is the model's data block without the priors.  Its header must repeat the training
// block's (but for the row count); `full` becomes the block smcn_ctx_create would take, the training priors spliced in
// behind the header.  "" or what is wrong.
inline std::string reg_splice(const RegLayout& train, const double* train_block, const double* block, int64_t len,
                              std::vector<double>& full) {
    const int64_t nh = train.nh;
    if (!block || len < nh) return "smcn_predict_set_data: the block is the model's data block without the priors";
    if (train.model == SMCN_MODEL_OGLM && block[4] != train_block[4])
        return "smcn_predict_set_data: the new rows' flags must repeat the training block's (" +
               std::to_string(train.flags) + ": new rows carry o where the model was fitted with offsets, and w = 1 where "
               "it was fitted with weights)";
    for (int64_t q = 0; q < nh; ++q)
        if (q != 1 && block[q] != train_block[q])
            return "smcn_predict_set_data: the new rows' header must repeat the training block's (family or K, p, "
                   "intercept, J): the column count differs from the training design?";
    full.clear();
    full.reserve((size_t)(len + train.npri));
    full.insert(full.end(), block, block + nh);
    full.insert(full.end(), train_block + nh, train_block + nh + train.npri);
    full.insert(full.end(), block + nh, block + len);
    return "";
}

}  // namespace smcn
