// What smcn_predict_draws and smcn_forecast_draws share on the host: the refusal of their arguments, the front of their
// work area and the NaN count of a result.  Plain C++17 with no HIP types, like smcn_devbuf.hpp and smcn_regdata.hpp: it
// compiles without a device compiler, so the arithmetic on caller-supplied lengths and the walk over the caller's
// ancestors run under the host sanitizers (tests/test_draw_plan_host.py).
#pragma once
#include <stdint.h>

#include <string>

namespace smcn {

// Empty, or why `who` refuses to draw the slots s_first .. s_first + s_count - 1 of S `noun` ("draws", "paths") from M
// particles into y_out; ancestors: NULL, or the caller's [S]
inline std::string draw_refusal(const char* who, const char* noun, int64_t M, int64_t S, int64_t s_first, int64_t s_count,
                                const double* y_out, const int64_t* ancestors) {
    const std::string w = std::string(who) + ": ";
    if (M < 1) return w + "M must be at least 1";
    if (S < 1 || S > 2147483647LL) return w + "the number of " + noun + " S must be in 1..2^31-1";
    if (s_first < 0 || s_count < 1 || s_first + s_count > S)
        return w + "the slot range [s_first, s_first + s_count) must be non-empty and lie in 0..S";
    if (!y_out) return w + "y_out is null";
    if (ancestors)
        for (int64_t s = 0; s < S; ++s)
            if (ancestors[s] < 0 || ancestors[s] >= M)
                return w + "ancestors[" + std::to_string(s) + "] is not a particle in 0..M-1";
    return {};
}

// The front of a draw call's work area, in doubles, every region at a multiple of 16:
// [header 16 | lw M | w M | scan M | tile totals nt | tile offsets nt + 1 | ancestors n | the caller's own regions]
struct DrawPlan {
    int nt;   // the scan tiles of M
    int64_t o_lw, o_w, o_loc, o_tt, o_to, o_anc, o_tail;
    static int64_t pad(int64_t v) { return (v + 15) / 16 * 16; }
    DrawPlan(int64_t M, int64_t n, int scan_tile) : nt((int)((M + scan_tile - 1) / scan_tile)) {
        o_lw = 16, o_w = o_lw + pad(M), o_loc = o_w + pad(M), o_tt = o_loc + pad(M), o_to = o_tt + pad(nt);
        o_anc = o_to + pad(nt + 1), o_tail = o_anc + pad(n);
    }
};

inline int64_t count_nan(const double* y, int64_t len) {
    int64_t nb = 0;
    for (int64_t e = 0; e < len; ++e) nb += y[e] != y[e] ? 1 : 0;
    return nb;
}

}  // namespace smcn
