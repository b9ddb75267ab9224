// Stand-alone check of smcnuts_amd/csrc/smcn_draw_plan.hpp under the host sanitizers (tests/test_draw_plan_host.py):
// the work area's offsets against the formulas the two entry points used to spell out, the refusals by their smallest
// triggering inputs with their exact texts, and the NaN count.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "smcn_draw_plan.hpp"

using namespace smcn;

static int failures = 0;
#define EXPECT(cond)                                                     \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("line %d: %s does not hold\n", __LINE__, #cond); \
            ++failures;                                                  \
        }                                                                \
    } while (0)

static int64_t pad(int64_t v) { return (v + 15) / 16 * 16; }

static void check_layout(int64_t M, int64_t n) {
    const DrawPlan p(M, n, 1024);
    const int64_t nt = (M + 1023) / 1024;
    EXPECT(p.nt == nt);
    EXPECT(p.o_lw == 16);
    EXPECT(p.o_w == 16 + pad(M));
    EXPECT(p.o_loc == 16 + pad(M) + pad(M));
    EXPECT(p.o_tt == 16 + pad(M) + pad(M) + pad(M));
    EXPECT(p.o_to == 16 + pad(M) + pad(M) + pad(M) + pad(nt));
    EXPECT(p.o_anc == 16 + pad(M) + pad(M) + pad(M) + pad(nt) + pad(nt + 1));
    EXPECT(p.o_tail == 16 + pad(M) + pad(M) + pad(M) + pad(nt) + pad(nt + 1) + pad(n));
    EXPECT(DrawPlan::pad(M) == pad(M));
    // [begin, begin + length) of the regions in their order: header 16, lw, w, scan, tile totals, tile offsets, ancestors
    const int64_t begin[] = {0, p.o_lw, p.o_w, p.o_loc, p.o_tt, p.o_to, p.o_anc, p.o_tail};
    const int64_t len[] = {16, M, M, M, nt, nt + 1, n};
    for (int r = 0; r < 7; ++r) {
        EXPECT(begin[r] % 16 == 0);
        EXPECT(begin[r] + len[r] <= begin[r + 1]);
    }
}

static void check_refusals(const char* noun) {
    const std::string who = "smcn_x_draws", w = who + ": ";
    double y = 0.0;
    const auto why = [&](int64_t M, int64_t S, int64_t s_first, int64_t s_count, const double* y_out, const int64_t* anc) {
        return draw_refusal(who.c_str(), noun, M, S, s_first, s_count, y_out, anc);
    };
    const std::string range = w + "the slot range [s_first, s_first + s_count) must be non-empty and lie in 0..S";
    const std::string count = w + "the number of " + noun + " S must be in 1..2^31-1";
    EXPECT(why(1, 1, 0, 1, &y, nullptr).empty());
    EXPECT(why(1, 2147483647LL, 2147483646LL, 1, &y, nullptr).empty());
    EXPECT(why(0, 1, 0, 1, &y, nullptr) == w + "M must be at least 1");
    EXPECT(why(1, 0, 0, 1, &y, nullptr) == count);
    EXPECT(why(1, 2147483648LL, 0, 1, &y, nullptr) == count);
    EXPECT(why(1, 1, -1, 1, &y, nullptr) == range);
    EXPECT(why(1, 1, 0, 0, &y, nullptr) == range);
    EXPECT(why(1, 3, 2, 2, &y, nullptr) == range);
    EXPECT(why(1, 3, 0, 4, &y, nullptr) == range);
    EXPECT(why(1, 1, 0, 1, nullptr, nullptr) == w + "y_out is null");
    const int64_t M = 5;
    std::vector<int64_t> anc = {0, 4, 2};
    EXPECT(why(M, 3, 1, 1, &y, anc.data()).empty());
    anc[2] = -1;
    EXPECT(why(M, 3, 1, 1, &y, anc.data()) == w + "ancestors[2] is not a particle in 0..M-1");
    anc[2] = 2, anc[0] = M;
    EXPECT(why(M, 3, 1, 1, &y, anc.data()) == w + "ancestors[0] is not a particle in 0..M-1");
    // today's order: M, S, the range, y_out, the ancestors
    EXPECT(why(0, 0, -1, 0, nullptr, anc.data()) == w + "M must be at least 1");
    EXPECT(why(M, 0, -1, 0, nullptr, anc.data()) == count);
    EXPECT(why(M, 3, -1, 0, nullptr, anc.data()) == range);
    EXPECT(why(M, 3, 0, 3, nullptr, anc.data()) == w + "y_out is null");
}

static void check_nan_count() {
    const double nan = std::nan("");
    std::vector<double> y(17, 1.5);
    EXPECT(count_nan(y.data(), 17) == 0);
    EXPECT(count_nan(y.data(), 0) == 0);
    y[0] = nan;
    EXPECT(count_nan(y.data(), 17) == 1);
    y[16] = nan;
    EXPECT(count_nan(y.data(), 17) == 2);
    EXPECT(count_nan(y.data(), 16) == 1);
    y[0] = INFINITY, y[7] = nan;
    EXPECT(count_nan(y.data(), 17) == 2);
}

int main() {
    for (int64_t M : {1, 15, 16, 17, 1023, 1024, 1025, 2049})
        for (int64_t n : {1, 16, 17}) check_layout(M, n);
    check_refusals("draws");
    check_refusals("paths");
    check_nan_count();
    if (failures) return 1;
    std::printf("draw plan ok\n");
    return 0;
}
