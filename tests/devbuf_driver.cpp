// Stand-alone check of the owner types of smcnuts_amd/csrc/smcn_devbuf.hpp (tests/test_devbuf_host.py builds it with
// g++ -fsanitize=address,undefined and runs it once).  The allocator counts its calls, keeps the blocks it has handed
// out, and fails the k-th allocation on request; exits non-zero at the first rule that does not hold.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "smcn_devbuf.hpp"

namespace {
struct Counting {
    static inline int allocs = 0, frees = 0, fail_at = 0, double_frees = 0, synced_frees = 0;
    static inline std::set<void*> live;
    static inline std::vector<std::string> log;      // "a<bytes>" / "f" in call order
    static inline std::vector<size_t> bytes;
    static int alloc(void** p, size_t n) {
        ++allocs;
        if (allocs == fail_at) return 2;             // (what an out-of-memory error looks like to the owner)
        *p = malloc(n);
        live.insert(*p);
        bytes.push_back(n);
        log.push_back("a" + std::to_string(n));
        return 0;
    }
    static void free(void* p, bool synced) {
        ++frees;
        synced_frees += synced ? 1 : 0;
        if (!live.erase(p)) { ++double_frees; return; }
        ::free(p);
        log.push_back("f");
    }
    static void start() { allocs = frees = fail_at = double_frees = synced_frees = 0; log.clear(); bytes.clear(); }
};
struct CountingEv {
    using event = int*;
    using stream = int;
    static inline int created = 0, destroyed = 0, records = 0, timing_created = 0;
    static int create(event* e, bool timing) { *e = new int(0); ++created; timing_created += timing ? 1 : 0; return 0; }
    static int record(event e, stream s) { *e = s; ++records; return 0; }
    static int wait(event e) { return e ? 0 : 1; }
    static int elapsed(float* ms, event from, event to) {
        if (!from || !to) return 1;
        *ms = (float)(*to - *from);
        return 0;
    }
    static void destroy(event e) { delete e; ++destroyed; }
};
using Buf = smcn::DevBuf<double, Counting>;
static_assert(!std::is_copy_constructible_v<Buf> && !std::is_copy_assignable_v<Buf>, "a buffer has one owner");
static_assert(std::is_move_constructible_v<Buf> && std::is_move_assignable_v<Buf>, "... which may change");
static_assert(!std::is_copy_constructible_v<smcn::DevEvent<CountingEv>>, "an event has one owner");

int failures = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #cond); \
            ++failures;                                                     \
        }                                                                   \
    } while (0)
}  // namespace

int main() {
    using C = Counting;
    // grow: nothing within the length, one free BEFORE the allocation beyond it
    C::start();
    {
        Buf b;
        CHECK((double*)b == nullptr && b.len() == 0);
        CHECK(b.grow(0) == 0 && C::allocs == 0 && (double*)b == nullptr);        // an empty buffer holds 0 elements
        CHECK(b.grow(2) == 0 && b.len() == 2 && (double*)b != nullptr);
        CHECK(C::allocs == 1 && C::frees == 0 && C::bytes.back() == 2 * sizeof(double));
        double* const p2 = b;
        b[0] = 1.0; b[1] = 2.0;                                                   // (the sanitizer checks the two elements)
        for (int64_t need : {0, 1, 2}) CHECK(b.grow(need) == 0 && (double*)b == p2 && b.len() == 2);
        CHECK(C::allocs == 1 && C::frees == 0);
        CHECK(b.grow(3) == 0 && b.len() == 3 && C::allocs == 2 && C::frees == 1);
        CHECK((C::log == std::vector<std::string>{"a16", "f", "a24"}));
        b[2] = 3.0;
        const double* cp = b;                                                     // (reads as the pointer it owns)
        CHECK(cp + 1 == b + 1);
    }
    CHECK(C::frees == 2 && C::synced_frees == 1 && C::live.empty());              // the destructor frees synced, once

    // a failed allocation leaves nothing, and a SMALLER need than the old length allocates again
    C::start();
    {
        Buf b;
        CHECK(b.grow(2) == 0);
        C::fail_at = 2;
        CHECK(b.grow(3) == 2);
        CHECK((double*)b == nullptr && b.len() == 0 && C::frees == 1 && C::live.empty());
        CHECK(b.grow(1) == 0 && (double*)b != nullptr && b.len() == 1 && C::allocs == 3);
        CHECK(C::bytes.back() == sizeof(double));
        C::fail_at = 4;
        CHECK(b.reset(1) == 2 && (double*)b == nullptr && b.len() == 0);          // reset follows the same rule
        CHECK(b.grow(1) == 0 && b.len() == 1);
    }
    CHECK(C::live.empty() && C::double_frees == 0 && C::frees == 3);

    // reset: fresh memory also at the same size; 0 elements are one element of memory
    C::start();
    {
        Buf b;
        CHECK(b.reset(3) == 0 && b.len() == 3 && C::allocs == 1 && C::frees == 0);
        CHECK(b.reset(3) == 0 && b.len() == 3 && C::allocs == 2 && C::frees == 1);
        CHECK((C::log == std::vector<std::string>{"a24", "f", "a24"}));
        CHECK(b.reset(0) == 0 && b.len() == 0 && (double*)b != nullptr && C::bytes.back() == sizeof(double));
        b.release();
        CHECK((double*)b == nullptr && b.len() == 0 && C::frees == 3 && C::synced_frees == 0);
        b.release();                                                              // (nothing to free)
        CHECK(C::frees == 3);
    }
    CHECK(C::frees == 3 && C::live.empty());

    // move: the source holds nothing, the destination owns; assignment frees what the destination held
    C::start();
    {
        Buf a;
        CHECK(a.reset(2) == 0);
        double* const pa = a;
        Buf b(std::move(a));
        CHECK((double*)a == nullptr && a.len() == 0 && (double*)b == pa && b.len() == 2 && C::frees == 0);
        Buf c;
        CHECK(c.reset(1) == 0);
        double* const pc = c;
        c = std::move(b);
        CHECK((double*)c == pa && c.len() == 2 && (double*)b == nullptr && C::frees == 1 && !C::live.count(pc));
        Buf d;
        CHECK(d.reset(3) == 0);
        double* const pd = d;
        std::swap(c, d);                                                          // (the population and its proposal trade places)
        CHECK((double*)c == pd && c.len() == 3 && (double*)d == pa && d.len() == 2 && C::frees == 1);
        CHECK(C::live.size() == 2);
    }
    CHECK(C::allocs == 3 && C::frees == 3 && C::double_frees == 0 && C::live.empty());

    // events: created at the first use, once; destroyed once
    {
        smcn::DevEvent<CountingEv> e0, e1;
        smcn::DevEvent<CountingEv, false> untimed;
        double ms = -1.0;
        CHECK(CountingEv::created == 0 && e0.wait() != 0 && e1.since(e0, &ms) != 0 && ms == -1.0);
        CHECK(e0.record(3) == 0 && e0.record(5) == 0 && e1.record(12) == 0);
        CHECK(CountingEv::created == 2 && CountingEv::records == 3);
        CHECK(e0.create() == 0 && CountingEv::created == 2);
        CHECK(e1.wait() == 0 && e1.since(e0, &ms) == 0 && ms == 7.0);
        CHECK(untimed.create() == 0 && CountingEv::created == 3 && CountingEv::timing_created == 2);
    }
    CHECK(CountingEv::created == 3 && CountingEv::destroyed == 3);

    if (failures) return 1;
    printf("devbuf ok\n");
    return 0;
}
