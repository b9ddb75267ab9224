// Owners of what a context keeps on the device: its buffers and its timing events (smcn_ctx.hpp).  Host-only and free of
// HIP: the runtime's calls come in through a policy, so that tests/devbuf_driver.cpp checks the rules below with a
// counting allocator under the host sanitizers.
//   - a buffer is a member of smcn_ctx and releases itself with it; nothing names it a second time in order to free it
//   - after a failed allocation a buffer holds nothing (null, length 0), so the next call allocates again
#pragma once
#include <cstddef>
#include <cstdint>

namespace smcn {

// `len` elements of T.  Mem: static int alloc(void** p, size_t bytes) (0: success) and static void free(void* p, bool
// synced) -- synced: the caller has waited for every stream that used the buffer.
template <class T, class Mem>
class DevBuf {
    T* p_ = nullptr;
    int64_t len_ = 0;

public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_), len_(o.len_) { o.p_ = nullptr; o.len_ = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            release();
            p_ = o.p_; len_ = o.len_;
            o.p_ = nullptr; o.len_ = 0;
        }
        return *this;
    }
    ~DevBuf() { release(true); }   // (a context's teardown has waited ONCE for its streams: free_all)

    operator T*() const { return p_; }
    int64_t len() const { return len_; }

    void release(bool synced = false) {
        if (p_) Mem::free(p_, synced);
        p_ = nullptr;
        len_ = 0;
    }
    // exactly n elements of fresh memory, also where it held n before (n <= 0 allocates one element)
    int reset(int64_t n) {
        release();
        void* q = nullptr;
        if (const int rc = Mem::alloc(&q, sizeof(T) * (size_t)(n > 0 ? n : 1))) return rc;
        p_ = (T*)q;
        len_ = n;
        return 0;
    }
    // at least `need` elements: untouched if it holds them, else the old memory goes BEFORE the new is asked for
    int grow(int64_t need) { return need <= len_ ? 0 : reset(need); }
};

// An event of the stream's timeline, created at its first use.  Ev: types event and stream; static int create(event*,
// bool timing), record(event, stream), wait(event), elapsed(float* ms, event from, event to); static void destroy(event).
template <class Ev, bool Timing = true>
class DevEvent {
    typename Ev::event e_{};

public:
    DevEvent() = default;
    DevEvent(const DevEvent&) = delete;
    DevEvent& operator=(const DevEvent&) = delete;
    ~DevEvent() { if (e_) Ev::destroy(e_); }

    int create() { return e_ ? 0 : Ev::create(&e_, Timing); }
    int record(typename Ev::stream s) {
        if (const int rc = create()) return rc;
        return Ev::record(e_, s);
    }
    int wait() const { return Ev::wait(e_); }
    // *ms = the time from `from` to this event (both recorded and reached); untouched on failure
    int since(const DevEvent& from, double* ms) const {
        float f = 0.f;
        if (const int rc = Ev::elapsed(&f, from.e_, e_)) return rc;
        *ms = (double)f;
        return 0;
    }
};

}  // namespace smcn
