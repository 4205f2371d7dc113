// Who owns memory on the host side of the C-ABI: the only place that allocates.  A Buf owns one allocation of a memory source
// (accel.hpp has the real ones: device, pinned; a test counts with malloc), knows its capacity in ELEMENTS and frees in its
// destructor; an Event owns one lazily made handle.  How much a buffer takes when it has to grow is a rule, a pure function
// below.  No HIP, nothing else of the project: tests/cpp/dev_mem_check.cpp runs it.  A source is
//   struct Mem { static int alloc(void **p, size_t bytes); static void free(void *p); };        (0 = success, else its status)
//   struct Ev  { using handle = ...; static int create(handle *h); static void destroy(handle h); };
#pragma once

#include <cstddef>
#include <utility>

namespace rtk {

// ---- rules: elements to allocate for a request of n elements of `each` bytes.  `refit`: the buffer is re-made whenever its
// capacity differs from n (in either direction), not only when it is too small.
struct grow_exact { static constexpr bool refit = false; size_t operator()(size_t n, size_t) const { return n; } };
struct set_exactly { static constexpr bool refit = true; size_t operator()(size_t n, size_t) const { return n; } };
// need + need / 2 + 256 BYTES, at least one byte needed; a typed buffer rounds up to whole elements, never down
struct grow_bytes {
    static constexpr bool refit = false;
    size_t operator()(size_t n, size_t each) const {
        const size_t need = n * each > 0 ? n * each : 1;
        return (need + need / 2 + 256 + each - 1) / each;
    }
};
template <size_t Pad> struct grow_half { static constexpr bool refit = false; size_t operator()(size_t n, size_t) const { return n + n / 2 + Pad; } };
using grow_table = grow_half<16>;        // entries of the regions table
using grow_lights = grow_half<8>;        // rows of the light table
struct grow_capped {                     // n + n / 2, but not past `cap` (and never below n)
    static constexpr bool refit = false;
    size_t cap;
    size_t operator()(size_t n, size_t) const { const size_t g = n + n / 2 < cap ? n + n / 2 : cap; return g > n ? g : n; }
};

template <typename T, typename Mem>
class Buf {
    T *p_ = nullptr;
    size_t cap_ = 0;
    int remake(size_t n) {                // (an empty request still gets a valid pointer)
        reset();
        if (n == 0) n = 1;
        void *p = nullptr;
        const int e = Mem::alloc(&p, n * sizeof(T));
        if (e != 0) return e;
        p_ = static_cast<T *>(p); cap_ = n;
        return 0;
    }
public:
    Buf() = default;
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    Buf(Buf &&o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    Buf &operator=(Buf &&o) noexcept { if (this != &o) { reset(); swap(o); } return *this; }
    ~Buf() { reset(); }
    T *get() const { return p_; }
    size_t capacity() const { return cap_; }
    void swap(Buf &o) noexcept { std::swap(p_, o.p_); std::swap(cap_, o.cap_); }
    void reset() { if (p_) Mem::free(p_); p_ = nullptr; cap_ = 0; }
    // Room for n elements.  Within capacity: nothing happens, no call to the source.  Else the old allocation is freed, what the
    // rule gives is allocated and the old contents are NOT kept; on failure the buffer is empty and the source's status comes back.
    template <typename Rule = grow_exact>
    int reserve(size_t n, Rule rule = Rule()) {
        if (p_ && (Rule::refit ? n == cap_ : n <= cap_)) return 0;
        return remake(rule(n, sizeof(T)));
    }
};

template <typename Ev>
class Event {
    typename Ev::handle h_ = nullptr;
public:
    Event() = default;
    Event(const Event &) = delete;
    Event &operator=(const Event &) = delete;
    Event(Event &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    Event &operator=(Event &&o) noexcept { if (this != &o) { reset(); std::swap(h_, o.h_); } return *this; }
    ~Event() { reset(); }
    typename Ev::handle get() const { return h_; }
    int ensure() { return h_ ? 0 : Ev::create(&h_); }      // made on first use
    void reset() { if (h_) Ev::destroy(h_); h_ = nullptr; }
};

}  // namespace rtk
