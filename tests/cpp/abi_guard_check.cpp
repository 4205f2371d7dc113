// abi_guard.hpp on the host (tests/test_cpp_abi_guard.py): what the guard of every C entry point returns and records.  Plain g++,
// no HIP; set_error is this program's own (the library's is in api.hip).  Prints one "... ok" line per group; any failure is
// reported and exits 1.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <new>
#include <stdexcept>
#include <string>

#include "abi_guard.hpp"

namespace {

std::string g_last;
int g_sets = 0;
bool g_set_throws = false;

int g_failed = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("FAILED %s (line %d): ", #cond, __LINE__);           \
            std::printf(__VA_ARGS__);                                        \
            std::printf("\n");                                               \
            if (++g_failed > 20) std::exit(1);                               \
        }                                                                    \
    } while (0)

void reset() { g_last = "untouched"; g_sets = 0; g_set_throws = false; }

// an entry point as the library writes them: a status out of a guarded body, which may itself call a guarded entry point
int inner_entry(int what) {
    return rtk::abi_guard([&]() -> int {
        if (what == 1) throw std::runtime_error("inner failed");
        if (what == 2) throw 7;
        return what == 0 ? RTK_OK : RTK_ERR_IO;
    });
}

int outer_entry(int what, bool then_throw) {
    return rtk::abi_guard([&]() -> int {
        const int rc = inner_entry(what);
        if (then_throw) throw std::runtime_error("outer failed");
        return rc;
    });
}

}  // namespace

namespace rtk {
void set_error(const std::string &msg) {
    if (g_set_throws) throw std::bad_alloc();
    g_last = msg;
    g_sets += 1;
}
}  // namespace rtk

int main() {
    using rtk::abi_guard;
    const auto returns_zero = []() -> int { return 0; };
    static_assert(noexcept(abi_guard(returns_zero)), "the guard itself never throws");

    // ---- a returned status passes through, whatever it is, and the last error is left alone
    reset();
    for (int rc : {int(RTK_OK), int(RTK_ERR_INVALID), int(RTK_ERR_UNSUPPORTED), int(RTK_ERR_HIP), int(RTK_ERR_IO), -12345, 77})
        CHECK(abi_guard([&]() -> int { return rc; }) == rc, "status %d", rc);
    CHECK(g_sets == 0 && g_last == "untouched", "sets %d last '%s'", g_sets, g_last.c_str());
    // (a body that records an error and returns its code, as fail() does)
    CHECK(abi_guard([&]() -> int { rtk::set_error("refused"); return RTK_ERR_UNSUPPORTED; }) == RTK_ERR_UNSUPPORTED && g_last == "refused" && g_sets == 1,
          "a refusal: sets %d last '%s'", g_sets, g_last.c_str());
    if (!g_failed) std::printf("status ok\n");

    // ---- a std::exception: RTK_ERR_INVALID and what()
    reset();
    CHECK(abi_guard([]() -> int { throw std::runtime_error("the table is full"); }) == RTK_ERR_INVALID, "runtime_error: code");
    CHECK(g_last == "the table is full" && g_sets == 1, "runtime_error: sets %d last '%s'", g_sets, g_last.c_str());
    reset();
    CHECK(abi_guard([]() -> int { throw std::bad_alloc(); }) == RTK_ERR_INVALID, "bad_alloc: code");
    CHECK(g_last == std::bad_alloc().what() && g_sets == 1, "bad_alloc: sets %d last '%s'", g_sets, g_last.c_str());
    reset();
    CHECK(abi_guard([]() -> int { return int(std::string("abc").at(9)); }) == RTK_ERR_INVALID && g_sets == 1 && g_last != "untouched" && !g_last.empty(),
          "out_of_range from the standard library: sets %d last '%s'", g_sets, g_last.c_str());
    if (!g_failed) std::printf("std::exception ok\n");

    // ---- anything else: RTK_ERR_INVALID and a fixed message
    reset();
    CHECK(abi_guard([]() -> int { throw 7; }) == RTK_ERR_INVALID, "throw 7: code");
    const std::string fixed = g_last;
    CHECK(g_sets == 1 && fixed != "untouched" && !fixed.empty(), "throw 7: sets %d last '%s'", g_sets, fixed.c_str());
    reset();
    CHECK(abi_guard([]() -> int { throw "a string literal"; }) == RTK_ERR_INVALID && g_last == fixed, "another type, the same message: '%s'", g_last.c_str());
    if (!g_failed) std::printf("other exceptions ok\n");

    // ---- recording the message throws: the code all the same
    reset(); g_set_throws = true;
    CHECK(abi_guard([]() -> int { throw std::runtime_error("lost"); }) == RTK_ERR_INVALID, "set_error throws under a std::exception");
    CHECK(abi_guard([]() -> int { throw std::bad_alloc(); }) == RTK_ERR_INVALID, "set_error throws under a bad_alloc");
    CHECK(abi_guard([]() -> int { throw 7; }) == RTK_ERR_INVALID, "set_error throws under throw 7");
    CHECK(abi_guard([]() -> int { rtk::set_error("x"); return RTK_OK; }) == RTK_ERR_INVALID, "set_error throws inside the body");
    CHECK(g_sets == 0 && g_last == "untouched", "nothing recorded: sets %d last '%s'", g_sets, g_last.c_str());
    if (!g_failed) std::printf("throwing set_error ok\n");

    // ---- a guarded call inside a guarded call: the inner guard ends the inner exception, the outer sees a status
    reset();
    CHECK(outer_entry(0, false) == RTK_OK && g_sets == 0, "nested, nothing thrown: sets %d", g_sets);
    CHECK(outer_entry(3, false) == RTK_ERR_IO && g_sets == 0, "nested, the inner status passes through both");
    reset();
    CHECK(outer_entry(1, false) == RTK_ERR_INVALID && g_last == "inner failed" && g_sets == 1, "nested, inner throws: sets %d last '%s'", g_sets, g_last.c_str());
    reset();
    CHECK(outer_entry(2, false) == RTK_ERR_INVALID && g_last == fixed && g_sets == 1, "nested, inner throws 7: sets %d last '%s'", g_sets, g_last.c_str());
    reset();
    CHECK(outer_entry(1, true) == RTK_ERR_INVALID && g_last == "outer failed" && g_sets == 2, "nested, both throw: the outer's message is the last: sets %d last '%s'",
          g_sets, g_last.c_str());
    reset();
    CHECK(outer_entry(0, true) == RTK_ERR_INVALID && g_last == "outer failed" && g_sets == 1, "nested, outer throws after the inner returned");
    if (!g_failed) std::printf("nested ok\n");

    if (g_failed) { std::printf("%d check(s) FAILED\n", g_failed); return 1; }
    std::printf("all ok\n");
    return 0;
}
