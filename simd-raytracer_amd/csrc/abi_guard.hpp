// The one place where C++ exceptions end: every extern "C" function of api*.hip that returns a status runs its body through
// abi_guard, so nothing unwinds into a C caller (a std::bad_alloc from a vector or from building an error message included).
// No HIP, no accel: tests/cpp/abi_guard_check.cpp compiles it alone and brings its own set_error.
#pragma once

#include <exception>
#include <string>

#include "../../include/rtk.h"

namespace rtk {

void set_error(const std::string &msg);            // api.hip: the thread's rtk_last_error()

// What `body` returns.  A std::exception becomes RTK_ERR_INVALID with what() as the last error, anything else RTK_ERR_INVALID
// with a fixed message; if recording the message throws in its turn, the code is returned all the same.
template <typename Body>
int abi_guard(Body &&body) noexcept {
    const auto record = [](const char *msg) noexcept {
        try { set_error(msg); } catch (...) {}
    };
    try {
        return body();
    } catch (const std::exception &e) {
        record(e.what());
    } catch (...) {
        record("an exception that is no std::exception reached the C boundary");
    }
    return RTK_ERR_INVALID;
}

}  // namespace rtk
