// std::optional<T>::transform (C++23) for the one type the reference's scalar kd-tree calls it on, hit<float>, as a
// specialisation of std::optional for that program-defined type.  Included only by the scalar build of oracle/ref_probe.cpp,
// after render/hit.hpp and before accel/kd_tree.hpp, and only when the standard library has no monadic optional.
#pragma once

#include <cstring>
#include <new>
#include <optional>
#include <type_traits>

#if !defined(__cpp_lib_optional) || __cpp_lib_optional < 202110L
template <>
class std::optional<hit<float>> {
    using T = hit<float>;
    static_assert(std::is_trivially_copyable_v<T>);
    alignas(T) unsigned char buf[sizeof(T)];
    bool has = false;

public:
    using value_type = T;
    optional() noexcept {}
    optional(std::nullopt_t) noexcept {}
    optional(const T& v) noexcept { std::memcpy(buf, &v, sizeof(T)); has = true; }
    optional& operator=(const T& v) noexcept { std::memcpy(buf, &v, sizeof(T)); has = true; return *this; }
    optional& operator=(std::nullopt_t) noexcept { has = false; return *this; }
    bool has_value() const noexcept { return has; }
    explicit operator bool() const noexcept { return has; }
    const T* operator->() const noexcept { return std::launder(reinterpret_cast<const T*>(buf)); }
    const T& operator*() const noexcept { return *operator->(); }
    const T& value() const { if (!has) throw std::bad_optional_access(); return *operator->(); }
    template <class Fn>
    auto transform(Fn&& fn) const {
        using U = std::remove_cv_t<std::invoke_result_t<Fn, const T&>>;
        return has ? std::optional<U>(fn(**this)) : std::optional<U>();
    }
};
#endif
