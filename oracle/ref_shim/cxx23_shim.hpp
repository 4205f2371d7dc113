// Stand-ins for the C++23 library pieces the reference's headers use and an older libstdc++ lacks.
// Force-included (-include) ahead of every reference header by oracle/ref.mk; our own code, test infrastructure only.
#pragma once

#include <cstddef>
#include <iterator>
#include <optional>
#include <ranges>
#include <utility>
#include <version>

#if !defined(__cpp_lib_unreachable)
namespace std {
[[noreturn]] inline void unreachable() { __builtin_unreachable(); }
}  // namespace std
#endif

#if !defined(__cpp_lib_ranges_enumerate)
// `range | std::views::enumerate` for a sized random-access range: yields (index, reference) pairs, index signed as in C++23.
namespace std::ranges::views {
struct rtk_enumerate_fn {};
inline constexpr rtk_enumerate_fn enumerate{};

template <class R>
struct rtk_enumerate_view {
    R* range;
    using base_iter = decltype(std::begin(std::declval<R&>()));
    using ref = decltype(*std::declval<base_iter>());
    struct iterator {
        std::ptrdiff_t idx;
        base_iter it;
        std::pair<std::ptrdiff_t, ref> operator*() const { return {idx, *it}; }
        iterator& operator++() { ++idx; ++it; return *this; }
        bool operator!=(const iterator& o) const { return it != o.it; }
    };
    iterator begin() const { return {0, std::begin(*range)}; }
    iterator end() const { return {0, std::end(*range)}; }
};

template <class R>
rtk_enumerate_view<std::remove_reference_t<R>> operator|(R&& r, rtk_enumerate_fn) { return {&r}; }
}  // namespace std::ranges::views
#endif
