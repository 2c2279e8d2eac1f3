// qoc_pick.h -- the one idiom for the template ladders of the host code (MFMA path: qoc_mfma_plan.h and its resolvers; GEMM path: qoc_gemm_launch.h)
#pragma once
#include <type_traits>

// qoc_pick(f, QocOneOf<4, 8>{kc}, QocOneOf<8, 7, 6, 5>{qa}) calls f(integral_constant<int, kc>, integral_constant<int, qa>) -- each run-time value as
// the compile-time constant of its list that equals it, the LAST of the list when none does
template <int... Vs> struct QocOneOf { int v; };
template <class F> static inline void qoc_pick(F&& f) { f(); }
template <class F, int V0, int... Vs, class... Rest> static inline void qoc_pick(F&& f, QocOneOf<V0, Vs...> a, Rest... rest) {
    if constexpr (sizeof...(Vs) > 0) { if (a.v != V0) { qoc_pick(f, QocOneOf<Vs...>{a.v}, rest...); return; } }
    qoc_pick([&](auto... c) { f(std::integral_constant<int, V0>{}, c...); }, rest...);
}
