// (nx, nu) instances compiled into the library. Anything else is ALQP_E_UNSUPPORTED:
// the product path fails loudly rather than falling back to a slow generic route.
#pragma once
#ifndef ALQP_FOR_EACH_DIMS   // debug builds (tools/phase_timing.sh) compile one size only
#define ALQP_FOR_EACH_DIMS(X) \
    X(2, 1) X(4, 1) X(4, 2) X(6, 1) X(6, 2) X(8, 2) X(10, 3) X(12, 4) X(13, 4) X(14, 4)
#endif

#include <type_traits>

namespace alqp {
// fn(std::integral_constant<int, NX>{}, std::integral_constant<int, NU>{}) for the compiled pair that matches (nx, nu),
// `otherwise` when none does. A generic lambda takes the two as `auto NX, auto NU` and uses them as template arguments.
template <typename R, typename Fn>
inline R for_dims(int nx, int nu, R otherwise, Fn &&fn) {
#define X(NX, NU) \
    if (nx == NX && nu == NU) return fn(std::integral_constant<int, NX>{}, std::integral_constant<int, NU>{});
    ALQP_FOR_EACH_DIMS(X)
#undef X
    return otherwise;
}
}  // namespace alqp
