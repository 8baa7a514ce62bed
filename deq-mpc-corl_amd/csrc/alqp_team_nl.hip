// alqp_team_nl.hip - the nonlinear fused solve with state box rows and / or general rows on the team kernel
// (k_solve_nonlin_team, alqp_team_nl.hpp) and its launcher. One object per row mask (-DALQP_NL_UNIT=<mask>, mask =
// 2 state bounds | 4 general rows; build.sh): the models of alqp_dyn.hpp that build without spilling (pendulum1l,
// cartpole1l, cartpole1l_v2), both dtypes, and a TRACE twin each (tests only). Uncapped builds only.
#ifndef ALQP_NL_UNIT
#error "compile with -DALQP_NL_UNIT=2, 4 or 6"
#endif
#include <hip/hip_runtime.h>

#include "alqp_team_nl.hpp"
#include "alqp_launch.hpp"

namespace alqp {

template <typename real, class Dyn, bool XBOX, bool POLY>
int launch_nonlin_team(const NlRowsSolveArgs<real> &a, const TraceArgs<real> *tr, hipStream_t stream) {
    using C = Cfg<real, Dyn::NX, Dyn::NU>;
    const size_t words = (size_t)C::team_words(a.T) + (POLY ? 2 * pad4(a.m) : 0);
    const size_t lds = (size_t)C::QPW * words * sizeof(real);
    if (lds > kMaxLds) return ALQP_E_UNSUPPORTED;
    const unsigned grid = (unsigned)((a.B + C::QPW - 1) / C::QPW);
    auto go = [&](auto fn, const TraceArgs<real> &t) {
        if (lds > 48 * 1024) {
            if (hipFuncSetAttribute(reinterpret_cast<const void *>(fn), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lds) != hipSuccess)
                return (int)ALQP_E_LAUNCH;
        }
        hipLaunchKernelGGL(fn, dim3(grid), dim3(64), lds, stream, a, t);
        return hipGetLastError() == hipSuccess ? 0 : (int)ALQP_E_LAUNCH;
    };
    if (tr) return go(k_solve_nonlin_team<real, Dyn, XBOX, POLY, true>, *tr);
    return go(k_solve_nonlin_team<real, Dyn, XBOX, POLY, false>, TraceArgs<real>{});
}

template <typename real, int MASK>
int dispatch_solve_nonlin_rows(int dyn_id, int nx, int nu, const NlRowsSolveArgs<real> &a, const TraceArgs<real> *tr,
                               hipStream_t stream) {
    constexpr bool X = (MASK & kGenXbox) != 0, P = (MASK & kGenPoly) != 0;
    if (dyn_id == DynPendulum1l<real>::ID && nx == 2 && nu == 1)
        return launch_nonlin_team<real, DynPendulum1l<real>, X, P>(a, tr, stream);
    if (dyn_id == DynCartpole1l<real>::ID && nx == 4 && nu == 1)
        return launch_nonlin_team<real, DynCartpole1l<real>, X, P>(a, tr, stream);
    if (dyn_id == DynCartpole1l<real, 2>::ID && nx == 4 && nu == 1)
        return launch_nonlin_team<real, DynCartpole1l<real, 2>, X, P>(a, tr, stream);
    // cartpole2l is left out: its builds spill (fp64: 72-188 B of scratch per lane at 512 registers, fp32: 6 registers
    // parked in AGPRs, every mask; tools/spill_report.py), and a spilling build of Team's sweeps is what alqp_team.hip's
    // header comment warns of. A caller gets ALQP_E_UNSUPPORTED and keeps the launch-per-step route.
    return ALQP_E_UNSUPPORTED;
}

template int dispatch_solve_nonlin_rows<float, ALQP_NL_UNIT>(int, int, int, const NlRowsSolveArgs<float> &,
                                                             const TraceArgs<float> *, hipStream_t);
template int dispatch_solve_nonlin_rows<double, ALQP_NL_UNIT>(int, int, int, const NlRowsSolveArgs<double> &,
                                                              const TraceArgs<double> *, hipStream_t);

}  // namespace alqp
