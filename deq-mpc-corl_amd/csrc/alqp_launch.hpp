// alqp_launch.hpp - how a kernel goes out (plain or cooperative) and the entry points through which the host unit
// (alqp_abi.hip) reaches the kernel units: alqp_team.hip (both dtypes in one object) and alqp_quad.hip (one object
// per dtype). Each returns 0 or an ALQP_E_* code; ALQP_E_UNSUPPORTED when (nx, nu) is not a compiled instance.
#pragma once
#include <hip/hip_runtime.h>

#include "alqp_args.hpp"
#include "mi_alqp.h"

namespace alqp {

constexpr size_t kMaxLds = 160 * 1024;

// A launch whose first argument carries ALQP_EXIT_IN_KERNEL goes out as a COOPERATIVE launch (the kernel then uses
// grid-wide barriers; the runtime refuses grids that cannot be co-resident: ALQP_E_COOP, the caller falls back to the
// launch-per-step route); everything else as a plain launch.
template <typename T>
inline int flags_of(const T &) { return 0; }
template <typename real>
inline int flags_of(const SolveArgs<real> &a) { return a.flags; }
template <typename real>
inline int flags_of(const ShdynSolveArgs<real> &a) { return a.flags; }
template <typename real>
inline int flags_of(const GenSolveArgs<real> &a) { return a.flags; }
template <typename Fn, typename A0, typename... Rest>
int launch_maybe_coop(Fn fn, unsigned grid, size_t lds, hipStream_t stream, A0 a0, Rest... rest) {
    if (flags_of(a0) & ALQP_EXIT_IN_KERNEL) {
        void *argv[] = {(void *)&a0, (void *)&rest...};
        // Any refusal of the cooperative launch (grid too large, cooperative launches not supported by the device or the
        // queue, ...) is ALQP_E_COOP: the caller then takes the launch-per-step route, which needs no co-residency.
        static int coop_ok = -1;
        if (coop_ok < 0) {
            int dev = 0, v = 0;
            coop_ok = (hipGetDevice(&dev) == hipSuccess &&
                       hipDeviceGetAttribute(&v, hipDeviceAttributeCooperativeLaunch, dev) == hipSuccess && v) ? 1 : 0;
        }
        if (!coop_ok) return ALQP_E_COOP;
        hipError_t e = hipLaunchCooperativeKernel(reinterpret_cast<const void *>(fn), dim3(grid), dim3(64), argv, (unsigned)lds, stream);
        if (e != hipSuccess) { (void)hipGetLastError(); return ALQP_E_COOP; }
        return 0;
    }
    hipLaunchKernelGGL(fn, dim3(grid), dim3(64), lds, stream, a0, rest...);
    return hipGetLastError() == hipSuccess ? 0 : ALQP_E_LAUNCH;
}

inline bool dims_ok(const AlqpDims *d) { return d && d->B > 0 && d->T >= 2 && d->nx > 0 && d->nu > 0; }

// The nullable AlqpObstacles of the C ABI -> the obs, nobs, obs_r2, no_init fields, which StepArgs and AuxArgs name alike
// (`a` zero-initialised). false: ALQP_E_BADARG.
template <typename real, typename Args>
inline bool set_obstacles(const AlqpDims *dims, const AlqpObstacles *obs, Args &a) {
    if (!obs) return true;
    if (obs->nobs < 0 || (obs->nobs > 0 && (!obs->pos || dims->nx < 3))) return false;
    if (obs->nobs > 0) { a.obs = (const real *)obs->pos; a.nobs = obs->nobs; a.obs_r2 = (real)(obs->radius * obs->radius); }
    a.no_init = obs->state_estimator;
    return true;
}

// alqp_team.hip
template <typename real>
int dispatch_solve(int nx, int nu, const SolveArgs<real> &a, const TraceArgs<real> *tr, hipStream_t stream);
template <typename real>
int dispatch_step(int nx, int nu, const StepArgs<real> &a, hipStream_t stream);
template <typename real, bool DYN>
int dispatch_backward(int nx, int nu, const BwdArgs<real, DYN> &a, hipStream_t stream);
template <typename real>
int dispatch_step_xbox(int nx, int nu, const XboxStepArgs<real> &a, hipStream_t stream);   // the state-bound step unit
template <typename real>
int dispatch_step_rows(int nx, int nu, const RowsStepArgs<real> &a, hipStream_t stream);   // the row-step unit; XBOX iff a.xlo
// the dense-step units, one object per POLY (alqp_team_dense_step, alqp_team_dense_step_rows); XBOX iff a.xlo
template <typename real, bool POLY>
int dispatch_step_dense(int nx, int nu, const DenseStepArgs<real> &a, hipStream_t stream);
template <typename real>
int dispatch_solve_shdyn(int nx, int nu, const ShdynSolveArgs<real> &a, const TraceArgs<real> *tr, hipStream_t stream);
// MASK: kGenDense | kGenXbox | kGenPoly, at least one of them; one object per mask (alqp_team_gen_*, -DALQP_GEN_UNIT=<mask>)
constexpr int kGenDense = 1, kGenXbox = 2, kGenPoly = 4;
template <typename real, int MASK>
int dispatch_solve_gen(int nx, int nu, const GenSolveArgs<real> &a, const TraceArgs<real> *tr, hipStream_t stream);
template <typename real>
size_t lds_query(int nx, int nu, int T);   // bytes of the team LDS image, 0: no such instance

// alqp_quad.hip
template <typename real>
int dispatch_solve_quad(int nx, int nu, const SolveArgs<real> &a, const TraceArgs<real> *tr, real *ws,
                        hipStream_t stream);
template <typename real>
int dispatch_solve_quad_shdyn(int nx, int nu, const ShdynSolveArgs<real> &a, const TraceArgs<real> *tr, real *ws,
                              hipStream_t stream);
template <typename real, bool DYN>
int dispatch_backward_quad(int nx, int nu, const BwdArgs<real, DYN> &a, real *ws, hipStream_t stream);
template <typename real>
int dispatch_solve_nonlin(int dyn_id, int nx, int nu, const SolveArgs<real> &a, real *ws, hipStream_t stream);
template <typename real>
int dispatch_step_quad(int nx, int nu, const StepArgs<real> &a, real *ws, hipStream_t stream);

}  // namespace alqp
