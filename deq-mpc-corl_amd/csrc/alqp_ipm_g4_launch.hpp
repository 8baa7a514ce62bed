// Entry points of alqp_ipm_g4.hip (one translation unit per dtype) for the dispatcher in alqp_ipm.hip.
// Return 0, ALQP_E_UNSUPPORTED when the problem does not fit the register-resident kernel (T > 20, LDS image
// above 64 KB, strides beyond its 32-bit offsets: resident_addressable - the caller then takes the generic kernel),
// ALQP_E_LAUNCH.
#pragma once
#include "alqp_ipm_args.hpp"

namespace alqp_ipm_g4 {
int launch_f64(int nx, int nu, const alqp_ipm::IpmArgs<double> &a, const double *lams, const double *slacks,
               bool backward, void *stream);
int launch_f32(int nx, int nu, const alqp_ipm::IpmArgs<float> &a, const float *lams, const float *slacks,
               bool backward, void *stream);

// k * s + add < lim for k, s, add >= 0, without forming the product
inline bool lin_below(long k, long s, long add, long lim) {
    return add < lim && (k == 0 || s <= (lim - 1 - add) / k);
}

// Whether the register-resident kernel can address a problem with these element strides (IpmArgs::sC_t, sF_t, sf_t).
// It reads Cd / c, F and f as (the instance's base pointer) + (unsigned 32-bit BYTE offset of t * stride + element)
// (GpuX::g_ld in alqp_ipm_g4_gpu.hpp). The highest element it reads is
//   Cd, c: (T-1) * sC_t + n - 1      F: (T-2) * sF_t + nx * n - 1      f: (T-2) * sf_t + nx - 1
// and each must start below 2^32 bytes: time-major data (strides B * ...) crosses that at B ~ 135 k in fp64 and 270 k
// in fp32 at (20,13,4), where an offset would wrap silently into an earlier stage of the same array. Those element
// offsets are then below 2^30 and fit the kernel's 32-bit int arithmetic as well. Every other global access of the
// kernel (workspace slab, outputs, gbar, lams / slacks, ry_ext, x0, bounds) is an instance's base + an index below the
// instance's own size, which does not grow with B.
inline bool resident_addressable(int T, int nx, int nu, int real_bytes, long sC_t, long sF_t, long sf_t) {
    if (T < 2 || nx < 1 || nu < 1 || (real_bytes != 4 && real_bytes != 8) || sC_t < 0 || sF_t < 0 || sf_t < 0)
        return false;
    const long n = nx + nu, E = (1L << 32) / real_bytes;   // E: elements that start below 2^32 bytes
    return lin_below(T - 1, sC_t, n - 1, E) && lin_below(T - 2, sF_t, (long)nx * n - 1, E) &&
           lin_below(T - 2, sf_t, nx - 1, E);
}
}  // namespace alqp_ipm_g4
