// alqp_dyn_casadi.hip - dynamics + Jacobian providers of the reference's CasADi-generated robots (pendulum1l,
// cartpole1l, cartpole1l_v2, cartpole2l) with their C ABI. The torch-coded robots are in alqp_dyn_rigid.hip.
#include <hip/hip_runtime.h>

#include "alqp_quad.hpp"   // gld4, gst4
#include "alqp_dyn.hpp"    // Dual, DynCartpole2l
#include "mi_alqp.h"

namespace alqp {

// ---- dynamics provider: pendulum1l (deqmpc/my_envs/pendulum1l/src/generated_dynamics.c:55-140,
//      generated_derivatives.c:52-222). One RK4 step of theta'' = 4 tau - 19.62 sin(theta) with the
//      tangents w.r.t. (theta, omega, tau) carried along; one point per lane, outputs in the
//      solver's packed layout (x_next, F = [A | B] row-major 2x3). HBM-bound: 12 words per point.
template <typename real>
struct Dual3 {
    real v, d0, d1, d2;
};
template <typename real>
__device__ __forceinline__ Dual3<real> dadd(Dual3<real> a, real s, Dual3<real> b) {  // a + s b
    return {fma_(s, b.v, a.v), fma_(s, b.d0, a.d0), fma_(s, b.d1, a.d1), fma_(s, b.d2, a.d2)};
}
template <typename real>
__device__ __forceinline__ Dual3<real> pend_acc(Dual3<real> th, Dual3<real> ta) {
    const real sn = sin(th.v), cs = cos(th.v);
    const real kt = real(4), kg = real(19.62);
    return {kt * ta.v - kg * sn, kt * ta.d0 - kg * cs * th.d0, kt * ta.d1 - kg * cs * th.d1, kt * ta.d2 - kg * cs * th.d2};
}
template <typename real>
__global__ __launch_bounds__(256) void k_dyn_pendulum1l(long K, const real *x, const real *u, real h, const real *hpt, real *xn, real *F) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= K) return;
    if (hpt) h = hpt[i];
    using D = Dual3<real>;
    const D th = {x[2 * i], 1, 0, 0}, om = {x[2 * i + 1], 0, 1, 0}, ta = {u[i], 0, 0, 1};
    const real hh = real(0.5) * h;
    const D k1t = om, k1o = pend_acc(th, ta);
    const D om2 = dadd(om, hh, k1o), k2o = pend_acc(dadd(th, hh, k1t), ta);
    const D om3 = dadd(om, hh, k2o), k3o = pend_acc(dadd(th, hh, om2), ta);
    const D om4 = dadd(om, h, k3o), k4o = pend_acc(dadd(th, h, om3), ta);
    const real two = real(2), h6 = h / real(6);
    const D st = dadd(dadd(k1t, two, om2), real(1), dadd(om4, two, om3));
    const D so = dadd(dadd(k1o, two, k2o), real(1), dadd(k4o, two, k3o));
    const D tn = dadd(th, h6, st), on = dadd(om, h6, so);
    if (xn) {
        xn[2 * i] = tn.v;
        xn[2 * i + 1] = on.v;
    }
    if (F) {
        real *f = F + 6 * i;
        f[0] = tn.d0; f[1] = tn.d1; f[2] = tn.d2;
        f[3] = on.d0; f[4] = on.d1; f[5] = on.d2;
    }
}

template <typename real>
int dyn_pendulum1l_impl(long K, const void *x, const void *u, double h, const void *hpt, void *xn, void *F, void *stream) {
    if (K < 0 || !x || !u || (!xn && !F)) return ALQP_E_BADARG;
    if (K == 0) return 0;
    hipLaunchKernelGGL(k_dyn_pendulum1l<real>, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, (hipStream_t)stream, K,
                       (const real *)x, (const real *)u, (real)h, (const real *)hpt, (real *)xn, (real *)F);
    return hipGetLastError() == hipSuccess ? 0 : ALQP_E_LAUNCH;
}

// ---- dynamics provider: cartpole1l (deqmpc/my_envs/cartpole1l/src/generated_dynamics.c,
//      generated_derivatives.c). RK4 of M(th) q'' = tau - (mb sin th th'^2, 0) + (0, 9.81 mb sin th),
//      M = [[ma, -mb cos th], [-mb cos th, md]], with the six tangents w.r.t. (q, qdot, tau).
//      cartpole1l: (ma, mb, md) = (11, 1, 2); cartpole1l_v2 (my_envs/cartpole1l_v2, same model, lighter cart
//      and pole): (0.7, 0.1, 0.05) - oracle/dyn_oracle.c, pinned by tests/golden/dyn_cartpole1l{,_v2}.npz.
template <typename real>
struct CartPar {
    real ma, mb, md;
};
template <typename real>
struct Dual6 {
    real v, d[6];
};
template <typename real>
__device__ __forceinline__ Dual6<real> d6c(real v) {
    Dual6<real> r;
    r.v = v;
#pragma unroll
    for (int i = 0; i < 6; ++i) r.d[i] = 0;
    return r;
}
template <typename real>
__device__ __forceinline__ Dual6<real> d6axpy(Dual6<real> a, real s, Dual6<real> b) {  // a + s b
    Dual6<real> r;
    r.v = fma_(s, b.v, a.v);
#pragma unroll
    for (int i = 0; i < 6; ++i) r.d[i] = fma_(s, b.d[i], a.d[i]);
    return r;
}
template <typename real>
__device__ __forceinline__ Dual6<real> d6mul(Dual6<real> a, Dual6<real> b) {
    Dual6<real> r;
    r.v = a.v * b.v;
#pragma unroll
    for (int i = 0; i < 6; ++i) r.d[i] = fma_(a.d[i], b.v, a.v * b.d[i]);
    return r;
}
template <typename real>
__device__ __forceinline__ void cart_acc(CartPar<real> p, Dual6<real> th, Dual6<real> thd, Dual6<real> t0, Dual6<real> t1,
                                         Dual6<real> &xdd, Dual6<real> &thdd) {
    using D = Dual6<real>;
    const real snv = sin(th.v), csv = cos(th.v);
    D sn, cs;
    sn.v = snv;
    cs.v = csv;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        sn.d[i] = csv * th.d[i];
        cs.d[i] = -snv * th.d[i];
    }
    const D r0 = d6axpy(t0, -p.mb, d6mul(sn, d6mul(thd, thd)));       // tau0 - mb sin(th) thd^2
    const D r1 = d6axpy(t1, real(9.81) * p.mb, sn);                   // tau1 + 9.81 mb sin(th)
    const D det = d6axpy(d6c<real>(p.ma * p.md), -p.mb * p.mb, d6mul(cs, cs));
    D idet;
    idet.v = real(1) / det.v;
#pragma unroll
    for (int i = 0; i < 6; ++i) idet.d[i] = -det.d[i] * idet.v * idet.v;
    const D zero = d6c<real>(real(0));
    xdd = d6mul(idet, d6axpy(d6axpy(zero, p.mb, d6mul(cs, r1)), p.md, r0));    // M^-1 = [[md, mb c], [mb c, ma]] / det
    thdd = d6mul(idet, d6axpy(d6axpy(zero, p.mb, d6mul(cs, r0)), p.ma, r1));
}
template <typename real>
__global__ __launch_bounds__(256) void k_dyn_cartpole1l(long K, const real *x, const real *tau, real h, const real *hpt,
                                                        real *xn, real *J, CartPar<real> par) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= K) return;
    if (hpt) h = hpt[i];
    using D = Dual6<real>;
    real x0, x1, x2, x3;
    gld4(x + 4 * i, x0, x1, x2, x3);
    D px = d6c(x0), th = d6c(x1), xd = d6c(x2), thd = d6c(x3);
    D t0 = d6c(tau[2 * i]), t1 = d6c(tau[2 * i + 1]);
    px.d[0] = 1; th.d[1] = 1; xd.d[2] = 1; thd.d[3] = 1; t0.d[4] = 1; t1.d[5] = 1;
    const real hh = real(0.5) * h, two = real(2), h6 = h / real(6);
    D k1xd, k1td, k2xd, k2td, k3xd, k3td, k4xd, k4td;
    cart_acc(par, th, thd, t0, t1, k1xd, k1td);
    const D k2x = d6axpy(xd, hh, k1xd), k2t = d6axpy(thd, hh, k1td);
    cart_acc(par, d6axpy(th, hh, thd), k2t, t0, t1, k2xd, k2td);
    const D k3x = d6axpy(xd, hh, k2xd), k3t = d6axpy(thd, hh, k2td);
    cart_acc(par, d6axpy(th, hh, k2t), k3t, t0, t1, k3xd, k3td);
    const D k4x = d6axpy(xd, h, k3xd), k4t = d6axpy(thd, h, k3td);
    cart_acc(par, d6axpy(th, h, k3t), k4t, t0, t1, k4xd, k4td);
    D o[4];
    o[0] = d6axpy(px, h6, d6axpy(d6axpy(xd, two, k2x), real(1), d6axpy(k4x, two, k3x)));
    o[1] = d6axpy(th, h6, d6axpy(d6axpy(thd, two, k2t), real(1), d6axpy(k4t, two, k3t)));
    o[2] = d6axpy(xd, h6, d6axpy(d6axpy(k1xd, two, k2xd), real(1), d6axpy(k4xd, two, k3xd)));
    o[3] = d6axpy(thd, h6, d6axpy(d6axpy(k1td, two, k2td), real(1), d6axpy(k4td, two, k3td)));
    // 16-byte stores: a lane's 4 + 24 outputs are contiguous
    if (xn) gst4(xn + 4 * i, o[0].v, o[1].v, o[2].v, o[3].v);
    if (J) {
        real *jp = J + 24 * i;
        real f[24];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 6; ++c) f[6 * r + c] = o[r].d[c];
#pragma unroll
        for (int g = 0; g < 6; ++g) gst4(jp + 4 * g, f[4 * g], f[4 * g + 1], f[4 * g + 2], f[4 * g + 3]);
    }
}

template <typename real>
int dyn_cartpole1l_impl(long K, const void *x, const void *tau, double h, const void *hpt, void *xn, void *J, void *stream,
                        int version = 1) {
    if (K < 0 || !x || !tau || (!xn && !J)) return ALQP_E_BADARG;
    if (K == 0) return 0;
    const CartPar<real> par = version == 2 ? CartPar<real>{real(0.7), real(0.1), real(0.05)} : CartPar<real>{real(11), real(1), real(2)};
    hipLaunchKernelGGL(k_dyn_cartpole1l<real>, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, (hipStream_t)stream, K,
                       (const real *)x, (const real *)tau, (real)h, (const real *)hpt, (real *)xn, (real *)J, par);
    return hipGetLastError() == hipSuccess ? 0 : ALQP_E_LAUNCH;
}

// ---- dynamics provider: cartpole2l (model and dual-number step: alqp_dyn.hpp DynCartpole2l) -----
template <typename real>
__global__ __launch_bounds__(128) void k_dyn_cartpole2l(long K, const real *x, const real *tau, real h, const real *hpt,
                                                        real *xn, real *J) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= K) return;
    if (hpt) h = hpt[i];
    if (J) {
        Dual<real, 9> xd[6], td[3], on[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            xd[k] = dconst<real, 9>(x[6 * i + k]);
            xd[k].d[k] = 1;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            td[k] = dconst<real, 9>(tau[3 * i + k]);
            td[k].d[6 + k] = 1;
        }
        DynCartpole2l<real>::template step_full<9>(xd, td, h, on);
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            if (xn) xn[6 * i + r] = on[r].v;
#pragma unroll
            for (int c = 0; c < 9; ++c) J[54 * i + 9 * r + c] = on[r].d[c];
        }
    } else {
        Dual<real, 0> xd[6], td[3], on[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) xd[k].v = x[6 * i + k];
#pragma unroll
        for (int k = 0; k < 3; ++k) td[k].v = tau[3 * i + k];
        DynCartpole2l<real>::template step_full<0>(xd, td, h, on);
#pragma unroll
        for (int r = 0; r < 6; ++r) xn[6 * i + r] = on[r].v;
    }
}

template <typename real>
int dyn_cartpole2l_impl(long K, const void *x, const void *tau, double h, const void *hpt, void *xn, void *J, void *stream) {
    if (K < 0 || !x || !tau || (!xn && !J)) return ALQP_E_BADARG;
    if (K == 0) return 0;
    hipLaunchKernelGGL(k_dyn_cartpole2l<real>, dim3((unsigned)((K + 127) / 128)), dim3(128), 0, (hipStream_t)stream, K,
                       (const real *)x, (const real *)tau, (real)h, (const real *)hpt, (real *)xn, (real *)J);
    return hipGetLastError() == hipSuccess ? 0 : ALQP_E_LAUNCH;
}

}  // namespace alqp

extern "C" {

int alqp_dyn_pendulum1l_f32(long K, const void *x, const void *u, double h, const void *h_pt, void *xnext, void *F, void *stream) {
    return alqp::dyn_pendulum1l_impl<float>(K, x, u, h, h_pt, xnext, F, stream);
}
int alqp_dyn_pendulum1l_f64(long K, const void *x, const void *u, double h, const void *h_pt, void *xnext, void *F, void *stream) {
    return alqp::dyn_pendulum1l_impl<double>(K, x, u, h, h_pt, xnext, F, stream);
}

int alqp_dyn_cartpole1l_f32(long K, const void *x, const void *tau, double h, const void *h_pt, void *xnext, void *J, void *stream) {
    return alqp::dyn_cartpole1l_impl<float>(K, x, tau, h, h_pt, xnext, J, stream);
}
int alqp_dyn_cartpole1l_f64(long K, const void *x, const void *tau, double h, const void *h_pt, void *xnext, void *J, void *stream) {
    return alqp::dyn_cartpole1l_impl<double>(K, x, tau, h, h_pt, xnext, J, stream);
}
int alqp_dyn_cartpole1l_v2_f32(long K, const void *x, const void *tau, double h, const void *h_pt, void *xnext, void *J, void *stream) {
    return alqp::dyn_cartpole1l_impl<float>(K, x, tau, h, h_pt, xnext, J, stream, 2);
}
int alqp_dyn_cartpole1l_v2_f64(long K, const void *x, const void *tau, double h, const void *h_pt, void *xnext, void *J, void *stream) {
    return alqp::dyn_cartpole1l_impl<double>(K, x, tau, h, h_pt, xnext, J, stream, 2);
}

int alqp_dyn_cartpole2l_f32(long K, const void *x, const void *tau, double h, const void *h_pt, void *xnext, void *J, void *stream) {
    return alqp::dyn_cartpole2l_impl<float>(K, x, tau, h, h_pt, xnext, J, stream);
}
int alqp_dyn_cartpole2l_f64(long K, const void *x, const void *tau, double h, const void *h_pt, void *xnext, void *J, void *stream) {
    return alqp::dyn_cartpole2l_impl<double>(K, x, tau, h, h_pt, xnext, J, stream);
}

}  // extern "C"
