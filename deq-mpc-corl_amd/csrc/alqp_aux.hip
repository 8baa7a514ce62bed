// alqp_aux.hip - the size-generic helper kernels of the launch-per-step routes (merit, line-search pick, dual update,
// batch-global exit test; one wavefront per instance) with their C ABI, and the _xbox (state bounds), _rows (general rows,
// with or without state bounds) and _dense (dense stage cost, with or without either) kernels of merit, pick and dual: merit
// and dual are one shared body each, which the kernels of the three families wrap, and one host-side filler and launcher
// serve all of them.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "alqp_launch.hpp"   // dims_ok, set_obstacles
#include "mi_alqp.h"

namespace alqp {

// ---- size-generic helper kernels (one wavefront per instance) ----------------------
template <typename real>
__device__ inline real wave_sum(real v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <typename real>
struct AuxArgs {
    int B, T, nx, nu, K, n_ls;
    const real *zc, *xnext, *x0, *lam, *rho, *Qd, *q, *ulo, *uhi;
    long sb_u, st_u;
    real *phi, *rnorm2;
    // pick
    const real *phi_all, *d;
    real *phi_prev, *z;
    int *k_out, *accept_out;
    // dual
    real *lam_io, *rho_io;
    real rho_scale;
    // obstacle rows (nullable): centres [B][T][nobs][3], radius^2
    const real *obs;
    int nobs;
    real obs_r2;
    int no_init;   // state-estimator row set: the initial-state rows (row block T-1) do not exist
};

// c_k = r^2 - |x_t[0:3] - o_k|^2 for obstacle row e = t*nobs + k of instance b (al_utils.py:313-323)
template <typename real>
__device__ inline real obs_row(const AuxArgs<real> &a, const real *z, int b, int e) {
    const int t = e / a.nobs, n = a.nx + a.nu;
    const real *o = a.obs + ((size_t)b * a.T * a.nobs + e) * 3;
    const real d0 = z[t * n] - o[0], d1 = z[t * n + 1] - o[1], d2 = z[t * n + 2] - o[2];
    return a.obs_r2 - (d0 * d0 + d1 * d1 + d2 * d2);
}

// merit of candidate kk for instance b (al_utils.py:73-77), block = (kk, b)
template <typename real>
__global__ __launch_bounds__(64) void k_merit(AuxArgs<real> a) {
    const int lane = threadIdx.x;
    const int b = blockIdx.x % a.B, kk = blockIdx.x / a.B;
    const int T = a.T, nx = a.nx, nu = a.nu, n = nx + nu, neq = T * nx;
    const real *z = a.zc + ((size_t)kk * a.B + b) * T * n;
    const real *xn = a.xnext + ((size_t)kk * a.B + b) * (T - 1) * nx;
    const int nit = 2 * nu + a.nobs;   // inequality rows per stage
    const real *lam = a.lam + (size_t)b * (neq + T * nit);
    const real *Qd = a.Qd + (size_t)b * T * n, *q = a.q + (size_t)b * T * n;
    const real *ulo = a.ulo + (size_t)b * a.sb_u, *uhi = a.uhi + (size_t)b * a.sb_u;
    const real rho = a.rho[b];
    real acc = 0, sq = 0;
    for (int e = lane; e < T * n; e += 64) {
        int t = e / n, j = e - t * n;
        real v = z[e];
        acc += (real(0.5) * Qd[e] * v + q[e]) * v;
        if (j >= nx) {
            int ju = j - nx;
            real vu = v - uhi[t * a.st_u + ju], vl = -v + ulo[t * a.st_u + ju];
            real cu = vu > 0 ? vu : real(0), cl = vl > 0 ? vl : real(0);
            int ru = neq + t * nit + ju;
            acc += lam[ru] * vu + lam[ru + nu] * vl;
            sq += cu * cu + cl * cl;
        }
    }
    for (int e = lane; e < T * a.nobs; e += 64) {
        const real ck = obs_row(a, z, b, e), cp = ck > 0 ? ck : real(0);
        acc += lam[neq + (e / a.nobs) * nit + 2 * nu + e % a.nobs] * ck;
        sq += cp * cp;
    }
    const int neq_rows = a.no_init ? neq - nx : neq;
    for (int e = lane; e < neq_rows; e += 64) {
        int t = e / nx, i = e - t * nx;
        real r = (t < T - 1) ? z[(t + 1) * n + i] - xn[t * nx + i] : z[i] - a.x0[(size_t)b * nx + i];
        acc += lam[e] * r;
        sq += r * r;
    }
    acc = wave_sum(acc);
    sq = wave_sum(sq);
    if (lane == 0) {
        a.phi[(size_t)kk * a.B + b] = acc + real(0.5) * rho * sq;
        if (a.rnorm2) a.rnorm2[(size_t)kk * a.B + b] = sq;
    }
}

// The whole line search of one Newton step in ONE launch (nonlinear-caller mode at scale): the merits of
// the n_ls candidates z + 2^-k d (al_utils.py:618-633; x_next of every candidate was evaluated by the
// caller's dynamics: xnext_all [n_ls][B][T-1][nx]), first-argmin with NaN winning like torch.min, strict
// accept, z <- z + alpha d in place, phi_prev <- phi_min regardless (:569), rnorm2 <- sum r+^2 of the
// chosen candidate when accepted. One wavefront per instance: it reads z, d once (not the 20-fold stack
// the reference materialises) and its 20 x_next slabs; everything else comes from registers.
template <typename real>
__global__ __launch_bounds__(64) void k_merit_pick(AuxArgs<real> a) {
    const int lane = threadIdx.x, b = blockIdx.x;
    const int T = a.T, nx = a.nx, nu = a.nu, n = nx + nu, neq = T * nx, nit = 2 * nu + a.nobs;
    real *z = a.z + (size_t)b * T * n;
    const real *d = a.d + (size_t)b * T * n;
    const real *lam = a.lam + (size_t)b * (neq + T * nit);
    const real *Qd = a.Qd + (size_t)b * T * n, *q = a.q + (size_t)b * T * n;
    const real *ulo = a.ulo + (size_t)b * a.sb_u, *uhi = a.uhi + (size_t)b * a.sb_u;
    const real rho = a.rho[b];
    real acc[20], sq[20];
#pragma unroll
    for (int k = 0; k < 20; ++k) { acc[k] = 0; sq[k] = 0; }
    // cost + bound rows: every lane walks its elements once, all candidates from registers
    for (int e = lane; e < T * n; e += 64) {
        const int t = e / n, j = e - t * n;
        const real zv = z[e], dv = d[e], Qv = Qd[e], qv = q[e];
        real bu = 0, bl = 0, lu = 0, ll = 0;
        const bool isu = j >= nx;
        if (isu) {
            bu = uhi[t * a.st_u + j - nx]; bl = ulo[t * a.st_u + j - nx];
            lu = lam[neq + t * nit + j - nx]; ll = lam[neq + t * nit + nu + j - nx];
        }
        real alpha = 1;
#pragma unroll
        for (int k = 0; k < 20; ++k) {
            const real v = zv + alpha * dv;
            acc[k] += (real(0.5) * Qv * v + qv) * v;
            if (isu) {
                const real vu = v - bu, vl = -v + bl;
                const real cu = vu > 0 ? vu : real(0), cl = vl > 0 ? vl : real(0);
                acc[k] += lu * vu + ll * vl;
                sq[k] += cu * cu + cl * cl;
            }
            alpha *= real(0.5);
        }
    }
    // equality rows: r = x_{t+1}(candidate) - xnext_k, init rows x_0 - x0
    for (int e = lane; e < (a.no_init ? neq - nx : neq); e += 64) {
        const int t = e / nx, i = e - t * nx;
        const real le = lam[e];
        const int zi = (t < T - 1) ? (t + 1) * n + i : i;
        const real zv = z[zi], dv = d[zi];
        const real x0v = (t < T - 1) ? real(0) : a.x0[(size_t)b * nx + i];
        real alpha = 1;
#pragma unroll
        for (int k = 0; k < 20; ++k) {
            if (k < a.n_ls) {
                const real ref = (t < T - 1) ? a.xnext[(((size_t)k * a.B + b) * (T - 1) + t) * nx + i] : x0v;
                const real r = zv + alpha * dv - ref;
                acc[k] += le * r;
                sq[k] += r * r;
            }
            alpha *= real(0.5);
        }
    }
    // obstacle rows (Obstacle_MPC): c_k at the candidate's position
    for (int e = lane; e < T * a.nobs; e += 64) {
        const int t = e / a.nobs;
        const real *o = a.obs + ((size_t)b * T * a.nobs + e) * 3;
        const real lk = lam[neq + t * nit + 2 * nu + e % a.nobs];
        real alpha = 1;
#pragma unroll
        for (int k = 0; k < 20; ++k) {
            const real d0 = z[t * n] + alpha * d[t * n] - o[0], d1 = z[t * n + 1] + alpha * d[t * n + 1] - o[1],
                       d2 = z[t * n + 2] + alpha * d[t * n + 2] - o[2];
            const real ck = a.obs_r2 - (d0 * d0 + d1 * d1 + d2 * d2), cp = ck > 0 ? ck : real(0);
            acc[k] += lk * ck;
            sq[k] += cp * cp;
            alpha *= real(0.5);
        }
    }
    int kbest = 0;
    real best = 0, sqbest = 0;
#pragma unroll
    for (int k = 0; k < 20; ++k) {
        if (k < a.n_ls) {
            const real s2 = wave_sum(sq[k]);
            const real v = wave_sum(acc[k]) + real(0.5) * rho * s2;
            if (a.phi) a.phi[(size_t)k * a.B + b] = v;     // (all lanes hold the same value)
            if (k == 0) { best = v; sqbest = s2; }
            else if (!(best != best) && (v != v || v < best)) { best = v; kbest = k; sqbest = s2; }
        }
    }
    const real prev = a.phi_prev[b];
    const bool ok = best < prev;
    if (ok) {
        const real alpha = real(1) / real(1 << kbest);
        for (int e = lane; e < T * n; e += 64) z[e] += alpha * d[e];
    }
    if (lane == 0) {
        a.phi_prev[b] = best;
        if (a.k_out) a.k_out[b] = kbest;
        if (a.accept_out) a.accept_out[b] = ok ? 1 : 0;
        if (a.rnorm2 && ok) a.rnorm2[b] = sqbest;
    }
}

// line-search decision + update (al_utils.py:634-641), block = instance
template <typename real>
__global__ __launch_bounds__(64) void k_pick(AuxArgs<real> a) {
    const int lane = threadIdx.x, b = blockIdx.x;
    const int Tn = a.T * (a.nx + a.nu);
    int kbest = 0;
    real best = a.phi_all[b];
    for (int k = 1; k < a.n_ls; ++k) {
        real v = a.phi_all[(size_t)k * a.B + b];
        if (!(best != best) && (v != v || v < best)) { best = v; kbest = k; }
    }
    const real prev = a.phi_prev[b];
    const bool acc = best < prev;
    // 2^-kbest in `real`: n_ls has no upper limit here, an integer shift would be undefined from kbest = 31 on
    const real alpha = acc ? ldexp(real(1), -kbest) : real(0);
    real *z = a.z + (size_t)b * Tn;
    const real *d = a.d + (size_t)b * Tn;
    if (acc)
        for (int e = lane; e < Tn; e += 64) z[e] += alpha * d[e];
    __syncthreads();
    if (lane == 0) {
        a.phi_prev[b] = best;
        if (a.k_out) a.k_out[b] = kbest;
        if (a.accept_out) a.accept_out[b] = acc ? 1 : 0;
    }
}

// dual update + projection + rho growth (AL_mpc.py:315-317,325), block = instance
template <typename real>
__global__ __launch_bounds__(64) void k_dual(AuxArgs<real> a) {
    const int lane = threadIdx.x, b = blockIdx.x;
    const int T = a.T, nx = a.nx, nu = a.nu, n = nx + nu, neq = T * nx;
    const real *z = a.zc + (size_t)b * T * n;
    const real *xn = a.xnext + (size_t)b * (T - 1) * nx;
    const int nit = 2 * nu + a.nobs;
    real *lam = a.lam_io + (size_t)b * (neq + T * nit);
    const real *ulo = a.ulo + (size_t)b * a.sb_u, *uhi = a.uhi + (size_t)b * a.sb_u;
    const real rho = a.rho_io[b];
    for (int e = lane; e < (a.no_init ? neq - nx : neq); e += 64) {
        int t = e / nx, i = e - t * nx;
        real r = (t < T - 1) ? z[(t + 1) * n + i] - xn[t * nx + i] : z[i] - a.x0[(size_t)b * nx + i];
        lam[e] += rho * r;
    }
    for (int e = lane; e < T * nu; e += 64) {
        int t = e / nu, j = e - t * nu;
        real u = z[t * n + nx + j];
        int ru = neq + t * nit + j, rl = ru + nu;
        real v1 = lam[ru] + rho * (u - uhi[t * a.st_u + j]);
        real v2 = lam[rl] + rho * (-u + ulo[t * a.st_u + j]);
        lam[ru] = v1 < 0 ? real(0) : v1;
        lam[rl] = v2 < 0 ? real(0) : v2;
    }
    for (int e = lane; e < T * a.nobs; e += 64) {
        const int r = neq + (e / a.nobs) * nit + 2 * nu + e % a.nobs;
        const real v = lam[r] + rho * obs_row(a, z, b, e);
        lam[r] = v < 0 ? real(0) : v;
    }
    __syncthreads();
    if (lane == 0) a.rho_io[b] = rho * a.rho_scale;
}

// batch-global exit test of the Newton loop, taken on the device (al_utils.py:551-564)
__global__ void k_exit_test(const double *sumsq, double *ctl, int mode, double tol) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double nw = sqrt(sumsq[0]);
    if (mode == 0) {
        ctl[0] = 0.0;
        ctl[1] = 0.0;
        ctl[2] = nw;
    } else if (ctl[0] == 0.0) {
        ctl[1] += 1.0;
        const double old = ctl[2];
        if (nw < tol || fabs(old - nw) / nw < tol) ctl[0] = 1.0;   // nw = inf (a tripped instance): NaN, no exit
        else ctl[2] = nw;
    }
}

template <typename real>
int merit_impl(const AlqpDims *dims, int K, const void *zc, const void *xnext, const void *x0,
               const void *lam, const void *rho, const void *Qd, const void *q, const void *u_lo,
               const void *u_hi, long sb_u, long st_u, const AlqpObstacles *obs, void *phi, void *rnorm2,
               void *stream) {
    if (!dims_ok(dims) || K < 1 || !zc || !xnext || !x0 || !lam || !rho || !Qd || !q || !u_lo || !u_hi || !phi)
        return ALQP_E_BADARG;
    AuxArgs<real> a = {};
    if (!set_obstacles<real>(dims, obs, a)) return ALQP_E_BADARG;
    a.B = dims->B; a.T = dims->T; a.nx = dims->nx; a.nu = dims->nu; a.K = K;
    a.zc = (const real *)zc; a.xnext = (const real *)xnext; a.x0 = (const real *)x0;
    a.lam = (const real *)lam; a.rho = (const real *)rho; a.Qd = (const real *)Qd; a.q = (const real *)q;
    a.ulo = (const real *)u_lo; a.uhi = (const real *)u_hi; a.sb_u = sb_u; a.st_u = st_u;
    a.phi = (real *)phi; a.rnorm2 = (real *)rnorm2;
    hipLaunchKernelGGL(k_merit<real>, dim3((unsigned)((size_t)K * dims->B)), dim3(64), 0,
                       (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : ALQP_E_LAUNCH;
}

template <typename real>
int merit_pick_impl(const AlqpDims *dims, int n_ls, const void *d, const void *xnext_all, const void *x0,
                    const void *lam, const void *rho, const void *Qd, const void *q, const void *u_lo,
                    const void *u_hi, long sb_u, long st_u, const AlqpObstacles *obs, void *z, void *phi_prev,
                    void *rnorm2, void *phi_all, int *k_out, int *accept_out, void *stream) {
    if (!dims_ok(dims) || n_ls < 1 || n_ls > 20 || !d || !xnext_all || !x0 || !lam || !rho || !Qd || !q || !u_lo ||
        !u_hi || !z || !phi_prev)
        return ALQP_E_BADARG;
    AuxArgs<real> a = {};
    if (!set_obstacles<real>(dims, obs, a)) return ALQP_E_BADARG;
    a.B = dims->B; a.T = dims->T; a.nx = dims->nx; a.nu = dims->nu; a.n_ls = n_ls;
    a.d = (const real *)d; a.xnext = (const real *)xnext_all; a.x0 = (const real *)x0;
    a.lam = (const real *)lam; a.rho = (const real *)rho; a.Qd = (const real *)Qd; a.q = (const real *)q;
    a.ulo = (const real *)u_lo; a.uhi = (const real *)u_hi; a.sb_u = sb_u; a.st_u = st_u;
    a.z = (real *)z; a.phi_prev = (real *)phi_prev; a.rnorm2 = (real *)rnorm2; a.phi = (real *)phi_all;
    a.k_out = k_out; a.accept_out = accept_out;
    hipLaunchKernelGGL(k_merit_pick<real>, dim3(dims->B), dim3(64), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : ALQP_E_LAUNCH;
}

template <typename real>
int pick_impl(const AlqpDims *dims, int n_ls, const void *phi, void *phi_prev, const void *d, void *z,
              int *k_out, int *accept_out, void *stream) {
    if (!dims_ok(dims) || n_ls < 1 || !phi || !phi_prev || !d || !z) return ALQP_E_BADARG;
    AuxArgs<real> a = {};
    a.B = dims->B; a.T = dims->T; a.nx = dims->nx; a.nu = dims->nu; a.n_ls = n_ls;
    a.phi_all = (const real *)phi; a.phi_prev = (real *)phi_prev; a.d = (const real *)d; a.z = (real *)z;
    a.k_out = k_out; a.accept_out = accept_out;
    hipLaunchKernelGGL(k_pick<real>, dim3(dims->B), dim3(64), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : ALQP_E_LAUNCH;
}

template <typename real>
int dual_impl(const AlqpDims *dims, const void *z, const void *xnext, const void *x0, const void *u_lo,
              const void *u_hi, long sb_u, long st_u, const AlqpObstacles *obs, void *lam, void *rho,
              double rho_scale, void *stream) {
    if (!dims_ok(dims) || !z || !xnext || !x0 || !u_lo || !u_hi || !lam || !rho) return ALQP_E_BADARG;
    AuxArgs<real> a = {};
    if (!set_obstacles<real>(dims, obs, a)) return ALQP_E_BADARG;
    a.B = dims->B; a.T = dims->T; a.nx = dims->nx; a.nu = dims->nu;
    a.zc = (const real *)z; a.xnext = (const real *)xnext; a.x0 = (const real *)x0;
    a.ulo = (const real *)u_lo; a.uhi = (const real *)u_hi; a.sb_u = sb_u; a.st_u = st_u;
    a.lam_io = (real *)lam; a.rho_io = (real *)rho; a.rho_scale = (real)rho_scale;
    hipLaunchKernelGGL(k_dual<real>, dim3(dims->B), dim3(64), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : ALQP_E_LAUNCH;
}

// ---- the same three with more rows per stage, for MPC with a callable dx: state box rows xlo[t] <= x_t <= xhi[t]
// (x_lower=, x_upper=; flag XB), general rows G_t z_t <= h_t (ineqG=, ineqh=; flag PL), and merit and pick with a dense stage
// cost 1/2 z_t' C_t z_t + q_t' z_t (diag_cost=False; flag DENSE) -------------------------------------------------------------
// One body for merit and one for the dual update (merit_body, dual_body), templated on the flags and on the argument type,
// and three families of __global__ kernels that are one-line wrappers of the bodies, each family with an argument type of its
// own: _xbox (XboxAuxArgs; XB), _rows<XB> (RowsAuxArgs; PL) and _dense<XB, PL> (DenseAuxArgs; DENSE). The flags are template
// parameters, so every choice is wave-uniform and costs the other builds nothing; a body touches the members that only some
// of the types have (Qd, C, G, h, m) inside `if constexpr`. AuxArgs and the kernels above take no part in this. No obstacle
// rows and no state-estimator row set (obs / nobs / obs_r2 / no_init of the base are unused).
// Multipliers per stage [u - uhi | -u + ulo | (x - xhi | -x + xlo) | (G_t z_t - h_t)], stage stride 2 nu + XR + (PL ? m : 0)
// with XR = 2 nx when there are state bounds and 0 when there are none (Team's XBOX / POLY layout). A state bound is addressed
// b sb_x + t st_x + i; row k of stage t of instance b is read in place at G + b sb_g + t st_g + k n, its right-hand side at
// h + b sb_h + t st_h + k. State rows and general rows follow the control rows' conventions
// (tests/poly_rows_reference.py:poly_rows): lam r with the unclamped r plus rho/2 max(r, 0)^2 in the merit, max(r, 0)^2 in
// rnorm2, max(0, lam + rho r) in the dual update; stage 0 included.
// General rows, lanes and rows: a lane per row (row e = t m + k to lane e mod 64), the n-long dot product inside the lane in
// the order j = 0 .. n-1. n is at most 17 at the compiled sizes, so spreading one row over lanes would leave three quarters of
// the wavefront idle and pay a cross-lane reduction per row, and the sum's order would depend on the lane split; with a lane
// per row the 64 lanes read 64 consecutive rows of a stage's [m][n] block, n loads of stride n words that together use every
// byte of the cache lines they touch, z_t comes as a broadcast (every lane of a stage reads the same address), and the only
// cross-lane step is the wave_sum the kernels take anyway. Any m in 1..64, T m below or above 64 (the row loop strides 64).
// The dense cost term, a lane per element: element e = t n + i (lane e mod 64) reads row i of C_t once, n consecutive words,
// and forms (C_t z_t)_i in the order j = 0 .. n-1 with z_t as a broadcast; 64 lanes cover consecutive rows, so every byte of
// the lines they touch is used, and the sum's order does not depend on a lane split (the lane-per-row reasoning of the rows).
// The dual update reads no cost and has no _dense kernels.
template <typename real>
struct XboxAuxArgs : AuxArgs<real> {
    const real *xlo, *xhi;   // [nx] (sb_x = st_x = 0) or [B][T][nx] (sb_x = T nx, st_x = nx)
    long sb_x, st_x;
};

template <typename real>
struct RowsAuxArgs : XboxAuxArgs<real> {
    const real *G, *h;
    int m;
    long sb_g, st_g;
    long sb_h, st_h;
};

// RowsAuxArgs with C ([B][T][n][n] row-major, symmetric) where Qd stood, without the fields no _dense kernel reads
template <typename real>
struct DenseAuxArgs {
    int B, T, nx, nu, K, n_ls;
    const real *zc, *xnext, *x0, *lam, *rho, *C, *q, *ulo, *uhi;
    long sb_u, st_u;
    const real *xlo, *xhi;
    long sb_x, st_x;
    const real *G, *h;
    int m;
    long sb_g, st_g;
    long sb_h, st_h;
    real *phi, *rnorm2;
    // pick
    const real *d;
    real *phi_prev, *z;
    int *k_out, *accept_out;
};

// k_merit's statements; Args by value, like a kernel's argument
template <typename real, bool DENSE, bool XB, bool PL, typename Args>
__device__ __forceinline__ void merit_body(Args a) {
    const int lane = threadIdx.x;
    const int b = blockIdx.x % a.B, kk = blockIdx.x / a.B;
    const int T = a.T, nx = a.nx, nu = a.nu, n = nx + nu, neq = T * nx;
    int m = 0;
    if constexpr (PL) m = a.m;
    const real *z = a.zc + ((size_t)kk * a.B + b) * T * n;
    const real *xn = a.xnext + ((size_t)kk * a.B + b) * (T - 1) * nx;
    const int xr = XB ? 2 * nx : 0, nit = 2 * nu + xr + m;   // inequality rows per stage
    const real *lam = a.lam + (size_t)b * ((size_t)neq + (size_t)T * nit);
    const real *cost;   // C_t blocks when DENSE, the diagonal otherwise
    if constexpr (DENSE) cost = a.C + (size_t)b * T * n * n;
    else cost = a.Qd + (size_t)b * T * n;
    const real *q = a.q + (size_t)b * T * n;
    const real *ulo = a.ulo + (size_t)b * a.sb_u, *uhi = a.uhi + (size_t)b * a.sb_u;
    const real *xlo = XB ? a.xlo + (size_t)b * a.sb_x : nullptr, *xhi = XB ? a.xhi + (size_t)b * a.sb_x : nullptr;
    const real rho = a.rho[b];
    real acc = 0, sq = 0;
    for (int e = lane; e < T * n; e += 64) {
        int t = e / n, j = e - t * n;
        real v = z[e];
        if constexpr (DENSE) {
            // row j of C_t (C_t is the t-th n x n block: row e of the [T n][n] image) against z_t
            const real *c = cost + (size_t)e * n, *zt = z + t * n;
            real cz = 0;
            for (int i = 0; i < n; ++i) cz += c[i] * zt[i];
            acc += (real(0.5) * cz + q[e]) * v;
        } else {
            acc += (real(0.5) * cost[e] * v + q[e]) * v;
        }
        // the element's two box rows: control rows at [0, 2 nu) of the stage, state rows (XB) at [2 nu, 2 nu + 2 nx)
        const bool isu = j >= nx;
        if (XB || isu) {
            const int jj = isu ? j - nx : j, w = isu ? nu : nx;
            real bh, bl;
            if constexpr (XB) {
                bh = isu ? uhi[t * a.st_u + jj] : xhi[t * a.st_x + jj];
                bl = isu ? ulo[t * a.st_u + jj] : xlo[t * a.st_x + jj];
            } else {
                bh = uhi[t * a.st_u + jj];
                bl = ulo[t * a.st_u + jj];
            }
            real vu = v - bh, vl = -v + bl;
            real cu = vu > 0 ? vu : real(0), cl = vl > 0 ? vl : real(0);
            int ru = neq + t * nit + (isu ? 0 : 2 * nu) + jj;
            acc += lam[ru] * vu + lam[ru + w] * vl;
            sq += cu * cu + cl * cl;
        }
    }
    for (int e = lane; e < neq; e += 64) {
        int t = e / nx, i = e - t * nx;
        real r = (t < T - 1) ? z[(t + 1) * n + i] - xn[t * nx + i] : z[i] - a.x0[(size_t)b * nx + i];
        acc += lam[e] * r;
        sq += r * r;
    }
    if constexpr (PL) {   // general rows: a lane per row
        const real *Gb = a.G + (size_t)b * a.sb_g, *hb = a.h + (size_t)b * a.sb_h;
        for (int e = lane; e < T * m; e += 64) {
            const int t = e / m, k = e - t * m;
            const real *g = Gb + (size_t)t * a.st_g + (size_t)k * n, *zt = z + t * n;
            real s = 0;
            for (int j = 0; j < n; ++j) s += g[j] * zt[j];
            const real r = s - hb[(size_t)t * a.st_h + k], p = r > 0 ? r : real(0);
            acc += lam[neq + t * nit + 2 * nu + xr + k] * r;
            sq += p * p;
        }
    }
    acc = wave_sum(acc);
    sq = wave_sum(sq);
    if (lane == 0) {
        a.phi[(size_t)kk * a.B + b] = acc + real(0.5) * rho * sq;
        if (a.rnorm2) a.rnorm2[(size_t)kk * a.B + b] = sq;
    }
}

// k_dual's statements
template <typename real, bool XB, bool PL, typename Args>
__device__ __forceinline__ void dual_body(Args a) {
    const int lane = threadIdx.x, b = blockIdx.x;
    const int T = a.T, nx = a.nx, nu = a.nu, n = nx + nu, neq = T * nx;
    int m = 0;
    if constexpr (PL) m = a.m;
    const real *z = a.zc + (size_t)b * T * n;
    const real *xn = a.xnext + (size_t)b * (T - 1) * nx;
    const int xr = XB ? 2 * nx : 0, nit = 2 * nu + xr + m;
    real *lam = a.lam_io + (size_t)b * ((size_t)neq + (size_t)T * nit);
    const real *ulo = a.ulo + (size_t)b * a.sb_u, *uhi = a.uhi + (size_t)b * a.sb_u;
    const real rho = a.rho_io[b];
    for (int e = lane; e < neq; e += 64) {
        int t = e / nx, i = e - t * nx;
        real r = (t < T - 1) ? z[(t + 1) * n + i] - xn[t * nx + i] : z[i] - a.x0[(size_t)b * nx + i];
        lam[e] += rho * r;
    }
    for (int e = lane; e < T * nu; e += 64) {
        int t = e / nu, j = e - t * nu;
        real u = z[t * n + nx + j];
        int ru = neq + t * nit + j, rl = ru + nu;
        real v1 = lam[ru] + rho * (u - uhi[t * a.st_u + j]);
        real v2 = lam[rl] + rho * (-u + ulo[t * a.st_u + j]);
        lam[ru] = v1 < 0 ? real(0) : v1;
        lam[rl] = v2 < 0 ? real(0) : v2;
    }
    if constexpr (XB) {
        const real *xlo = a.xlo + (size_t)b * a.sb_x, *xhi = a.xhi + (size_t)b * a.sb_x;
        for (int e = lane; e < T * nx; e += 64) {
            int t = e / nx, i = e - t * nx;
            real x = z[t * n + i];
            int ru = neq + t * nit + 2 * nu + i, rl = ru + nx;
            real v1 = lam[ru] + rho * (x - xhi[t * a.st_x + i]);
            real v2 = lam[rl] + rho * (-x + xlo[t * a.st_x + i]);
            lam[ru] = v1 < 0 ? real(0) : v1;
            lam[rl] = v2 < 0 ? real(0) : v2;
        }
    }
    if constexpr (PL) {
        const real *Gb = a.G + (size_t)b * a.sb_g, *hb = a.h + (size_t)b * a.sb_h;
        for (int e = lane; e < T * m; e += 64) {
            const int t = e / m, k = e - t * m;
            const real *g = Gb + (size_t)t * a.st_g + (size_t)k * n, *zt = z + t * n;
            real s = 0;
            for (int j = 0; j < n; ++j) s += g[j] * zt[j];
            const int row = neq + t * nit + 2 * nu + xr + k;
            const real v = lam[row] + rho * (s - hb[(size_t)t * a.st_h + k]);
            lam[row] = v < 0 ? real(0) : v;
        }
    }
    __syncthreads();
    if (lane == 0) a.rho_io[b] = rho * a.rho_scale;
}

template <typename real>
__global__ __launch_bounds__(64) void k_merit_xbox(XboxAuxArgs<real> a) { merit_body<real, false, true, false>(a); }
template <typename real>
__global__ __launch_bounds__(64) void k_dual_xbox(XboxAuxArgs<real> a) { dual_body<real, true, false>(a); }

template <typename real, bool XB>
__global__ __launch_bounds__(64) void k_merit_rows(RowsAuxArgs<real> a) { merit_body<real, false, XB, true>(a); }
template <typename real, bool XB>
__global__ __launch_bounds__(64) void k_dual_rows(RowsAuxArgs<real> a) { dual_body<real, XB, true>(a); }

template <typename real, bool XB, bool PL>
__global__ __launch_bounds__(64) void k_merit_dense(DenseAuxArgs<real> a) { merit_body<real, true, XB, PL>(a); }

// The pick kernels of the three families keep a body each. Unrolled over the 20 candidates they sit at the SGPR limit, and
// their register allocation does not survive the detour through an inlined body: with these very statements in a shared
// body the VGPR counts move in 8 of the 14 instantiations and k_merit_pick_xbox<float> drops from 6 to 5 waves per SIMD
// (profiles/r18/README.md). A change to the merit conventions goes into merit_body and into these three.

// k_merit_pick with the state rows: a state element gets what a control element gets, its two bounds and two multipliers
// loaded once and all 20 candidates from registers.
template <typename real>
__global__ __launch_bounds__(64) void k_merit_pick_xbox(XboxAuxArgs<real> a) {
    const int lane = threadIdx.x, b = blockIdx.x;
    const int T = a.T, nx = a.nx, nu = a.nu, n = nx + nu, neq = T * nx, nit = 2 * nu + 2 * nx;
    real *z = a.z + (size_t)b * T * n;
    const real *d = a.d + (size_t)b * T * n;
    const real *lam = a.lam + (size_t)b * ((size_t)neq + (size_t)T * nit);
    const real *Qd = a.Qd + (size_t)b * T * n, *q = a.q + (size_t)b * T * n;
    const real *ulo = a.ulo + (size_t)b * a.sb_u, *uhi = a.uhi + (size_t)b * a.sb_u;
    const real *xlo = a.xlo + (size_t)b * a.sb_x, *xhi = a.xhi + (size_t)b * a.sb_x;
    const real rho = a.rho[b];
    real acc[20], sq[20];
#pragma unroll
    for (int k = 0; k < 20; ++k) { acc[k] = 0; sq[k] = 0; }
    // cost + box rows (controls and states): every lane walks its elements once, all candidates from registers
    for (int e = lane; e < T * n; e += 64) {
        const int t = e / n, j = e - t * n;
        const real zv = z[e], dv = d[e], Qv = Qd[e], qv = q[e];
        const bool isu = j >= nx;
        const int jj = isu ? j - nx : j, w = isu ? nu : nx;
        const int ru = neq + t * nit + (isu ? 0 : 2 * nu) + jj;
        const real bu = isu ? uhi[t * a.st_u + jj] : xhi[t * a.st_x + jj];
        const real bl = isu ? ulo[t * a.st_u + jj] : xlo[t * a.st_x + jj];
        const real lu = lam[ru], ll = lam[ru + w];
        real alpha = 1;
#pragma unroll
        for (int k = 0; k < 20; ++k) {
            const real v = zv + alpha * dv;
            acc[k] += (real(0.5) * Qv * v + qv) * v;
            const real vu = v - bu, vl = -v + bl;
            const real cu = vu > 0 ? vu : real(0), cl = vl > 0 ? vl : real(0);
            acc[k] += lu * vu + ll * vl;
            sq[k] += cu * cu + cl * cl;
            alpha *= real(0.5);
        }
    }
    // equality rows: r = x_{t+1}(candidate) - xnext_k, init rows x_0 - x0
    for (int e = lane; e < neq; e += 64) {
        const int t = e / nx, i = e - t * nx;
        const real le = lam[e];
        const int zi = (t < T - 1) ? (t + 1) * n + i : i;
        const real zv = z[zi], dv = d[zi];
        const real x0v = (t < T - 1) ? real(0) : a.x0[(size_t)b * nx + i];
        real alpha = 1;
#pragma unroll
        for (int k = 0; k < 20; ++k) {
            if (k < a.n_ls) {
                const real ref = (t < T - 1) ? a.xnext[(((size_t)k * a.B + b) * (T - 1) + t) * nx + i] : x0v;
                const real r = zv + alpha * dv - ref;
                acc[k] += le * r;
                sq[k] += r * r;
            }
            alpha *= real(0.5);
        }
    }
    int kbest = 0;
    real best = 0, sqbest = 0;
#pragma unroll
    for (int k = 0; k < 20; ++k) {
        if (k < a.n_ls) {
            const real s2 = wave_sum(sq[k]);
            const real v = wave_sum(acc[k]) + real(0.5) * rho * s2;
            if (a.phi) a.phi[(size_t)k * a.B + b] = v;     // (all lanes hold the same value)
            if (k == 0) { best = v; sqbest = s2; }
            else if (!(best != best) && (v != v || v < best)) { best = v; kbest = k; sqbest = s2; }
        }
    }
    const real prev = a.phi_prev[b];
    const bool ok = best < prev;
    if (ok) {
        const real alpha = real(1) / real(1 << kbest);
        for (int e = lane; e < T * n; e += 64) z[e] += alpha * d[e];
    }
    if (lane == 0) {
        a.phi_prev[b] = best;
        if (a.k_out) a.k_out[b] = kbest;
        if (a.accept_out) a.accept_out[b] = ok ? 1 : 0;
        if (a.rnorm2 && ok) a.rnorm2[b] = sqbest;
    }
}

// k_merit_pick with the rows. A row is affine in the step length: one pass over G_k gives r0 = G_k . z_t - h_k and
// gd = G_k . d_t, and the 20 candidates r0 + alpha gd come from registers like the box rows' candidates.
template <typename real, bool XB>
__global__ __launch_bounds__(64) void k_merit_pick_rows(RowsAuxArgs<real> a) {
    const int lane = threadIdx.x, b = blockIdx.x;
    const int T = a.T, nx = a.nx, nu = a.nu, n = nx + nu, neq = T * nx, m = a.m;
    const int xr = XB ? 2 * nx : 0, nit = 2 * nu + xr + m;
    real *z = a.z + (size_t)b * T * n;
    const real *d = a.d + (size_t)b * T * n;
    const real *lam = a.lam + (size_t)b * ((size_t)neq + (size_t)T * nit);
    const real *Qd = a.Qd + (size_t)b * T * n, *q = a.q + (size_t)b * T * n;
    const real *ulo = a.ulo + (size_t)b * a.sb_u, *uhi = a.uhi + (size_t)b * a.sb_u;
    const real *xlo = XB ? a.xlo + (size_t)b * a.sb_x : nullptr, *xhi = XB ? a.xhi + (size_t)b * a.sb_x : nullptr;
    const real *Gb = a.G + (size_t)b * a.sb_g, *hb = a.h + (size_t)b * a.sb_h;
    const real rho = a.rho[b];
    real acc[20], sq[20];
#pragma unroll
    for (int k = 0; k < 20; ++k) { acc[k] = 0; sq[k] = 0; }
    // cost + box rows (controls, and states when XB): every lane walks its elements once, all candidates from registers
    for (int e = lane; e < T * n; e += 64) {
        const int t = e / n, j = e - t * n;
        const real zv = z[e], dv = d[e], Qv = Qd[e], qv = q[e];
        real bu = 0, bl = 0, lu = 0, ll = 0;
        const bool isu = j >= nx;
        const bool has = XB || isu;
        if (has) {
            const int jj = isu ? j - nx : j, w = isu ? nu : nx;
            const int ru = neq + t * nit + (isu ? 0 : 2 * nu) + jj;
            if constexpr (XB) {
                bu = isu ? uhi[t * a.st_u + jj] : xhi[t * a.st_x + jj];
                bl = isu ? ulo[t * a.st_u + jj] : xlo[t * a.st_x + jj];
            } else {
                bu = uhi[t * a.st_u + jj];
                bl = ulo[t * a.st_u + jj];
            }
            lu = lam[ru]; ll = lam[ru + w];
        }
        real alpha = 1;
#pragma unroll
        for (int k = 0; k < 20; ++k) {
            const real v = zv + alpha * dv;
            acc[k] += (real(0.5) * Qv * v + qv) * v;
            if (has) {
                const real vu = v - bu, vl = -v + bl;
                const real cu = vu > 0 ? vu : real(0), cl = vl > 0 ? vl : real(0);
                acc[k] += lu * vu + ll * vl;
                sq[k] += cu * cu + cl * cl;
            }
            alpha *= real(0.5);
        }
    }
    // equality rows: r = x_{t+1}(candidate) - xnext_k, init rows x_0 - x0
    for (int e = lane; e < neq; e += 64) {
        const int t = e / nx, i = e - t * nx;
        const real le = lam[e];
        const int zi = (t < T - 1) ? (t + 1) * n + i : i;
        const real zv = z[zi], dv = d[zi];
        const real x0v = (t < T - 1) ? real(0) : a.x0[(size_t)b * nx + i];
        real alpha = 1;
#pragma unroll
        for (int k = 0; k < 20; ++k) {
            if (k < a.n_ls) {
                const real ref = (t < T - 1) ? a.xnext[(((size_t)k * a.B + b) * (T - 1) + t) * nx + i] : x0v;
                const real r = zv + alpha * dv - ref;
                acc[k] += le * r;
                sq[k] += r * r;
            }
            alpha *= real(0.5);
        }
    }
    // general rows: a lane per row, one pass over G_k for both dot products
    for (int e = lane; e < T * m; e += 64) {
        const int t = e / m, k = e - t * m;
        const real *g = Gb + (size_t)t * a.st_g + (size_t)k * n, *zt = z + t * n, *dt = d + t * n;
        real sz = 0, gd = 0;
        for (int j = 0; j < n; ++j) {
            const real gj = g[j];
            sz += gj * zt[j];
            gd += gj * dt[j];
        }
        const real r0 = sz - hb[(size_t)t * a.st_h + k];
        const real lk = lam[neq + t * nit + 2 * nu + xr + k];
        real alpha = 1;
#pragma unroll
        for (int c = 0; c < 20; ++c) {
            const real r = r0 + alpha * gd, p = r > 0 ? r : real(0);
            acc[c] += lk * r;
            sq[c] += p * p;
            alpha *= real(0.5);
        }
    }
    int kbest = 0;
    real best = 0, sqbest = 0;
#pragma unroll
    for (int k = 0; k < 20; ++k) {
        if (k < a.n_ls) {
            const real s2 = wave_sum(sq[k]);
            const real v = wave_sum(acc[k]) + real(0.5) * rho * s2;
            if (a.phi) a.phi[(size_t)k * a.B + b] = v;     // (all lanes hold the same value)
            if (k == 0) { best = v; sqbest = s2; }
            else if (!(best != best) && (v != v || v < best)) { best = v; kbest = k; sqbest = s2; }
        }
    }
    const real prev = a.phi_prev[b];
    const bool ok = best < prev;
    if (ok) {
        const real alpha = real(1) / real(1 << kbest);
        for (int e = lane; e < T * n; e += 64) z[e] += alpha * d[e];
    }
    if (lane == 0) {
        a.phi_prev[b] = best;
        if (a.k_out) a.k_out[b] = kbest;
        if (a.accept_out) a.accept_out[b] = ok ? 1 : 0;
        if (a.rnorm2 && ok) a.rnorm2[b] = sqbest;
    }
}

// k_merit_pick with the dense cost. The cost is quadratic in the step length, and row i of C_t is read ONCE for all n_ls
// candidates: one pass gives cz = C_t[i,:] . z_t and cd = C_t[i,:] . d_t, and candidate alpha is
// (1/2 (cz + alpha cd) + q_i) (z_i + alpha d_i) from registers, like a general row's r0 + alpha gd. (n is a run-time number
// in these size-generic kernels, so a row held in registers for a dot product per candidate would need an array of the
// largest n and 20 n-long passes; two scalars cost two registers at any n.)
template <typename real, bool XB, bool PL>
__global__ __launch_bounds__(64) void k_merit_pick_dense(DenseAuxArgs<real> a) {
    const int lane = threadIdx.x, b = blockIdx.x;
    const int T = a.T, nx = a.nx, nu = a.nu, n = nx + nu, neq = T * nx, m = PL ? a.m : 0;
    const int xr = XB ? 2 * nx : 0, nit = 2 * nu + xr + m;
    real *z = a.z + (size_t)b * T * n;
    const real *d = a.d + (size_t)b * T * n;
    const real *lam = a.lam + (size_t)b * ((size_t)neq + (size_t)T * nit);
    const real *Cb = a.C + (size_t)b * T * n * n, *q = a.q + (size_t)b * T * n;
    const real *ulo = a.ulo + (size_t)b * a.sb_u, *uhi = a.uhi + (size_t)b * a.sb_u;
    const real *xlo = XB ? a.xlo + (size_t)b * a.sb_x : nullptr, *xhi = XB ? a.xhi + (size_t)b * a.sb_x : nullptr;
    const real rho = a.rho[b];
    real acc[20], sq[20];
#pragma unroll
    for (int k = 0; k < 20; ++k) { acc[k] = 0; sq[k] = 0; }
    // cost + box rows (controls, and states when XB): every lane walks its elements once, all candidates from registers
    for (int e = lane; e < T * n; e += 64) {
        const int t = e / n, j = e - t * n;
        const real zv = z[e], dv = d[e], qv = q[e];
        const real *c = Cb + (size_t)e * n, *zt = z + t * n, *dt = d + t * n;
        real cz = 0, cd = 0;
        for (int i = 0; i < n; ++i) {
            const real ci = c[i];
            cz += ci * zt[i];
            cd += ci * dt[i];
        }
        real bu = 0, bl = 0, lu = 0, ll = 0;
        const bool isu = j >= nx;
        const bool has = XB || isu;
        if (has) {
            const int jj = isu ? j - nx : j, w = isu ? nu : nx;
            const int ru = neq + t * nit + (isu ? 0 : 2 * nu) + jj;
            if constexpr (XB) {
                bu = isu ? uhi[t * a.st_u + jj] : xhi[t * a.st_x + jj];
                bl = isu ? ulo[t * a.st_u + jj] : xlo[t * a.st_x + jj];
            } else {
                bu = uhi[t * a.st_u + jj];
                bl = ulo[t * a.st_u + jj];
            }
            lu = lam[ru]; ll = lam[ru + w];
        }
        real alpha = 1;
#pragma unroll
        for (int k = 0; k < 20; ++k) {
            const real v = zv + alpha * dv;
            acc[k] += (real(0.5) * (cz + alpha * cd) + qv) * v;
            if (has) {
                const real vu = v - bu, vl = -v + bl;
                const real cu = vu > 0 ? vu : real(0), cl = vl > 0 ? vl : real(0);
                acc[k] += lu * vu + ll * vl;
                sq[k] += cu * cu + cl * cl;
            }
            alpha *= real(0.5);
        }
    }
    // equality rows: r = x_{t+1}(candidate) - xnext_k, init rows x_0 - x0
    for (int e = lane; e < neq; e += 64) {
        const int t = e / nx, i = e - t * nx;
        const real le = lam[e];
        const int zi = (t < T - 1) ? (t + 1) * n + i : i;
        const real zv = z[zi], dv = d[zi];
        const real x0v = (t < T - 1) ? real(0) : a.x0[(size_t)b * nx + i];
        real alpha = 1;
#pragma unroll
        for (int k = 0; k < 20; ++k) {
            if (k < a.n_ls) {
                const real ref = (t < T - 1) ? a.xnext[(((size_t)k * a.B + b) * (T - 1) + t) * nx + i] : x0v;
                const real r = zv + alpha * dv - ref;
                acc[k] += le * r;
                sq[k] += r * r;
            }
            alpha *= real(0.5);
        }
    }
    if constexpr (PL) {   // general rows: a lane per row, one pass over G_k for both dot products
        const real *Gb = a.G + (size_t)b * a.sb_g, *hb = a.h + (size_t)b * a.sb_h;
        for (int e = lane; e < T * m; e += 64) {
            const int t = e / m, k = e - t * m;
            const real *g = Gb + (size_t)t * a.st_g + (size_t)k * n, *zt = z + t * n, *dt = d + t * n;
            real sz = 0, gd = 0;
            for (int j = 0; j < n; ++j) {
                const real gj = g[j];
                sz += gj * zt[j];
                gd += gj * dt[j];
            }
            const real r0 = sz - hb[(size_t)t * a.st_h + k];
            const real lk = lam[neq + t * nit + 2 * nu + xr + k];
            real alpha = 1;
#pragma unroll
            for (int c = 0; c < 20; ++c) {
                const real r = r0 + alpha * gd, p = r > 0 ? r : real(0);
                acc[c] += lk * r;
                sq[c] += p * p;
                alpha *= real(0.5);
            }
        }
    }
    int kbest = 0;
    real best = 0, sqbest = 0;
#pragma unroll
    for (int k = 0; k < 20; ++k) {
        if (k < a.n_ls) {
            const real s2 = wave_sum(sq[k]);
            const real v = wave_sum(acc[k]) + real(0.5) * rho * s2;
            if (a.phi) a.phi[(size_t)k * a.B + b] = v;     // (all lanes hold the same value)
            if (k == 0) { best = v; sqbest = s2; }
            else if (!(best != best) && (v != v || v < best)) { best = v; kbest = k; sqbest = s2; }
        }
    }
    const real prev = a.phi_prev[b];
    const bool ok = best < prev;
    if (ok) {
        const real alpha = real(1) / real(1 << kbest);
        for (int e = lane; e < T * n; e += 64) z[e] += alpha * d[e];
    }
    if (lane == 0) {
        a.phi_prev[b] = best;
        if (a.k_out) a.k_out[b] = kbest;
        if (a.accept_out) a.accept_out[b] = ok ? 1 : 0;
        if (a.rnorm2 && ok) a.rnorm2[b] = sqbest;
    }
}

// A family's kernels of one operation by [XB][PL]; null where the family's argument checks rule the combination out
template <typename Args>
using AuxKernels = void (*const[2][2])(Args);
#define ALQP_AUX_TABLE(NAME, ARGS, ...) \
    template <typename real>            \
    constexpr AuxKernels<ARGS<real>> NAME = {__VA_ARGS__}
ALQP_AUX_TABLE(kMeritXbox, XboxAuxArgs, {nullptr, nullptr}, {k_merit_xbox<real>, nullptr});
ALQP_AUX_TABLE(kMeritPickXbox, XboxAuxArgs, {nullptr, nullptr}, {k_merit_pick_xbox<real>, nullptr});
ALQP_AUX_TABLE(kDualXbox, XboxAuxArgs, {nullptr, nullptr}, {k_dual_xbox<real>, nullptr});
ALQP_AUX_TABLE(kMeritRows, RowsAuxArgs, {nullptr, k_merit_rows<real, false>}, {nullptr, k_merit_rows<real, true>});
ALQP_AUX_TABLE(kMeritPickRows, RowsAuxArgs, {nullptr, k_merit_pick_rows<real, false>}, {nullptr, k_merit_pick_rows<real, true>});
ALQP_AUX_TABLE(kDualRows, RowsAuxArgs, {nullptr, k_dual_rows<real, false>}, {nullptr, k_dual_rows<real, true>});
ALQP_AUX_TABLE(kMeritDense, DenseAuxArgs, {k_merit_dense<real, false, false>, k_merit_dense<real, false, true>},
               {k_merit_dense<real, true, false>, k_merit_dense<real, true, true>});
ALQP_AUX_TABLE(kMeritPickDense, DenseAuxArgs, {k_merit_pick_dense<real, false, false>, k_merit_pick_dense<real, false, true>},
               {k_merit_pick_dense<real, true, false>, k_merit_pick_dense<real, true, true>});
#undef ALQP_AUX_TABLE

// the _xbox arguments, then G, h, m and the four strides right behind the state-bound arguments: what the _rows and _dense
// entry points take, and the _xbox ones with no rows (G, h null, m = 0)
#define ALQP_ROWS_PARAMS                                                                              \
    const void *x_lo, const void *x_hi, long sb_x, long st_x, const void *G, const void *h, int m,    \
    long sb_g, long st_g, long sb_h, long st_h
#define ALQP_ROWS_ARGS x_lo, x_hi, sb_x, st_x, G, h, m, sb_g, st_g, sb_h, st_h

// What the entry points of the three families fill alike, with each family's checks; false: ALQP_E_BADARG. _xbox: both state
// bounds. _rows: x_lo and x_hi both null (no state bounds) or neither, G, h and m in 1..64. _dense: the same state bounds;
// G and h both null with m == 0 (no general rows) or neither. `cost` (Qd, or C for _dense) is filled unchecked.
template <typename real, typename Args>
bool set_rows_aux(const AlqpDims *dims, const void *x0, const void *cost, const void *u_lo, const void *u_hi, long sb_u,
                  long st_u, ALQP_ROWS_PARAMS, Args &a) {
    constexpr bool kXbox = std::is_same_v<Args, XboxAuxArgs<real>>, kDense = std::is_same_v<Args, DenseAuxArgs<real>>;
    if (!dims_ok(dims) || !x0 || !u_lo || !u_hi || sb_x < 0 || st_x < 0) return false;
    if (kXbox ? (!x_lo || !x_hi) : (!x_lo != !x_hi)) return false;
    a.B = dims->B; a.T = dims->T; a.nx = dims->nx; a.nu = dims->nu;
    a.x0 = (const real *)x0;
    a.ulo = (const real *)u_lo; a.uhi = (const real *)u_hi; a.sb_u = sb_u; a.st_u = st_u;
    a.xlo = (const real *)x_lo; a.xhi = (const real *)x_hi; a.sb_x = sb_x; a.st_x = st_x;
    if constexpr (kDense) a.C = (const real *)cost;
    else a.Qd = (const real *)cost;
    if constexpr (!kXbox) {
        if (kDense ? (!G != !h || (G ? (m < 1 || m > 64) : m != 0)) : (!G || !h || m < 1 || m > 64)) return false;
        if (sb_g < 0 || st_g < 0 || sb_h < 0 || st_h < 0) return false;
        a.G = (const real *)G; a.h = (const real *)h; a.m = m;
        a.sb_g = sb_g; a.st_g = st_g; a.sb_h = sb_h; a.st_h = st_h;
    }
    return true;
}

// launches kern[XB][PL] with XB = (x_lo != null), PL = (G != null)
template <typename Args>
int launch_aux(AuxKernels<Args> &kern, const void *x_lo, const void *G, dim3 grid, void *stream, const Args &a) {
    hipLaunchKernelGGL(kern[x_lo != nullptr][G != nullptr], grid, dim3(64), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : ALQP_E_LAUNCH;
}

template <typename real, typename Args>
int merit_ext_impl(AuxKernels<Args> &kern, const AlqpDims *dims, int K, const void *zc, const void *xnext, const void *x0,
                   const void *lam, const void *rho, const void *cost, const void *q, const void *u_lo, const void *u_hi,
                   long sb_u, long st_u, ALQP_ROWS_PARAMS, void *phi, void *rnorm2, void *stream) {
    Args a = {};
    if (!set_rows_aux<real>(dims, x0, cost, u_lo, u_hi, sb_u, st_u, ALQP_ROWS_ARGS, a) || K < 1 || !zc || !xnext || !lam ||
        !rho || !cost || !q || !phi)
        return ALQP_E_BADARG;
    a.K = K;
    a.zc = (const real *)zc; a.xnext = (const real *)xnext;
    a.lam = (const real *)lam; a.rho = (const real *)rho; a.q = (const real *)q;
    a.phi = (real *)phi; a.rnorm2 = (real *)rnorm2;
    return launch_aux(kern, x_lo, G, dim3((unsigned)((size_t)K * dims->B)), stream, a);
}

template <typename real, typename Args>
int merit_pick_ext_impl(AuxKernels<Args> &kern, const AlqpDims *dims, int n_ls, const void *d, const void *xnext_all,
                        const void *x0, const void *lam, const void *rho, const void *cost, const void *q, const void *u_lo,
                        const void *u_hi, long sb_u, long st_u, ALQP_ROWS_PARAMS, void *z, void *phi_prev, void *rnorm2,
                        void *phi_all, int *k_out, int *accept_out, void *stream) {
    Args a = {};
    if (!set_rows_aux<real>(dims, x0, cost, u_lo, u_hi, sb_u, st_u, ALQP_ROWS_ARGS, a) || n_ls < 1 || n_ls > 20 || !d ||
        !xnext_all || !lam || !rho || !cost || !q || !z || !phi_prev)
        return ALQP_E_BADARG;
    a.n_ls = n_ls;
    a.d = (const real *)d; a.xnext = (const real *)xnext_all;
    a.lam = (const real *)lam; a.rho = (const real *)rho; a.q = (const real *)q;
    a.z = (real *)z; a.phi_prev = (real *)phi_prev; a.rnorm2 = (real *)rnorm2; a.phi = (real *)phi_all;
    a.k_out = k_out; a.accept_out = accept_out;
    return launch_aux(kern, x_lo, G, dim3(dims->B), stream, a);
}

template <typename real, typename Args>
int dual_ext_impl(AuxKernels<Args> &kern, const AlqpDims *dims, const void *z, const void *xnext, const void *x0,
                  const void *u_lo, const void *u_hi, long sb_u, long st_u, ALQP_ROWS_PARAMS, void *lam, void *rho,
                  double rho_scale, void *stream) {
    Args a = {};
    if (!set_rows_aux<real>(dims, x0, nullptr, u_lo, u_hi, sb_u, st_u, ALQP_ROWS_ARGS, a) || !z || !xnext || !lam || !rho)
        return ALQP_E_BADARG;
    a.zc = (const real *)z; a.xnext = (const real *)xnext;
    a.lam_io = (real *)lam; a.rho_io = (real *)rho; a.rho_scale = (real)rho_scale;
    return launch_aux(kern, x_lo, G, dim3(dims->B), stream, a);
}

}  // namespace alqp

extern "C" {

int alqp_exit_test(const double *sumsq, double *ctl, int mode, double tol, void *stream) {
    if (!sumsq || !ctl || (mode != 0 && mode != 1)) return ALQP_E_BADARG;
    hipLaunchKernelGGL(alqp::k_exit_test, dim3(1), dim3(64), 0, (hipStream_t)stream, sumsq, ctl, mode, tol);
    return hipGetLastError() == hipSuccess ? 0 : ALQP_E_LAUNCH;
}

#define ALQP_DEFINE_AUX(SFX, REAL)                                                                    \
    int alqp_merit_##SFX(const AlqpDims *dims, int K, const void *zc, const void *xnext,              \
                         const void *x0, const void *lam, const void *rho, const void *Qd,            \
                         const void *q, const void *u_lo, const void *u_hi, long sb_u, long st_u,     \
                         const AlqpObstacles *obs, void *phi, void *rnorm2, void *stream) {           \
        return alqp::merit_impl<REAL>(dims, K, zc, xnext, x0, lam, rho, Qd, q, u_lo, u_hi, sb_u,      \
                                      st_u, obs, phi, rnorm2, stream);                                \
    }                                                                                                 \
    int alqp_merit_pick_##SFX(const AlqpDims *dims, int n_ls, const void *d, const void *xnext_all,   \
                              const void *x0, const void *lam, const void *rho, const void *Qd,       \
                              const void *q, const void *u_lo, const void *u_hi, long sb_u, long st_u, \
                              const AlqpObstacles *obs, void *z, void *phi_prev, void *rnorm2,        \
                              void *phi_all, int *k_out, int *accept_out, void *stream) {             \
        return alqp::merit_pick_impl<REAL>(dims, n_ls, d, xnext_all, x0, lam, rho, Qd, q, u_lo, u_hi, \
                                           sb_u, st_u, obs, z, phi_prev, rnorm2, phi_all, k_out,      \
                                           accept_out, stream);                                       \
    }                                                                                                 \
    int alqp_linesearch_pick_##SFX(const AlqpDims *dims, int n_ls, const void *phi, void *phi_prev,   \
                                   const void *d, void *z, int *k_out, int *accept_out,               \
                                   void *stream) {                                                    \
        return alqp::pick_impl<REAL>(dims, n_ls, phi, phi_prev, d, z, k_out, accept_out, stream);     \
    }                                                                                                 \
    int alqp_dual_update_##SFX(const AlqpDims *dims, const void *z, const void *xnext,                \
                               const void *x0, const void *u_lo, const void *u_hi, long sb_u,         \
                               long st_u, const AlqpObstacles *obs, void *lam, void *rho,             \
                               double rho_scale, void *stream) {                                      \
        return alqp::dual_impl<REAL>(dims, z, xnext, x0, u_lo, u_hi, sb_u, st_u, obs, lam, rho,       \
                                     rho_scale, stream);                                              \
    }

ALQP_DEFINE_AUX(f32, float)
ALQP_DEFINE_AUX(f64, double)

// The three families with more rows: one set of entry points per family (FAM: xbox, rows, dense), all through the same
// implementations. XPARAMS / XARGS: what the family takes behind st_u, and what of ALQP_ROWS_ARGS it passes on.
#define ALQP_XBOX_PARAMS const void *x_lo, const void *x_hi, long sb_x, long st_x
#define ALQP_XBOX_ARGS x_lo, x_hi, sb_x, st_x, nullptr, nullptr, 0, 0, 0, 0, 0
#define ALQP_DEFINE_AUX_MERIT(FAM, Fam, SFX, REAL, COST, XPARAMS, XARGS)                              \
    int alqp_merit_##FAM##_##SFX(const AlqpDims *dims, int K, const void *zc, const void *xnext,      \
                                 const void *x0, const void *lam, const void *rho, const void *COST,  \
                                 const void *q, const void *u_lo, const void *u_hi, long sb_u,        \
                                 long st_u, XPARAMS, void *phi, void *rnorm2, void *stream) {         \
        return alqp::merit_ext_impl<REAL>(alqp::kMerit##Fam<REAL>, dims, K, zc, xnext, x0, lam, rho,  \
                                          COST, q, u_lo, u_hi, sb_u, st_u, XARGS, phi, rnorm2,        \
                                          stream);                                                    \
    }                                                                                                 \
    int alqp_merit_pick_##FAM##_##SFX(const AlqpDims *dims, int n_ls, const void *d,                  \
                                      const void *xnext_all, const void *x0, const void *lam,         \
                                      const void *rho, const void *COST, const void *q,               \
                                      const void *u_lo, const void *u_hi, long sb_u, long st_u,       \
                                      XPARAMS, void *z, void *phi_prev, void *rnorm2, void *phi_all,  \
                                      int *k_out, int *accept_out, void *stream) {                    \
        return alqp::merit_pick_ext_impl<REAL>(alqp::kMeritPick##Fam<REAL>, dims, n_ls, d, xnext_all, \
                                               x0, lam, rho, COST, q, u_lo, u_hi, sb_u, st_u, XARGS,  \
                                               z, phi_prev, rnorm2, phi_all, k_out, accept_out,       \
                                               stream);                                               \
    }
#define ALQP_DEFINE_AUX_DUAL(FAM, Fam, SFX, REAL, XPARAMS, XARGS)                                     \
    int alqp_dual_update_##FAM##_##SFX(const AlqpDims *dims, const void *z, const void *xnext,        \
                                       const void *x0, const void *u_lo, const void *u_hi, long sb_u, \
                                       long st_u, XPARAMS, void *lam, void *rho, double rho_scale,    \
                                       void *stream) {                                                \
        return alqp::dual_ext_impl<REAL>(alqp::kDual##Fam<REAL>, dims, z, xnext, x0, u_lo, u_hi,      \
                                         sb_u, st_u, XARGS, lam, rho, rho_scale, stream);             \
    }
#define ALQP_DEFINE_AUX_EXT(SFX, REAL)                                                                \
    ALQP_DEFINE_AUX_MERIT(xbox, Xbox, SFX, REAL, Qd, ALQP_XBOX_PARAMS, ALQP_XBOX_ARGS)                \
    ALQP_DEFINE_AUX_DUAL(xbox, Xbox, SFX, REAL, ALQP_XBOX_PARAMS, ALQP_XBOX_ARGS)                     \
    ALQP_DEFINE_AUX_MERIT(rows, Rows, SFX, REAL, Qd, ALQP_ROWS_PARAMS, ALQP_ROWS_ARGS)                \
    ALQP_DEFINE_AUX_DUAL(rows, Rows, SFX, REAL, ALQP_ROWS_PARAMS, ALQP_ROWS_ARGS)                     \
    ALQP_DEFINE_AUX_MERIT(dense, Dense, SFX, REAL, C, ALQP_ROWS_PARAMS, ALQP_ROWS_ARGS)

ALQP_DEFINE_AUX_EXT(f32, float)
ALQP_DEFINE_AUX_EXT(f64, double)

}  // extern "C"
