// alqp_team_nl.hpp - the nonlinear fused solve on the team kernel: one launch runs a whole nonlinear MPC call with state
// box rows and / or general rows (alqp_solve_nonlin_rows, include/mi_alqp.h). The dynamics model (alqp_dyn.hpp) is inlined:
// the team makes its own linearisation, runs Team's unchanged sweeps on it in nonlinear-caller mode (gxnext), and
// evaluates the 20 line-search candidates with the TRUE dynamics. DESIGN.md section 28.
//
// Nothing here is a member of Team (a new member changes the register allocation of the existing instantiations, DESIGN
// sections 24-26): the three device functions below are free function templates over a Team&.
//
// Per-instance workspace in global memory: F[T-1][NX][N], then xnext[T-1][NX]; Team's gF / gxnext point into it.
// Store-to-load hand-off: the linearisation is stored by some lanes of the wavefront and loaded by others of the SAME
// wavefront in the next phase, with only a compiler fence (wave_sync) in between - what k_solve_lin does for `lams` and
// the quad fused solve for gFw. What this relies on: a wavefront's vector memory operations reach its CU's one vector L1 in
// issue order, and a store that hits a line resident there (the F region was read one Newton step earlier) updates or
// drops it, so that a later load of the same wavefront, from whichever lane, sees the stored value. This same-wavefront,
// cross-lane property is not a documented hardware rule the project can cite: it rests on the precedent of those two
// kernels and on the tests passing on the MI355X (workspace independence and the per-step traces, whose second to fourth
// Newton steps read F lines the previous step left in L1). Every team is inside one wavefront and no other workgroup
// touches its workspace, so no scope wider than the wavefront is involved.
#pragma once
#include <hip/hip_runtime.h>

#include "alqp_args.hpp"
#include "mi_alqp.h"

namespace alqp {

// GenSolveArgs' members (C, F, c unused) and the workspace
template <typename real>
struct NlRowsSolveArgs : GenSolveArgs<real> {
    real *ws;   // [B][(T-1) nx (n + 1)]: per instance F[T-1][nx][n], then xnext[T-1][nx]
};

// alqp_team_nl.hip, one object per row mask (kGenXbox | kGenPoly of alqp_launch.hpp: 2, 4, 6; -DALQP_NL_UNIT=<mask>).
// ALQP_E_UNSUPPORTED: no such model, (nx, nu) not the model's, or an LDS image that does not fit.
template <typename real, int MASK>
int dispatch_solve_nonlin_rows(int dyn_id, int nx, int nu, const NlRowsSolveArgs<real> &a, const TraceArgs<real> *tr,
                               hipStream_t stream);

}  // namespace alqp

#ifdef ALQP_NL_UNIT
#include "alqp_team.hpp"
#include "alqp_dyn.hpp"

namespace alqp {

__device__ __forceinline__ float pow2neg(int k, float) { return __builtin_ldexpf(1.0f, -k); }
__device__ __forceinline__ double pow2neg(int k, double) { return __builtin_ldexp(1.0, -k); }

// One lane's full tangent set (n tangents) or, where that takes too many registers (a dual number is 1 + n words, and an
// RK4 step keeps some thirty of them alive), a quarter of it on each of four lanes per stage
template <class Dyn>
constexpr bool nl_split_jac() { return Dyn::NX + Dyn::NU > 4; }

// linearize: xnext_t <- f(z_t), F_t <- df/dz at z_t for every t < T-1, stages dealt over the team's lanes
template <class Dyn, typename real, class TM>
__device__ __forceinline__ void nl_linearize(TM &tm, real h, real *gFw, real *gxn, bool active) {
    constexpr int NX = Dyn::NX, N = Dyn::NX + Dyn::NU, G = TM::G;
    const int T = tm.T;
    if constexpr (!nl_split_jac<Dyn>()) {
        for (int t = tm.li; t < T - 1; t += G) {
            real z[N], xn[NX], J[NX][N];
#pragma unroll
            for (int j = 0; j < N; ++j) z[j] = tm.zs[t * N + j];
            dyn_value_jac<Dyn, real>(z, h, xn, J);
            if (active) {
#pragma unroll
                for (int i = 0; i < NX; ++i) {
                    gxn[t * NX + i] = xn[i];
#pragma unroll
                    for (int j = 0; j < N; ++j) gFw[(size_t)(t * NX + i) * N + j] = J[i][j];
                }
            }
        }
    } else {
        constexpr int NTL = (N + 3) / 4;
        static_assert(G % 4 == 0, "four lanes per stage");
        const int q = tm.li & 3;
        for (int t = tm.li >> 2; t < T - 1; t += G / 4) {
            real z[N], xn[NX], Jl[NX][NTL];
#pragma unroll
            for (int j = 0; j < N; ++j) z[j] = tm.zs[t * N + j];
            dyn_value_jac_split<Dyn, real>(z, h, q, xn, Jl);   // lane q: columns 4 c + q
            if (active) {
#pragma unroll
                for (int i = 0; i < NX; ++i) {
                    if (q == 0) gxn[t * NX + i] = xn[i];
#pragma unroll
                    for (int c = 0; c < NTL; ++c)
                        if (4 * c + q < N) gFw[(size_t)(t * NX + i) * N + 4 * c + q] = Jl[i][c];
                }
            }
        }
    }
    wave_sync();
}

// values only: xnext_t <- f(z_t); the F region is not touched
template <class Dyn, typename real, class TM>
__device__ __forceinline__ void nl_values(TM &tm, real h, real *gxn, bool active) {
    constexpr int NX = Dyn::NX, N = Dyn::NX + Dyn::NU, G = TM::G;
    for (int t = tm.li; t < tm.T - 1; t += G) {
        real z[N], xn[NX];
#pragma unroll
        for (int j = 0; j < N; ++j) z[j] = tm.zs[t * N + j];
        dyn_value<Dyn, real>(z, h, xn);
        if (active) {
#pragma unroll
            for (int i = 0; i < NX; ++i) gxn[t * NX + i] = xn[i];
        }
    }
    wave_sync();
}

// Merit of the 20 candidates z + 2^-k d with the TRUE dynamics (al_utils.py:618-633). Team::merit_candidates' statements
// for the cost, the initial-state rows (both exactly quadratic in alpha) and the control, state and general rows (per
// candidate); the dynamics rows per candidate with the model, r = (z_{t+1} + alpha d_{t+1})[x] - f(z_t + alpha d_t), the
// (stage, candidate) pairs dealt over the team's lanes. Every lane returns all 20 values.
template <class Dyn, bool POLY, typename real, class TM>
__device__ __forceinline__ void nl_merit_candidates(TM &tm, real h, real (&phi)[20]) {
    constexpr int NX = Dyn::NX, NU = Dyn::NU, N = NX + NU, G = TM::G, XR = TM::XR, K = 20;
    constexpr bool XBOX = XR != 0;
    const int T = tm.T, neq = T * NX, li = tm.li, pm = tm.pm;
    const real rho = tm.rho;
    const real *lams = tm.lams;
    real acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0;
    // the dynamics rows first (only acc is alive across the model): pair e = (stage t, candidate k); every lane takes the
    // same number of trips, the pairs past the end are evaluated on pair 0 and count as zero
    const int P = (T - 1) * K;
    for (int e0 = 0; e0 < P; e0 += G) {
        const bool ok = e0 + li < P;
        const int e = ok ? e0 + li : 0;
        const int t = e / K, k = e - t * K;
        const real alpha = pow2neg(k, real(0));
        real zc[N], xn[NX];
#pragma unroll
        for (int j = 0; j < N; ++j) zc[j] = fma_(alpha, tm.ds[t * N + j], tm.zs[t * N + j]);
        dyn_value<Dyn, real>(zc, h, xn);
        real v = 0;
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            const real r = fma_(alpha, tm.ds[(t + 1) * N + i], tm.zs[(t + 1) * N + i]) - xn[i];
            v = fma_(fma_(real(0.5) * rho, r, lams[t * NX + i]), r, v);
        }
        v = ok ? v : real(0);
#pragma unroll
        for (int kc = 0; kc < K; ++kc) acc[kc] += (k == kc) ? v : real(0);
    }
    real c0 = 0, c1 = 0, c2 = 0;
    for (int e = li; e < T * N; e += G) {
        real z = tm.zs[e], d = tm.ds[e];
        real Qv = tm.gQd[e], qv = tm.gq[e];
        real gz = fma_(Qv, z, qv);
        c0 = fma_(fma_(real(0.5) * Qv, z, qv), z, c0);
        c1 = fma_(gz, d, c1);
        c2 = fma_(real(0.5) * Qv * d, d, c2);
    }
    for (int e = (T - 1) * NX + li; e < neq; e += G) {   // the initial-state rows: r + alpha s, affine
        real r = tm.req[e], sv = tm.seq[e], lm = lams[e];
        c0 = fma_(fma_(real(0.5) * rho, r, lm), r, c0);
        c1 = fma_(fma_(rho, r, lm), sv, c1);
        c2 = fma_(real(0.5) * rho * sv, sv, c2);
    }
    for (int e = li; e < T * NU; e += G) {
        int t = e / NU, j = e - t * NU;
        real z = tm.zs[t * N + NX + j], d = tm.ds[t * N + NX + j];
        int ru = neq + t * (2 * NU + XR + (POLY ? pm : 0)) + j;
        real lu = lams[ru], ll = lams[ru + NU];
        real bu = tm.uhi(t, j), bl = tm.ulo(t, j);
        real alpha = 1;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            real zk = fma_(alpha, d, z);
            real vu = zk - bu, vl = bl - zk;
            real cu = fmax_(vu, real(0)), cl = fmax_(vl, real(0));
            acc[k] += fma_(lu, vu, ll * vl) + real(0.5) * rho * fma_(cu, cu, cl * cl);
            alpha *= real(0.5);
        }
    }
    if constexpr (XBOX) {
        for (int e = li; e < T * NX; e += G) {
            int t = e / NX, i = e - t * NX;
            real z = tm.zs[t * N + i], d = tm.ds[t * N + i];
            int ru = neq + t * (2 * NU + XR + (POLY ? pm : 0)) + 2 * NU + i;
            real lu = lams[ru], ll = lams[ru + NX];
            real bu = tm.xhi(t, i), bl = tm.xlo(t, i);
            real alpha = 1;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                real zk = fma_(alpha, d, z);
                real vu = zk - bu, vl = bl - zk;
                real cu = fmax_(vu, real(0)), cl = fmax_(vl, real(0));
                acc[k] += fma_(lu, vu, ll * vl) + real(0.5) * rho * fma_(cu, cu, cl * cl);
                alpha *= real(0.5);
            }
        }
    }
    if constexpr (POLY) {
        for (int e = li; e < T * pm; e += G) {
            int t = e / pm, k = e - t * pm;
            const real *Gk = tm.grow(t, k);
            real r0 = -tm.hrow(t, k), sd = 0;   // the candidate's residual is r0 + alpha sd
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const real gv = Gk[j];
                r0 = fma_(gv, tm.zs[t * N + j], r0);
                sd = fma_(gv, tm.ds[t * N + j], sd);
            }
            const real lk = lams[neq + t * (2 * NU + XR + pm) + 2 * NU + XR + k];
            real alpha = 1;
#pragma unroll
            for (int kc = 0; kc < K; ++kc) {
                real r = fma_(alpha, sd, r0);
                real cp = fmax_(r, real(0));
                acc[kc] += fma_(lk, r, real(0.5) * rho * cp * cp);
                alpha *= real(0.5);
            }
        }
    }
    c0 = team_sum<G>(c0);
    c1 = team_sum<G>(c1);
    c2 = team_sum<G>(c2);
    real alpha = 1;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        phi[k] = team_sum<G>(acc[k]) + fma_(alpha, fma_(alpha, c2, c1), c0);
        alpha *= real(0.5);
    }
}

// ---- the fused nonlinear solve with rows: k_solve_lin's statements around the three functions above -----------------
// One team of Cfg::G lanes per instance; LDS image that of k_solve_lin_gen with the same flags. Uncapped builds only and no
// spilling instantiation (tools/spill_report.py), for the reason alqp_team.hip's header comment gives.
template <typename real, class Dyn, bool XBOX, bool POLY, bool TRACE>
__global__ __launch_bounds__(64, 1) void k_solve_nonlin_team(NlRowsSolveArgs<real> a, TraceArgs<real> tr) {
    if (a.skip && *a.skip != 0.0) return;  // block-uniform, before any barrier
    constexpr int NX = Dyn::NX, NU = Dyn::NU;
    using C = Cfg<real, NX, NU>;
    constexpr int G = C::G, N = C::N;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    real *smem = reinterpret_cast<real *>(smem_raw);
    const int lane = threadIdx.x, team = lane / G, li = lane % G;
    const int b_raw = blockIdx.x * C::QPW + team;
    const bool active = b_raw < a.B;
    const int b = active ? b_raw : a.B - 1;
    int m = 0;
    if constexpr (POLY) m = a.m;
    const int T = a.T, M = C::M(T) + (XBOX ? 2 * T * NX : 0) + (POLY ? T * m : 0);
    const int team_words = C::team_words(T) + (POLY ? 2 * pad4(m) : 0);   // the team image, then the hand-over region

    Team<real, NX, NU, false, XBOX, POLY> tm;
    tm.init(smem + (size_t)team * team_words + opaque_zero(), li, team * G, T, b);
    tm.gQd = a.Qd + (size_t)b * T * N;
    tm.gq = a.q + (size_t)b * T * N;
    real *gFw = a.ws + (size_t)b * (T - 1) * NX * (N + 1);
    real *gxn = gFw + (size_t)(T - 1) * NX * N;
    tm.gF = gFw;
    tm.gc = nullptr;
    tm.gxnext = gxn;
    tm.gx0 = a.x0 + (size_t)b * NX;
    tm.gulo = a.ulo + (size_t)b * a.sb_u;
    tm.guhi = a.uhi + (size_t)b * a.sb_u;
    tm.st_u = a.st_u;
    if constexpr (XBOX) {
        tm.gxlo = a.xlo + (size_t)b * a.sb_x;
        tm.gxhi = a.xhi + (size_t)b * a.sb_x;
        tm.st_x = a.st_x;
    }
    if constexpr (POLY) {
        tm.gG = a.G + (size_t)b * a.sb_g;
        tm.gh = a.h + (size_t)b * a.sb_h;
        tm.st_g = a.st_g; tm.st_h = a.st_h; tm.pm = a.m;
        tm.ps = tm.Xp + pad4(T * C::XT);
    }
    const real h = a.dyn_h;

    real *gz = a.z + (size_t)b * T * N;
    tm.lams = a.lam + (size_t)b * M;  // multipliers stay in global memory (L2), updated in place
    for (int e = li; e < T * N; e += G) tm.zs[e] = gz[e];
    tm.rho = a.rho[b];
    real phi_prev = a.phi[b];
    wave_sync();
    if (a.al_iter <= 0) {   // nothing below refreshes req: the residual rplus2 reads
        nl_values<Dyn>(tm, h, gxn, active);
        tm.residual_sweep();
    }

    int step_id = 0;
    for (int it = 0; it < a.al_iter; ++it) {
        if (a.flags & ALQP_INIT_MERIT) {
            nl_values<Dyn>(tm, h, gxn, active);
            tm.residual_sweep();
            real p1[1];
            tm.template merit_candidates<1>(p1, true);
            phi_prev = p1[0];
        }
        for (int st = 0; st < a.max_newton; ++st, ++step_id) {
            nl_linearize<Dyn>(tm, h, gFw, gxn, active);
            real *tg = nullptr;
            if constexpr (TRACE) tg = (tr.g && active) ? tr.g + ((size_t)step_id * a.B + b) * T * N : nullptr;
            tm.forward_sweep(tg);
            tm.backward_sweep();
            if constexpr (TRACE) {
                if (tr.d && active) {
                    real *td = tr.d + ((size_t)step_id * a.B + b) * T * N;
                    for (int e = li; e < T * N; e += G) td[e] = tm.ds[e];
                }
            }
            real ph[20];
            nl_merit_candidates<Dyn, POLY>(tm, h, ph);
            // first argmin, a NaN wins like torch.min (al_utils.py:634)
            int kbest = 0;
            real best = ph[0];
#pragma unroll
            for (int k = 1; k < 20; ++k) {
                if (!(best != best) && (ph[k] != ph[k] || ph[k] < best)) {
                    best = ph[k];
                    kbest = k;
                }
            }
            const bool acc = best < phi_prev;
            if constexpr (TRACE) {
                if (active && li == 0) {
                    if (tr.phi)
#pragma unroll
                        for (int k = 0; k < 20; ++k) tr.phi[((size_t)step_id * 20 + k) * a.B + b] = ph[k];
                    if (tr.phi_prev) tr.phi_prev[(size_t)step_id * a.B + b] = phi_prev;
                    if (tr.k) tr.k[(size_t)step_id * a.B + b] = kbest;
                    if (tr.accept) tr.accept[(size_t)step_id * a.B + b] = acc ? 1 : 0;
                }
            }
            const real alpha = acc ? real(1) / real(1 << kbest) : real(0);
            for (int e = li; e < T * N; e += G) tm.zs[e] += alpha * tm.ds[e];
            wave_sync();
            phi_prev = best;  // merit <- new_merit even when rejected (al_utils.py:569)
        }
        // the true residual at the iterate the iteration ends on (values only: F keeps the last Newton step's linearisation)
        nl_values<Dyn>(tm, h, gxn, active);
        tm.residual_sweep();
        if (a.flags & ALQP_DUAL_UPDATE) {
            if (active) tm.dual_update();  // in-place on global lam: padding teams must not touch it
            tm.rho *= a.rho_scale;
        }
    }

    const real rn2 = tm.rplus2();
    int bad = 0;
    for (int e = li; e < T * N; e += G) {
        real v = tm.zs[e];
        bad |= !(v - v == real(0));
    }
    bad = team_or<G>(bad);
    if (active) {
        for (int e = li; e < T * N; e += G) gz[e] = tm.zs[e];
        if ((a.flags & ALQP_SAVE_FACTOR) && a.factor && step_id > 0) {
            real *gf = a.factor + (size_t)b * T * C::XT;
            for (int e = li; e < T * C::XT; e += G) gf[e] = tm.Xp[e];
        }
        if (li == 0) {
            a.rho[b] = tm.rho;
            a.phi[b] = phi_prev;
            if (a.rnorm2) a.rnorm2[b] = rn2;
            if (a.info && tm.info && a.info[b] == 0) a.info[b] = tm.info;  // sticky: first failure of the solve
            if (a.status) a.status[b] = bad ? 0 : 1;
        }
    }
}

}  // namespace alqp
#endif  // ALQP_NL_UNIT
