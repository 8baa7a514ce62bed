// alqp_team.hip - the team kernels (one QP per lane team, factor in LDS: alqp_team.hpp) and their launchers, fp32
// and fp64 in one object.
#if defined(ALQP_BWD_DYN_UNIT) || defined(ALQP_XBOX_STEP_UNIT) || defined(ALQP_SHDYN_UNIT) || defined(ALQP_GEN_UNIT) || \
    defined(ALQP_ROWS_STEP_UNIT) || defined(ALQP_DENSE_STEP_UNIT)
#undef ALQP_PHASE_TIMING   // the debug counters live in the product unit only
#endif
#include <hip/hip_runtime.h>

#include "alqp_team.hpp"
#include "alqp_dims.hpp"
#include "alqp_launch.hpp"

namespace alqp {

#ifdef ALQP_PHASE_TIMING
__device__ unsigned long long g_team_cycles[8];   // debug build only (tools/team_timing.py)
#endif
// ---- fused LinDx solve -------------------------------------------------------------
// One body under three headers, each in compile units of its own (build.sh):
//   k_solve_lin (the product unit): the plain problem, SolveArgs.
//   k_solve_lin_shdyn (-DALQP_SHDYN_UNIT): the plain problem with F and c addressed through an instance stride and a stage
//     stride (a.sb_F / a.mt_F, a.sb_c / a.mt_c; ALQP_F_STAGE / ALQP_C_STAGE in Team), so that one F, or one sequence F_t,
//     serves the whole batch. Same arithmetic in the same order on the same values as k_solve_lin.
//   k_solve_lin_gen<.., DENSE, XBOX, POLY, ..> (-DALQP_GEN_UNIT=<mask>, mask = 1 dense | 2 state bounds | 4 general rows, one
//     object per non-zero mask): every feature's arguments in one GenSolveArgs, an instantiation reads those of its flags.
//     DENSE: the stage cost's full C_t at a.C, [B][T][N][N], in place of a.Qd. XBOX: state box rows xlo <= x_t <= xhi behind
//     every stage's control rows, the bounds at a.xlo / a.xhi. POLY: a.m rows G_t z_t <= h_t behind those, rows and right-hand
//     sides at a.G / a.h; the LDS image is then the team image plus a hand-over region of 2 pad4(a.m) words per team.
//     Multipliers per stage [u | x | G] (Team).
// Headers, not a shared device function: called through one, every plain instantiation came out with different register
// allocation. The plain and the shdyn header stay apart from the gen one so that the hot path's argument blocks and code
// stay what they are.
// OCC: wavefronts per SIMD the register allocation is capped for. 2 (256 registers) lets a CU hold the 8 teams its
// LDS has room for, but costs 80 B (fp32) / 252 B (fp64) of scratch per lane at (13,4); 1 (no cap) has no scratch.
// Measured (profiles/r02/experiments): fp64 is faster uncapped at every batch the team kernels see (B = 200: 1.27 ->
// 1.22 ms, B = 2048: 3.43 -> 2.85 ms); fp32 only while there is at most one wavefront per SIMD anyway (B = 200: 0.84 ->
// 0.80 ms, B = 1024: 0.91 -> 0.87 ms; B = 2048: 1.07 against 1.71 ms). dispatch_solve() picks accordingly, and
// dispatch_solve_shdyn() by the same rule. The gen kernels have uncapped builds only: a capped one spills.
// The TRACE instantiations (tests only) are never capped: with their extra live pointers the capped fp64 builds spill ~70-150
// registers, and this hipcc (ROCm 7.2) can place such a spill store at the head of a divergent loop's exit block IN FRONT OF the
// `s_or_b64 exec` that re-enables the lanes - the store then runs with EXEC = 0 and the reload returns stale scratch. Seen once
// (k_solve_lin<double,12,4,true,2>: the zs base offset spilled after the `for (e = li; e < T*N; e += G)` load loop, every row
// of the returned z one repeated value); the uncapped builds have no spills (checked per kernel: tools/spill_report.py), and
// no instantiation of this body may ship with one.
#if defined(ALQP_GEN_UNIT)
template <typename real, int NX, int NU, bool DENSE, bool XBOX, bool POLY, bool TRACE>
__global__ __launch_bounds__(64, 1) void k_solve_lin_gen(GenSolveArgs<real> a, TraceArgs<real> tr) {
#elif defined(ALQP_SHDYN_UNIT)
template <typename real, int NX, int NU, bool TRACE, int OCC = TRACE ? 1 : 2>
__global__ __launch_bounds__(64, OCC) void k_solve_lin_shdyn(ShdynSolveArgs<real> a, TraceArgs<real> tr) {
    constexpr bool DENSE = false, XBOX = false, POLY = false;
#else
template <typename real, int NX, int NU, bool TRACE, int OCC = TRACE ? 1 : 2>
__global__ __launch_bounds__(64, OCC) void k_solve_lin(SolveArgs<real> a, TraceArgs<real> tr) {
    constexpr bool DENSE = false, XBOX = false, POLY = false;
#endif
    if (a.skip && *a.skip != 0.0) return;  // block-uniform, before any barrier
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
    const int T = a.T, M = C::M(T) + (XBOX ? 2 * T * NX : 0) + (POLY ? T * m : 0), neq = T * NX;
    const int team_words = C::team_words(T) + (POLY ? 2 * pad4(m) : 0);   // the team image, then the hand-over region

    Team<real, NX, NU, DENSE, XBOX, POLY> tm;
#ifdef ALQP_PHASE_TIMING
    for (int i = 0; i < 8; ++i) tm.tacc[i] = 0;
    tm.stamp(-1);
#endif
    tm.init(smem + (size_t)team * team_words + opaque_zero(), li, team * G, T, b);
    if constexpr (DENSE) tm.gC = a.C + (size_t)b * T * N * N;   // size_t: B T n n words pass 2^32 bytes at large batches
    else tm.gQd = a.Qd + (size_t)b * T * N;
    tm.gq = a.q + (size_t)b * T * N;
#ifdef ALQP_SHDYN_UNIT
    tm.gF = a.F + (size_t)b * a.sb_F;
    tm.gc = a.c + (size_t)b * a.sb_c;
    tm.mt_F = a.mt_F; tm.mt_c = a.mt_c;
#else
    tm.gF = a.F + (size_t)b * (T - 1) * NX * N;
    tm.gc = a.c + (size_t)b * (T - 1) * NX;
#endif
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

    real *gz = a.z + (size_t)b * T * N;
    tm.lams = a.lam + (size_t)b * M;  // multipliers stay in global memory (L2), updated in place
    for (int e = li; e < T * N; e += G) tm.zs[e] = gz[e];
    tm.rho = a.rho[b];
    real phi_prev = a.phi[b];
    wave_sync();
    tm.residual_sweep();

    int step_id = 0;
    const bool ref_exit = (a.flags & ALQP_EXIT_IN_KERNEL) != 0;   // grid-uniform
    int gphase = 0;
    for (int it = 0; it < a.al_iter; ++it) {
        if (a.flags & ALQP_INIT_MERIT) {
            real p1[1];
            tm.template merit_candidates<1>(p1, true);
            phi_prev = p1[0];
        }
        double nrm_old = 0;
        int n_done = 0;
        if (ref_exit) {   // ||r+|| over the whole batch at the start of the Newton loop (al_utils.py:486)
            const real r0 = tm.rplus2();
            nrm_old = sqrt(grid_sum_ordered(wave_sum_leaders(exit_term(r0, tm.info), active && li == 0), a.exit_scratch, gphase));
        }
        for (int st = 0; st < a.max_newton; ++st, ++step_id) {
            real *tg = nullptr;
            if constexpr (TRACE) tg = (tr.g && active) ? tr.g + ((size_t)step_id * a.B + b) * T * N : nullptr;
            tm.forward_sweep(tg);
#ifdef ALQP_PHASE_TIMING
            tm.stamp(-1);
#endif
            tm.backward_sweep();
#ifdef ALQP_PHASE_TIMING
            tm.stamp(4);
#endif
            if constexpr (TRACE) {
                if (tr.d && active) {
                    real *td = tr.d + ((size_t)step_id * a.B + b) * T * N;
                    for (int e = li; e < T * N; e += G) td[e] = tm.ds[e];
                }
            }
            real ph[20];
            tm.template merit_candidates<20>(ph, false);
#ifdef ALQP_PHASE_TIMING
            tm.stamp(5);
#endif
            // first argmin, a NaN wins like torch.min (al_utils.py:634)
            int kbest = 0;
            real best = ph[0];
            if (a.n_ls == 20) {
#pragma unroll
                for (int k = 1; k < 20; ++k) {
                    if (!(best != best) && (ph[k] != ph[k] || ph[k] < best)) {
                        best = ph[k];
                        kbest = k;
                    }
                }
            } else if constexpr (C::RB * C::NXP >= 20) {
                // fewer candidates (tests): go through LDS (the Ft region is free here)
                // instead of 20 hoisted lane masks
                if (li == 0) {
#pragma unroll
                    for (int k = 0; k < 20; ++k) tm.Ft[k] = ph[k];
                }
                wave_sync();
                for (int k = 1; k < a.n_ls; ++k) {
                    real v = tm.Ft[k];
                    if (!(best != best) && (v != v || v < best)) {
                        best = v;
                        kbest = k;
                    }
                }
                wave_sync();
                if (li < 20) tm.Ft[li] = 0;  // restore the constant zeros of the SYRK operand
                wave_sync();
            } else {
#pragma unroll
                for (int k = 1; k < 20; ++k) {
                    if (k < a.n_ls && !(best != best) && (ph[k] != ph[k] || ph[k] < best)) {
                        best = ph[k];
                        kbest = k;
                    }
                }
            }
            const bool acc = best < phi_prev;
            if constexpr (TRACE) {
                if (active && li == 0) {
                    if (tr.phi)
#pragma unroll
                        for (int k = 0; k < 20; ++k)
                            if (k < a.n_ls) tr.phi[((size_t)step_id * a.n_ls + k) * a.B + b] = ph[k];
                    if (tr.phi_prev) tr.phi_prev[(size_t)step_id * a.B + b] = phi_prev;
                    if (tr.k) tr.k[(size_t)step_id * a.B + b] = kbest;
                    if (tr.accept) tr.accept[(size_t)step_id * a.B + b] = acc ? 1 : 0;
                }
            }
            const real alpha = acc ? real(1) / real(1 << kbest) : real(0);
            for (int e = li; e < T * N; e += G) tm.zs[e] += alpha * tm.ds[e];
            for (int e = li; e < neq; e += G) tm.req[e] += alpha * tm.seq[e];
            wave_sync();
#ifdef ALQP_PHASE_TIMING
            tm.stamp(6);
#endif
            phi_prev = best;  // merit <- new_merit even when rejected (al_utils.py:569)
            if (ref_exit) {   // al_utils.py:551-564, the same test alqp_exit_test takes between launches
                const real r1 = tm.rplus2();
                const double nw = sqrt(grid_sum_ordered(wave_sum_leaders(exit_term(r1, tm.info), active && li == 0), a.exit_scratch, gphase));
                ++n_done;
                if (nw < a.exit_tol || fabs(nrm_old - nw) / nw < a.exit_tol) break;
                nrm_old = nw;
            }
        }
        if (ref_exit && a.newton_counts && blockIdx.x == 0 && lane == 0) a.newton_counts[it] = grid_barrier_timed_out(a.exit_scratch) ? -1 : n_done;
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
#ifdef ALQP_PHASE_TIMING
    tm.stamp(7);
    if (lane == 0)
        for (int i = 0; i < 8; ++i) atomicAdd(&g_team_cycles[i], tm.tacc[i]);
#endif
    if (active) {
        for (int e = li; e < T * N; e += G) gz[e] = tm.zs[e];
        if ((a.flags & ALQP_SAVE_FACTOR) && a.factor) {
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

// ---- one Newton direction (nonlinear-caller mode) ----------------------------------
template <typename real, int NX, int NU>
__global__ __launch_bounds__(64) void k_newton_step(StepArgs<real> a) {
    using C = Cfg<real, NX, NU>;
    constexpr int G = C::G, N = C::N;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    real *smem = reinterpret_cast<real *>(smem_raw);
    const int lane = threadIdx.x, team = lane / G, li = lane % G;
    const int b_raw = blockIdx.x * C::QPW + team;
    const bool active = b_raw < a.B;
    const int b = active ? b_raw : a.B - 1;
    const int T = a.T, M = C::M(T) + T * a.nobs;

    Team<real, NX, NU> tm;
    tm.init(smem + (size_t)team * C::team_words(T) + opaque_zero(), li, team * G, T, b);
    if (a.nobs > 0) { tm.gobs = a.obs + (size_t)b * T * a.nobs * 3; tm.nobs = a.nobs; tm.obs_r2 = a.obs_r2; }
    tm.no_init = a.no_init != 0;
    tm.gQd = a.Qd + (size_t)b * T * N;
    tm.gq = a.q + (size_t)b * T * N;
    tm.gF = a.F + (size_t)b * (T - 1) * NX * N;
    tm.gc = nullptr;
    tm.gx0 = a.x0 + (size_t)b * NX;
    tm.gulo = a.ulo + (size_t)b * a.sb_u;
    tm.guhi = a.uhi + (size_t)b * a.sb_u;
    tm.st_u = a.st_u;
    tm.gxnext = a.xnext + (size_t)b * (T - 1) * NX;
    const real *gz = a.z + (size_t)b * T * N;
    tm.lams = const_cast<real *>(a.lam) + (size_t)b * M;  // read-only here
    for (int e = li; e < T * N; e += G) tm.zs[e] = gz[e];
    tm.rho = a.rho[b];
    wave_sync();
    tm.forward_sweep((active && a.g_out) ? a.g_out + (size_t)b * T * N : nullptr);
    tm.backward_sweep();
    if (active) {
        real *gd = a.d_out + (size_t)b * T * N;
        for (int e = li; e < T * N; e += G) gd[e] = tm.ds[e];
        if (a.factor) {
            real *gf = a.factor + (size_t)b * T * C::XT;
            for (int e = li; e < T * C::XT; e += G) gf[e] = tm.Xp[e];
        }
        if (li == 0 && a.info && tm.info && a.info[b] == 0) a.info[b] = tm.info;
    }
}

#if defined(ALQP_XBOX_STEP_UNIT) || defined(ALQP_ROWS_STEP_UNIT) || defined(ALQP_DENSE_STEP_UNIT)
// The same with more rows per stage and / or a dense stage cost: k_newton_step's statements over Team<.., DENSE, XBOX, POLY>.
// Three kernels, each in a unit of its own, and like the fused solve above three headers over one body (a shared device
// function does not keep their register allocation either: profiles/r18/README.md). The members only some of the argument
// types have (Qd, C, G, h, m) are touched inside `if constexpr`.
// XBOX: state box rows, the bounds at gxlo / gxhi. POLY: general rows G_t z_t <= h_t, and the LDS image is the team image plus
// the hand-over region of 2 pad4(m) words per team, set up as k_solve_lin_gen sets it up. DENSE: stage cost
// 1/2 z_t' C_t z_t + q_t' z_t with C at a.C ([B][T][N][N]) and no gQd. Multipliers per stage [u | (x) | (G)],
// M = T nx + T (2 nu + (XBOX ? 2 nx : 0) + (POLY ? m : 0)) per instance. No obstacle rows and no state-estimator row set:
// forward_sweep's obstacle offset is written without XR.
#if defined(ALQP_XBOX_STEP_UNIT)   // the state-bound step unit: state box rows
template <typename real, int NX, int NU>
__global__ __launch_bounds__(64) void k_newton_step_xbox(XboxStepArgs<real> a) {
    constexpr bool DENSE = false, XBOX = true, POLY = false;
#elif defined(ALQP_ROWS_STEP_UNIT)   // the row-step unit: general rows, with or without state box rows
template <typename real, int NX, int NU, bool XBOX>
__global__ __launch_bounds__(64, 1) void k_newton_step_rows(RowsStepArgs<real> a) {
    constexpr bool DENSE = false, POLY = true;
#else   // the dense-step units: a dense cost, alone or with state box rows and / or general rows
template <typename real, int NX, int NU, bool XBOX, bool POLY>
__global__ __launch_bounds__(64, 1) void k_newton_step_dense(DenseStepArgs<real> a) {
    constexpr bool DENSE = true;
#endif
    using C = Cfg<real, NX, NU>;
    constexpr int G = C::G, N = C::N;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    real *smem = reinterpret_cast<real *>(smem_raw);
    const int lane = threadIdx.x, team = lane / G, li = lane % G;
    const int b_raw = blockIdx.x * C::QPW + team;
    const bool active = b_raw < a.B;
    const int b = active ? b_raw : a.B - 1;
    const int T = a.T;
    int m = 0;
    if constexpr (POLY) m = a.m;
    const size_t M = (size_t)C::M(T) + (XBOX ? (size_t)2 * T * NX : 0) + (POLY ? (size_t)T * m : 0);
    const int team_words = C::team_words(T) + (POLY ? 2 * pad4(m) : 0);   // the team image, then the hand-over region

    Team<real, NX, NU, DENSE, XBOX, POLY> tm;
    tm.init(smem + (size_t)team * team_words + opaque_zero(), li, team * G, T, b);
    if constexpr (DENSE) tm.gC = a.C + (size_t)b * T * N * N;   // size_t: B T n n words pass 2^32 bytes at large batches
    else tm.gQd = a.Qd + (size_t)b * T * N;
    tm.gq = a.q + (size_t)b * T * N;
    tm.gF = a.F + (size_t)b * (T - 1) * NX * N;
    tm.gc = nullptr;
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
    tm.gxnext = a.xnext + (size_t)b * (T - 1) * NX;
    const real *gz = a.z + (size_t)b * T * N;
    tm.lams = const_cast<real *>(a.lam) + (size_t)b * M;  // read-only here
    for (int e = li; e < T * N; e += G) tm.zs[e] = gz[e];
    tm.rho = a.rho[b];
    wave_sync();
    tm.forward_sweep((active && a.g_out) ? a.g_out + (size_t)b * T * N : nullptr);
    tm.backward_sweep();
    if (active) {
        real *gd = a.d_out + (size_t)b * T * N;
        for (int e = li; e < T * N; e += G) gd[e] = tm.ds[e];
        if (a.factor) {
            real *gf = a.factor + (size_t)b * T * C::XT;
            for (int e = li; e < T * C::XT; e += G) gf[e] = tm.Xp[e];
        }
        if (li == 0 && a.info && tm.info && a.info[b] == 0) a.info[b] = tm.info;
    }
}
#endif

// ---- backward of the implicit layer -------------------------------------------------
// DYN: also the gradients w.r.t. the affine dynamics and the initial state (mi_alqp.h, alqp_backward_* with an AlqpBwdDyn). With
// w = -H^{-1} gbar in ds, s_t = w_{t+1}[x] - F_t w_t in seq (what backward_sweep leaves there as (J d)_eq) and
// v_t = the returned lam's dynamics rows: dF_t[i][j] = -v_t[i] w_t[j] - rho s_t[i] z_t[j], dc_t[i] = -rho s_t[i],
// dx0[i] = -rho w_0[i].
template <typename real, int NX, int NU, bool DYN = false>
__global__ __launch_bounds__(64) void k_backward(BwdArgs<real, DYN> a) {
    using C = Cfg<real, NX, NU>;
    constexpr int G = C::G, N = C::N;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    real *smem = reinterpret_cast<real *>(smem_raw);
    const int lane = threadIdx.x, team = lane / G, li = lane % G;
    const int b_raw = blockIdx.x * C::QPW + team;
    const bool active = b_raw < a.B;
    const int b = active ? b_raw : a.B - 1;
    const int T = a.T;

    Team<real, NX, NU> tm;
    tm.init(smem + (size_t)team * C::team_words(T) + opaque_zero(), li, team * G, T, b);
    tm.gF = a.F + (size_t)b * (T - 1) * NX * N;
    const real *gf = a.factor + (size_t)b * T * C::XT;
    const real *gg = a.gbar + (size_t)b * T * N;
    for (int e = li; e < T * C::XT; e += G) tm.Xp[e] = gf[e];
    for (int e = li; e < T * N; e += G) tm.ds[e] = -gg[e];
    tm.rho = a.rho[b];
    wave_sync();
    tm.forward_solve_only();
    tm.backward_sweep();
    if (active) {
        const real *zf = a.z_final + (size_t)b * T * N;
        real *qg = a.q_grad + (size_t)b * T * N;
        real *Qg = a.Qd_grad + (size_t)b * T * N;
        for (int e = li; e < T * N; e += G) {
            real w = tm.ds[e];
            qg[e] = w;
            Qg[e] = w * zf[e];
        }
    }
    if constexpr (DYN) {
        // z_final and v into the slabs the backward pass leaves unused (zs, req); every team has its own
        const real *zf = a.z_final + (size_t)b * T * N;
        const int ND = (T - 1) * NX;
        if (a.dF) {
            const real *lm = a.lam + (size_t)b * a.sb_lam;
            for (int e = li; e < T * N; e += G) tm.zs[e] = zf[e];
            for (int e = li; e < ND; e += G) tm.req[e] = lm[e];
        }
        wave_sync();
        if (active) {
            const real rho = tm.rho;
            if (a.dF) {
                real *gd = a.dF + (size_t)b * ND * N;
                for (int e = li; e < ND * N; e += G) {
                    const int ti = e / N, j = e - ti * N, t = ti / NX;   // ti = t * NX + i
                    gd[e] = -tm.req[ti] * tm.ds[t * N + j] - rho * tm.seq[ti] * tm.zs[t * N + j];
                }
            }
            if (a.dc) {
                real *gd = a.dc + (size_t)b * ND;
                for (int e = li; e < ND; e += G) gd[e] = -rho * tm.seq[e];
            }
            if (a.dx0 && li < NX) a.dx0[(size_t)b * NX + li] = -rho * tm.ds[li];
        }
    }
}

template <typename real, int NX, int NU>
size_t lds_bytes_for(int T) {
    using C = Cfg<real, NX, NU>;
    return (size_t)C::QPW * C::team_words(T) * sizeof(real);
}

// Launches `fn` with one wavefront per workgroup and the team LDS image as dynamic LDS.
// `extra_words`: LDS words per team behind the team image (the hand-over region of the kernels with general rows).
template <typename real, int NX, int NU, typename Fn, typename... Args>
int launch_team_kernel_extra(Fn fn, int B, int T, int extra_words, hipStream_t stream, Args... args) {
    using C = Cfg<real, NX, NU>;
    const size_t lds = lds_bytes_for<real, NX, NU>(T) + (size_t)C::QPW * extra_words * sizeof(real);
    if (lds > kMaxLds) return ALQP_E_UNSUPPORTED;
    const unsigned grid = (unsigned)((B + C::QPW - 1) / C::QPW);
    if (lds > 48 * 1024) {
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(fn),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return ALQP_E_LAUNCH;
    }
    return launch_maybe_coop(fn, grid, lds, stream, args...);
}
template <typename real, int NX, int NU, typename Fn, typename... Args>
int launch_team_kernel(Fn fn, int B, int T, hipStream_t stream, Args... args) {
    return launch_team_kernel_extra<real, NX, NU>(fn, B, T, 0, stream, args...);
}

inline long team_simds() {   // SIMDs of the device (4 per CU)
    static long n = 0;
    if (n == 0) {
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
            cus = 256;
        n = 4L * cus;
    }
    return n;
}

#if defined(ALQP_GEN_UNIT)
template <typename real, int MASK>
int dispatch_solve_gen(int nx, int nu, const GenSolveArgs<real> &a, const TraceArgs<real> *tr, hipStream_t stream) {
    constexpr bool D = (MASK & kGenDense) != 0, X = (MASK & kGenXbox) != 0, P = (MASK & kGenPoly) != 0;
    const int extra = P ? 2 * pad4(a.m) : 0;
    return for_dims(nx, nu, ALQP_E_UNSUPPORTED, [&](auto NX, auto NU) {
        if (tr) return launch_team_kernel_extra<real, NX, NU>(k_solve_lin_gen<real, NX, NU, D, X, P, true>, a.B, a.T, extra, stream, a, *tr);
        return launch_team_kernel_extra<real, NX, NU>(k_solve_lin_gen<real, NX, NU, D, X, P, false>, a.B, a.T, extra, stream, a, TraceArgs<real>{});
    });
}
#elif defined(ALQP_ROWS_STEP_UNIT)
template <typename real>
int dispatch_step_rows(int nx, int nu, const RowsStepArgs<real> &a, hipStream_t stream) {
    const int extra = 2 * pad4(a.m);
    return for_dims(nx, nu, ALQP_E_UNSUPPORTED, [&](auto NX, auto NU) {
        if (a.xlo) return launch_team_kernel_extra<real, NX, NU>(k_newton_step_rows<real, NX, NU, true>, a.B, a.T, extra, stream, a);
        return launch_team_kernel_extra<real, NX, NU>(k_newton_step_rows<real, NX, NU, false>, a.B, a.T, extra, stream, a);
    });
}
#elif defined(ALQP_DENSE_STEP_UNIT)
template <typename real, bool POLY>
int dispatch_step_dense(int nx, int nu, const DenseStepArgs<real> &a, hipStream_t stream) {
    const int extra = POLY ? 2 * pad4(a.m) : 0;
    return for_dims(nx, nu, ALQP_E_UNSUPPORTED, [&](auto NX, auto NU) {
        if (a.xlo) return launch_team_kernel_extra<real, NX, NU>(k_newton_step_dense<real, NX, NU, true, POLY>, a.B, a.T, extra, stream, a);
        return launch_team_kernel_extra<real, NX, NU>(k_newton_step_dense<real, NX, NU, false, POLY>, a.B, a.T, extra, stream, a);
    });
}
#elif defined(ALQP_SHDYN_UNIT)
template <typename real>
int dispatch_solve_shdyn(int nx, int nu, const ShdynSolveArgs<real> &a, const TraceArgs<real> *tr, hipStream_t stream) {
    return for_dims(nx, nu, ALQP_E_UNSUPPORTED, [&](auto NX, auto NU) {   // dispatch_solve's occupancy rule
        if (tr) return launch_team_kernel<real, NX, NU>(k_solve_lin_shdyn<real, NX, NU, true>, a.B, a.T, stream, a, *tr);
        if constexpr (sizeof(real) == 4) {
            const long waves = (a.B + Cfg<real, NX, NU>::QPW - 1) / Cfg<real, NX, NU>::QPW;
            if (waves > team_simds())
                return launch_team_kernel<real, NX, NU>(k_solve_lin_shdyn<real, NX, NU, false, 2>, a.B, a.T, stream, a, TraceArgs<real>{});
        }
        return launch_team_kernel<real, NX, NU>(k_solve_lin_shdyn<real, NX, NU, false, 1>, a.B, a.T, stream, a, TraceArgs<real>{});
    });
}
#elif defined(ALQP_XBOX_STEP_UNIT)
template <typename real>
int dispatch_step_xbox(int nx, int nu, const XboxStepArgs<real> &a, hipStream_t stream) {
    return for_dims(nx, nu, ALQP_E_UNSUPPORTED, [&](auto NX, auto NU) {
        return launch_team_kernel<real, NX, NU>(k_newton_step_xbox<real, NX, NU>, a.B, a.T, stream, a);
    });
}
#else
template <typename real>
int dispatch_solve(int nx, int nu, const SolveArgs<real> &a, const TraceArgs<real> *tr, hipStream_t stream) {
    return for_dims(nx, nu, ALQP_E_UNSUPPORTED, [&](auto NX, auto NU) {
        if (tr) return launch_team_kernel<real, NX, NU>(k_solve_lin<real, NX, NU, true>, a.B, a.T, stream, a, *tr);
        if constexpr (sizeof(real) == 4) {   // only fp32 has a capped build, for more than one wavefront per SIMD
            const long waves = (a.B + Cfg<real, NX, NU>::QPW - 1) / Cfg<real, NX, NU>::QPW;
            if (waves > team_simds())
                return launch_team_kernel<real, NX, NU>(k_solve_lin<real, NX, NU, false, 2>, a.B, a.T, stream, a, TraceArgs<real>{});
        }
        return launch_team_kernel<real, NX, NU>(k_solve_lin<real, NX, NU, false, 1>, a.B, a.T, stream, a, TraceArgs<real>{});
    });
}

template <typename real>
int dispatch_step(int nx, int nu, const StepArgs<real> &a, hipStream_t stream) {
    return for_dims(nx, nu, ALQP_E_UNSUPPORTED, [&](auto NX, auto NU) {
        return launch_team_kernel<real, NX, NU>(k_newton_step<real, NX, NU>, a.B, a.T, stream, a);
    });
}
#endif

template <typename real, bool DYN>
int dispatch_backward(int nx, int nu, const BwdArgs<real, DYN> &a, hipStream_t stream) {
    return for_dims(nx, nu, ALQP_E_UNSUPPORTED, [&](auto NX, auto NU) {
        return launch_team_kernel<real, NX, NU>(k_backward<real, NX, NU, DYN>, a.B, a.T, stream, a);
    });
}

template <typename real>
size_t lds_query(int nx, int nu, int T) {
    return for_dims(nx, nu, size_t(0), [&](auto NX, auto NU) { return lds_bytes_for<real, NX, NU>(T); });
}

// The DYN instantiations of k_backward are a compile unit of their own (-DALQP_BWD_DYN_UNIT, build.sh): the unit every
// other team kernel comes out of then holds exactly the instantiations it held before they existed.
// So are the shared-dynamics instantiations of the fused solve (-DALQP_SHDYN_UNIT) and each set of its feature flags
// (-DALQP_GEN_UNIT=<mask>), and the one-step kernels with state bounds (-DALQP_XBOX_STEP_UNIT), with general rows
// (-DALQP_ROWS_STEP_UNIT) and with a dense cost (-DALQP_DENSE_STEP_UNIT=<POLY>).
#if defined(ALQP_GEN_UNIT)
template int dispatch_solve_gen<float, ALQP_GEN_UNIT>(int, int, const GenSolveArgs<float> &, const TraceArgs<float> *, hipStream_t);
template int dispatch_solve_gen<double, ALQP_GEN_UNIT>(int, int, const GenSolveArgs<double> &, const TraceArgs<double> *, hipStream_t);
#elif defined(ALQP_ROWS_STEP_UNIT)
template int dispatch_step_rows<float>(int, int, const RowsStepArgs<float> &, hipStream_t);
template int dispatch_step_rows<double>(int, int, const RowsStepArgs<double> &, hipStream_t);
#elif defined(ALQP_DENSE_STEP_UNIT)
template int dispatch_step_dense<float, ALQP_DENSE_STEP_UNIT != 0>(int, int, const DenseStepArgs<float> &, hipStream_t);
template int dispatch_step_dense<double, ALQP_DENSE_STEP_UNIT != 0>(int, int, const DenseStepArgs<double> &, hipStream_t);
#elif defined(ALQP_SHDYN_UNIT)
template int dispatch_solve_shdyn<float>(int, int, const ShdynSolveArgs<float> &, const TraceArgs<float> *, hipStream_t);
template int dispatch_solve_shdyn<double>(int, int, const ShdynSolveArgs<double> &, const TraceArgs<double> *, hipStream_t);
#elif defined(ALQP_XBOX_STEP_UNIT)
template int dispatch_step_xbox<float>(int, int, const XboxStepArgs<float> &, hipStream_t);
template int dispatch_step_xbox<double>(int, int, const XboxStepArgs<double> &, hipStream_t);
#elif !defined(ALQP_BWD_DYN_UNIT)
template int dispatch_solve<float>(int, int, const SolveArgs<float> &, const TraceArgs<float> *, hipStream_t);
template int dispatch_solve<double>(int, int, const SolveArgs<double> &, const TraceArgs<double> *, hipStream_t);
template int dispatch_step<float>(int, int, const StepArgs<float> &, hipStream_t);
template int dispatch_step<double>(int, int, const StepArgs<double> &, hipStream_t);
template int dispatch_backward<float, false>(int, int, const BwdArgs<float, false> &, hipStream_t);
template int dispatch_backward<double, false>(int, int, const BwdArgs<double, false> &, hipStream_t);
template size_t lds_query<float>(int, int, int);
template size_t lds_query<double>(int, int, int);
#else
template int dispatch_backward<float, true>(int, int, const BwdArgs<float, true> &, hipStream_t);
template int dispatch_backward<double, true>(int, int, const BwdArgs<double, true> &, hipStream_t);
#endif

}  // namespace alqp

#ifdef ALQP_PHASE_TIMING
// debug build only: read (and optionally reset) the per-phase cycle counters of k_solve_lin (team kernel)
extern "C" int alqp_debug_team_cycles(unsigned long long *out8, int reset) {
    if (out8 && hipMemcpyFromSymbol(out8, HIP_SYMBOL(alqp::g_team_cycles), 8 * sizeof(unsigned long long)) != hipSuccess) return -1;
    if (reset) {
        unsigned long long z[8] = {0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(alqp::g_team_cycles), z, sizeof(z)) != hipSuccess) return -1;
    }
    return 0;
}
#endif
