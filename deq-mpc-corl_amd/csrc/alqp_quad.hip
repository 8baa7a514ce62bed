// alqp_quad.hip - the quad kernels (4 lanes per QP, registers + DPP, HBM workspace: alqp_quad.hpp) and their
// launchers. Compiled once per dtype (-DALQP_QUAD_F32 / -DALQP_QUAD_F64), one object each.
#if defined(ALQP_BWD_DYN_UNIT) || defined(ALQP_SHDYN_UNIT)
#undef ALQP_PHASE_TIMING   // the debug counters live in the product unit only
#endif
#include <hip/hip_runtime.h>

#include "alqp_quad.hpp"
#include "alqp_dims.hpp"
#include "alqp_launch.hpp"

#if defined(ALQP_QUAD_F32) == defined(ALQP_QUAD_F64)
#error "compile alqp_quad.hip with exactly one of -DALQP_QUAD_F32, -DALQP_QUAD_F64"
#endif

namespace alqp {

// line-search merits accumulated inside the backward sweep (1) or by a pass of their own (0)
#ifndef ALQP_FUSE_LS
#define ALQP_FUSE_LS 1
#endif
// ---- fused LinDx solve, quad variant (4 lanes per instance, HBM workspace) --------------
#ifdef ALQP_PHASE_TIMING
__device__ unsigned long long g_phase_cycles[10];
#define QSTAMP(b) qd.stamp(b)
#else
#define QSTAMP(b)
#endif
// Dyn = NoDyn: affine dynamics from the caller's F, c (alqp_solve_lin). Dyn = a model of alqp_dyn.hpp:
// the nonlinear solve with that model inlined (alqp_solve_nonlin): every Newton step re-linearises
// on the device, the line search and the dual update use the true dynamics; a.F then points at the
// F region of the workspace (behind the records) and a.c is unused.
// The shared-dynamics units (-DALQP_SHDYN_UNIT, one per dtype) compile this same body as k_solve_lin_quad_shdyn, NoDyn only:
// F and c addressed through an instance stride and a stage stride (a.sb_F / a.mt_F, a.sb_c / a.mt_c; ALQP_F_STAGE /
// ALQP_C_STAGE in Quad). Two headers over one body, as in alqp_team.hip, and for the same reason.
#ifdef ALQP_SHDYN_UNIT
template <typename real, int NX, int NU, bool TRACE, class Dyn = NoDyn>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_solve_lin_quad_shdyn(ShdynSolveArgs<real> a, TraceArgs<real> tr, real *ws) {
#else
template <typename real, int NX, int NU, bool TRACE, class Dyn = NoDyn>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_solve_lin_quad(SolveArgs<real> a, TraceArgs<real> tr, real *ws) {
#endif
    using C = QCfg<real, NX, NU>;
    constexpr bool NL = Dyn::ID != 0;
    // fp64 is short of registers already: its line search keeps a pass of its own
#ifndef ALQP_FUSE_LS_F64
#define ALQP_FUSE_LS_F64 1
#endif
    constexpr bool FUSE_LS = ALQP_FUSE_LS && (sizeof(real) == 4 || ALQP_FUSE_LS_F64) && !NL;
    constexpr int N = C::N;
    if (a.skip && *a.skip != 0.0) return;  // wave-uniform
    const int lane = threadIdx.x, qi = lane >> 2;
    const int b_raw = blockIdx.x * 16 + qi;
    const bool active = b_raw < a.B;
    {
        // Phase shift between the four wavefronts of a CU (one per SIMD, all running the same sweeps): the wave
        // on SIMD s starts s * stagger * ~1024 clocks late. Started together they march in lock step and queue
        // on the CU's vector-memory pipeline in their load phases while it idles in their arithmetic phases;
        // a fifth of a sweep apart, one wave's memory phase runs under the others' panels (+5 % at the headline
        // size, delay included; shifting whole XCDs instead buys nothing: the contention is inside the CU).
        // a.stagger is set by the host (quad_stagger(): only when the grid fills the SIMDs and the launch is long
        // enough to amortise the delay); flags bits 24-31 / 20-23 override it for experiments.
        int stag = a.stagger;
        const int mode = (a.flags >> 20) & 0xf;
        if ((a.flags >> 24) & 0xff) stag = (a.flags >> 24) & 0xff;
        if (stag > 0) {
            const unsigned hw = __builtin_amdgcn_s_getreg(4 | (0 << 6) | (31 << 11));   // HW_REG_HW_ID: SIMD id in bits 5:4
            int simd = (hw >> 4) & 3;
            if (mode == 1) simd = simd * 16 + ((hw >> 8) & 0xf);   // all 64 (SIMD, CU-in-array) pairs apart
            if (mode == 2) simd &= 1;                              // two groups per CU
            if (mode == 3) simd = blockIdx.x & 1;                  // two groups of XCDs
            if (mode == 4) simd = (simd & 1) ^ (blockIdx.x & 1);   // two groups, mixed over SIMDs and XCDs
            if (mode == 5) simd = (hw >> 8) & 3;                   // four groups of CUs, a CU's SIMDs together
            for (int i = 0; i < simd * stag; ++i) __builtin_amdgcn_s_sleep(16);
        }
    }
#ifdef ALQP_ALIAS_ALL
    // experiment only (tools/phase_timing.sh -DALQP_ALIAS_ALL): every instance of an XCD-sized group
    // works on the same data, so the launch runs out of L2: what remains is the on-chip time
    const int b = (active ? b_raw : a.B - 1) % ALQP_ALIAS_ALL;
#else
    const int b = active ? b_raw : a.B - 1;
#endif
    const int T = a.T, M = C::M(T);

    Quad<real, NX, NU> qd;
    __shared__ real w_lds[QCfg<real, NX, NU>::WLDS_WORDS];   // fp64: the W panel (WPanel); one word otherwise
    qd.wl = w_lds + threadIdx.x;
    // fp32: the factor of the first stages stays in LDS between the sweeps (QCfg::KL, Quad::fchunk)
    constexpr bool FL = C::KL > 0;
    if constexpr (FL) {
        __shared__ __attribute__((aligned(16))) real l_lds[C::KL * C::FLW];
        qd.fl = (ALQP_LDS real *)l_lds;
        qd.kl = (a.flags & ALQP_FACTOR_IN_WS) ? 0 : (T < C::KL ? T : C::KL);
    }
    qd.q = lane & 3;
    qd.T = T;
    qd.active = active;
    qd.gQd = a.Qd + (size_t)b * T * N;
    qd.gq = a.q + (size_t)b * T * N;
#ifdef ALQP_SHDYN_UNIT
    qd.gF = a.F + (size_t)b * a.sb_F;
    qd.gc = a.c + (size_t)b * a.sb_c;
    qd.mt_F = a.mt_F; qd.mt_c = a.mt_c;
#else
    qd.gF = a.F + (size_t)b * (T - 1) * NX * N;
    qd.gc = a.c + (size_t)b * (T - 1) * NX;
#endif
    qd.gx0 = a.x0 + (size_t)b * NX;
    qd.gulo = a.ulo + (size_t)b * a.sb_u;
    qd.guhi = a.uhi + (size_t)b * a.sb_u;
    qd.st_u = a.st_u;
    qd.gz = a.z + (size_t)b * T * N;
    qd.glam = a.lam + (size_t)b * M;
    qd.rec = ws + C::rec_base(b, T);
    qd.gFw = const_cast<real *>(qd.gF);
    qd.dyn_h = a.dyn_h;
    qd.rho = a.rho[b];
    qd.info = 0;
    real phi_prev = a.phi[b];
#ifdef ALQP_PHASE_TIMING
    for (int i = 0; i < 10; ++i) qd.tacc[i] = 0;
#endif
    QSTAMP(-1);
    // the residual pre-pass is only needed when no forward sweep will run before r is used
    if (!(a.flags & ALQP_WS_PRIMED)) {
        if constexpr (NL) qd.stage_in(false, false);
        else qd.stage_in(a.max_newton == 0 || a.al_iter == 0 || (a.flags & ALQP_EXIT_IN_KERNEL) ||
                         (!C::PHI0_FWD && (a.flags & ALQP_INIT_MERIT)));
    }
    const bool ref_exit = (a.flags & ALQP_EXIT_IN_KERNEL) != 0;   // grid-uniform
    int gphase = 0;

    int step_id = 0;
    bool pend = false;  // a chosen step not yet applied (the next forward sweep applies it)
    real alpha_pend = 0;
    int bad = 0;
    real rn2 = 0, phi_next = 0;
    for (int it = 0; it < a.al_iter; ++it) {
        // starting merit of the iteration (al_utils.py:481): iterations > 0 get it from iter_end() of
        // the previous one; the first gets it from its first forward sweep, or from a pass of its
        // own when the launch has no Newton step
        bool phi_from_forward = false;
        if (a.flags & ALQP_INIT_MERIT) {
            if (it > 0) {
                phi_prev = phi_next;
            } else if (C::PHI0_FWD && a.max_newton > 0 && !ref_exit) {
                phi_from_forward = true;
            } else {
                if constexpr (NL) qd.template linearize<Dyn>(real(0), false);  // true residuals for the merit
                real p1[1];
                qd.template merit_candidates<1>(p1, true);
                phi_prev = p1[0];
            }
        }
        pend = false;
        double nrm_old = 0;
        int n_done = 0;
        if (ref_exit) {   // ||r+|| over the whole batch at the start of the Newton loop (al_utils.py:486)
            int bad0 = 0;
            const real r0 = it == 0 ? qd.rplus2(bad0) : rn2;   // later iterations: from iter_end() of the previous one
            nrm_old = sqrt(grid_sum_ordered(wave_sum_leaders(exit_term(r0, qor(qd.info)), active && qd.q == 0), a.exit_scratch, gphase));
        }
        for (int st = 0; st < a.max_newton; ++st, ++step_id) {
            real *tg = nullptr;
            if constexpr (TRACE) tg = (tr.g && active) ? tr.g + ((size_t)step_id * a.B + b) * T * N : nullptr;
            QSTAMP(9);  // everything between Newton steps
            if constexpr (NL) {
                qd.template linearize<Dyn>(alpha_pend, pend);
                pend = false;
            }
            // the records a launch leaves behind hold the factor of its last Newton step at every stage
            // (k_backward_quad reads it there): that step's sweep stores the LDS-held stages to the records too. With
            // the in-kernel exit any step can be the last.
            if constexpr (FL) qd.fl_ws = ref_exit || (it + 1 == a.al_iter && st + 1 == a.max_newton);
            qd.template forward<false, FL>(tg, alpha_pend, pend, (phi_from_forward && st == 0) ? &phi_prev : nullptr);
            real ph[20];
            // s_t is read again only by a merit pass of its own, by the in-kernel exit's iter_end() after every step and
            // by the iter_end() behind the last step
            const bool store_s = !FUSE_LS || ref_exit || st + 1 == a.max_newton;
            qd.template backward<FUSE_LS, FL>(ph, nullptr, store_s);
            QSTAMP(-1);
            if constexpr (TRACE) {
                if (tr.d && active) {
                    real *td = tr.d + ((size_t)step_id * a.B + b) * T * N;
                    for (int t = 0; t < T; ++t)
                        for (int j = qd.q; j < N; j += 4) td[t * N + j] = qd.recp(t)[C::wn(C::oY, j)];
                }
            }
            if constexpr (NL) qd.template merit_nonlin<Dyn>(ph);
            else if constexpr (!FUSE_LS) qd.template merit_candidates<20>(ph, false);
            QSTAMP(6);  // line-search candidates
            int kbest = 0;
            real best = ph[0];
#pragma unroll
            for (int k = 1; k < 20; ++k) {
                if (k < a.n_ls && !(best != best) && (ph[k] != ph[k] || ph[k] < best)) {
                    best = ph[k];
                    kbest = k;
                }
            }
            const bool acc = best < phi_prev;
            if constexpr (TRACE) {
                if (active && qd.q == 0) {
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
            pend = true;  // applied by the next forward sweep or by iter_end()
            alpha_pend = alpha;
            QSTAMP(7);  // pick
            phi_prev = best;  // merit <- new_merit even when rejected (al_utils.py:569)
            if (ref_exit) {
                // apply the step now (what the end of a one-step launch does), ||r+||^2 at the new iterate, then the
                // reference's batch-global test (al_utils.py:551-564; alqp_exit_test between launches otherwise)
                int bad1 = 0;
                real ph_unused = 0, r1 = 0;
                qd.template iter_end<Dyn>(alpha_pend, pend, false, (real)a.rho_scale, false, ph_unused, r1, bad1);
                pend = false;
                const double nw = sqrt(grid_sum_ordered(wave_sum_leaders(exit_term(r1, qor(qd.info)), active && qd.q == 0), a.exit_scratch, gphase));
                ++n_done;
                if (nw < a.exit_tol || fabs(nrm_old - nw) / nw < a.exit_tol) break;
                nrm_old = nw;
            }
        }
        if (ref_exit && a.newton_counts && blockIdx.x == 0 && lane == 0) a.newton_counts[it] = grid_barrier_timed_out(a.exit_scratch) ? -1 : n_done;
        bad = 0;
        qd.template iter_end<Dyn>(alpha_pend, pend, (a.flags & ALQP_DUAL_UPDATE) != 0, (real)a.rho_scale, it + 1 == a.al_iter,
                    phi_next, rn2, bad);
        pend = false;
    }
    if (a.al_iter <= 0) {
        rn2 = qd.rplus2(bad);
        qd.stage_out();
    }
#ifdef ALQP_PHASE_TIMING
    QSTAMP(9);
    if (lane == 0)
        for (int i = 0; i < 10; ++i) atomicAdd(&g_phase_cycles[i], qd.tacc[i]);
#endif
    if (active && qd.q == 0) {
        a.rho[b] = qd.rho;
        a.phi[b] = phi_prev;
        if (a.rnorm2) a.rnorm2[b] = rn2;
        if (a.info && qd.info && a.info[b] == 0) a.info[b] = qd.info;  // sticky: first failure of the solve
        if (a.status) a.status[b] = bad ? 0 : 1;
    }
}

// ---- backward of the implicit layer, quad variant: the factor is the workspace a previous
//      quad solve left behind (per-stage lower triangles of L) ---------------------------------
// DYN: also the gradients w.r.t. the affine dynamics and the initial state (mi_alqp.h, alqp_backward_* with an AlqpBwdDyn). w_t is
// the record's y/d field; a lane owns rows i = q (mod 4) of F_t as in the sweeps and, per own row, forms
// s_t[i] = w_{t+1}[i] - F_t[i] . w_t from F and w (the record's s group is not relied on) and writes the row of dF_t.
template <typename real, int NX, int NU, bool DYN = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_backward_quad(BwdArgs<real, DYN> a, real *ws) {
    using C = QCfg<real, NX, NU>;
    constexpr int N = C::N;
    const int lane = threadIdx.x, qi = lane >> 2;
    const int b_raw = blockIdx.x * 16 + qi;
    const bool active = b_raw < a.B;
    const int b = active ? b_raw : a.B - 1;
    const int T = a.T;
    Quad<real, NX, NU> qd;
    __shared__ real w_lds[QCfg<real, NX, NU>::WLDS_WORDS];   // fp64: the W panel (WPanel); one word otherwise
    qd.wl = w_lds + threadIdx.x;
    qd.q = lane & 3;
    qd.T = T;
    qd.active = active;
    qd.gF = a.F + (size_t)b * (T - 1) * NX * N;
    qd.gQd = nullptr; qd.gq = nullptr; qd.gc = nullptr; qd.gx0 = nullptr; qd.gulo = nullptr; qd.guhi = nullptr;
    qd.st_u = 0;
    qd.gz = nullptr; qd.glam = nullptr;
    qd.rec = ws + C::rec_base(b, T);
    qd.rho = a.rho[b];
    qd.info = 0;
    qd.solve_forward(a.gbar + (size_t)b * T * N);
    real unused[20];
    qd.template backward<false>(unused);
    if (active) {
        const real *zf = a.z_final + (size_t)b * T * N;
        real *qg = a.q_grad + (size_t)b * T * N;
        real *Qg = a.Qd_grad + (size_t)b * T * N;
        for (int t = 0; t < T; ++t)
            for (int j = qd.q; j < N; j += 4) {
                const real w = qd.recp(t)[C::wn(C::oY, j)];
                qg[t * N + j] = w;
                Qg[t * N + j] = w * zf[t * N + j];
            }
    }
    if constexpr (DYN) {
        constexpr int SW = C::SW;
        const real rho = qd.rho;
        const size_t bd = (size_t)b * (T - 1) * NX;   // this instance's first dynamics row
        const real *zf = a.z_final + (size_t)b * T * N;
        const real *lm = a.lam ? a.lam + (size_t)b * a.sb_lam : nullptr;
        for (int t = 0; t + 1 < T; ++t) {
            real wt[N], wnx[SW];
            qd.ld_rep_n(qd.recp(t) + C::oY, wt);
            qd.ld_ownx_of_n(qd.recp(t + 1) + C::oY, wnx);
            real zt[N];
            if (a.dF) gload<N>(zf + t * N, zt);
#pragma unroll
            for (int s = 0; s < SW; ++s) {
                const int r = 4 * s + qd.q;
                const bool own = (4 * s + 3 < NX || r < NX) && active;   // padding quads alias instance B - 1: no writes
                const int rc = (4 * s + 3 < NX || r < NX) ? r : NX - 1;
                real fr[N];
                gload<N>(qd.gF + ((size_t)t * NX + rc) * N, fr);
                real p = 0;
#pragma unroll
                for (int k = 0; k < N; ++k) p = fma_(fr[k], wt[k], p);
                const real si = wnx[s] - p;
                if (a.dF) {
                    const real v = lm[t * NX + rc];
                    real row[N];
#pragma unroll
                    for (int k = 0; k < N; ++k) row[k] = -v * wt[k] - rho * si * zt[k];
                    if (own) qd.template gstore<N>(a.dF + (bd + (size_t)t * NX + r) * N, row);
                }
                if (a.dc && own) a.dc[bd + (size_t)t * NX + r] = -rho * si;
            }
        }
        if (a.dx0) {
            real w0[SW];
            qd.ld_ownx_of_n(qd.recp(0) + C::oY, w0);
#pragma unroll
            for (int s = 0; s < SW; ++s) {
                const int r = 4 * s + qd.q;
                if ((4 * s + 3 < NX || r < NX) && active) a.dx0[(size_t)b * NX + r] = -rho * w0[s];
            }
        }
    }
}

// ---- one Newton direction (nonlinear-caller mode), quad variant: 16 instances per wavefront, the
//      factor streamed through (and left in) the workspace records, like the fused quad solve. The
//      caller evaluated dx_jac -> (xnext = f(z), F) in PyTorch (al_utils.py:233-248); the sweeps run on the
//      linearisation F at z with the true residual z_{t+1}[x] - xnext_t.
template <typename real, int NX, int NU>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_newton_step_quad(StepArgs<real> a, real *ws) {
    using C = QCfg<real, NX, NU>;
    constexpr int N = C::N, SW = C::SW;
    const int lane = threadIdx.x, qi = lane >> 2;
    const int b_raw = blockIdx.x * 16 + qi;
    const bool active = b_raw < a.B;
    const int b = active ? b_raw : a.B - 1;
    const int T = a.T, M = C::M(T) + T * a.nobs;   // obstacle rows behind each stage's bound rows
    Quad<real, NX, NU> qd;
    __shared__ real w_lds[QCfg<real, NX, NU>::WLDS_WORDS];   // fp64: the W panel (WPanel); one word otherwise
    qd.wl = w_lds + threadIdx.x;
    qd.q = lane & 3;
    qd.T = T;
    qd.active = active;
    qd.gQd = a.Qd + (size_t)b * T * N;
    qd.gq = a.q + (size_t)b * T * N;
    qd.gF = a.F + (size_t)b * (T - 1) * NX * N;
    qd.gc = nullptr;
    qd.gx0 = a.x0 + (size_t)b * NX;
    qd.gulo = a.ulo + (size_t)b * a.sb_u;
    qd.guhi = a.uhi + (size_t)b * a.sb_u;
    qd.st_u = a.st_u;
    qd.gz = const_cast<real *>(a.z) + (size_t)b * T * N;        // read-only here
    qd.glam = const_cast<real *>(a.lam) + (size_t)b * M;        // read-only here
    qd.rec = ws + C::rec_base(b, T);
    qd.gFw = const_cast<real *>(qd.gF);
    qd.dyn_h = 0;
    qd.rho = a.rho[b];
    qd.info = 0;
    qd.nobs = a.nobs;
    qd.gobs = a.nobs > 0 ? a.obs + (size_t)b * T * a.nobs * 3 : nullptr;
    qd.obs_r2 = a.obs_r2;
    qd.no_init = a.no_init != 0;
    // no copy-in: the forward sweep reads the caller's arrays itself and takes r_t = z_{t+1}[x] - xnext_t
    const real *gxn = a.xnext + (size_t)b * (T - 1) * NX;
    real *tg = (a.g_out && active) ? a.g_out + (size_t)b * T * N : nullptr;
    qd.template forward<true>(tg, real(0), false, nullptr, gxn);
    real unused[20];
    qd.template backward<false>(unused, a.d_out + (size_t)b * T * N);
    if (active) {
        if (qd.q == 0 && a.info && qd.info && a.info[b] == 0) a.info[b] = qd.info;
    }
}


template <typename real, int NX, int NU, typename Fn, typename... Args>
int launch_quad_kernel(Fn fn, int B, hipStream_t stream, Args... args) {
    const unsigned grid = (unsigned)((B + 15) / 16);
    return launch_maybe_coop(fn, grid, 0, stream, args...);
}

#ifdef ALQP_SHDYN_UNIT
template <typename real>
int dispatch_solve_quad_shdyn(int nx, int nu, const ShdynSolveArgs<real> &a, const TraceArgs<real> *tr, real *ws,
                              hipStream_t stream) {
    return for_dims(nx, nu, ALQP_E_UNSUPPORTED, [&](auto NX, auto NU) {
        if (tr) return launch_quad_kernel<real, NX, NU>(k_solve_lin_quad_shdyn<real, NX, NU, true>, a.B, stream, a, *tr, ws);
        return launch_quad_kernel<real, NX, NU>(k_solve_lin_quad_shdyn<real, NX, NU, false>, a.B, stream, a, TraceArgs<real>{}, ws);
    });
}
#else
template <typename real>
int dispatch_solve_quad(int nx, int nu, const SolveArgs<real> &a, const TraceArgs<real> *tr, real *ws,
                        hipStream_t stream) {
    return for_dims(nx, nu, ALQP_E_UNSUPPORTED, [&](auto NX, auto NU) {
        if (tr) return launch_quad_kernel<real, NX, NU>(k_solve_lin_quad<real, NX, NU, true>, a.B, stream, a, *tr, ws);
        return launch_quad_kernel<real, NX, NU>(k_solve_lin_quad<real, NX, NU, false>, a.B, stream, a, TraceArgs<real>{}, ws);
    });
}

template <typename real, bool DYN>
int dispatch_backward_quad(int nx, int nu, const BwdArgs<real, DYN> &a, real *ws, hipStream_t stream) {
    return for_dims(nx, nu, ALQP_E_UNSUPPORTED, [&](auto NX, auto NU) {
        return launch_quad_kernel<real, NX, NU>(k_backward_quad<real, NX, NU, DYN>, a.B, stream, a, ws);
    });
}

// nonlinear fused solve: the models of alqp_dyn.hpp, each with its own (nx, nu)
template <typename real>
int dispatch_solve_nonlin(int dyn_id, int nx, int nu, const SolveArgs<real> &a, real *ws, hipStream_t stream) {
    if (dyn_id == DynPendulum1l<real>::ID && nx == 2 && nu == 1)
        return launch_quad_kernel<real, 2, 1>(k_solve_lin_quad<real, 2, 1, false, DynPendulum1l<real>>, a.B, stream, a,
                                              TraceArgs<real>{}, ws);
    if (dyn_id == DynCartpole1l<real>::ID && nx == 4 && nu == 1)
        return launch_quad_kernel<real, 4, 1>(k_solve_lin_quad<real, 4, 1, false, DynCartpole1l<real>>, a.B, stream, a,
                                              TraceArgs<real>{}, ws);
    if (dyn_id == DynCartpole1l<real, 2>::ID && nx == 4 && nu == 1)
        return launch_quad_kernel<real, 4, 1>(k_solve_lin_quad<real, 4, 1, false, DynCartpole1l<real, 2>>, a.B, stream, a,
                                              TraceArgs<real>{}, ws);
    if (dyn_id == DynCartpole2l<real>::ID && nx == 6 && nu == 1)
        return launch_quad_kernel<real, 6, 1>(k_solve_lin_quad<real, 6, 1, false, DynCartpole2l<real>>, a.B, stream, a,
                                              TraceArgs<real>{}, ws);
    return ALQP_E_UNSUPPORTED;
}

template <typename real>
int dispatch_step_quad(int nx, int nu, const StepArgs<real> &a, real *ws, hipStream_t stream) {
    return for_dims(nx, nu, ALQP_E_UNSUPPORTED, [&](auto NX, auto NU) {
        return launch_quad_kernel<real, NX, NU>(k_newton_step_quad<real, NX, NU>, a.B, stream, a, ws);
    });
}
#endif

#ifdef ALQP_QUAD_F32
using quad_real = float;
#else
using quad_real = double;
#endif
// The DYN instantiations of k_backward_quad are a compile unit of their own per dtype (-DALQP_BWD_DYN_UNIT, build.sh): the
// unit every other quad kernel comes out of then holds exactly the instantiations it held before they existed.
// So are the shared-dynamics instantiations of the fused solve (-DALQP_SHDYN_UNIT).
#if defined(ALQP_SHDYN_UNIT)
template int dispatch_solve_quad_shdyn<quad_real>(int, int, const ShdynSolveArgs<quad_real> &, const TraceArgs<quad_real> *, quad_real *, hipStream_t);
#elif !defined(ALQP_BWD_DYN_UNIT)
template int dispatch_solve_quad<quad_real>(int, int, const SolveArgs<quad_real> &, const TraceArgs<quad_real> *, quad_real *, hipStream_t);
template int dispatch_backward_quad<quad_real, false>(int, int, const BwdArgs<quad_real, false> &, quad_real *, hipStream_t);
template int dispatch_solve_nonlin<quad_real>(int, int, int, const SolveArgs<quad_real> &, quad_real *, hipStream_t);
template int dispatch_step_quad<quad_real>(int, int, const StepArgs<quad_real> &, quad_real *, hipStream_t);
#else
template int dispatch_backward_quad<quad_real, true>(int, int, const BwdArgs<quad_real, true> &, quad_real *, hipStream_t);
#endif

}  // namespace alqp

#if defined(ALQP_PHASE_TIMING) && defined(ALQP_QUAD_F32)
// debug build only: read (and optionally reset) the per-phase cycle counters of k_solve_lin_quad
extern "C" int alqp_debug_phase_cycles(unsigned long long *out10, int reset) {
    if (out10 && hipMemcpyFromSymbol(out10, HIP_SYMBOL(alqp::g_phase_cycles), 10 * sizeof(unsigned long long)) != hipSuccess) return -1;
    if (reset) {
        unsigned long long z[10] = {0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(alqp::g_phase_cycles), z, sizeof(z)) != hipSuccess) return -1;
    }
    return 0;
}
#endif
