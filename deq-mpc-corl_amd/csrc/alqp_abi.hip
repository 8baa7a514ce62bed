// alqp_abi.hip - host side of the C ABI of include/mi_alqp.h: argument checks, the choice between the team and the
// quad kernels, workspace sizes. No kernel is defined or instantiated here; launches go through alqp_launch.hpp.
// No torch types anywhere: plain device pointers in, kernel launches on the caller's stream.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "alqp_team.hpp"   // Cfg
#include "alqp_quad.hpp"   // QCfg
#include "alqp_dims.hpp"
#include "alqp_launch.hpp"
#include "alqp_team_nl.hpp"   // NlRowsSolveArgs, dispatch_solve_nonlin_rows
#include "mi_alqp.h"

namespace alqp {

template <typename real>
size_t quad_ws_bytes(int nx, int nu, int B, int T) {
    return for_dims(nx, nu, size_t(0), [&](auto NX, auto NU) {
        using C = QCfg<real, NX, NU>;
        return C::ws_covers(B, T) ? C::ws_words(B, T) * sizeof(real) : size_t(0);
    });
}

static int qpw_query(int nx, int nu) {
    return for_dims(nx, nu, 0, [](auto NX, auto NU) { return (int)Cfg<float, NX, NU>::QPW; });
}

// ---- start offset between the wavefronts of a CU for the quad solve (SolveArgs::stagger) -------------------
// mode = AlqpParams.quad_stagger: 0 automatic, < 0 off, > 0 explicit units of ~1024 clocks (a per-call argument: the library
// keeps no process state)
static int quad_stagger(int mode, int B, int T, int nx, int nu, int newton_steps, bool f64) {
    if (mode < 0) return 0;
    if (mode > 0) return mode;
    static int n_simd = 0;
    if (n_simd == 0) {
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
            cus = 256;
        n_simd = 4 * cus;
    }
    const long waves = (B + 15) / 16;
    if (4 * waves < 3 * (long)n_simd || newton_steps < 1) return 0;   // SIMDs not filled: nothing to de-phase
    // measured per size at B = 16384 (profiles/r02/experiments): (13,4) T=20 +1.7 %, T=50 +1.2 %, (14,4) +1.7 %,
    // (6,2) +0.8 %, (8,2) -0.3 %, (2,1) at B = 65536 -2.5 %: only the sizes with long stages gain
    if (nx + nu < 12) return 0;
    // clocks per stage and sweep, fitted on the compiled sizes ((13,4): 26 k, (8,2): 12 k, (6,2): 7 k)
    const int n = nx + nu;
    double period = 2000.0 * n - 8000.0;
    if (period < 3000.0) period = 3000.0;
    if (f64) period *= 1.4;   // fp64 sweeps take 2.4x as long; measured: 140 units beat 100 at (13,4), T = 20
    // a fifth of a sweep between neighbouring SIMDs (measured optimum at (13,4), T = 20: 100-125 units), but the
    // last wave's delay (3 offsets) stays below ~6 % of the launch
    double frac = 0.04 * newton_steps;
    if (frac > 0.2) frac = 0.2;
    return (int)(frac * T * period / 1024.0 + 0.5);
}

// The automatic choice between the team and the quad kernels of the fused solve (alqp_pick_variant, AlqpParams.variant
// 0): the only copy of the rule. 1 team, 2 quad, 0: no (nx, nu) instance.
// Quad once the batch fills the chip (16 instances per wavefront, 1024 SIMDs), team below (2-2.4x lower latency at small
// batches; measured on MI355X at (13,4) T=20: B=128 0.83 vs 1.94 ms, B=4096 2.11 vs 2.08 ms, B=16384 8.2 vs 3.4 ms; (8,2)
// T=10 crosses near B=5000). The team kernels' time is a step function of the batch - 2048 (fp32) / 1024 (fp64) teams
// fit the chip at once - and B = 4096 is exactly two / four full rounds: measured at (13,4) T=20 after round 3's
// team-kernel work, fp32 B = 4096 team 1.83 vs quad 2.00 ms, B = 5120 2.36 vs 2.08; fp64 B = 4096 4.35 vs 4.71, B = 5120
// 5.42 vs 5.02 (profiles/r03/experiments/README.md).
template <typename real>
int pick_variant(const AlqpDims *dims, int flags, long quad_min_batch) {
    const size_t team_lds = lds_query<real>(dims->nx, dims->nu, dims->T);
    if (team_lds == 0) return 0;
    if (flags & ALQP_SAVE_FACTOR) return 1;   // only the team kernels write the packed factor
    long qmin = quad_min_batch;
    if (qmin < 0) {
        // whole-wavefront teams (2n + nx + 1 > 32 rows, e.g. (13,4)): team through B = 4096 (full rounds), quad beyond;
        // smaller teams share a wavefront and were not re-measured: round 2's rule
        const bool wave_team = 2 * (dims->nx + dims->nu) + dims->nx + 1 > 32;
        qmin = wave_team ? 4097 : (sizeof(real) == 8 ? 4608 : 4096);
    }
    // long horizons whose factor does not fit the team's LDS image run on the quad kernels at any batch
    return (dims->B >= qmin || team_lds > kMaxLds) ? 2 : 1;
}

// The nullable AlqpTrace of the C ABI -> the kernels' TraceArgs (all null without one).
template <typename real>
TraceArgs<real> trace_args(const AlqpTrace *trace) {
    TraceArgs<real> tr = {};
    if (trace) {
        tr.g = (real *)trace->g; tr.d = (real *)trace->d; tr.phi = (real *)trace->phi;
        tr.phi_prev = (real *)trace->phi_prev; tr.k = trace->k; tr.accept = trace->accept;
    }
    return tr;
}

// The SolveArgs fields that alqp_solve_lin and alqp_solve_nonlin fill alike; F, c, factor, stagger and dyn_h are the
// caller's. false: ALQP_EXIT_IN_KERNEL without its scratch or together with a skip flag (ALQP_E_BADARG).
template <typename real>
bool set_solve(const AlqpDims *dims, const AlqpParams *prm, const void *Qd, const void *q, const void *x0,
               const void *u_lo, const void *u_hi, long sb_u, long st_u, void *z, void *lam, void *rho, void *phi,
               void *rnorm2, int *info, unsigned char *status, SolveArgs<real> &a) {
    a.B = dims->B; a.T = dims->T;
    a.al_iter = prm->al_iter; a.max_newton = prm->max_newton; a.n_ls = prm->n_ls; a.flags = prm->flags;
    a.rho_scale = (real)prm->rho_scale;
    a.Qd = (const real *)Qd; a.q = (const real *)q; a.x0 = (const real *)x0;
    a.ulo = (const real *)u_lo; a.uhi = (const real *)u_hi; a.sb_u = sb_u; a.st_u = st_u;
    a.z = (real *)z; a.lam = (real *)lam; a.rho = (real *)rho; a.phi = (real *)phi;
    a.rnorm2 = (real *)rnorm2; a.info = info; a.status = status;
    a.skip = prm->skip_flag;
    if (prm->flags & ALQP_EXIT_IN_KERNEL) {
        if (!prm->exit_scratch || prm->skip_flag) return false;
        a.exit_tol = prm->exit_tol; a.newton_counts = prm->newton_counts; a.exit_scratch = prm->exit_scratch;
    }
    return true;
}

// Args: SolveArgs (alqp_solve_lin_*) or ShdynSolveArgs with its strides set by the caller (alqp_solve_lin_shared_*);
// `team` / `quad`: the two kernel families' launchers for that type. Checks, kernel choice and workspace handling are
// this one function for both entry points.
template <typename real, typename Args>
int solve_lin_impl(const AlqpDims *dims, const AlqpParams *prm, const void *Qd, const void *q,
                   const void *F, const void *c, const void *x0, const void *u_lo, const void *u_hi,
                   long sb_u, long st_u, void *z, void *lam, void *rho, void *phi, void *rnorm2,
                   int *info, unsigned char *status, void *factor_out, const AlqpTrace *trace,
                   void *workspace, size_t ws_bytes, void *stream, Args a,
                   int (*team)(int, int, const Args &, const TraceArgs<real> *, hipStream_t),
                   int (*quad)(int, int, const Args &, const TraceArgs<real> *, real *, hipStream_t)) {
    if (!dims_ok(dims) || !prm || !Qd || !q || !F || !c || !x0 || !u_lo || !u_hi || !z || !lam || !rho || !phi)
        return ALQP_E_BADARG;
    if (prm->n_ls < 1 || prm->n_ls > 20 || prm->al_iter < 0 || prm->max_newton < 0) return ALQP_E_BADARG;
    if ((prm->flags & ALQP_SAVE_FACTOR) && !factor_out) return ALQP_E_BADARG;
    if ((prm->flags & ALQP_EXIT_IN_KERNEL) && trace) return ALQP_E_BADARG;
    if (!set_solve<real>(dims, prm, Qd, q, x0, u_lo, u_hi, sb_u, st_u, z, lam, rho, phi, rnorm2, info, status, a))
        return ALQP_E_BADARG;
    a.F = (const real *)F; a.c = (const real *)c; a.factor = (real *)factor_out;
    a.stagger = quad_stagger(prm->quad_stagger, dims->B, dims->T, dims->nx, dims->nu, prm->al_iter * prm->max_newton, sizeof(real) == 8);
    const TraceArgs<real> tr = trace_args<real>(trace);
    // variant: 1 = team (factor in LDS), 2 = quad (4 lanes/instance, HBM workspace), 0 = auto
    const size_t need = quad_ws_bytes<real>(dims->nx, dims->nu, dims->B, dims->T);
    int variant = prm->variant;
    if (variant == 0) {
        variant = pick_variant<real>(dims, prm->flags, -1);
        if (variant == 0) return ALQP_E_UNSUPPORTED;
        if (variant == 2 && !(need > 0 && workspace && ws_bytes >= need)) variant = 1;   // no workspace to run quad on
    }
    if (variant == 2) {
        if (prm->flags & ALQP_SAVE_FACTOR) return ALQP_E_UNSUPPORTED;
        if (need == 0) return ALQP_E_UNSUPPORTED;
        if (!workspace || ws_bytes < need) return ALQP_E_BADARG;
        return quad(dims->nx, dims->nu, a, trace ? &tr : nullptr, (real *)workspace, (hipStream_t)stream);
    }
    if (variant != 1) return ALQP_E_BADARG;
    return team(dims->nx, dims->nu, a, trace ? &tr : nullptr, (hipStream_t)stream);
}

// Batch-shared dynamics: the plain solve with F and c behind an instance stride and a stage stride. Only the three
// layouts of mi_alqp.h are taken (any other pair would be a bug in the caller, and a stride beyond the caller's tensor an
// out-of-bounds read).
template <typename real>
int solve_lin_shared_impl(const AlqpDims *dims, const AlqpParams *prm, const void *Qd, const void *q, const void *F,
                          const void *c, long sb_F, long st_F, long sb_c, long st_c, const void *x0, const void *u_lo,
                          const void *u_hi, long sb_u, long st_u, void *z, void *lam, void *rho, void *phi,
                          void *rnorm2, int *info, unsigned char *status, void *factor_out, const AlqpTrace *trace,
                          void *workspace, size_t ws_bytes, void *stream) {
    if (!dims_ok(dims) || !F || !c) return ALQP_E_BADARG;
    const long wF = (long)dims->nx * (dims->nx + dims->nu), wc = dims->nx, Tm = dims->T - 1;
    auto form_ok = [&](long sb, long st, long w) {
        return (sb == 0 && st == 0) || (sb == 0 && st == w) || (sb == Tm * w && st == w);
    };
    if (sb_F < 0 || st_F < 0 || sb_c < 0 || st_c < 0 || !form_ok(sb_F, st_F, wF) || !form_ok(sb_c, st_c, wc))
        return ALQP_E_BADARG;
    ShdynSolveArgs<real> a = {};
    a.sb_F = sb_F; a.sb_c = sb_c;
    a.mt_F = st_F ? -1 : 0; a.mt_c = st_c ? -1 : 0;   // (form_ok: a stage stride is 0 or the packed one)
    return solve_lin_impl<real, ShdynSolveArgs<real>>(dims, prm, Qd, q, F, c, x0, u_lo, u_hi, sb_u, st_u, z, lam, rho, phi,
                                                      rnorm2, info, status, factor_out, trace, workspace, ws_bytes, stream,
                                                      a, dispatch_solve_shdyn<real>, dispatch_solve_quad_shdyn<real>);
}

// Dense stage cost (C), state box rows (x_lo, x_hi) and general rows G_t z_t <= h_t (G, h, m), any non-empty set of them:
// the non-null set is the mask that picks the object (build.sh, alqp_team_gen_*), and `accept` holds bit (1 << mask) for
// every mask the calling entry point takes (alqp_solve_lin_dense_* / _xbox_* / _poly_*: its own feature alone;
// alqp_solve_lin_gen_*: two or three). The team kernel only: no quad kernel reads a full C or knows such rows, so no
// workspace and variant 0 / 1 alike. Qd is ignored with a C.
template <typename real>
int solve_lin_feat_impl(int accept, const AlqpDims *dims, const AlqpParams *prm, const void *Qd, const void *q,
                        const void *F, const void *c, const void *x0, const void *u_lo, const void *u_hi, long sb_u,
                        long st_u, void *z, void *lam, void *rho, void *phi, void *rnorm2, int *info,
                        unsigned char *status, void *factor_out, const AlqpTrace *trace, void *stream, const void *Cm,
                        const void *x_lo, const void *x_hi, long sb_x, long st_x, const void *G, const void *h, int m,
                        long sb_g, long st_g, long sb_h, long st_h) {
    if (!dims_ok(dims) || !prm || !q || !F || !c || !x0 || !u_lo || !u_hi || !z || !lam || !rho || !phi)
        return ALQP_E_BADARG;
    if (!x_lo != !x_hi || !G != !h) return ALQP_E_BADARG;
    const int mask = (Cm ? kGenDense : 0) | (x_lo ? kGenXbox : 0) | (G ? kGenPoly : 0);
    if (!(accept >> mask & 1)) return ALQP_E_BADARG;   // a feature's pointers missing, or not this entry point's set
    if (!Cm && !Qd) return ALQP_E_BADARG;
    if (prm->n_ls < 1 || prm->n_ls > 20 || prm->al_iter < 0 || prm->max_newton < 0) return ALQP_E_BADARG;
    if (prm->variant != 0 && prm->variant != 1) return ALQP_E_BADARG;
    if (x_lo && (sb_x < 0 || st_x < 0)) return ALQP_E_BADARG;
    if (G && (m < 1 || m > 64 || sb_g < 0 || st_g < 0 || sb_h < 0 || st_h < 0)) return ALQP_E_BADARG;
    if ((prm->flags & ALQP_SAVE_FACTOR) && !factor_out) return ALQP_E_BADARG;
    if ((prm->flags & ALQP_EXIT_IN_KERNEL) && trace) return ALQP_E_BADARG;
    // the horizon must fit the LDS: the team image, plus the hand-over region of 2 pad4(m) words per team with rows (there is
    // no quad kernel to fall back on). Not with the dense cost alone: that entry point has always left this to the launcher,
    // which answers the same ALQP_E_UNSUPPORTED, but behind set_solve's ALQP_E_BADARG.
    if (mask != kGenDense) {
        const size_t img = lds_query<real>(dims->nx, dims->nu, dims->T);
        if (img == 0) return ALQP_E_UNSUPPORTED;
        const size_t lds = img + (G ? (size_t)qpw_query(dims->nx, dims->nu) * 2 * pad4(m) * sizeof(real) : 0);
        if (lds > kMaxLds) return ALQP_E_UNSUPPORTED;
    }
    GenSolveArgs<real> a = {};
    if (!set_solve<real>(dims, prm, Cm ? nullptr : Qd, q, x0, u_lo, u_hi, sb_u, st_u, z, lam, rho, phi, rnorm2, info,
                         status, a))
        return ALQP_E_BADARG;
    a.C = (const real *)Cm;
    if (x_lo) { a.xlo = (const real *)x_lo; a.xhi = (const real *)x_hi; a.sb_x = sb_x; a.st_x = st_x; }
    if (G) {
        a.G = (const real *)G; a.h = (const real *)h; a.m = m;
        a.sb_g = sb_g; a.st_g = st_g; a.sb_h = sb_h; a.st_h = st_h;
    }
    a.F = (const real *)F; a.c = (const real *)c; a.factor = (real *)factor_out;
    const TraceArgs<real> tr = trace_args<real>(trace);
    const TraceArgs<real> *trp = trace ? &tr : nullptr;
    const hipStream_t s = (hipStream_t)stream;
    switch (mask) {
        case 1: return dispatch_solve_gen<real, 1>(dims->nx, dims->nu, a, trp, s);
        case 2: return dispatch_solve_gen<real, 2>(dims->nx, dims->nu, a, trp, s);
        case 3: return dispatch_solve_gen<real, 3>(dims->nx, dims->nu, a, trp, s);
        case 4: return dispatch_solve_gen<real, 4>(dims->nx, dims->nu, a, trp, s);
        case 5: return dispatch_solve_gen<real, 5>(dims->nx, dims->nu, a, trp, s);
        case 6: return dispatch_solve_gen<real, 6>(dims->nx, dims->nu, a, trp, s);
        default: return dispatch_solve_gen<real, 7>(dims->nx, dims->nu, a, trp, s);
    }
}
// the masks an entry point takes, as solve_lin_feat_impl's `accept`
constexpr int kAcceptDense = 1 << kGenDense, kAcceptXbox = 1 << kGenXbox, kAcceptPoly = 1 << kGenPoly;
constexpr int kAcceptGen = 1 << 3 | 1 << 5 | 1 << 6 | 1 << 7;   // two or three features

// nonlinear fused solve: workspace = [records | F linearisations [B][T-1][nx][n]]
template <typename real>
size_t nonlin_ws_bytes(int nx, int nu, int B, int T) {
    const size_t rec = quad_ws_bytes<real>(nx, nu, B, T);
    if (rec == 0) return 0;
    return rec + (size_t)B * (T - 1) * nx * (nx + nu) * sizeof(real);
}

template <typename real>
int solve_nonlin_impl(const AlqpDims *dims, const AlqpParams *prm, int dyn_id, double dyn_h, const void *Qd, const void *q,
                      const void *x0, const void *u_lo, const void *u_hi, long sb_u, long st_u, void *z, void *lam,
                      void *rho, void *phi, void *rnorm2, int *info, unsigned char *status, void *workspace,
                      size_t ws_bytes, void *stream) {
    if (!dims_ok(dims) || !prm || !Qd || !q || !x0 || !u_lo || !u_hi || !z || !lam || !rho || !phi || !workspace)
        return ALQP_E_BADARG;
    if (prm->n_ls != 20 || prm->al_iter < 0 || prm->max_newton < 0) return ALQP_E_BADARG;
    if (prm->flags & (ALQP_SAVE_FACTOR | ALQP_WS_PRIMED)) return ALQP_E_UNSUPPORTED;
    const size_t need = nonlin_ws_bytes<real>(dims->nx, dims->nu, dims->B, dims->T);
    if (need == 0) return ALQP_E_UNSUPPORTED;
    if (ws_bytes < need) return ALQP_E_BADARG;
    SolveArgs<real> a = {};
    if (!set_solve(dims, prm, Qd, q, x0, u_lo, u_hi, sb_u, st_u, z, lam, rho, phi, rnorm2, info, status, a))
        return ALQP_E_BADARG;
    a.F = (const real *)((const char *)workspace + quad_ws_bytes<real>(dims->nx, dims->nu, dims->B, dims->T));
    a.dyn_h = (real)dyn_h;
    return dispatch_solve_nonlin<real>(dyn_id, dims->nx, dims->nu, a, (real *)workspace, (hipStream_t)stream);
}

// nonlinear fused solve with state bounds and / or general rows (team kernel, alqp_team_nl.hpp): per instance
// F[T-1][nx][n], then xnext[T-1][nx]. 0: no compiled-in model has this (nx, nu) on that route.
template <typename real>
size_t nonlin_rows_ws_bytes(int nx, int nu, int B, int T) {
    if (nu != 1 || (nx != 2 && nx != 4)) return 0;   // pendulum1l, cartpole1l / cartpole1l_v2
    return (size_t)B * (T - 1) * nx * (nx + nu + 1) * sizeof(real);
}

template <typename real>
int solve_nonlin_rows_impl(const AlqpDims *dims, const AlqpParams *prm, int dyn_id, double dyn_h, const void *Qd,
                           const void *q, const void *x0, const void *u_lo, const void *u_hi, long sb_u, long st_u,
                           const void *x_lo, const void *x_hi, long sb_x, long st_x, const void *G, const void *h, int m,
                           long sb_g, long st_g, long sb_h, long st_h, void *z, void *lam, void *rho, void *phi,
                           void *rnorm2, int *info, unsigned char *status, void *factor_out, const AlqpTrace *trace,
                           void *workspace, size_t ws_bytes, void *stream) {
    if (!dims || dims->B <= 0 || dims->T < 2 || dims->nx <= 0 || dims->nu <= 0) return ALQP_E_BADARG;   // (an empty batch too)
    if (!prm || !Qd || !q || !x0 || !u_lo || !u_hi || !z || !lam || !rho || !phi) return ALQP_E_BADARG;
    if (!x_lo != !x_hi || !G != !h) return ALQP_E_BADARG;
    if (!x_lo && !G) return ALQP_E_BADARG;   // the plain row set is alqp_solve_nonlin's
    if (prm->n_ls != 20 || prm->al_iter < 0 || prm->max_newton < 0) return ALQP_E_BADARG;
    if (prm->flags & ALQP_EXIT_IN_KERNEL) return ALQP_E_BADARG;   // no cooperative exit on this route
    if (x_lo && (sb_x < 0 || st_x < 0)) return ALQP_E_BADARG;
    if (G ? (m < 1 || m > 64 || sb_g < 0 || st_g < 0 || sb_h < 0 || st_h < 0) : m != 0) return ALQP_E_BADARG;
    if ((prm->flags & ALQP_SAVE_FACTOR) && !factor_out) return ALQP_E_BADARG;
    const size_t need = nonlin_rows_ws_bytes<real>(dims->nx, dims->nu, dims->B, dims->T);
    if (need == 0) return ALQP_E_UNSUPPORTED;
    if (!workspace || ws_bytes < need) return ALQP_E_BADARG;
    // the horizon must fit the LDS: the team image, plus the hand-over region of 2 pad4(m) words per team with rows
    const size_t img = lds_query<real>(dims->nx, dims->nu, dims->T);
    if (img == 0) return ALQP_E_UNSUPPORTED;
    if (img + (G ? (size_t)qpw_query(dims->nx, dims->nu) * 2 * pad4(m) * sizeof(real) : 0) > kMaxLds) return ALQP_E_UNSUPPORTED;
    NlRowsSolveArgs<real> a = {};
    AlqpParams p = *prm;
    p.flags &= ~ALQP_WS_PRIMED;   // ignored: every launch loads z, lam and rho from the caller's arrays
    if (!set_solve<real>(dims, &p, Qd, q, x0, u_lo, u_hi, sb_u, st_u, z, lam, rho, phi, rnorm2, info, status, a))
        return ALQP_E_BADARG;
    if (x_lo) { a.xlo = (const real *)x_lo; a.xhi = (const real *)x_hi; a.sb_x = sb_x; a.st_x = st_x; }
    if (G) {
        a.G = (const real *)G; a.h = (const real *)h; a.m = m;
        a.sb_g = sb_g; a.st_g = st_g; a.sb_h = sb_h; a.st_h = st_h;
    }
    a.factor = (real *)factor_out;
    a.dyn_h = (real)dyn_h;
    a.ws = (real *)workspace;
    const TraceArgs<real> tr = trace_args<real>(trace);
    const TraceArgs<real> *trp = trace ? &tr : nullptr;
    const hipStream_t s = (hipStream_t)stream;
    if (x_lo && G) return dispatch_solve_nonlin_rows<real, kGenXbox | kGenPoly>(dyn_id, dims->nx, dims->nu, a, trp, s);
    if (x_lo) return dispatch_solve_nonlin_rows<real, kGenXbox>(dyn_id, dims->nx, dims->nu, a, trp, s);
    return dispatch_solve_nonlin_rows<real, kGenPoly>(dyn_id, dims->nx, dims->nu, a, trp, s);
}

// a non-null workspace selects the quad kernels; ALQP_E_* when it cannot hold these dims, else 0
template <typename real>
int check_quad_ws(const AlqpDims *dims, size_t ws_bytes) {
    const size_t need = quad_ws_bytes<real>(dims->nx, dims->nu, dims->B, dims->T);
    if (need == 0) return ALQP_E_UNSUPPORTED;
    return ws_bytes < need ? ALQP_E_BADARG : 0;
}

template <typename real>
int newton_step_impl(const AlqpDims *dims, const void *z, const void *xnext, const void *F,
                     const void *x0, const void *lam, const void *rho, const void *Qd, const void *q,
                     const void *u_lo, const void *u_hi, long sb_u, long st_u, const AlqpObstacles *obs,
                     void *workspace, size_t ws_bytes, void *d_out, void *g_out, void *factor_out, int *info,
                     void *stream) {
    if (!dims_ok(dims) || !z || !xnext || !F || !x0 || !lam || !rho || !Qd || !q || !u_lo || !u_hi || !d_out)
        return ALQP_E_BADARG;
    StepArgs<real> a = {};
    if (!set_obstacles<real>(dims, obs, a)) return ALQP_E_BADARG;
    a.B = dims->B; a.T = dims->T;
    a.z = (const real *)z; a.xnext = (const real *)xnext; a.F = (const real *)F; a.x0 = (const real *)x0;
    a.lam = (const real *)lam; a.rho = (const real *)rho; a.Qd = (const real *)Qd; a.q = (const real *)q;
    a.ulo = (const real *)u_lo; a.uhi = (const real *)u_hi; a.sb_u = sb_u; a.st_u = st_u;
    a.d_out = (real *)d_out; a.g_out = (real *)g_out; a.factor = (real *)factor_out; a.info = info;
    if (workspace) {   // quad variant: the factor stays in the workspace records (for alqp_backward_*)
        if (factor_out) return ALQP_E_BADARG;
        if (const int rc = check_quad_ws<real>(dims, ws_bytes)) return rc;
        return dispatch_step_quad<real>(dims->nx, dims->nu, a, (real *)workspace, (hipStream_t)stream);
    }
    return dispatch_step<real>(dims->nx, dims->nu, a, (hipStream_t)stream);
}

// One Newton direction with more rows per stage and / or a dense stage cost: alqp_newton_step_xbox (Args = XboxStepArgs),
// _rows (RowsStepArgs) and _dense (DenseStepArgs, `cost` is C). The team kernel only (no quad step kernel knows such rows), so
// no workspace, and the horizon must fit the team's LDS image like alqp_solve_lin_xbox's; with general rows the image grows by
// the hand-over region of 2 pad4(m) words per team, like alqp_solve_lin_poly's. _xbox: both state bounds and no rows. _rows:
// x_lo and x_hi both null (no state box rows) or neither; G, h and m in 1..64. _dense: the same state bounds; G and h both
// null with m == 0 (no general rows) or neither.
template <typename real, typename Args>
int newton_step_ext_impl(const AlqpDims *dims, const void *z, const void *xnext, const void *F, const void *x0,
                         const void *lam, const void *rho, const void *cost, const void *q, const void *u_lo,
                         const void *u_hi, long sb_u, long st_u, const void *x_lo, const void *x_hi, long sb_x,
                         long st_x, const void *G, const void *h, int m, long sb_g, long st_g, long sb_h, long st_h,
                         void *d_out, void *g_out, void *factor_out, int *info, void *stream) {
    constexpr bool kXbox = std::is_same_v<Args, XboxStepArgs<real>>, kDense = std::is_same_v<Args, DenseStepArgs<real>>;
    if (!dims_ok(dims) || !z || !xnext || !F || !x0 || !lam || !rho || !cost || !q || !u_lo || !u_hi || !d_out)
        return ALQP_E_BADARG;
    if ((kXbox ? (!x_lo || !x_hi) : (!x_lo != !x_hi)) || sb_x < 0 || st_x < 0) return ALQP_E_BADARG;
    if constexpr (!kXbox) {
        if (kDense ? (!G != !h || (G ? (m < 1 || m > 64) : m != 0)) : (!G || !h || m < 1 || m > 64)) return ALQP_E_BADARG;
        if (sb_g < 0 || st_g < 0 || sb_h < 0 || st_h < 0) return ALQP_E_BADARG;
    }
    const size_t img = lds_query<real>(dims->nx, dims->nu, dims->T);
    if (img == 0) return ALQP_E_UNSUPPORTED;
    const size_t lds = img + (G ? (size_t)qpw_query(dims->nx, dims->nu) * 2 * pad4(m) * sizeof(real) : 0);
    if (lds > kMaxLds) return ALQP_E_UNSUPPORTED;
    Args a = {};
    a.B = dims->B; a.T = dims->T;
    a.z = (const real *)z; a.xnext = (const real *)xnext; a.F = (const real *)F; a.x0 = (const real *)x0;
    a.lam = (const real *)lam; a.rho = (const real *)rho; a.q = (const real *)q;
    a.ulo = (const real *)u_lo; a.uhi = (const real *)u_hi; a.sb_u = sb_u; a.st_u = st_u;
    a.xlo = (const real *)x_lo; a.xhi = (const real *)x_hi; a.sb_x = sb_x; a.st_x = st_x;
    a.d_out = (real *)d_out; a.g_out = (real *)g_out; a.factor = (real *)factor_out; a.info = info;
    if constexpr (kDense) a.C = (const real *)cost;
    else a.Qd = (const real *)cost;
    if constexpr (kXbox) {
        return dispatch_step_xbox<real>(dims->nx, dims->nu, a, (hipStream_t)stream);
    } else {
        a.G = (const real *)G; a.h = (const real *)h; a.m = m;
        a.sb_g = sb_g; a.st_g = st_g; a.sb_h = sb_h; a.st_h = st_h;
        if constexpr (!kDense) return dispatch_step_rows<real>(dims->nx, dims->nu, a, (hipStream_t)stream);
        else if (G) return dispatch_step_dense<real, true>(dims->nx, dims->nu, a, (hipStream_t)stream);
        else return dispatch_step_dense<real, false>(dims->nx, dims->nu, a, (hipStream_t)stream);
    }
}


// fills what the plain and the DYN backward share and launches: quad kernels on a workspace, team kernels on a factor
template <typename real, bool DYN>
int launch_backward(const AlqpDims *dims, const void *factor, void *workspace, const void *F, const void *rho,
                    const void *z_final, const void *gbar, void *q_grad, void *Qd_grad, BwdArgs<real, DYN> &a,
                    void *stream) {
    a.B = dims->B; a.T = dims->T;
    a.factor = (const real *)factor; a.F = (const real *)F; a.rho = (const real *)rho;
    a.z_final = (const real *)z_final; a.gbar = (const real *)gbar;
    a.q_grad = (real *)q_grad; a.Qd_grad = (real *)Qd_grad;
    if (workspace)
        return dispatch_backward_quad<real, DYN>(dims->nx, dims->nu, a, (real *)workspace, (hipStream_t)stream);
    return dispatch_backward<real, DYN>(dims->nx, dims->nu, a, (hipStream_t)stream);
}

template <typename real>
int backward_impl(const AlqpDims *dims, const void *factor, void *workspace, size_t ws_bytes, const void *F,
                  const void *rho, const void *z_final, const void *gbar, void *q_grad, void *Qd_grad,
                  const AlqpBwdDyn *dyn, void *stream) {
    if (!dims_ok(dims) || !factor == !workspace || !F || !rho || !z_final || !gbar || !q_grad || !Qd_grad)
        return ALQP_E_BADARG;
    if (workspace)
        if (const int rc = check_quad_ws<real>(dims, ws_bytes)) return rc;
    if (!dyn) {   // the plain kernels, the kernel arguments they always had
        BwdArgs<real> a = {};
        return launch_backward(dims, factor, workspace, F, rho, z_final, gbar, q_grad, Qd_grad, a, stream);
    }
    if (dyn->dF && (!dyn->lam || dyn->sb_lam < (long)(dims->T - 1) * dims->nx)) return ALQP_E_BADARG;
    BwdArgs<real, true> a = {};
    a.lam = (const real *)dyn->lam; a.sb_lam = dyn->sb_lam;
    a.dF = (real *)dyn->dF; a.dc = (real *)dyn->dc; a.dx0 = (real *)dyn->dx0;
    return launch_backward(dims, factor, workspace, F, rho, z_final, gbar, q_grad, Qd_grad, a, stream);
}

}  // namespace alqp

// ---- C ABI -------------------------------------------------------------------------------
extern "C" {

int alqp_abi_version(void) { return 17; }

size_t alqp_workspace_bytes_nonlin(const AlqpDims *dims, int is_f64) {
    if (!alqp::dims_ok(dims)) return 0;
    return is_f64 ? alqp::nonlin_ws_bytes<double>(dims->nx, dims->nu, dims->B, dims->T)
                  : alqp::nonlin_ws_bytes<float>(dims->nx, dims->nu, dims->B, dims->T);
}
int alqp_solve_nonlin_f32(const AlqpDims *dims, const AlqpParams *prm, int dyn_id, double dyn_h, const void *Qd,
                          const void *q, const void *x0, const void *u_lo, const void *u_hi, long sb_u, long st_u, void *z,
                          void *lam, void *rho, void *phi, void *rnorm2, int *info, unsigned char *status, void *workspace,
                          size_t ws_bytes, void *stream) {
    return alqp::solve_nonlin_impl<float>(dims, prm, dyn_id, dyn_h, Qd, q, x0, u_lo, u_hi, sb_u, st_u, z, lam, rho, phi,
                                          rnorm2, info, status, workspace, ws_bytes, stream);
}
int alqp_solve_nonlin_f64(const AlqpDims *dims, const AlqpParams *prm, int dyn_id, double dyn_h, const void *Qd,
                          const void *q, const void *x0, const void *u_lo, const void *u_hi, long sb_u, long st_u, void *z,
                          void *lam, void *rho, void *phi, void *rnorm2, int *info, unsigned char *status, void *workspace,
                          size_t ws_bytes, void *stream) {
    return alqp::solve_nonlin_impl<double>(dims, prm, dyn_id, dyn_h, Qd, q, x0, u_lo, u_hi, sb_u, st_u, z, lam, rho, phi,
                                           rnorm2, info, status, workspace, ws_bytes, stream);
}

size_t alqp_workspace_bytes_nonlin_rows(const AlqpDims *dims, int is_f64) {
    if (!alqp::dims_ok(dims)) return 0;
    return is_f64 ? alqp::nonlin_rows_ws_bytes<double>(dims->nx, dims->nu, dims->B, dims->T)
                  : alqp::nonlin_rows_ws_bytes<float>(dims->nx, dims->nu, dims->B, dims->T);
}
#define ALQP_DEFINE_NONLIN_ROWS(SFX, REAL)                                                                              \
    int alqp_solve_nonlin_rows_##SFX(                                                                                   \
        const AlqpDims *dims, const AlqpParams *prm, int dyn_id, double dyn_h, const void *Qd, const void *q,           \
        const void *x0, const void *u_lo, const void *u_hi, long sb_u, long st_u, const void *x_lo, const void *x_hi,   \
        long sb_x, long st_x, const void *G, const void *h, int m, long sb_g, long st_g, long sb_h, long st_h, void *z, \
        void *lam, void *rho, void *phi, void *rnorm2, int *info, unsigned char *status, void *factor_out,              \
        const AlqpTrace *trace, void *workspace, size_t ws_bytes, void *stream) {                                       \
        return alqp::solve_nonlin_rows_impl<REAL>(dims, prm, dyn_id, dyn_h, Qd, q, x0, u_lo, u_hi, sb_u, st_u, x_lo,    \
                                                  x_hi, sb_x, st_x, G, h, m, sb_g, st_g, sb_h, st_h, z, lam, rho, phi,  \
                                                  rnorm2, info, status, factor_out, trace, workspace, ws_bytes, stream);\
    }
ALQP_DEFINE_NONLIN_ROWS(f32, float)
ALQP_DEFINE_NONLIN_ROWS(f64, double)

size_t alqp_workspace_bytes(const AlqpDims *dims, int is_f64) {
    if (!alqp::dims_ok(dims)) return 0;
    return is_f64 ? alqp::quad_ws_bytes<double>(dims->nx, dims->nu, dims->B, dims->T)
                  : alqp::quad_ws_bytes<float>(dims->nx, dims->nu, dims->B, dims->T);
}

size_t alqp_lds_bytes(const AlqpDims *dims, int is_f64) {
    if (!alqp::dims_ok(dims)) return 0;
    size_t v = is_f64 ? alqp::lds_query<double>(dims->nx, dims->nu, dims->T)
                      : alqp::lds_query<float>(dims->nx, dims->nu, dims->T);
    return v;
}

int alqp_supported(const AlqpDims *dims, int is_f64) {
    // an (nx, nu) instance exists: the quad variant (HBM workspace) runs any horizon; the team variant
    // additionally needs its LDS image to fit (alqp_supported_variant)
    return alqp_workspace_bytes(dims, is_f64) > 0;
}

int alqp_supported_variant(const AlqpDims *dims, int is_f64, int variant) {
    if (variant == 2) return alqp_workspace_bytes(dims, is_f64) > 0;
    if (variant == 1) {
        size_t v = alqp_lds_bytes(dims, is_f64);
        return v > 0 && v <= alqp::kMaxLds;
    }
    return 0;
}

int alqp_pick_variant(const AlqpDims *dims, int is_f64, int flags, long quad_min_batch) {
    if (!alqp::dims_ok(dims)) return 0;
    return is_f64 ? alqp::pick_variant<double>(dims, flags, quad_min_batch)
                  : alqp::pick_variant<float>(dims, flags, quad_min_batch);
}

int alqp_qps_per_wave(const AlqpDims *dims, int is_f64) {
    (void)is_f64;
    if (!alqp::dims_ok(dims)) return 0;
    return alqp::qpw_query(dims->nx, dims->nu);
}

#define ALQP_DEFINE(SFX, REAL)                                                                        \
    int alqp_solve_lin_##SFX(const AlqpDims *dims, const AlqpParams *prm, const void *Qd,             \
                             const void *q, const void *F, const void *c, const void *x0,             \
                             const void *u_lo, const void *u_hi, long sb_u, long st_u, void *z,       \
                             void *lam, void *rho, void *phi, void *rnorm2, int *info,                \
                             unsigned char *status, void *factor_out, const AlqpTrace *trace,         \
                             void *workspace, size_t ws_bytes, void *stream) {                        \
        return alqp::solve_lin_impl<REAL, alqp::SolveArgs<REAL>>(                                     \
            dims, prm, Qd, q, F, c, x0, u_lo, u_hi, sb_u, st_u, z, lam, rho, phi, rnorm2, info,       \
            status, factor_out, trace, workspace, ws_bytes, stream, alqp::SolveArgs<REAL>{},          \
            alqp::dispatch_solve<REAL>, alqp::dispatch_solve_quad<REAL>);                             \
    }                                                                                                 \
    int alqp_solve_lin_shared_##SFX(const AlqpDims *dims, const AlqpParams *prm, const void *Qd,      \
                                    const void *q, const void *F, const void *c, long sb_F,           \
                                    long st_F, long sb_c, long st_c, const void *x0,                  \
                                    const void *u_lo, const void *u_hi, long sb_u, long st_u,         \
                                    void *z, void *lam, void *rho, void *phi, void *rnorm2,           \
                                    int *info, unsigned char *status, void *factor_out,               \
                                    const AlqpTrace *trace, void *workspace, size_t ws_bytes,         \
                                    void *stream) {                                                   \
        return alqp::solve_lin_shared_impl<REAL>(dims, prm, Qd, q, F, c, sb_F, st_F, sb_c, st_c, x0,  \
                                                 u_lo, u_hi, sb_u, st_u, z, lam, rho, phi, rnorm2,    \
                                                 info, status, factor_out, trace, workspace,          \
                                                 ws_bytes, stream);                                   \
    }                                                                                                 \
    int alqp_solve_lin_dense_##SFX(const AlqpDims *dims, const AlqpParams *prm, const void *C,        \
                                   const void *q, const void *F, const void *c, const void *x0,       \
                                   const void *u_lo, const void *u_hi, long sb_u, long st_u, void *z, \
                                   void *lam, void *rho, void *phi, void *rnorm2, int *info,          \
                                   unsigned char *status, void *factor_out, const AlqpTrace *trace,   \
                                   void *stream) {                                                    \
        return alqp::solve_lin_feat_impl<REAL>(                                                       \
            alqp::kAcceptDense, dims, prm, nullptr, q, F, c, x0, u_lo, u_hi, sb_u, st_u, z, lam, rho, \
            phi, rnorm2, info, status, factor_out, trace, stream, C, nullptr, nullptr, 0, 0, nullptr, \
            nullptr, 0, 0, 0, 0, 0);                                                                  \
    }                                                                                                 \
    int alqp_solve_lin_xbox_##SFX(const AlqpDims *dims, const AlqpParams *prm, const void *Qd,        \
                                  const void *q, const void *F, const void *c, const void *x0,        \
                                  const void *u_lo, const void *u_hi, long sb_u, long st_u,           \
                                  const void *x_lo, const void *x_hi, long sb_x, long st_x, void *z,  \
                                  void *lam, void *rho, void *phi, void *rnorm2, int *info,           \
                                  unsigned char *status, void *factor_out, const AlqpTrace *trace,    \
                                  void *stream) {                                                     \
        return alqp::solve_lin_feat_impl<REAL>(                                                       \
            alqp::kAcceptXbox, dims, prm, Qd, q, F, c, x0, u_lo, u_hi, sb_u, st_u, z, lam, rho, phi,  \
            rnorm2, info, status, factor_out, trace, stream, nullptr, x_lo, x_hi, sb_x, st_x,         \
            nullptr, nullptr, 0, 0, 0, 0, 0);                                                         \
    }                                                                                                 \
    int alqp_solve_lin_poly_##SFX(const AlqpDims *dims, const AlqpParams *prm, const void *Qd,        \
                                  const void *q, const void *F, const void *c, const void *x0,        \
                                  const void *u_lo, const void *u_hi, long sb_u, long st_u,           \
                                  const void *G, const void *h, int m, long sb_g, long st_g,          \
                                  long sb_h, long st_h, void *z, void *lam, void *rho, void *phi,     \
                                  void *rnorm2, int *info, unsigned char *status, void *factor_out,   \
                                  const AlqpTrace *trace, void *stream) {                             \
        return alqp::solve_lin_feat_impl<REAL>(                                                       \
            alqp::kAcceptPoly, dims, prm, Qd, q, F, c, x0, u_lo, u_hi, sb_u, st_u, z, lam, rho, phi,  \
            rnorm2, info, status, factor_out, trace, stream, nullptr, nullptr, nullptr, 0, 0, G, h,   \
            m, sb_g, st_g, sb_h, st_h);                                                               \
    }                                                                                                 \
    int alqp_solve_lin_gen_##SFX(const AlqpDims *dims, const AlqpParams *prm, const void *Qd,         \
                                 const void *q, const void *F, const void *c, const void *x0,         \
                                 const void *u_lo, const void *u_hi, long sb_u, long st_u, void *z,   \
                                 void *lam, void *rho, void *phi, void *rnorm2, int *info,            \
                                 unsigned char *status, void *factor_out, const AlqpTrace *trace,     \
                                 void *workspace, size_t ws_bytes, void *stream, const void *C,       \
                                 const void *x_lo, const void *x_hi, long sb_x, long st_x,            \
                                 const void *G, const void *h, int m, long sb_g, long st_g,           \
                                 long sb_h, long st_h) {                                              \
        (void)workspace; (void)ws_bytes;                                                              \
        return alqp::solve_lin_feat_impl<REAL>(                                                       \
            alqp::kAcceptGen, dims, prm, Qd, q, F, c, x0, u_lo, u_hi, sb_u, st_u, z, lam, rho, phi,   \
            rnorm2, info, status, factor_out, trace, stream, C, x_lo, x_hi, sb_x, st_x, G, h, m,      \
            sb_g, st_g, sb_h, st_h);                                                                  \
    }                                                                                                 \
    int alqp_newton_step_##SFX(const AlqpDims *dims, const void *z, const void *xnext, const void *F, \
                               const void *x0, const void *lam, const void *rho, const void *Qd,      \
                               const void *q, const void *u_lo, const void *u_hi, long sb_u,          \
                               long st_u, const AlqpObstacles *obs, void *workspace, size_t ws_bytes, \
                               void *d_out, void *g_out, void *factor_out, int *info, void *stream) { \
        return alqp::newton_step_impl<REAL>(dims, z, xnext, F, x0, lam, rho, Qd, q, u_lo, u_hi, sb_u, \
                                            st_u, obs, workspace, ws_bytes, d_out, g_out, factor_out, \
                                            info, stream);                                            \
    }                                                                                                 \
    int alqp_newton_step_xbox_##SFX(const AlqpDims *dims, const void *z, const void *xnext,           \
                                    const void *F, const void *x0, const void *lam, const void *rho,  \
                                    const void *Qd, const void *q, const void *u_lo,                  \
                                    const void *u_hi, long sb_u, long st_u, const void *x_lo,         \
                                    const void *x_hi, long sb_x, long st_x, void *d_out, void *g_out, \
                                    void *factor_out, int *info, void *stream) {                      \
        return alqp::newton_step_ext_impl<REAL, alqp::XboxStepArgs<REAL>>(                            \
            dims, z, xnext, F, x0, lam, rho, Qd, q, u_lo, u_hi, sb_u, st_u, x_lo, x_hi, sb_x, st_x,   \
            nullptr, nullptr, 0, 0, 0, 0, 0, d_out, g_out, factor_out, info, stream);                 \
    }                                                                                                 \
    int alqp_newton_step_rows_##SFX(const AlqpDims *dims, const void *z, const void *xnext,           \
                                    const void *F, const void *x0, const void *lam, const void *rho,  \
                                    const void *Qd, const void *q, const void *u_lo,                  \
                                    const void *u_hi, long sb_u, long st_u, const void *x_lo,         \
                                    const void *x_hi, long sb_x, long st_x, const void *G,            \
                                    const void *h, int m, long sb_g, long st_g, long sb_h, long st_h, \
                                    void *d_out, void *g_out, void *factor_out, int *info,            \
                                    void *stream) {                                                   \
        return alqp::newton_step_ext_impl<REAL, alqp::RowsStepArgs<REAL>>(                            \
            dims, z, xnext, F, x0, lam, rho, Qd, q, u_lo, u_hi, sb_u, st_u, x_lo, x_hi, sb_x, st_x,   \
            G, h, m, sb_g, st_g, sb_h, st_h, d_out, g_out, factor_out, info, stream);                 \
    }                                                                                                 \
    int alqp_newton_step_dense_##SFX(const AlqpDims *dims, const void *z, const void *xnext,          \
                                     const void *F, const void *x0, const void *lam, const void *rho, \
                                     const void *C, const void *q, const void *u_lo,                  \
                                     const void *u_hi, long sb_u, long st_u, const void *x_lo,        \
                                     const void *x_hi, long sb_x, long st_x, const void *G,           \
                                     const void *h, int m, long sb_g, long st_g, long sb_h,           \
                                     long st_h, void *d_out, void *g_out, void *factor_out,           \
                                     int *info, void *stream) {                                       \
        return alqp::newton_step_ext_impl<REAL, alqp::DenseStepArgs<REAL>>(                           \
            dims, z, xnext, F, x0, lam, rho, C, q, u_lo, u_hi, sb_u, st_u, x_lo, x_hi, sb_x, st_x,    \
            G, h, m, sb_g, st_g, sb_h, st_h, d_out, g_out, factor_out, info, stream);                 \
    }                                                                                                 \
    int alqp_backward_##SFX(const AlqpDims *dims, const void *factor, void *workspace,                \
                            size_t ws_bytes, const void *F, const void *rho, const void *z_final,     \
                            const void *gbar, void *q_grad, void *Qd_grad, const AlqpBwdDyn *dyn,     \
                            void *stream) {                                                           \
        return alqp::backward_impl<REAL>(dims, factor, workspace, ws_bytes, F, rho, z_final, gbar,    \
                                         q_grad, Qd_grad, dyn, stream);                               \
    }

ALQP_DEFINE(f32, float)
ALQP_DEFINE(f64, double)

}  // extern "C"
