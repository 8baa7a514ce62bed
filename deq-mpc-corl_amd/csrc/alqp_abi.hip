// alqp_abi.hip - host side of the C ABI of include/mi_alqp.h: argument checks, the choice between the team and the
// quad kernels, workspace sizes. No kernel is defined or instantiated here; launches go through alqp_launch.hpp.
// No torch types anywhere: plain device pointers in, kernel launches on the caller's stream.
#include <hip/hip_runtime.h>

#include "alqp_team.hpp"   // Cfg
#include "alqp_quad.hpp"   // QCfg
#include "alqp_dims.hpp"
#include "alqp_launch.hpp"
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

template <typename real>
int solve_lin_impl(const AlqpDims *dims, const AlqpParams *prm, const void *Qd, const void *q,
                   const void *F, const void *c, const void *x0, const void *u_lo, const void *u_hi,
                   long sb_u, long st_u, void *z, void *lam, void *rho, void *phi, void *rnorm2,
                   int *info, unsigned char *status, void *factor_out, const AlqpTrace *trace,
                   void *workspace, size_t ws_bytes, void *stream) {
    if (!dims_ok(dims) || !prm || !Qd || !q || !F || !c || !x0 || !u_lo || !u_hi || !z || !lam || !rho || !phi)
        return ALQP_E_BADARG;
    if (prm->n_ls < 1 || prm->n_ls > 20 || prm->al_iter < 0 || prm->max_newton < 0) return ALQP_E_BADARG;
    if ((prm->flags & ALQP_SAVE_FACTOR) && !factor_out) return ALQP_E_BADARG;
    SolveArgs<real> a = {};
    a.B = dims->B; a.T = dims->T;
    a.al_iter = prm->al_iter; a.max_newton = prm->max_newton; a.n_ls = prm->n_ls; a.flags = prm->flags;
    a.rho_scale = (real)prm->rho_scale;
    a.Qd = (const real *)Qd; a.q = (const real *)q; a.F = (const real *)F; a.c = (const real *)c;
    a.x0 = (const real *)x0; a.ulo = (const real *)u_lo; a.uhi = (const real *)u_hi;
    a.sb_u = sb_u; a.st_u = st_u;
    a.z = (real *)z; a.lam = (real *)lam; a.rho = (real *)rho; a.phi = (real *)phi;
    a.rnorm2 = (real *)rnorm2; a.info = info; a.status = status; a.factor = (real *)factor_out;
    a.skip = prm->skip_flag;
    a.stagger = quad_stagger(prm->quad_stagger, dims->B, dims->T, dims->nx, dims->nu, prm->al_iter * prm->max_newton, sizeof(real) == 8);
    if (prm->flags & ALQP_EXIT_IN_KERNEL) {
        if (!prm->exit_scratch || trace || prm->skip_flag) return ALQP_E_BADARG;
        a.exit_tol = prm->exit_tol; a.newton_counts = prm->newton_counts; a.exit_scratch = prm->exit_scratch;
    }
    TraceArgs<real> tr = {};
    if (trace) {
        tr.g = (real *)trace->g; tr.d = (real *)trace->d; tr.phi = (real *)trace->phi;
        tr.phi_prev = (real *)trace->phi_prev; tr.k = trace->k; tr.accept = trace->accept;
    }
    // variant: 1 = team (factor in LDS), 2 = quad (4 lanes/instance, HBM workspace), 0 = auto
    const size_t need = quad_ws_bytes<real>(dims->nx, dims->nu, dims->B, dims->T);
    int variant = prm->variant;
    // auto: quad once the batch fills the chip (16 instances per wavefront, 1024 SIMDs), team below
    // (2-2.4x lower latency at small batches). The team kernels' time is a step function of the batch - 2048 (fp32) /
    // 1024 (fp64) teams fit the chip at once - and B = 4096 is exactly two / four full rounds: measured at (13,4) T=20
    // after round 3's team-kernel work, fp32 B = 4096 team 1.83 vs quad 2.00 ms, B = 5120 2.36 vs 2.08; fp64 B = 4096 4.35
    // vs 4.71, B = 5120 5.42 vs 5.02 (profiles/r03/experiments/README.md).
    if (variant == 0) {
        const size_t team_lds = lds_query<real>(dims->nx, dims->nu, dims->T);
        const bool team_fits = team_lds > 0 && team_lds <= kMaxLds;
        const bool quad_ok = need > 0 && workspace && ws_bytes >= need && !(prm->flags & ALQP_SAVE_FACTOR);
        // long horizons whose factor does not fit the team's LDS image run on the quad kernels at any batch
        // whole-wavefront teams (2n + nx + 1 > 32 rows, e.g. (13,4)): team through B = 4096 (full rounds), quad beyond;
        // smaller teams share a wavefront and were not re-measured: round 2's rule
        const bool wave_team = 2 * (dims->nx + dims->nu) + dims->nx + 1 > 32;
        const int qmin = wave_team ? 4097 : (sizeof(real) == 8 ? 4608 : 4096);
        variant = (quad_ok && (dims->B >= qmin || !team_fits)) ? 2 : 1;
    }
    if (variant == 2) {
        if (prm->flags & ALQP_SAVE_FACTOR) return ALQP_E_UNSUPPORTED;
        if (need == 0) return ALQP_E_UNSUPPORTED;
        if (!workspace || ws_bytes < need) return ALQP_E_BADARG;
        return dispatch_solve_quad<real>(dims->nx, dims->nu, a, trace ? &tr : nullptr, (real *)workspace,
                                         (hipStream_t)stream);
    }
    if (variant != 1) return ALQP_E_BADARG;
    return dispatch_solve<real>(dims->nx, dims->nu, a, trace ? &tr : nullptr, (hipStream_t)stream);
}

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
    a.B = dims->B; a.T = dims->T;
    a.al_iter = prm->al_iter; a.max_newton = prm->max_newton; a.n_ls = prm->n_ls; a.flags = prm->flags;
    a.rho_scale = (real)prm->rho_scale;
    a.Qd = (const real *)Qd; a.q = (const real *)q; a.c = nullptr; a.x0 = (const real *)x0;
    a.F = (const real *)((const char *)workspace + quad_ws_bytes<real>(dims->nx, dims->nu, dims->B, dims->T));
    a.ulo = (const real *)u_lo; a.uhi = (const real *)u_hi; a.sb_u = sb_u; a.st_u = st_u;
    a.z = (real *)z; a.lam = (real *)lam; a.rho = (real *)rho; a.phi = (real *)phi;
    a.rnorm2 = (real *)rnorm2; a.info = info; a.status = status; a.factor = nullptr;
    a.skip = prm->skip_flag;
    a.dyn_h = (real)dyn_h;
    if (prm->flags & ALQP_EXIT_IN_KERNEL) {
        if (!prm->exit_scratch || prm->skip_flag) return ALQP_E_BADARG;
        a.exit_tol = prm->exit_tol; a.newton_counts = prm->newton_counts; a.exit_scratch = prm->exit_scratch;
    }
    return dispatch_solve_nonlin<real>(dyn_id, dims->nx, dims->nu, a, (real *)workspace, (hipStream_t)stream);
}

template <typename real>
int newton_step_impl(const AlqpDims *dims, const void *z, const void *xnext, const void *F,
                     const void *x0, const void *lam, const void *rho, const void *Qd, const void *q,
                     const void *u_lo, const void *u_hi, long sb_u, long st_u, void *d_out,
                     void *g_out, void *factor_out, int *info, void *stream, const AlqpObstacles *obs = nullptr,
                     void *workspace = nullptr, size_t ws_bytes = 0) {
    if (!dims_ok(dims) || !z || !xnext || !F || !x0 || !lam || !rho || !Qd || !q || !u_lo || !u_hi || !d_out)
        return ALQP_E_BADARG;
    if (obs && (obs->nobs < 0 || (obs->nobs > 0 && (!obs->pos || dims->nx < 3)))) return ALQP_E_BADARG;
    StepArgs<real> a = {};
    if (obs && obs->nobs > 0) { a.obs = (const real *)obs->pos; a.nobs = obs->nobs; a.obs_r2 = (real)(obs->radius * obs->radius); }
    if (obs) a.no_init = obs->state_estimator;
    a.B = dims->B; a.T = dims->T;
    a.z = (const real *)z; a.xnext = (const real *)xnext; a.F = (const real *)F; a.x0 = (const real *)x0;
    a.lam = (const real *)lam; a.rho = (const real *)rho; a.Qd = (const real *)Qd; a.q = (const real *)q;
    a.ulo = (const real *)u_lo; a.uhi = (const real *)u_hi; a.sb_u = sb_u; a.st_u = st_u;
    a.d_out = (real *)d_out; a.g_out = (real *)g_out; a.factor = (real *)factor_out; a.info = info;
    if (workspace) {   // quad variant: the factor stays in the workspace records (alqp_backward_ws)
        if (factor_out) return ALQP_E_BADARG;
        const size_t need = quad_ws_bytes<real>(dims->nx, dims->nu, dims->B, dims->T);
        if (need == 0) return ALQP_E_UNSUPPORTED;
        if (ws_bytes < need) return ALQP_E_BADARG;
        return dispatch_step_quad<real>(dims->nx, dims->nu, a, (real *)workspace, (hipStream_t)stream);
    }
    return dispatch_step<real>(dims->nx, dims->nu, a, (hipStream_t)stream);
}

// the dynamics-gradient outputs of alqp_backward_dyn_* / alqp_backward_ws_dyn_* (all null: the plain backward)
struct BwdDyn {
    const void *lam = nullptr;
    long sb_lam = 0;
    void *dF = nullptr, *dc = nullptr, *dx0 = nullptr;
};
template <typename real, bool DYN>
void set_bwd(const AlqpDims *dims, const void *factor, const void *F, const void *rho, const void *z_final,
             const void *gbar, void *q_grad, void *Qd_grad, BwdArgs<real, DYN> &a) {
    a.B = dims->B; a.T = dims->T;
    a.factor = (const real *)factor; a.F = (const real *)F; a.rho = (const real *)rho;
    a.z_final = (const real *)z_final; a.gbar = (const real *)gbar;
    a.q_grad = (real *)q_grad; a.Qd_grad = (real *)Qd_grad;
}
template <typename real>
bool set_dyn(const AlqpDims *dims, const BwdDyn &d, BwdArgs<real, true> &a) {
    if (d.dF && (!d.lam || d.sb_lam < (long)(dims->T - 1) * dims->nx)) return false;
    a.lam = (const real *)d.lam; a.sb_lam = d.sb_lam;
    a.dF = (real *)d.dF; a.dc = (real *)d.dc; a.dx0 = (real *)d.dx0;
    return true;
}

template <typename real>
int backward_impl(const AlqpDims *dims, const void *factor, const void *F, const void *rho,
                  const void *z_final, const void *gbar, void *q_grad, void *Qd_grad, void *stream,
                  const BwdDyn *dyn = nullptr) {
    if (!dims_ok(dims) || !factor || !F || !rho || !z_final || !gbar || !q_grad || !Qd_grad)
        return ALQP_E_BADARG;
    if (dyn) {
        BwdArgs<real, true> a = {};
        set_bwd(dims, factor, F, rho, z_final, gbar, q_grad, Qd_grad, a);
        if (!set_dyn(dims, *dyn, a)) return ALQP_E_BADARG;
        return dispatch_backward<real, true>(dims->nx, dims->nu, a, (hipStream_t)stream);
    }
    BwdArgs<real> a = {};
    set_bwd(dims, factor, F, rho, z_final, gbar, q_grad, Qd_grad, a);
    return dispatch_backward<real, false>(dims->nx, dims->nu, a, (hipStream_t)stream);
}

template <typename real>
int backward_ws_impl(const AlqpDims *dims, void *workspace, size_t ws_bytes, const void *F, const void *rho,
                     const void *z_final, const void *gbar, void *q_grad, void *Qd_grad, void *stream,
                     const BwdDyn *dyn = nullptr) {
    if (!dims_ok(dims) || !workspace || !F || !rho || !z_final || !gbar || !q_grad || !Qd_grad)
        return ALQP_E_BADARG;
    const size_t need = quad_ws_bytes<real>(dims->nx, dims->nu, dims->B, dims->T);
    if (need == 0) return ALQP_E_UNSUPPORTED;
    if (ws_bytes < need) return ALQP_E_BADARG;
    if (dyn) {
        BwdArgs<real, true> a = {};
        set_bwd(dims, nullptr, F, rho, z_final, gbar, q_grad, Qd_grad, a);
        if (!set_dyn(dims, *dyn, a)) return ALQP_E_BADARG;
        return dispatch_backward_quad<real, true>(dims->nx, dims->nu, a, (real *)workspace, (hipStream_t)stream);
    }
    BwdArgs<real> a = {};
    set_bwd(dims, nullptr, F, rho, z_final, gbar, q_grad, Qd_grad, a);
    return dispatch_backward_quad<real, false>(dims->nx, dims->nu, a, (real *)workspace, (hipStream_t)stream);
}

}  // namespace alqp

// ---- C ABI -------------------------------------------------------------------------------
extern "C" {

int alqp_abi_version(void) { return 11; }

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
        return alqp::solve_lin_impl<REAL>(dims, prm, Qd, q, F, c, x0, u_lo, u_hi, sb_u, st_u, z, lam, \
                                          rho, phi, rnorm2, info, status, factor_out, trace,          \
                                          workspace, ws_bytes, stream);                               \
    }                                                                                                 \
    int alqp_newton_step_##SFX(const AlqpDims *dims, const void *z, const void *xnext, const void *F, \
                               const void *x0, const void *lam, const void *rho, const void *Qd,      \
                               const void *q, const void *u_lo, const void *u_hi, long sb_u,          \
                               long st_u, void *d_out, void *g_out, void *factor_out, int *info,      \
                               void *stream) {                                                        \
        return alqp::newton_step_impl<REAL>(dims, z, xnext, F, x0, lam, rho, Qd, q, u_lo, u_hi, sb_u, \
                                            st_u, d_out, g_out, factor_out, info, stream);            \
    }                                                                                                 \
    int alqp_newton_step_obs_##SFX(const AlqpDims *dims, const void *z, const void *xnext, const void *F, \
                                   const void *x0, const void *lam, const void *rho, const void *Qd,  \
                                   const void *q, const void *u_lo, const void *u_hi, long sb_u,      \
                                   long st_u, const AlqpObstacles *obs, void *d_out, void *g_out,     \
                                   void *factor_out, int *info, void *stream) {                       \
        return alqp::newton_step_impl<REAL>(dims, z, xnext, F, x0, lam, rho, Qd, q, u_lo, u_hi, sb_u, \
                                            st_u, d_out, g_out, factor_out, info, stream, obs);       \
    }                                                                                                 \
    int alqp_backward_##SFX(const AlqpDims *dims, const void *factor, const void *F, const void *rho, \
                            const void *z_final, const void *gbar, void *q_grad, void *Qd_grad,       \
                            void *stream) {                                                           \
        return alqp::backward_impl<REAL>(dims, factor, F, rho, z_final, gbar, q_grad, Qd_grad,        \
                                         stream);                                                     \
    }

ALQP_DEFINE(f32, float)
ALQP_DEFINE(f64, double)

#define ALQP_DEFINE_STEP_WS(SFX, REAL)                                                                \
    int alqp_newton_step_ws_##SFX(const AlqpDims *dims, const void *z, const void *xnext, const void *F, \
                                  const void *x0, const void *lam, const void *rho, const void *Qd,   \
                                  const void *q, const void *u_lo, const void *u_hi, long sb_u,       \
                                  long st_u, void *workspace, size_t ws_bytes, void *d_out,           \
                                  void *g_out, int *info, void *stream) {                             \
        if (!workspace) return ALQP_E_BADARG;                                                         \
        return alqp::newton_step_impl<REAL>(dims, z, xnext, F, x0, lam, rho, Qd, q, u_lo, u_hi, sb_u, \
                                            st_u, d_out, g_out, nullptr, info, stream, nullptr,       \
                                            workspace, ws_bytes);                                     \
    }                                                                                                 \
    int alqp_newton_step_ws_obs_##SFX(const AlqpDims *dims, const void *z, const void *xnext, const void *F, \
                                      const void *x0, const void *lam, const void *rho, const void *Qd, \
                                      const void *q, const void *u_lo, const void *u_hi, long sb_u,   \
                                      long st_u, const AlqpObstacles *obs, void *workspace, size_t ws_bytes, \
                                      void *d_out, void *g_out, int *info, void *stream) {            \
        if (!workspace) return ALQP_E_BADARG;                                                         \
        return alqp::newton_step_impl<REAL>(dims, z, xnext, F, x0, lam, rho, Qd, q, u_lo, u_hi, sb_u, \
                                            st_u, d_out, g_out, nullptr, info, stream, obs,           \
                                            workspace, ws_bytes);                                     \
    }
ALQP_DEFINE_STEP_WS(f32, float)
ALQP_DEFINE_STEP_WS(f64, double)

int alqp_backward_ws_f32(const AlqpDims *dims, void *workspace, size_t ws_bytes, const void *F,
                         const void *rho, const void *z_final, const void *gbar, void *q_grad,
                         void *Qd_grad, void *stream) {
    return alqp::backward_ws_impl<float>(dims, workspace, ws_bytes, F, rho, z_final, gbar, q_grad, Qd_grad, stream);
}
int alqp_backward_ws_f64(const AlqpDims *dims, void *workspace, size_t ws_bytes, const void *F,
                         const void *rho, const void *z_final, const void *gbar, void *q_grad,
                         void *Qd_grad, void *stream) {
    return alqp::backward_ws_impl<double>(dims, workspace, ws_bytes, F, rho, z_final, gbar, q_grad, Qd_grad, stream);
}

#define ALQP_DEFINE_BWD_DYN(SFX, REAL)                                                                \
    int alqp_backward_dyn_##SFX(const AlqpDims *dims, const void *factor, const void *F, const void *rho, \
                                const void *z_final, const void *gbar, void *q_grad, void *Qd_grad,   \
                                const void *lam, long sb_lam, void *dF, void *dc, void *dx0,          \
                                void *stream) {                                                       \
        const alqp::BwdDyn d = {lam, sb_lam, dF, dc, dx0};                                            \
        return alqp::backward_impl<REAL>(dims, factor, F, rho, z_final, gbar, q_grad, Qd_grad,        \
                                         stream, &d);                                                 \
    }                                                                                                 \
    int alqp_backward_ws_dyn_##SFX(const AlqpDims *dims, void *workspace, size_t ws_bytes, const void *F, \
                                   const void *rho, const void *z_final, const void *gbar,            \
                                   void *q_grad, void *Qd_grad, const void *lam, long sb_lam,         \
                                   void *dF, void *dc, void *dx0, void *stream) {                     \
        const alqp::BwdDyn d = {lam, sb_lam, dF, dc, dx0};                                            \
        return alqp::backward_ws_impl<REAL>(dims, workspace, ws_bytes, F, rho, z_final, gbar, q_grad, \
                                            Qd_grad, stream, &d);                                     \
    }
ALQP_DEFINE_BWD_DYN(f32, float)
ALQP_DEFINE_BWD_DYN(f64, double)

}  // extern "C"
