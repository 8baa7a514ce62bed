/*
 * mi_alqp.h - C ABI of the MI355X-native batched augmented-Lagrangian MPC/QP solver.
 *
 * The reference (anonymous-author-918/deq-mpc-corl) has no native interface for this
 * path: its AL solver is eager PyTorch (qpth/AL_mpc.py, qpth/al_utils.py). The entry
 * points below are what a binding for that path would call; each one names the
 * reference code it replaces. INTEGRATION.md shows the ctypes stub.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (e.g. PyTorch's caching
 *     allocator); the library never allocates, frees or synchronises;
 *   - work is enqueued on `stream` (a hipStream_t passed as void*), so ordering is
 *     stream order; every call is re-entrant (no global state);
 *   - return value: 0 on success, <0 on bad arguments / unsupported dims / launch
 *     failure (ALQP_E_*). Numerical trouble is reported per instance in info[] / status[];
 *   - dtype suffix _f32 / _f64 is the arithmetic AND storage type of all real arrays;
 *   - batch-first row-major layouts, as the reference uses them:
 *       z   [B][T][n]        n = nx+nu, state first        (xu in al_utils.py)
 *       Qd,q[B][T][n]        diagonal of QuadCost.C and QuadCost.c (AL_mpc.py:250)
 *       C   [B][T][n][n]     all of QuadCost.C, symmetric (alqp_solve_lin_dense_* only)
 *       F   [B][T-1][nx][n]  [A_t B_t]  (dynamics Jacobian, al_utils.py:242-248)
 *       c   [B][T-1][nx]     affine offset of LinDx-style dynamics
 *       xnext[B][T-1][nx]    f(x_t,u_t) evaluated by the caller (nonlinear mode)
 *       x0  [B][nx]
 *       lam [B][M]           M = T*nx + 2*T*nu; eq rows t*nx+i (t<T-1 dynamics, t=T-1 the
 *                            initial-state row), then ineq rows T*nx + t*2nu + j
 *                            (j<nu upper, j>=nu lower)  (al_utils.py:218-225, 293)
 *       rho [B]              (the reference's [B,1])
 *       u_lo,u_hi            element (b,t,j) at b*sb_u + t*st_u + j  (0 strides broadcast)
 *       factor[B][T][n(n+1)/2]  packed rows of X_t = L_tt^{-T} of the block-tridiagonal
 *                            Cholesky factor (row i holds X[i][i..n-1])
 */
#ifndef MI_ALQP_H
#define MI_ALQP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct AlqpDims {
    int B;   /* instances */
    int T;   /* horizon, >= 2 */
    int nx;  /* state dim */
    int nu;  /* control dim */
} AlqpDims;

/* obstacle rows of Obstacle_MPC (documented under "Obstacle inequalities" below); nullable wherever it is taken */
typedef struct AlqpObstacles {
    const void *pos;   /* DEVICE [B][T][nobs][3], the real type of the call */
    double radius;
    int nobs;          /* reference: 4 nearest of 40 (AL_mpc_custom.py:52-54, 112-115); 0: no obstacle rows */
    int state_estimator; /* 1: the state-estimator variant (qpth/al_utils_se.py): no initial-state rows (row block
                          T-1 of lam is ignored, x_0 gets no E'E term: :92-105, 186-200) and a cost gradient that is
                          zero on the given controls (:300-310) while H keeps diag(Q) there (:66-68), so du = 0 exactly.
                          The rest of that variant is data the caller prepares: B columns of F zeroed (:151), bounds
                          out of reach (the variant has no bound rows, AL_mpc.py:198) */
} AlqpObstacles;

/* flags for alqp_solve_lin_* */
#define ALQP_INIT_MERIT   1  /* evaluate merit(z) at the start of every AL iteration (al_utils.py:481) */
#define ALQP_DUAL_UPDATE  2  /* lam += rho*r, clamp, rho *= rho_scale after the Newton steps (AL_mpc.py:315-325) */
#define ALQP_SAVE_FACTOR  4  /* write the factor of the last executed Newton step to factor_out */
#define ALQP_WS_PRIMED    8  /* quad variant: the workspace still holds this solve's records from the previous
                               launch on it (same z, lam, Qd, q, c, bounds as the arrays passed now): skip the
                               copy-in pass. Only for back-to-back launches of one solve, see INTEGRATION.md */

#define ALQP_EXIT_IN_KERNEL 16 /* alqp_solve_lin: the reference's batch-global exit test of the Newton loop
                               (al_utils.py:486, 551-564: stop when ||r+|| over the WHOLE batch is below exit_tol or moved
                               by less than exit_tol relative) is taken INSIDE the launch: one cooperative launch does what
                               a merit launch + up to max_newton one-step launches + alqp_exit_test in between do, with a
                               grid-wide barrier and an ordered sum per Newton step. Needs exit_scratch; no trace, no
                               skip_flag. Returns ALQP_E_COOP when the grid cannot be co-resident (the caller then uses
                               the launch-per-step route). Single-GPU batches only: a batch sharded over ranks needs the
                               all-reduce between the steps. */
#define ALQP_FACTOR_IN_WS 32 /* quad variant, fp32: the fused solve keeps the factor of every stage in the workspace records
                               between its two sweeps, none in LDS (csrc/alqp_quad.hpp, QCfg::KL). Results and the workspace
                               left behind are the same bits either way; for tests and A/B timing. Ignored elsewhere.
                               (Bits 20-31: wavefront stagger experiments.) */

typedef struct AlqpParams {
    int al_iter;      /* AL outer iterations done by this call (AL_mpc.py:290) */
    int max_newton;   /* Newton steps per AL iteration, reference: 4 (al_utils.py:485) */
    int n_ls;         /* line-search candidates 2^-k, reference: 20 (al_utils.py:619); <= 20 */
    int flags;        /* ALQP_* */
    double rho_scale; /* reference: 10 (AL_mpc.py:325) */
    int variant;      /* kernel variant of alqp_solve_lin: 0 auto, 1 team (factor in LDS, no
                         workspace), 2 quad (4 lanes per instance, factor streamed through the
                         HBM workspace; no ALQP_SAVE_FACTOR) */
    const double *skip_flag; /* nullable DEVICE pointer: when *skip_flag != 0 at launch time the call
                         does nothing at all (ctl[0] of alqp_exit_test: the batch-global exit of the
                         reference's Newton loop taken on the device, no host round trip) */
    /* ALQP_EXIT_IN_KERNEL only (ignored otherwise): */
    double exit_tol;      /* reference: 1e-3 (al_utils.py:552, 560) */
    int *newton_counts;   /* nullable DEVICE [al_iter]: executed Newton steps per AL iteration (-1: barrier time-out) */
    double *exit_scratch; /* DEVICE, at least 2 * B + 2 doubles, zeroed before every call (arrival counter, partial sums,
                             time-out flag: a grid barrier that waited ~1 s gives up, newton_counts then holds -1) */
    int quad_stagger;     /* quad solve (variant 2 / auto at B >= 4096): start offset between the four wavefronts of a CU.
                             All wavefronts run the same sweeps; started together they queue on the CU's vector-memory
                             pipeline in lock step. 0 (default): automatic - a fifth of a sweep between neighbouring SIMDs
                             when the grid fills the SIMDs, nx + nu >= 12 and the launch holds enough Newton steps to
                             amortise the delay; < 0: off; > 0: that many units of ~1024 clocks. Timing only: results do
                             not depend on it. No counterpart in the reference (a scheduling control of this library). */
} AlqpParams;

/* optional per-step trace (all nullable, for tests): S = al_iter*max_newton steps */
typedef struct AlqpTrace {
    void *g;        /* [S][B][T][n] merit gradient */
    void *d;        /* [S][B][T][n] Newton update */
    void *phi;      /* [S][n_ls][B] candidate merits */
    void *phi_prev; /* [S][B] */
    int *k;         /* [S][B] chosen candidate */
    int *accept;    /* [S][B] */
} AlqpTrace;

#define ALQP_E_BADARG     (-1)
#define ALQP_E_UNSUPPORTED (-2)  /* (nx,nu) not instantiated or LDS budget exceeded */
#define ALQP_E_LAUNCH     (-3)
#define ALQP_E_COOP       (-4)  /* ALQP_EXIT_IN_KERNEL: the grid is too large for a cooperative launch */

/* 1 if (nx,nu) has a compiled kernel instance (the quad variant then runs any horizon). */
int alqp_supported(const AlqpDims *dims, int is_f64);
/* Per variant (AlqpParams.variant): 1 team - additionally the horizon's factor must fit the LDS image;
 * 2 quad - needs alqp_workspace_bytes() of workspace, no LDS. */
int alqp_supported_variant(const AlqpDims *dims, int is_f64, int variant);
/* Which kernel alqp_solve_lin's variant 0 resolves to, given a sufficient workspace: 1 team, 2 quad,
 * 0 when (nx, nu) has no compiled instance. quad_min_batch < 0: the measured table; >= 0: quad from that batch on
 * (test and experiment override). */
int alqp_pick_variant(const AlqpDims *dims, int is_f64, int flags, long quad_min_batch);
/* LDS bytes one workgroup of the fused kernel uses (0 if unsupported). */
size_t alqp_lds_bytes(const AlqpDims *dims, int is_f64);
/* QP instances one 64-lane wavefront solves concurrently (team variant). */
int alqp_qps_per_wave(const AlqpDims *dims, int is_f64);
/* Bytes of device workspace the quad variant of alqp_solve_lin needs for these dims
 * (0 if (nx,nu) is not instantiated). The caller allocates; contents need not be kept
 * between calls. Layout: fp32 [ceil(B/2)][T][RECW/16][2][16] (the records of instances 2i, 2i+1
 * interleaved in 64-byte blocks), fp64 [B][T][RECW]. */
size_t alqp_workspace_bytes(const AlqpDims *dims, int is_f64);

/*
 * Fused solve on affine ("LinDx") dynamics x_{t+1} = F_t [x_t;u_t] + c_t.
 * Replaces MPC.al_solve (qpth/AL_mpc.py:260-339) + NewtonAL.forward
 * (qpth/al_utils.py:451-576) + line_search_newton (:618-642) for one batch:
 * al_iter x [merit init; max_newton x (gradient, block-tridiagonal Cholesky,
 * Newton step, 20-point line search); dual update + projection; rho *= rho_scale].
 *   in/out: z (start iterate -> solution), lam, rho, phi (merit carried between
 *           calls when ALQP_INIT_MERIT is off)
 *   out   : rnorm2[B] = sum r+(z)^2 (what the reference's batch-global exit test
 *           sums, al_utils.py:552), info[B] (0 or stage*n+pivot+1 of the first
 *           non-positive pivot), status[B] (1 = iterate finite, al_utils.py:545-549),
 *           factor_out (nullable), trace (nullable)
 *   workspace: device scratch of >= alqp_workspace_bytes() for the quad variant (nullable
 *           -> team variant)
 */
int alqp_solve_lin_f32(const AlqpDims *dims, const AlqpParams *prm, const void *Qd, const void *q,
                       const void *F, const void *c, const void *x0, const void *u_lo,
                       const void *u_hi, long sb_u, long st_u, void *z, void *lam, void *rho,
                       void *phi, void *rnorm2, int *info, unsigned char *status,
                       void *factor_out, const AlqpTrace *trace, void *workspace, size_t ws_bytes,
                       void *stream);
int alqp_solve_lin_f64(const AlqpDims *dims, const AlqpParams *prm, const void *Qd, const void *q,
                       const void *F, const void *c, const void *x0, const void *u_lo,
                       const void *u_hi, long sb_u, long st_u, void *z, void *lam, void *rho,
                       void *phi, void *rnorm2, int *info, unsigned char *status,
                       void *factor_out, const AlqpTrace *trace, void *workspace, size_t ws_bytes,
                       void *stream);

/*
 * The same solve on BATCH-SHARED DYNAMICS: F and c are addressed with an instance stride and a stage stride (words), the
 * convention of sb_u / st_u, so that one model serves the whole batch without B copies of it:
 *   F [nx][n]          one F for every instance and stage (LTI)    sb_F = 0,             st_F = 0
 *   F [T-1][nx][n]     one sequence F_t for every instance (LTV)   sb_F = 0,             st_F = nx n
 *   F [B][T-1][nx][n]  per instance, as alqp_solve_lin_* reads it  sb_F = (T-1) nx n,    st_F = nx n
 * and c likewise without the [n] (0, 0 / 0, nx / (T-1) nx, nx), independently of F. Any other stride pair, a negative
 * stride or a null F or c is ALQP_E_BADARG; F and c must hold (B-1) sb + (T-2) st + nx n (nx) words. Everything else -
 * arguments, AlqpParams.variant 0 / 1 / 2 and alqp_pick_variant's rule, workspace, every flag, skip_flag, trace,
 * factor_out, what is refused - is alqp_solve_lin_*'s, and so is every number: the kernels (k_solve_lin_shdyn,
 * k_solve_lin_quad_shdyn) do the plain kernels' arithmetic in the same order, the result equals bit for bit that of
 * alqp_solve_lin_* on the expanded arrays. alqp_backward_* keeps reading a per-instance F.
 */
int alqp_solve_lin_shared_f32(const AlqpDims *dims, const AlqpParams *prm, const void *Qd, const void *q,
                              const void *F, const void *c, long sb_F, long st_F, long sb_c, long st_c,
                              const void *x0, const void *u_lo, const void *u_hi, long sb_u, long st_u, void *z,
                              void *lam, void *rho, void *phi, void *rnorm2, int *info, unsigned char *status,
                              void *factor_out, const AlqpTrace *trace, void *workspace, size_t ws_bytes,
                              void *stream);
int alqp_solve_lin_shared_f64(const AlqpDims *dims, const AlqpParams *prm, const void *Qd, const void *q,
                              const void *F, const void *c, long sb_F, long st_F, long sb_c, long st_c,
                              const void *x0, const void *u_lo, const void *u_hi, long sb_u, long st_u, void *z,
                              void *lam, void *rho, void *phi, void *rnorm2, int *info, unsigned char *status,
                              void *factor_out, const AlqpTrace *trace, void *workspace, size_t ws_bytes,
                              void *stream);

/*
 * The same solve with a DENSE stage cost 1/2 z_t' C_t z_t + q_t' z_t: C [B][T][n][n] row-major takes the place of Qd.
 * C_t must be symmetric (the caller symmetrises; the kernel reads whole rows) and H_tt = C_t + penalty terms positive
 * definite. The reference sketches this case (al_utils.compute_cost's diag_cost=False branch) but cannot run it.
 * Team kernel only: no workspace; AlqpParams.variant must be 0 or 1 (ALQP_E_BADARG otherwise); ALQP_E_UNSUPPORTED when
 * the horizon's LDS image does not fit (alqp_supported_variant(dims, is_f64, 1): the image is that of the plain team
 * kernel, row hi of C_t lives in registers). Every flag of alqp_solve_lin_* except ALQP_WS_PRIMED (ignored), skip_flag
 * and trace work as there. factor_out is the packed factor alqp_backward_* takes; with w = q_grad of that call the
 * gradient w.r.t. C is 0.5 (w z_final' + z_final w') per stage, which the caller forms (Qd_grad is its diagonal).
 */
int alqp_solve_lin_dense_f32(const AlqpDims *dims, const AlqpParams *prm, const void *C, const void *q,
                             const void *F, const void *c, const void *x0, const void *u_lo,
                             const void *u_hi, long sb_u, long st_u, void *z, void *lam, void *rho,
                             void *phi, void *rnorm2, int *info, unsigned char *status,
                             void *factor_out, const AlqpTrace *trace, void *stream);
int alqp_solve_lin_dense_f64(const AlqpDims *dims, const AlqpParams *prm, const void *C, const void *q,
                             const void *F, const void *c, const void *x0, const void *u_lo,
                             const void *u_hi, long sb_u, long st_u, void *z, void *lam, void *rho,
                             void *phi, void *rnorm2, int *info, unsigned char *status,
                             void *factor_out, const AlqpTrace *trace, void *stream);

/*
 * The same solve with STATE BOX ROWS x_lo[t] <= x_t <= x_hi[t] on all T stages (stage 0 included) next to the control
 * bounds. x_lo / x_hi: [nx] shared by every instance and stage (sb_x = st_x = 0) or [B][T][nx] (sb_x = T nx, st_x = nx).
 * Entries must be finite: "no bound" is a bound no state reaches whose product with the largest rho stays finite (the
 * host uses +-1e20); an infinity would make lam * r NaN in the merit. The reference carries x_lower / x_upper
 * (AL_mpc.py:154-155) but leaves their rows commented out (al_utils.py:294-302) and cannot run this case.
 * lam is [B][M] with M = T nx + T (2 nu + 2 nx): the T nx equality rows as everywhere, then per stage
 * [u - u_hi | -u + u_lo | x - x_hi | -x + x_lo] (the order of al_utils.py:293-302). Conventions of the control rows:
 * Hessian term where the residual is >= 0, gradient and merit terms max(r, 0), dual update max(0, lam + rho r).
 * Team kernel only: no workspace; AlqpParams.variant must be 0 or 1 (ALQP_E_BADARG otherwise); ALQP_E_UNSUPPORTED when
 * the horizon's LDS image does not fit (that of the plain team kernel: the rows need no LDS). Flags, skip_flag and trace
 * as alqp_solve_lin_dense_*. factor_out is the packed factor alqp_backward_* takes unchanged (the active rows' penalty
 * terms are on its diagonal: the active set is held fixed in the backward pass).
 */
int alqp_solve_lin_xbox_f32(const AlqpDims *dims, const AlqpParams *prm, const void *Qd, const void *q,
                            const void *F, const void *c, const void *x0, const void *u_lo,
                            const void *u_hi, long sb_u, long st_u, const void *x_lo, const void *x_hi,
                            long sb_x, long st_x, void *z, void *lam, void *rho, void *phi, void *rnorm2,
                            int *info, unsigned char *status, void *factor_out, const AlqpTrace *trace,
                            void *stream);
int alqp_solve_lin_xbox_f64(const AlqpDims *dims, const AlqpParams *prm, const void *Qd, const void *q,
                            const void *F, const void *c, const void *x0, const void *u_lo,
                            const void *u_hi, long sb_u, long st_u, const void *x_lo, const void *x_hi,
                            long sb_x, long st_x, void *z, void *lam, void *rho, void *phi, void *rnorm2,
                            int *info, unsigned char *status, void *factor_out, const AlqpTrace *trace,
                            void *stream);

/*
 * The same solve with m GENERAL LINEAR ROWS G_t z_t <= h_t per stage, z_t = [x_t; u_t], on all T stages next to the
 * control bounds (1 <= m <= 64, a run-time number). G: [m][n] shared by every instance and stage (sb_g = st_g = 0),
 * [T][m][n] per stage (0, m n) or [B][T][m][n] per instance (T m n, m n); h likewise without the [n] (sb_h, st_h: 0, 0 /
 * 0, m / T m, m), independently of G. Entries must be finite: "no row" is a right-hand side no stage reaches whose
 * product with the largest rho stays finite (the host uses 1e20). The reference carries ineqG / ineqh but never calls
 * the code that reads them (AL_mpc.py:496-498) and cannot run this case.
 * lam is [B][M] with M = T nx + T (2 nu + m): the T nx equality rows as everywhere, then per stage
 * [u - u_hi | -u + u_lo | G_t z_t - h_t]. Conventions of the control rows: for r = G_k z_t - h_k, Hessian term
 * rho G_k' G_k where r >= 0, gradient and merit terms max(r, 0), dual update max(0, lam + rho r).
 * Team kernel only: no workspace; AlqpParams.variant must be 0 or 1 (ALQP_E_BADARG otherwise, as for a null G or h and
 * an m outside 1..64); ALQP_E_UNSUPPORTED when (nx, nu) is no compiled instance or the horizon's LDS image does not fit:
 * alqp_lds_bytes plus alqp_qps_per_wave * 2 * ((m + 3) & ~3) words. Flags, skip_flag and trace as
 * alqp_solve_lin_dense_*. factor_out is the packed factor alqp_backward_* takes unchanged (the active rows' rank-one
 * terms are in it: the active set is held fixed in the backward pass).
 */
int alqp_solve_lin_poly_f32(const AlqpDims *dims, const AlqpParams *prm, const void *Qd, const void *q,
                            const void *F, const void *c, const void *x0, const void *u_lo,
                            const void *u_hi, long sb_u, long st_u, const void *G, const void *h, int m,
                            long sb_g, long st_g, long sb_h, long st_h, void *z, void *lam, void *rho,
                            void *phi, void *rnorm2, int *info, unsigned char *status, void *factor_out,
                            const AlqpTrace *trace, void *stream);
int alqp_solve_lin_poly_f64(const AlqpDims *dims, const AlqpParams *prm, const void *Qd, const void *q,
                            const void *F, const void *c, const void *x0, const void *u_lo,
                            const void *u_hi, long sb_u, long st_u, const void *G, const void *h, int m,
                            long sb_g, long st_g, long sb_h, long st_h, void *z, void *lam, void *rho,
                            void *phi, void *rnorm2, int *info, unsigned char *status, void *factor_out,
                            const AlqpTrace *trace, void *stream);

/*
 * The same solve with TWO OR THREE of the three additions above TOGETHER: the arguments of alqp_solve_lin_*, then those of
 * a dense cost (C), of state bounds (x_lo, x_hi, sb_x, st_x) and of general rows (G, h, m, sb_g, st_g, sb_h, st_h), each
 * as its own entry point above takes them. A null pointer means "feature absent", and the non-null set picks the kernel:
 * C + bounds, C + rows, bounds + rows, or all three. Qd is read only when C is null (and may be null otherwise).
 * lam is [B][M] with M = T nx + T (2 nu + [2 nx] + [m]): the T nx equality rows, then per stage
 * [u - u_hi | -u + u_lo | x - x_hi | -x + x_lo | G_t z_t - h_t], a feature's rows present exactly when the feature is.
 * Team kernel only: workspace / ws_bytes are not read, AlqpParams.variant must be 0 or 1. ALQP_E_BADARG: fewer than two
 * features present (the entry points above stay the way to run one), one half of a pair null, m outside 1..64 with rows
 * given, a negative stride, variant 2. ALQP_E_UNSUPPORTED: (nx, nu) is no compiled instance, or the horizon's LDS image
 * does not fit (that of alqp_solve_lin_poly_* with rows, the team image without). Flags, skip_flag, trace, factor_out and
 * an empty batch as for the entry points above.
 */
int alqp_solve_lin_gen_f32(const AlqpDims *dims, const AlqpParams *prm, const void *Qd, const void *q,
                           const void *F, const void *c, const void *x0, const void *u_lo, const void *u_hi,
                           long sb_u, long st_u, void *z, void *lam, void *rho, void *phi, void *rnorm2,
                           int *info, unsigned char *status, void *factor_out, const AlqpTrace *trace,
                           void *workspace, size_t ws_bytes, void *stream, const void *C, const void *x_lo,
                           const void *x_hi, long sb_x, long st_x, const void *G, const void *h, int m,
                           long sb_g, long st_g, long sb_h, long st_h);
int alqp_solve_lin_gen_f64(const AlqpDims *dims, const AlqpParams *prm, const void *Qd, const void *q,
                           const void *F, const void *c, const void *x0, const void *u_lo, const void *u_hi,
                           long sb_u, long st_u, void *z, void *lam, void *rho, void *phi, void *rnorm2,
                           int *info, unsigned char *status, void *factor_out, const AlqpTrace *trace,
                           void *workspace, size_t ws_bytes, void *stream, const void *C, const void *x_lo,
                           const void *x_hi, long sb_x, long st_x, const void *G, const void *h, int m,
                           long sb_g, long st_g, long sb_h, long st_h);

/*
 * One Newton direction for the nonlinear-caller mode: the caller evaluated
 * dx_jac(x,u) -> (xnext, F) in PyTorch (al_utils.py:233-248). Replaces
 * merit_grad_hessian (:80-123) + cholesky_ex/cholesky_solve (:510-515).
 *   out: d[B][T][n] = -H^{-1} g, g_out (nullable), factor_out (nullable), info[B]
 *   obs (nullable): the extra rows of "Obstacle inequalities" below.
 *   workspace (nullable): NULL runs the team kernel. Non-null selects the quad kernels (16 instances per wavefront; use
 *   them once the batch fills the chip, B >= 4096): the per-stage factor is streamed through - and left in - `workspace`
 *   (alqp_workspace_bytes()), where alqp_backward_* finds it for NewtonAL.backward; no packed factor_out then.
 */
int alqp_newton_step_f32(const AlqpDims *dims, const void *z, const void *xnext, const void *F,
                         const void *x0, const void *lam, const void *rho, const void *Qd,
                         const void *q, const void *u_lo, const void *u_hi, long sb_u, long st_u,
                         const AlqpObstacles *obs, void *workspace, size_t ws_bytes,
                         void *d_out, void *g_out, void *factor_out, int *info, void *stream);
int alqp_newton_step_f64(const AlqpDims *dims, const void *z, const void *xnext, const void *F,
                         const void *x0, const void *lam, const void *rho, const void *Qd,
                         const void *q, const void *u_lo, const void *u_hi, long sb_u, long st_u,
                         const AlqpObstacles *obs, void *workspace, size_t ws_bytes,
                         void *d_out, void *g_out, void *factor_out, int *info, void *stream);

/*
 * Merit of K stacked candidates (al_utils.py:52-77 with the [K,B,T,n] broadcast of
 * :56-70): zc[K][B][T][n], xnext[K][B][T-1][nx] -> phi[K][B], rnorm2[K][B] (nullable). obs nullable.
 */
int alqp_merit_f32(const AlqpDims *dims, int K, const void *zc, const void *xnext, const void *x0,
                   const void *lam, const void *rho, const void *Qd, const void *q,
                   const void *u_lo, const void *u_hi, long sb_u, long st_u, const AlqpObstacles *obs,
                   void *phi, void *rnorm2, void *stream);
int alqp_merit_f64(const AlqpDims *dims, int K, const void *zc, const void *xnext, const void *x0,
                   const void *lam, const void *rho, const void *Qd, const void *q,
                   const void *u_lo, const void *u_hi, long sb_u, long st_u, const AlqpObstacles *obs,
                   void *phi, void *rnorm2, void *stream);

/*
 * Line-search decision + update (al_utils.py:634-641): first argmin over phi[n_ls][B],
 * accept iff strictly below phi_prev; z <- accept ? z + 2^-k d : z (in place);
 * phi_prev <- phi_min regardless (al_utils.py:569). k_out/accept_out nullable.
 * Any n_ls >= 1: 2^-k is formed in the solve's precision for every k (zero once it underflows).
 */
int alqp_linesearch_pick_f32(const AlqpDims *dims, int n_ls, const void *phi, void *phi_prev,
                             const void *d, void *z, int *k_out, int *accept_out, void *stream);
int alqp_linesearch_pick_f64(const AlqpDims *dims, int n_ls, const void *phi, void *phi_prev,
                             const void *d, void *z, int *k_out, int *accept_out, void *stream);

/*
 * The whole line search of a Newton step in one launch (nonlinear-caller mode at scale): merits of the
 * n_ls candidates z + 2^-k d, given x_next of every candidate from the caller's dynamics
 * (xnext_all[n_ls][B][T-1][nx], what the reference's 20-fold replicated dx call returns,
 * al_utils.py:56-70, 629-633), then the decision and update of alqp_linesearch_pick. z, d are read
 * once; the stacked candidates the reference materialises are never formed for the merit.
 *   in/out: z, phi_prev; rnorm2[B] (nullable) <- sum r+^2 of the chosen candidate when accepted
 *   out   : phi_all[n_ls][B] (nullable), k_out, accept_out (nullable); obs nullable (Obstacle_MPC rows)
 */
int alqp_merit_pick_f32(const AlqpDims *dims, int n_ls, const void *d, const void *xnext_all, const void *x0,
                        const void *lam, const void *rho, const void *Qd, const void *q, const void *u_lo,
                        const void *u_hi, long sb_u, long st_u, const AlqpObstacles *obs, void *z,
                        void *phi_prev, void *rnorm2, void *phi_all, int *k_out, int *accept_out, void *stream);
int alqp_merit_pick_f64(const AlqpDims *dims, int n_ls, const void *d, const void *xnext_all, const void *x0,
                        const void *lam, const void *rho, const void *Qd, const void *q, const void *u_lo,
                        const void *u_hi, long sb_u, long st_u, const AlqpObstacles *obs, void *z,
                        void *phi_prev, void *rnorm2, void *phi_all, int *k_out, int *accept_out, void *stream);

/*
 * Dual update + projection + penalty growth (AL_mpc.py:315-317, 325) given
 * xnext = f(x_t,u_t) at the final iterate; lam, rho updated in place. obs nullable.
 */
int alqp_dual_update_f32(const AlqpDims *dims, const void *z, const void *xnext, const void *x0,
                         const void *u_lo, const void *u_hi, long sb_u, long st_u, const AlqpObstacles *obs,
                         void *lam, void *rho, double rho_scale, void *stream);
int alqp_dual_update_f64(const AlqpDims *dims, const void *z, const void *xnext, const void *x0,
                         const void *u_lo, const void *u_hi, long sb_u, long st_u, const AlqpObstacles *obs,
                         void *lam, void *rho, double rho_scale, void *stream);

/*
 * The four launch-per-step operations above with the state box rows of alqp_solve_lin_xbox_* (x_lo[t] <= x_t <= x_hi[t] on
 * all T stages, stage 0 included): state bounds with a caller-evaluated nonlinear model. Each takes its plain twin's
 * arguments without the AlqpObstacles (no obstacle rows, no state-estimator row set), with x_lo, x_hi, sb_x, st_x right
 * behind the control bounds: element (b,t,i) at b*sb_x + t*st_x + i, finite, [nx] (0, 0) or [B][T][nx] (T nx, nx).
 *   lam [B][T*nx + T*(2nu + 2nx)]: per stage [u - u_hi | -u + u_lo | x - x_hi | -x + x_lo] behind the equality rows.
 * A state row follows the control rows' conventions: lam * r with the unclamped r plus rho/2 max(r, 0)^2 in the merit,
 * rho on the diagonal of H_tt while r >= 0, max(0, lam + rho r) in the dual update.
 * alqp_newton_step_xbox_*: the team kernel only - no workspace argument; the packed factor_out is what alqp_backward_*
 * takes. ALQP_E_UNSUPPORTED for an (nx, nu) that is not compiled and for a horizon whose LDS image does not fit
 * (alqp_supported_variant(dims, is_f64, 1) == 0); ALQP_E_BADARG for a null bound, a negative stride, an empty batch, and
 * for n_ls outside 1..20 in alqp_merit_pick_xbox_*.
 * These symbols were ADDED under ABI version 17 (no existing signature changed, so the number did not move): a caller
 * that may meet an older library of version 17 detects them by symbol lookup.
 */
int alqp_newton_step_xbox_f32(const AlqpDims *dims, const void *z, const void *xnext, const void *F,
                              const void *x0, const void *lam, const void *rho, const void *Qd,
                              const void *q, const void *u_lo, const void *u_hi, long sb_u, long st_u,
                              const void *x_lo, const void *x_hi, long sb_x, long st_x,
                              void *d_out, void *g_out, void *factor_out, int *info, void *stream);
int alqp_newton_step_xbox_f64(const AlqpDims *dims, const void *z, const void *xnext, const void *F,
                              const void *x0, const void *lam, const void *rho, const void *Qd,
                              const void *q, const void *u_lo, const void *u_hi, long sb_u, long st_u,
                              const void *x_lo, const void *x_hi, long sb_x, long st_x,
                              void *d_out, void *g_out, void *factor_out, int *info, void *stream);
int alqp_merit_xbox_f32(const AlqpDims *dims, int K, const void *zc, const void *xnext, const void *x0,
                        const void *lam, const void *rho, const void *Qd, const void *q,
                        const void *u_lo, const void *u_hi, long sb_u, long st_u,
                        const void *x_lo, const void *x_hi, long sb_x, long st_x,
                        void *phi, void *rnorm2, void *stream);
int alqp_merit_xbox_f64(const AlqpDims *dims, int K, const void *zc, const void *xnext, const void *x0,
                        const void *lam, const void *rho, const void *Qd, const void *q,
                        const void *u_lo, const void *u_hi, long sb_u, long st_u,
                        const void *x_lo, const void *x_hi, long sb_x, long st_x,
                        void *phi, void *rnorm2, void *stream);
int alqp_merit_pick_xbox_f32(const AlqpDims *dims, int n_ls, const void *d, const void *xnext_all, const void *x0,
                             const void *lam, const void *rho, const void *Qd, const void *q, const void *u_lo,
                             const void *u_hi, long sb_u, long st_u, const void *x_lo, const void *x_hi,
                             long sb_x, long st_x, void *z, void *phi_prev, void *rnorm2, void *phi_all,
                             int *k_out, int *accept_out, void *stream);
int alqp_merit_pick_xbox_f64(const AlqpDims *dims, int n_ls, const void *d, const void *xnext_all, const void *x0,
                             const void *lam, const void *rho, const void *Qd, const void *q, const void *u_lo,
                             const void *u_hi, long sb_u, long st_u, const void *x_lo, const void *x_hi,
                             long sb_x, long st_x, void *z, void *phi_prev, void *rnorm2, void *phi_all,
                             int *k_out, int *accept_out, void *stream);
int alqp_dual_update_xbox_f32(const AlqpDims *dims, const void *z, const void *xnext, const void *x0,
                              const void *u_lo, const void *u_hi, long sb_u, long st_u,
                              const void *x_lo, const void *x_hi, long sb_x, long st_x,
                              void *lam, void *rho, double rho_scale, void *stream);
int alqp_dual_update_xbox_f64(const AlqpDims *dims, const void *z, const void *xnext, const void *x0,
                              const void *u_lo, const void *u_hi, long sb_u, long st_u,
                              const void *x_lo, const void *x_hi, long sb_x, long st_x,
                              void *lam, void *rho, double rho_scale, void *stream);

/*
 * The same four with the general rows of alqp_solve_lin_poly_* (m rows G_t [x_t; u_t] <= h_t per stage, on all T stages),
 * with or without the state box rows: general rows with a caller-evaluated nonlinear model. Each takes its _xbox twin's
 * arguments, with G, h, m, sb_g, st_g, sb_h, st_h right behind the state-bound arguments: row k of stage t of instance b
 * at G + b*sb_g + t*st_g + k*n, its right-hand side at h + b*sb_h + t*st_h + k ([m][n]: 0, 0; [T][m][n]: 0, m n;
 * [B][T][m][n]: T m n, m n; read in place), all finite. x_lo and x_hi may BOTH be null: no state bounds.
 *   lam [B][T*nx + T*(2nu + XR + m)], XR = 2nx with state bounds and 0 without: per stage
 *   [u - u_hi | -u + u_lo | (x - x_hi | -x + x_lo) | G_t z_t - h_t] behind the equality rows.
 * A row follows the box rows' conventions: lam_k r_k with the unclamped r_k = G_k . z_t - h_k plus rho/2 max(r_k, 0)^2 in
 * the merit, max(r_k, 0)^2 in rnorm2, rho G_k' G_k in H_tt while r_k >= 0, max(0, lam_k + rho r_k) in the dual update.
 * alqp_newton_step_rows_*: the team kernel only - no workspace argument; the packed factor_out is what alqp_backward_*
 * takes. ALQP_E_UNSUPPORTED for an (nx, nu) that is not compiled and for a horizon or m whose LDS image (the team image plus
 * 2 pad4(m) words per team) does not fit; ALQP_E_BADARG for a null G or h, m outside 1..64, one of x_lo / x_hi null alone,
 * a negative stride, an empty batch, and for n_ls outside 1..20 in alqp_merit_pick_rows_*.
 * ADDED under ABI version 17 like the _xbox symbols: detect them by symbol lookup.
 */
int alqp_newton_step_rows_f32(const AlqpDims *dims, const void *z, const void *xnext, const void *F,
                              const void *x0, const void *lam, const void *rho, const void *Qd,
                              const void *q, const void *u_lo, const void *u_hi, long sb_u, long st_u,
                              const void *x_lo, const void *x_hi, long sb_x, long st_x,
                              const void *G, const void *h, int m, long sb_g, long st_g, long sb_h, long st_h,
                              void *d_out, void *g_out, void *factor_out, int *info, void *stream);
int alqp_newton_step_rows_f64(const AlqpDims *dims, const void *z, const void *xnext, const void *F,
                              const void *x0, const void *lam, const void *rho, const void *Qd,
                              const void *q, const void *u_lo, const void *u_hi, long sb_u, long st_u,
                              const void *x_lo, const void *x_hi, long sb_x, long st_x,
                              const void *G, const void *h, int m, long sb_g, long st_g, long sb_h, long st_h,
                              void *d_out, void *g_out, void *factor_out, int *info, void *stream);
int alqp_merit_rows_f32(const AlqpDims *dims, int K, const void *zc, const void *xnext, const void *x0,
                        const void *lam, const void *rho, const void *Qd, const void *q,
                        const void *u_lo, const void *u_hi, long sb_u, long st_u,
                        const void *x_lo, const void *x_hi, long sb_x, long st_x,
                        const void *G, const void *h, int m, long sb_g, long st_g, long sb_h, long st_h,
                        void *phi, void *rnorm2, void *stream);
int alqp_merit_rows_f64(const AlqpDims *dims, int K, const void *zc, const void *xnext, const void *x0,
                        const void *lam, const void *rho, const void *Qd, const void *q,
                        const void *u_lo, const void *u_hi, long sb_u, long st_u,
                        const void *x_lo, const void *x_hi, long sb_x, long st_x,
                        const void *G, const void *h, int m, long sb_g, long st_g, long sb_h, long st_h,
                        void *phi, void *rnorm2, void *stream);
int alqp_merit_pick_rows_f32(const AlqpDims *dims, int n_ls, const void *d, const void *xnext_all, const void *x0,
                             const void *lam, const void *rho, const void *Qd, const void *q, const void *u_lo,
                             const void *u_hi, long sb_u, long st_u, const void *x_lo, const void *x_hi,
                             long sb_x, long st_x, const void *G, const void *h, int m, long sb_g, long st_g,
                             long sb_h, long st_h, void *z, void *phi_prev, void *rnorm2, void *phi_all,
                             int *k_out, int *accept_out, void *stream);
int alqp_merit_pick_rows_f64(const AlqpDims *dims, int n_ls, const void *d, const void *xnext_all, const void *x0,
                             const void *lam, const void *rho, const void *Qd, const void *q, const void *u_lo,
                             const void *u_hi, long sb_u, long st_u, const void *x_lo, const void *x_hi,
                             long sb_x, long st_x, const void *G, const void *h, int m, long sb_g, long st_g,
                             long sb_h, long st_h, void *z, void *phi_prev, void *rnorm2, void *phi_all,
                             int *k_out, int *accept_out, void *stream);
int alqp_dual_update_rows_f32(const AlqpDims *dims, const void *z, const void *xnext, const void *x0,
                              const void *u_lo, const void *u_hi, long sb_u, long st_u,
                              const void *x_lo, const void *x_hi, long sb_x, long st_x,
                              const void *G, const void *h, int m, long sb_g, long st_g, long sb_h, long st_h,
                              void *lam, void *rho, double rho_scale, void *stream);
int alqp_dual_update_rows_f64(const AlqpDims *dims, const void *z, const void *xnext, const void *x0,
                              const void *u_lo, const void *u_hi, long sb_u, long st_u,
                              const void *x_lo, const void *x_hi, long sb_x, long st_x,
                              const void *G, const void *h, int m, long sb_g, long st_g, long sb_h, long st_h,
                              void *lam, void *rho, double rho_scale, void *stream);

/*
 * Newton step, merit and pick with the dense stage cost of alqp_solve_lin_dense_* (1/2 z_t' C_t z_t + q_t' z_t, C [B][T][n][n]
 * row-major, symmetric, finite), alone or with state box rows and / or general rows: a dense cost with a caller-evaluated
 * nonlinear model. Each takes its _rows twin's arguments with C where Qd stood. x_lo and x_hi may BOTH be null (no state
 * bounds); G and h may BOTH be null with m == 0 (no general rows).
 *   lam [B][T*nx + T*(2nu + XR + m)], XR = 2nx with state bounds and 0 without, m = 0 without general rows.
 * The dual update reads no cost: alqp_dual_update_*, _xbox_* or _rows_* as the rows demand.
 * alqp_newton_step_dense_*: the team kernel only - no workspace argument; the packed factor_out is what alqp_backward_*
 * takes. ALQP_E_UNSUPPORTED for an (nx, nu) that is not compiled and for a horizon (or m) whose LDS image (the team image,
 * with general rows plus 2 pad4(m) words per team) does not fit; ALQP_E_BADARG for a null C, one of x_lo / x_hi null alone,
 * G without h or h without G, m outside 1..64 with G, a nonzero m without G, a negative stride, an empty batch, and for
 * n_ls outside 1..20 in alqp_merit_pick_dense_*.
 * ADDED under ABI version 17 like the _rows symbols: detect them by symbol lookup.
 */
int alqp_newton_step_dense_f32(const AlqpDims *dims, const void *z, const void *xnext, const void *F,
                               const void *x0, const void *lam, const void *rho, const void *C,
                               const void *q, const void *u_lo, const void *u_hi, long sb_u, long st_u,
                               const void *x_lo, const void *x_hi, long sb_x, long st_x,
                               const void *G, const void *h, int m, long sb_g, long st_g, long sb_h, long st_h,
                               void *d_out, void *g_out, void *factor_out, int *info, void *stream);
int alqp_newton_step_dense_f64(const AlqpDims *dims, const void *z, const void *xnext, const void *F,
                               const void *x0, const void *lam, const void *rho, const void *C,
                               const void *q, const void *u_lo, const void *u_hi, long sb_u, long st_u,
                               const void *x_lo, const void *x_hi, long sb_x, long st_x,
                               const void *G, const void *h, int m, long sb_g, long st_g, long sb_h, long st_h,
                               void *d_out, void *g_out, void *factor_out, int *info, void *stream);
int alqp_merit_dense_f32(const AlqpDims *dims, int K, const void *zc, const void *xnext, const void *x0,
                         const void *lam, const void *rho, const void *C, const void *q,
                         const void *u_lo, const void *u_hi, long sb_u, long st_u,
                         const void *x_lo, const void *x_hi, long sb_x, long st_x,
                         const void *G, const void *h, int m, long sb_g, long st_g, long sb_h, long st_h,
                         void *phi, void *rnorm2, void *stream);
int alqp_merit_dense_f64(const AlqpDims *dims, int K, const void *zc, const void *xnext, const void *x0,
                         const void *lam, const void *rho, const void *C, const void *q,
                         const void *u_lo, const void *u_hi, long sb_u, long st_u,
                         const void *x_lo, const void *x_hi, long sb_x, long st_x,
                         const void *G, const void *h, int m, long sb_g, long st_g, long sb_h, long st_h,
                         void *phi, void *rnorm2, void *stream);
int alqp_merit_pick_dense_f32(const AlqpDims *dims, int n_ls, const void *d, const void *xnext_all, const void *x0,
                              const void *lam, const void *rho, const void *C, const void *q, const void *u_lo,
                              const void *u_hi, long sb_u, long st_u, const void *x_lo, const void *x_hi,
                              long sb_x, long st_x, const void *G, const void *h, int m, long sb_g, long st_g,
                              long sb_h, long st_h, void *z, void *phi_prev, void *rnorm2, void *phi_all,
                              int *k_out, int *accept_out, void *stream);
int alqp_merit_pick_dense_f64(const AlqpDims *dims, int n_ls, const void *d, const void *xnext_all, const void *x0,
                              const void *lam, const void *rho, const void *C, const void *q, const void *u_lo,
                              const void *u_hi, long sb_u, long st_u, const void *x_lo, const void *x_hi,
                              long sb_x, long st_x, const void *G, const void *h, int m, long sb_g, long st_g,
                              long sb_h, long st_h, void *z, void *phi_prev, void *rnorm2, void *phi_all,
                              int *k_out, int *accept_out, void *stream);

/*
 * Backward of the implicit layer (NewtonAL.backward, al_utils.py:578-615):
 * w = -H^{-1} gbar with the saved factor; q_grad = w, Qd_grad = w * z_final.
 * rho is the penalty the factor was built with. Exactly one of `factor` and `workspace` is non-null:
 *   factor     the packed factor_out of the team kernels;
 *   workspace  the workspace a quad-variant alqp_solve_lin_* / alqp_newton_step_* call left behind (the caller must have
 *              kept it untouched: give such solves a dedicated workspace). Its y/d slots are overwritten.
 *
 * dyn (nullable; NULL runs the plain kernels): also return the gradients w.r.t. the affine dynamics
 * x_{t+1} = F_t z_t + c_t and the initial state (the reference has no such gradient). With w = -H^{-1} gbar as above,
 * rho[b] the penalty the factor was built with (that of the last executed Newton step: the rho the solve returned /
 * rho_scale once a dual update has grown it), v_t the dynamics rows t nx + i of the multipliers the solve RETURNED (after
 * the dual update that ends an AL iteration they hold lam + rho r(z_final) on the equality rows) and
 * s_t = w_{t+1}[0:nx] - F_t w_t:
 *     dF [b][t][i][j] = -v_t[i] w_t[j] - rho s_t[i] z_final_t[j]      [B][T-1][nx][n]
 *     dc [b][t][i]    = -rho s_t[i]                                   [B][T-1][nx]
 *     dx0[b][i]       = -rho w_0[i]                                   [B][nx]
 * i.e. dL/dtheta = w' dg/dtheta for the merit gradient g = Q z + q + J'(lam + rho r_+), with the multipliers and the
 * active set held fixed as q_grad / Qd_grad do. lam: instance b at lam + b * sb_lam (words), its first (T-1) nx
 * entries are read; only dF needs it. dF, dc, dx0 are nullable each (a null output is not computed);
 * ALQP_E_BADARG when dF is given without lam or with sb_lam < (T-1) nx. q_grad / Qd_grad are those of the plain call.
 */
typedef struct AlqpBwdDyn {
    const void *lam;
    long sb_lam;
    void *dF, *dc, *dx0;
} AlqpBwdDyn;
int alqp_backward_f32(const AlqpDims *dims, const void *factor, void *workspace, size_t ws_bytes, const void *F,
                      const void *rho, const void *z_final, const void *gbar, void *q_grad, void *Qd_grad,
                      const AlqpBwdDyn *dyn, void *stream);
int alqp_backward_f64(const AlqpDims *dims, const void *factor, void *workspace, size_t ws_bytes, const void *F,
                      const void *rho, const void *z_final, const void *gbar, void *q_grad, void *Qd_grad,
                      const AlqpBwdDyn *dyn, void *stream);

/*
 * The reference leaves its Newton loop on a BATCH-GLOBAL test (al_utils.py:486,551-564):
 * new = ||r_+||_F over the whole batch; stop when new < tol or |old - new| / new < tol.
 * This entry point takes that decision on the device so that the host can enqueue all Newton-step
 * launches of an AL iteration without synchronising: sumsq[0] = sum_b rnorm2[b] (the caller
 * reduces, and all-reduces over ranks when the batch is sharded), ctl = {done, steps, old_norm}.
 *   mode 0: ctl <- {0, 0, sqrt(sumsq)}                       (before the first step)
 *   mode 1: if (!done) { steps++; new = sqrt(sumsq); done = the test above; else old = new }
 * Pass ctl as AlqpParams.skip_flag of the following launches.
 */
int alqp_exit_test(const double *sumsq, double *ctl, int mode, double tol, void *stream);

/*
 * Dynamics provider for the nonlinear-caller mode, pendulum1l: replaces the reference's
 * CasADi-generated pair dynamics(q, qdot, tau, h) / derivatives(...) (deqmpc/my_envs/pendulum1l/
 * src/dynamics.cpp:13-47, generated_dynamics.c:55-140, generated_derivatives.c:52-222) with one
 * kernel that emits the MPC's packed operands: one RK4 step of theta'' = 4 tau - 19.62 sin(theta)
 * and its exact Jacobian.
 *   in : x[K][2] = (theta, omega), u[K][1] = tau, step length h, or h_pt[K] per point when not
 *        NULL (the reference passes a [bsz,1] tensor filled with dt, my_envs/dynamics.py:58)
 *   out: xnext[K][2] (nullable), F[K][2][3] = [A | B] (nullable: dynamics only)
 */
int alqp_dyn_pendulum1l_f32(long K, const void *x, const void *u, double h, const void *h_pt, void *xnext, void *F, void *stream);
int alqp_dyn_pendulum1l_f64(long K, const void *x, const void *u, double h, const void *h_pt, void *xnext, void *F, void *stream);

/*
 * Dynamics provider, cartpole1l (deqmpc/my_envs/cartpole1l/src/dynamics.cpp:13-47 and the two
 * generated files): one RK4 step of  M(th) q'' = tau - (sin(th) th'^2, 0) + (0, 9.81 sin(th)),
 * M = [[11, -cos th], [-cos th, 2]], q = (cart x, pole angle th; th = 0 upright), and its Jacobian.
 *   in : x[K][4] = (q, qdot), tau[K][2], h or h_pt[K]
 *   out: xnext[K][4] (nullable), J[K][4][6] = d xnext / d(q, qdot, tau) (nullable)
 */
int alqp_dyn_cartpole1l_f32(long K, const void *x, const void *tau, double h, const void *h_pt, void *xnext, void *J, void *stream);
int alqp_dyn_cartpole1l_f64(long K, const void *x, const void *tau, double h, const void *h_pt, void *xnext, void *J, void *stream);
/* cartpole1l_v2 (deqmpc/my_envs/cartpole1l_v2/src: a package the reference ships but does not import,
 * my_envs/cartpole.py:35): the same model with M = [[0.7, -0.1 cos th], [-0.1 cos th, 0.05]], Coriolis 0.1 sin(th) th'^2,
 * gravity 0.981 sin(th); same arrays as alqp_dyn_cartpole1l. */
int alqp_dyn_cartpole1l_v2_f32(long K, const void *x, const void *tau, double h, const void *h_pt, void *xnext, void *J, void *stream);
int alqp_dyn_cartpole1l_v2_f64(long K, const void *x, const void *tau, double h, const void *h_pt, void *xnext, void *J, void *stream);

/* cartpole2l (deqmpc/my_envs/cartpole2l/src): q = (cart x, th1, th2 relative to link 1); x[K][6], tau[K][3],
 * xnext[K][6] (nullable), J[K][6][9] = d xnext / d(q, qdot, tau) (nullable). Model: DESIGN.md section 9. */
int alqp_dyn_cartpole2l_f32(long K, const void *x, const void *tau, double h, const void *h_pt, void *xnext, void *J, void *stream);
int alqp_dyn_cartpole2l_f64(long K, const void *x, const void *tau, double h, const void *h_pt, void *xnext, void *J, void *stream);

/*
 * Nonlinear fused solve: the whole AL solve of MPC.al_solve (AL_mpc.py:260-339) with NONLINEAR
 * dynamics in ONE launch, for the robots whose dynamics model is compiled into the library
 * (dyn_id 1 = pendulum1l (nx=2, nu=1), 2 = cartpole1l (nx=4, nu=1, tau = (u, 0)), 3 = cartpole2l (nx=6, nu=1,
 * tau = (u, 0, 0)), 4 = cartpole1l_v2 (as 2, the second package's constants); dyn_h = step length).
 * Replaces the PyTorch round trips of NewtonAL.forward (al_utils.py:451-576): every Newton step
 * re-linearises on the device (dx_jac, :503), the 20 line-search candidates and the dual update
 * are evaluated with the true dynamics (:623-633, AL_mpc.py:315). Arguments as alqp_solve_lin
 * without F, c; n_ls must be 20; workspace of alqp_workspace_bytes_nonlin() bytes; no
 * ALQP_SAVE_FACTOR / ALQP_WS_PRIMED. Exit mode "fixed" (max_newton steps per AL iteration).
 */
size_t alqp_workspace_bytes_nonlin(const AlqpDims *dims, int is_f64);
int alqp_solve_nonlin_f32(const AlqpDims *dims, const AlqpParams *prm, int dyn_id, double dyn_h, const void *Qd,
                          const void *q, const void *x0, const void *u_lo, const void *u_hi, long sb_u, long st_u,
                          void *z, void *lam, void *rho, void *phi, void *rnorm2, int *info, unsigned char *status,
                          void *workspace, size_t ws_bytes, void *stream);
int alqp_solve_nonlin_f64(const AlqpDims *dims, const AlqpParams *prm, int dyn_id, double dyn_h, const void *Qd,
                          const void *q, const void *x0, const void *u_lo, const void *u_hi, long sb_u, long st_u,
                          void *z, void *lam, void *rho, void *phi, void *rnorm2, int *info, unsigned char *status,
                          void *workspace, size_t ws_bytes, void *stream);

/*
 * The nonlinear fused solve with state box rows and / or general rows (ABI 17, symbols added: detect them by lookup):
 * alqp_solve_nonlin's problem plus xlo[t] <= x_t <= xhi[t] and / or G_t z_t <= h_t on every stage, in ONE launch of a
 * team kernel (one lane team per instance, factor in LDS). dyn_id 1 (pendulum1l), 2 (cartpole1l)
 * and 4 (cartpole1l_v2); 3 (cartpole2l) has no instance on this route (ALQP_E_UNSUPPORTED: its builds spill registers).
 * x_lo / x_hi, sb_x, st_x as alqp_solve_lin_xbox takes them, both NULL: no state bounds. G, h, m and their strides as
 * alqp_solve_lin_poly takes them, both NULL and m == 0: no general rows. Every bound and every entry of G and h must be
 * finite (the host encodes "no bound" / "no row" as a value that is never active). lam is [B][M],
 * M = T nx + T (2 nu + [2 nx] + [m]), per stage [u - u_hi | -u + u_lo | x - x_hi | -x + x_lo | G_t z_t - h_t] behind the
 * equality rows, as alqp_solve_lin_gen's.
 * Per AL iteration: with ALQP_INIT_MERIT the merit at z with the true dynamics; max_newton times (linearise at z with
 * the model, Newton direction on that linearisation, the 20 candidate merits with the TRUE dynamics, first argmin,
 * accept iff below the previous merit); the true residual at the iterate the iteration ends on; with ALQP_DUAL_UPDATE
 * the dual update on that residual and rho *= rho_scale. Outputs, info (sticky), status, rnorm2 and trace as
 * alqp_solve_lin_*; factor_out (ALQP_SAVE_FACTOR) receives the packed factor of the last Newton step of a launch that
 * executes one, for alqp_backward_* together with the F region of the workspace.
 * workspace: alqp_workspace_bytes_nonlin_rows() bytes (0: no model of that (nx, nu) on this route), [B] times
 * (F[T-1][nx][n], then xnext[T-1][nx]). Its prior contents are never read before they are written. Launches with
 * max_newton == 0 (merit only, dual update only) and the end of every AL iteration write ONLY the xnext part: the F part
 * keeps the linearisation of the last executed Newton step.
 * n_ls must be 20. ALQP_INIT_MERIT, ALQP_DUAL_UPDATE, ALQP_SAVE_FACTOR and skip_flag as in alqp_solve_lin_*;
 * ALQP_WS_PRIMED is ignored; AlqpParams.variant is not read.
 * ALQP_E_BADARG: neither row family given, one half of a pair null, m outside 1..64 with rows (or m != 0 without), a
 * negative stride, an empty batch, n_ls != 20, a null or too small workspace, ALQP_EXIT_IN_KERNEL (this route has no
 * cooperative exit), ALQP_SAVE_FACTOR without factor_out. ALQP_E_UNSUPPORTED: an unknown dyn_id or one without an
 * instance here, an (nx, nu) that is not the model's, a horizon (or m) whose LDS image (the team image, with general rows
 * plus 2 pad4(m) words per team) does not fit.
 */
size_t alqp_workspace_bytes_nonlin_rows(const AlqpDims *dims, int is_f64);
int alqp_solve_nonlin_rows_f32(const AlqpDims *dims, const AlqpParams *prm, int dyn_id, double dyn_h, const void *Qd,
                               const void *q, const void *x0, const void *u_lo, const void *u_hi, long sb_u, long st_u,
                               const void *x_lo, const void *x_hi, long sb_x, long st_x, const void *G, const void *h,
                               int m, long sb_g, long st_g, long sb_h, long st_h, void *z, void *lam, void *rho,
                               void *phi, void *rnorm2, int *info, unsigned char *status, void *factor_out,
                               const AlqpTrace *trace, void *workspace, size_t ws_bytes, void *stream);
int alqp_solve_nonlin_rows_f64(const AlqpDims *dims, const AlqpParams *prm, int dyn_id, double dyn_h, const void *Qd,
                               const void *q, const void *x0, const void *u_lo, const void *u_hi, long sb_u, long st_u,
                               const void *x_lo, const void *x_hi, long sb_x, long st_x, const void *G, const void *h,
                               int m, long sb_g, long st_g, long sb_h, long st_h, void *z, void *lam, void *rho,
                               void *phi, void *rnorm2, int *info, unsigned char *status, void *factor_out,
                               const AlqpTrace *trace, void *workspace, size_t ws_bytes, void *stream);

/*
 * ---- Obstacle inequalities (Obstacle_MPC, qpth/AL_mpc_custom.py:22-135; al_utils.py:313-323, 351-388) ----
 * `nobs` spheres per stage add the rows  c_k = radius^2 - |x_t[0:3] - pos_k|^2 <= 0  behind the stage's
 * 2 nu bound rows: lam [B][M], M = T*nx + T*(2*nu + nobs), inequality row T*nx + t*(2*nu + nobs) + j with
 * j < nu upper, j < 2 nu lower, then obstacle j - 2 nu (the reference's stage-major order, al_utils.py:376).
 * The Newton step gets the rank-<=nobs Gauss-Newton update 4 rho (p - o_k)(p - o_k)' of the position corner
 * of H_tt for the rows with c_k >= 0 and the gradient term (lam_k + rho max(c_k, 0)) (-2)(p - o_k).
 * AlqpObstacles is a nullable argument of alqp_newton_step_* (team and quad kernels; the reference only reaches
 * Obstacle_MPC with PyTorch-coded dynamics), alqp_merit_*, alqp_merit_pick_* and alqp_dual_update_*. ALQP_E_BADARG when
 * nobs < 0, or nobs > 0 with a null pos or nx < 3.
 */

/*
 * ---- Interior-point QP solve (the `--solver_type ip` path) -------------------------------------------
 * Replaces qp.DenseQPFunction (qpth/qp.py:187-270) = pdipm_b_LU.forward / solve_kkt
 * (qpth/solvers/pdipm/batch_LU.py:29-244) on the QP that qp_wrapper.MPC.single_qp assembles
 * (qpth/qp_wrapper.py:295-321, 612-653):
 *     min 1/2 z'Qz + p'z  s.t.  u_lower <= u_t <= u_upper,  F_t tau_t + f_t = x_{t+1},  x_0 = x0
 * with DIAGONAL Q (what policies.Tracking_MPC builds). Same regularised KKT system (KKTeps = 1e-7), same
 * refinement step, same predictor-corrector iteration; no dense matrix is formed (csrc/alqp_ipm.hip).
 *   Cd, c  diag(C_t) and c_t, element (t, b, k) at t*sC_t + b*sC_b + k      (time-major [T,B,n]: sC_t = B*n, sC_b = n)
 *   F      [.][nx][n] blocks at t*sF_t + b*sF_b;  f [.][nx] at t*sf_t + b*sf_b
 *   x0 [B][nx]; u_hi, u_lo [nu]
 *   zhat [B][T*n]; nus [B][T*nx] (dynamics rows t*nx+i, then the initial-state rows);
 *   lams, slacks [B][2*T*nu] (upper-bound rows t*nu+j, then lower-bound rows T*nu + t*nu+j)   - the
 *   reference's orderings (qp_wrapper.py:194-207)
 *   ry_ext nullable [B][T*nx]: the caller's equality residual at the current iterate (the reference
 *   evaluates the TRUE dynamics there: dyn_res callback, qp_wrapper.py:306, batch_LU.py:95); NULL: A z - b
 *   workspace: alqp_ipm_workspace_bytes(); it carries the iterate between launches of one solve.
 * flags: ALQP_IPM_INIT  initial point (batch_LU.py:44-81)
 *        ALQP_IPM_LOOP  max_iter x [residuals + best iterate ; predictor-corrector step] in this launch
 *                       (exit mode "fixed": no batch-global exit rule, best iterate per instance)
 *        ALQP_IPM_RESID residuals + best-iterate update of iteration iter0 (improved[b], resid[b] = best
 *                       residual, mu[b] for the reference's batch-global exit rule, :147-151, taken by the host)
 *        ALQP_IPM_STEP  one predictor-corrector step (:153-197)
 *        ALQP_IPM_FINAL copy the best iterate to zhat / nus / lams / slacks
 * info[b]: 0, or block*nx + pivot + 1 of the first non-positive pivot of the Schur complement (sticky).
 */
#define ALQP_IPM_INIT  1
#define ALQP_IPM_RESID 2
#define ALQP_IPM_STEP  4
#define ALQP_IPM_LOOP  8
#define ALQP_IPM_FINAL 16

typedef struct AlqpIpmParams {
    int flags;       /* ALQP_IPM_* */
    int max_iter;    /* iterations of an ALQP_IPM_LOOP launch (reference: maxIter = 20, qp.py:203) */
    int iter0;       /* index of the (first) iteration this launch works on */
    double kkt_eps;  /* reference: 1e-7 (batch_LU.py:43) */
    int variant;     /* ALQP_IPM_VARIANT_*: which kernel. Results agree to rounding; a per-call argument, no process state */
} AlqpIpmParams;
/* 0: automatic - the register/LDS-resident kernel (one QP per wavefront, iterate and directions in registers, F and
 *    the Schur factor in LDS; HBM traffic = the inputs once + the best iterate when it improves) whenever the horizon
 *    fits its register slots (T <= 20), else the size-generic kernel with automatic factor placement;
 * 1 / 2: the size-generic kernel (vectors in the workspace) with the Schur factor in LDS / in the workspace;
 * 3: the register/LDS-resident kernel, ALQP_E_UNSUPPORTED when the problem does not fit it.
 * The resident kernel addresses Cd / c, F and f with 32-bit byte offsets from each instance's base, so it fits only
 * while the last element it reads of each array starts below 4 GiB: (T-1)*sC_t + n - 1, (T-2)*sF_t + nx*n - 1 and
 * (T-2)*sf_t + nx - 1 elements, times sizeof(real). Time-major data (qp_wrapper.MPC) passes that at B ~ 135 k in fp64
 * and ~ 270 k in fp32 for (T, nx, nu) = (20, 13, 4); beyond it variant 0 runs the generic kernel. */
#define ALQP_IPM_VARIANT_AUTO 0
#define ALQP_IPM_VARIANT_GENERIC_LDS 1
#define ALQP_IPM_VARIANT_GENERIC_WS 2
#define ALQP_IPM_VARIANT_RESIDENT 3

size_t alqp_ipm_workspace_bytes(const AlqpDims *dims, int is_f64);
int alqp_ipm_solve_f32(const AlqpDims *dims, const AlqpIpmParams *prm, const void *Cd, const void *c,
                       const void *F, const void *f, const void *x0, const void *u_hi, const void *u_lo,
                       long sC_t, long sC_b, long sF_t, long sF_b, long sf_t, long sf_b, void *workspace,
                       size_t ws_bytes, const void *ry_ext, void *zhat, void *nus, void *lams, void *slacks,
                       void *resid, void *mu, int *iter_best, int *improved, int *info, void *stream);
int alqp_ipm_solve_f64(const AlqpDims *dims, const AlqpIpmParams *prm, const void *Cd, const void *c,
                       const void *F, const void *f, const void *x0, const void *u_hi, const void *u_lo,
                       long sC_t, long sC_b, long sF_t, long sF_b, long sf_t, long sf_b, void *workspace,
                       size_t ws_bytes, const void *ry_ext, void *zhat, void *nus, void *lams, void *slacks,
                       void *resid, void *mu, int *iter_best, int *improved, int *info, void *stream);
/*
 * Backward of the QP layer (DenseQPFunction.backward, qp.py:238-252): one KKT solve, without
 * regularisation, at the returned lams / slacks: K (dx, ds, dlam, dnu) = -(gbar, 0, 0, 0).
 * The caller forms the reference's gradient formulas (:254-268) from dx, dlam, dnu. variant: ALQP_IPM_VARIANT_*.
 */
int alqp_ipm_backward_f32(const AlqpDims *dims, const void *Cd, const void *F, long sC_t, long sC_b, long sF_t,
                          long sF_b, const void *lams, const void *slacks, const void *gbar, void *workspace,
                          size_t ws_bytes, void *dx, void *dlam, void *dnu, int *info, int variant, void *stream);
int alqp_ipm_backward_f64(const AlqpDims *dims, const void *Cd, const void *F, long sC_t, long sC_b, long sF_t,
                          long sF_b, const void *lams, const void *slacks, const void *gbar, void *workspace,
                          size_t ws_bytes, void *dx, void *dlam, void *dnu, int *info, int variant, void *stream);

/*
 * ---- Dynamics + Jacobian providers of the reference's torch-coded robots -----------
 * RexQuadrotor (deqmpc/rex_quadrotor.py:98-144; x = (r, MRP, body velocity, body rate) [12], u [4]) and FlyingCartpole
 * (deqmpc/flying_cartpole2d.py:81-148; x = (r, MRP, theta, v, w, theta') [14], u [4]): one RK4 step of length h,
 * x+ [K][nx] and F = [A | B] = d x+ / d (x, u) [K][nx][nx+nu] (either output may be NULL). They replace the
 * reference's `dynamics` TorchScript module and its replicate-nx-times autograd Jacobian (rex_quadrotor.py:136-144).
 * PARITY UNPINNED: the reference files import `rexquad_utils`, which is not in the tree; mrp2quat, quatrot and
 * w2pdotkinematics_mrp are restated from their standard definitions (csrc/alqp_dyn_rigid.hip, oracle/rigid_py.py).
 * The struct carries the constructor values of the reference classes (the Python side fills it, rounding through
 * float32 where the reference builds float32 tensors).
 */
typedef struct AlqpRigidParams {
    double mass;        /* quadrotor: mass; flying cartpole: mass_q + mass_p */
    double J[9], Jinv[9];
    double g[3];
    double motor_dist, kf, bf, km;
    double act_scale;   /* 100 (quadrotor) / 10 (flying cartpole) */
    double u_hover;     /* flying cartpole: u <- act_scale (u + u_hover); 0 for the quadrotor */
    double pend_L;      /* flying cartpole: pendulum length */
    double ss[12];      /* motor arm directions [4][3], normalised */
    double bf_force;    /* quadrotor: Bf_z = 4 bf (rex_quadrotor.py:31-32) */
} AlqpRigidParams;
int alqp_dyn_rexquadrotor_f32(long K, const AlqpRigidParams *p, const void *x, const void *u, double h, void *xnext, void *F, void *stream);
int alqp_dyn_rexquadrotor_f64(long K, const AlqpRigidParams *p, const void *x, const void *u, double h, void *xnext, void *F, void *stream);
int alqp_dyn_flyingcartpole_f32(long K, const AlqpRigidParams *p, const void *x, const void *u, double h, void *xnext, void *F, void *stream);
int alqp_dyn_flyingcartpole_f64(long K, const AlqpRigidParams *p, const void *x, const void *u, double h, void *xnext, void *F, void *stream);

/* Library/ABI version, bumped when a signature changes. */
int alqp_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MI_ALQP_H */
