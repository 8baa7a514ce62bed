// alqp_args.hpp - what the team kernels (alqp_team.hip) and the quad kernels (alqp_quad.hip) share: the kernel argument
// structs and the in-kernel exit test (grid-wide sum with a bounded spin) of the cooperative launches.
#pragma once
#include <hip/hip_runtime.h>

namespace alqp {

// Kernel arguments are kept lean on purpose: every pointer is two SGPRs for the whole
// kernel, and SGPR spills (v_writelane/v_readlane) showed up in the hot loops otherwise.
template <typename real>
struct SolveArgs {
    int B, T;
    int al_iter, max_newton, n_ls, flags;
    real rho_scale;
    const real *Qd, *q, *F, *c, *x0, *ulo, *uhi;
    long sb_u, st_u;
    real *z, *lam, *rho, *phi, *rnorm2;
    int *info;
    unsigned char *status;
    real *factor;
    const double *skip;  // nullable: *skip != 0 -> the launch does nothing (device-side loop exit)
    real dyn_h;          // nonlinear fused solve: step length of the inlined dynamics model
    int stagger;         // quad solve: start offset between the four wavefronts of a CU, units of ~1024 clocks (0: none)
    // ALQP_EXIT_IN_KERNEL (cooperative launch): the reference's batch-global exit test of the Newton loop inside the launch
    double exit_tol;
    int *newton_counts;    // [al_iter] executed Newton steps per AL iteration
    double *exit_scratch;  // arrival counter, then [2][gridDim.x] per-workgroup partial sums (ping-pong), then a time-out flag
};

// The fused solve with a dense stage cost, state box rows and / or stage-wise linear rows G_t z_t <= h_t
// (k_solve_lin_gen<.., DENSE, XBOX, POLY, ..>): every feature's arguments behind the plain ones, in a type of its own so that
// SolveArgs, and with it the plain kernels' argument block, stays what it was. An instantiation reads the members of its
// flags (Qd only without DENSE).
template <typename real>
struct GenSolveArgs : SolveArgs<real> {
    const real *C;           // DENSE: [B][T][n][n] row-major, symmetric
    const real *xlo, *xhi;   // XBOX: [nx] (sb_x = st_x = 0) or [B][T][nx] (sb_x = T nx, st_x = nx)
    long sb_x, st_x;         // words from one instance's / one stage's bounds to the next
    const real *G, *h;       // POLY: G [m][n] (sb_g = st_g = 0), [T][m][n] (0, m n) or [B][T][m][n] (T m n, m n); h likewise without [n]
    int m;                   // rows per stage, 1 .. 64
    long sb_g, st_g;         // words from one instance's / one stage's G to the next
    long sb_h, st_h;
};

// The fused solve on batch-shared dynamics (k_solve_lin_shdyn, k_solve_lin_quad_shdyn): F and c addressed with an
// instance stride and a stage stride like the bounds (sb_u / st_u), again in a type of its own.
// The stage stride of either is 0 or the packed one (nx n / nx; alqp_solve_lin_shared_* takes nothing else), so the kernels
// get it as a mask on the packed stride: one 32-bit register each for the whole kernel instead of a 64-bit stride, and
// 32-bit offset arithmetic. (Measured on the register-capped fp32 builds, bytes of scratch against the plain twin's: 64-bit
// strides (10,3) 80 / 68, (12,4) 144 / 140, (8,2) 116 / 108; a mask on the stage index (10,3) 80 / 68; this form: none above.)
template <typename real>
struct ShdynSolveArgs : SolveArgs<real> {
    long sb_F, sb_c;   // words from one instance's F / c to the next: 0 (shared by the batch) or (T-1) nx n / (T-1) nx
    int mt_F, mt_c;    // -1: stage t's F / c lies t nx n / t nx words behind stage 0's; 0: one F / c for every stage
};

// Words from stage 0 to stage t of an instance's F / c, inside Team (alqp_team.hpp) and Quad (alqp_quad.hpp). The
// shared-dynamics units (-DALQP_SHDYN_UNIT, build.sh) mask the packed stride with the struct's members mt_F / mt_c; every
// other unit keeps the compile-time expression it always had, so its kernels compile to the same code.
#ifdef ALQP_SHDYN_UNIT
#define ALQP_F_STAGE(t) ((unsigned)(t) * (unsigned)((NX * N) & mt_F))   // (32 bits hold T nx n; the instance base is size_t)
#define ALQP_C_STAGE(t) ((unsigned)(t) * (unsigned)(NX & mt_c))
#else
#define ALQP_F_STAGE(t) ((size_t)(t) * NX * N)
#define ALQP_C_STAGE(t) ((t) * NX)
#endif

// sum of one value per workgroup over the whole (cooperatively launched) grid, the same bits in every lane of every
// workgroup: partials in workgroup order, 64 interleaved chains, xor butterfly. Every workgroup must call it.
__device__ inline double grid_sum_ordered(double block_val, double *scratch, int &phase) {
    // scratch: one arrival counter (8 bytes, zeroed by the host before the launch), then [2][gridDim.x] partials (ping-pong).
    // Only the partials and the counter are shared between workgroups and all of them are touched with agent-scope
    // atomics, so no cache write-back / invalidate (a full fence) is needed: a workgroup's own records are its own.
    // Co-residency of the grid is guaranteed by the cooperative launch, so the spin cannot starve anyone.
    double *p = scratch + 1 + (size_t)(phase & 1) * gridDim.x;
    unsigned *cnt = reinterpret_cast<unsigned *>(scratch);
    double *timed_out = scratch + 1 + 2 * (size_t)gridDim.x;
    if (threadIdx.x == 0) {
        // Ordering: the partial is an agent-scope store, the arrival an agent-scope RELEASE add (the partial is visible to
        // whoever observes the count), the consumer side one ACQUIRE load after the spin (its later loads of the partials
        // cannot be satisfied from before the count was seen). The spin itself polls relaxed (an acquire per poll is 2-3x
        // slower per hop, MI355X_MICROARCH.md "Invalid forms").
        __hip_atomic_store(p + blockIdx.x, block_val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned target = (unsigned)(phase + 1) * gridDim.x;
        // Bounded spin: ~1 s of wall clock (s_memrealtime ticks at 100 MHz), and none at all once a previous phase has
        // timed out - every wavefront reaches an exit even if an arrival never shows up; the caller then sees NaN, never
        // takes the early exit and reports -1 Newton steps, which the host turns into an error.
        if (__hip_atomic_load(timed_out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0.0) {
            const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
            bool late = false;
            while (__hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
                __builtin_amdgcn_s_sleep(2);
                if (__builtin_amdgcn_s_memrealtime() - t0 > 100000000ull ||
                    __hip_atomic_load(timed_out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0.0) { late = true; break; }
            }
            if (late) __hip_atomic_store(timed_out, 1.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else (void)__hip_atomic_load(cnt, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    __builtin_amdgcn_s_barrier();   // one wavefront per workgroup: re-converges the lanes behind lane 0's spin
    if (__hip_atomic_load(timed_out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0.0) {
        ++phase;
        return __builtin_nan("");
    }
    double s = 0;
    for (unsigned i = threadIdx.x; i < gridDim.x; i += 64) s += __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
    for (int off = 32; off; off >>= 1) s += __shfl_xor(s, off, 64);
    ++phase;
    return s;
}
// An instance's term of the batch norm the Newton loop exits on (al_utils.py:552). One whose factorisation hit a
// non-positive pivot counts as +inf, so that the exit does not fire: the reference's norm holds the undefined residuals
// of such instances and ran the full 4 steps in both recorded batches (tests/test_failure_path.py).
template <typename real>
__device__ inline double exit_term(real r2, int info) { return info ? (double)INFINITY : (double)r2; }
__device__ inline bool grid_barrier_timed_out(const double *scratch) {
    return __hip_atomic_load(scratch + 1 + 2 * (size_t)gridDim.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0.0;
}
// one value per lane group (teams / quads: `leader` marks one lane per instance) -> the workgroup's sum, fixed order
__device__ inline double wave_sum_leaders(double v, bool leader) {
    double s = leader ? v : 0.0;
#pragma unroll
    for (int off = 32; off; off >>= 1) s += __shfl_xor(s, off, 64);
    return s;
}

template <typename real>
struct TraceArgs {
    real *g, *d, *phi, *phi_prev;
    int *k, *accept;
};

template <typename real>
struct StepArgs {
    int B, T;
    const real *z, *xnext, *F, *x0, *lam, *rho, *Qd, *q, *ulo, *uhi;
    long sb_u, st_u;
    real *d_out, *g_out, *factor;
    int *info;
    const real *obs;   // nullable [B][T][nobs][3]: obstacle centres (Obstacle_MPC)
    int nobs;
    real obs_r2;
    int no_init;       // state-estimator row set (AlqpObstacles.state_estimator)
};

// The one-step kernel with state box rows (k_newton_step_xbox): the bounds behind the plain arguments, in a type of its own
// like GenSolveArgs, so that StepArgs and k_newton_step stay what they were. obs / nobs / obs_r2 / no_init are unused (0).
template <typename real>
struct XboxStepArgs : StepArgs<real> {
    const real *xlo, *xhi;   // [nx] (sb_x = st_x = 0) or [B][T][nx] (sb_x = T nx, st_x = nx)
    long sb_x, st_x;
};

// The one-step kernel with general rows G_t z_t <= h_t (k_newton_step_rows<.., XBOX>): the rows behind XboxStepArgs, with
// GenSolveArgs' strides. The state bounds are read only by the XBOX instantiations (null otherwise).
template <typename real>
struct RowsStepArgs : XboxStepArgs<real> {
    const real *G, *h;   // G: [m][n] (sb_g = st_g = 0), [T][m][n] (0, m n) or [B][T][m][n] (T m n, m n); h likewise without [n]
    int m;               // rows per stage, 1 .. 64
    long sb_g, st_g;
    long sb_h, st_h;
};

// The one-step kernel with a dense stage cost (k_newton_step_dense<.., XBOX, POLY>): RowsStepArgs with C where Qd stood and
// without the obstacle fields, a type of its own. The state bounds are read only by the XBOX instantiations, the rows only
// by the POLY ones (null / m = 0 otherwise).
template <typename real>
struct DenseStepArgs {
    int B, T;
    const real *z, *xnext, *F, *x0, *lam, *rho, *C, *q, *ulo, *uhi;   // C: [B][T][n][n] row-major, symmetric
    long sb_u, st_u;
    const real *xlo, *xhi;
    long sb_x, st_x;
    const real *G, *h;
    int m;
    long sb_g, st_g;
    long sb_h, st_h;
    real *d_out, *g_out, *factor;
    int *info;
};

// DYN = false: the plain backward (alqp_backward_* with dyn = NULL), the kernel arguments it always had. DYN = true (a
// non-null AlqpBwdDyn) adds the gradients w.r.t. the affine dynamics and the initial state behind them, in a type of
// its own so that the plain kernels' argument block, and with it their code, stays what it was.
template <typename real, bool DYN = false>
struct BwdArgs {
    int B, T;
    const real *factor, *F, *rho, *z_final, *gbar;
    real *q_grad, *Qd_grad;
};
template <typename real>
struct BwdArgs<real, true> : BwdArgs<real, false> {
    const real *lam;       // the multipliers the solve returned; rows [0, (T-1) nx) of an instance are read
    long sb_lam;           // words from one instance's lam to the next
    real *dF, *dc, *dx0;   // nullable each: [B][T-1][nx][n], [B][T-1][nx], [B][nx]
};

// A VGPR zero the compiler cannot see through: keeps LDS addresses "divergent", so that
// wave-uniform operand reads stay 16-byte vector ds_reads instead of being scalarised.
__device__ inline unsigned opaque_zero() {
    unsigned z;
    asm volatile("v_mov_b32 %0, 0" : "=v"(z));
    return z;
}

}  // namespace alqp
