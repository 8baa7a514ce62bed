// alqp_quad.hpp - "quad" variant of the fused LinDx solve: FOUR lanes per QP instance,
// 16 instances per 64-lane wavefront (gfx950 / MI355X only).
//
// Why a second variant. In the team variant (alqp_team.hpp) the whole factor lives in
// LDS: traffic stays at the algorithmic minimum, but 20 KB of LDS per instance caps a
// CU at 8 instances and a 64-lane wave works on a 17-wide problem (lane utilisation
// ~10 %). Here the n x n blocks are small enough that FOUR lanes hold a stage's panel
// entirely in registers (rows dealt cyclically, row i on lane i % 4) and every
// cross-lane operand is a DPP quad broadcast (a VALU operand modifier, no LDS, no
// v_readlane): ~6x fewer wave instructions per solve. The price: the per-stage factor
// and the step vectors are streamed through an HBM workspace, written in the forward
// sweep and read back in the backward sweep. MI355X's 8 TB/s HBM is otherwise idle on this
// problem, so spending bandwidth to buy lane utilisation is the right trade once the batch
// fills the chip (B >= 4096; below that the team variant has the lower latency).
//
// Workspace record of one (instance, stage) (QCfg): the unscaled root-free factor
// (Hh[k][j] = Lh[k][j] p_j, 1/p_j on the diagonal), y/d, r, s, and the stage's slice of
// z, lam, diag Q, q, c and the bounds: everything a sweep needs apart from F_t sits in a
// few whole 128-byte lines. stage_in() copies the slices in, iter_end() copies z, lam out.
// The n- and nx-vectors of a record are stored LANE-MAJOR (element k = 4m + q at word q*SY + m):
// the elements a lane owns are contiguous, so one 16-byte access (+ one word) moves them instead
// of one word per instruction - the CU's vector-memory pipeline, shared by its four wavefronts,
// is what this kernel queues on (profiles/r02/experiments/README.md).
//
// One Newton step = forward sweep (applies the pending line-search step, residual,
// gradient, H_tt, right-looking LDL' panel, Schur complement for the next stage) +
// backward sweep (substitutions, s_t = (J d)_t, and in fp32 the merits of the 20
// line-search candidates accumulated on the fly). One AL iteration ends with iter_end():
// apply, dual update, next starting merit, ||r+||^2, copy-out in ONE pass.
// With a dynamics model compiled in (alqp_dyn.hpp) the same sweeps run on linearisations
// made on the device (linearize) and the line search / dual update use the true dynamics
// (merit_nonlin, iter_end<Dyn>): the nonlinear MPC solve in one launch.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "alqp_team.hpp"  // fma_, rsqrt_, fmax_, fabs_, pad4
#include "alqp_dyn.hpp"   // inlinable dynamics models (nonlinear fused solve)

namespace alqp {

// ---- quad-level cross-lane primitives (DPP quad_perm) ------------------------------
template <int Q>
__device__ inline float qb(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), Q * 0x55, 0xF, 0xF, true));
}
template <int Q>
__device__ inline double qb(double v) {
    long long b = __builtin_bit_cast(long long, v);
    int lo = __builtin_amdgcn_mov_dpp((int)(b & 0xffffffffll), Q * 0x55, 0xF, 0xF, true);
    int hi = __builtin_amdgcn_mov_dpp((int)(b >> 32), Q * 0x55, 0xF, 0xF, true);
    return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned int)lo);
}
// broadcast from quad lane `src`; src is a compile-time constant after unrolling, the switch
// folds away (the builtin needs a literal control word at each call site)
template <typename real>
__device__ inline real qbv(real v, int src) {
    switch (src & 3) {
        case 0: return qb<0>(v);
        case 1: return qb<1>(v);
        case 2: return qb<2>(v);
        default: return qb<3>(v);
    }
}
template <int CTRL>
__device__ inline float qperm(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
template <int CTRL>
__device__ inline double qperm(double v) {
    long long b = __builtin_bit_cast(long long, v);
    int lo = __builtin_amdgcn_mov_dpp((int)(b & 0xffffffffll), CTRL, 0xF, 0xF, true);
    int hi = __builtin_amdgcn_mov_dpp((int)(b >> 32), CTRL, 0xF, 0xF, true);
    return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned int)lo);
}
// all-reduce over the 4 lanes of a quad
template <typename real>
__device__ inline real qsum(real v) {
    v += qperm<0xB1>(v);  // quad_perm [1,0,3,2]
    v += qperm<0x4E>(v);  // quad_perm [2,3,0,1]
    return v;
}
__device__ inline int qor(int v) {
    v |= __builtin_amdgcn_mov_dpp(v, 0xB1, 0xF, 0xF, true);
    v |= __builtin_amdgcn_mov_dpp(v, 0x4E, 0xF, 0xF, true);
    return v;
}
// element q of (a0,a1,a2,a3), q = lane within the quad
template <typename real>
__device__ inline real sel4(real a0, real a1, real a2, real a3, int q) {
    real lo = (q & 1) ? a1 : a0, hi = (q & 1) ? a3 : a2;
    return (q & 2) ? hi : lo;
}

// ---- 4-byte-aligned vector access to global memory ----------------------------------
struct __attribute__((packed, aligned(4))) f4u { float x, y, z, w; };
struct __attribute__((packed, aligned(8))) d4u { double x, y, z, w; };
__device__ inline void gld4(const float *p, float &a, float &b, float &c, float &d) {
    f4u t = *reinterpret_cast<const f4u *>(p);
    a = t.x; b = t.y; c = t.z; d = t.w;
}
__device__ inline void gld4(const double *p, double &a, double &b, double &c, double &d) {
    d4u t = *reinterpret_cast<const d4u *>(p);
    a = t.x; b = t.y; c = t.z; d = t.w;
}
__device__ inline void gst4(float *p, float a, float b, float c, float d) {
    f4u t; t.x = a; t.y = b; t.z = c; t.w = d;
    *reinterpret_cast<f4u *>(p) = t;
}
__device__ inline void gst4(double *p, double a, double b, double c, double d) {
    d4u t; t.x = a; t.y = b; t.z = c; t.w = d;
    *reinterpret_cast<d4u *>(p) = t;
}
// ---- 16-byte-aligned access to LDS (fp32: one ds_read_b128 / ds_write_b128). The pointers carry the address space:
// a generic pointer that is LDS in one branch and global memory in the other becomes flat accesses word by word.
#define ALQP_LDS __attribute__((address_space(3)))
template <typename real>
__device__ inline void lld4(const ALQP_LDS real *p, real &a, real &b, real &c, real &d) {
    typedef real v4 __attribute__((ext_vector_type(4)));
    const v4 t = *(const ALQP_LDS v4 *)p;
    a = t.x; b = t.y; c = t.z; d = t.w;
}
template <typename real>
__device__ inline void lst4(ALQP_LDS real *p, real a, real b, real c, real d) {
    typedef real v4 __attribute__((ext_vector_type(4)));
    v4 t; t.x = a; t.y = b; t.z = c; t.w = d;
    *(ALQP_LDS v4 *)p = t;
}
// LEN contiguous reals into a register array (static indices only)
template <int LEN, typename real>
__device__ inline void gload(const real *p, real (&dst)[LEN]) {
#pragma unroll
    for (int c = 0; c + 4 <= LEN; c += 4) gld4(p + c, dst[c], dst[c + 1], dst[c + 2], dst[c + 3]);
#pragma unroll
    for (int c = (LEN / 4) * 4; c < LEN; ++c) dst[c] = p[c];
}

// ---- the nx rows of (-rho) F_t a lane works on during a stage: W[s][k], s < SW, k < N -------------
// fp32: registers. fp64 (ALQP_W_LDS): LDS, one 64-lane column per word ((s*N + k)*64 + lane: every
// access is a conflict-free ds_read/write_b64) - the quad kernels use no LDS otherwise, and in fp64
// these 2*SW*N dwords per lane are what pushed 872 B per lane into scratch (14 GB of HBM traffic per
// headline launch). 4 x 17 x 64 x 8 B = 34 KB per wavefront, four wavefronts per CU.
#ifndef ALQP_W_LDS
#define ALQP_W_LDS 1
#endif
// Byte-diet upper bounds (round 3, profiles/r03/experiments/README.md): builds with one of these set drop the named
// memory accesses WITHOUT replacing what they deliver - results are invalid, the launch time says what the real
// change could gain at most. Never set in the product build.
#ifndef ALQP_EXP_NOQ
#define ALQP_EXP_NOQ 0     // diag Q neither copied into the record nor read back (uniform-Q-in-SGPRs bound)
#endif
#ifndef ALQP_EXP_NORS
#define ALQP_EXP_NORS 0    // r and s neither stored nor re-read (recompute-instead-of-store bound)
#endif
#ifndef ALQP_EXP_NOL
#define ALQP_EXP_NOL 0     // factor of the last ALQP_EXP_NOL stages neither stored nor re-read (LDS turn-around bound)
#endif
template <typename real, int SW, int N, bool IN_LDS>
struct WPanel {
    real a[SW][N];
    __device__ __forceinline__ real (&operator[](int s))[N] { return a[s]; }
    __device__ __forceinline__ const real (&operator[](int s) const)[N] { return a[s]; }
};
template <typename real, int N>
struct WRowLds {
    real *p;
    __device__ __forceinline__ real &operator[](int k) const { return p[k * 64]; }
};
template <typename real, int SW, int N>
struct WPanel<real, SW, N, true> {
    real *base;  // LDS, already offset by the lane
    __device__ __forceinline__ WRowLds<real, N> operator[](int s) const { return WRowLds<real, N>{base + s * N * 64}; }
};
template <int LEN, typename real>
__device__ __forceinline__ void gload(const real *p, WRowLds<real, LEN> row) {
    real tmp[LEN];
    gload<LEN>(p, tmp);
#pragma unroll
    for (int k = 0; k < LEN; ++k) row[k] = tmp[k];
}

// "no dynamics model": the affine (LinDx) solve reads F and c from the caller's arrays
struct NoDyn {
    static constexpr int ID = 0;
};

// a vector field of a workspace record (QCfg): word offsets of its head and its tail; `record pointer + field` names
// the field of that record for the ld_* / st_* accessors of Quad
struct Fld {
    int h, t;
};
// the fields of QCfg carry their offsets in the type (a static constexpr object of class type is read from memory at
// run time in device code)
template <int H, int T>
struct FldT {
    static constexpr int h = H, t = T;
    __host__ __device__ constexpr operator Fld() const { return {H, T}; }
};
template <typename real>
struct FRef {
    real *p;
    Fld f;
};
template <typename real, int H, int T>
__device__ __forceinline__ FRef<std::remove_const_t<real>> operator+(real *p, FldT<H, T>) {
    return {const_cast<std::remove_const_t<real> *>(p), Fld{H, T}};
}

template <typename real, int NX_, int NU_>
struct QCfg {
    static constexpr int NX = NX_, NU = NU_, N = NX_ + NU_;
    static constexpr int SH = (N + 3) / 4;   // slots of H rows per lane (row 4s+q)
    static constexpr int SW = (NX + 3) / 4;  // slots of W / F rows per lane
    static constexpr int SY = SH;            // own elements of an n-vector (k = 4m+q)
    static constexpr int HT = 2 * SH * (SH + 1);  // registers of the trimmed H panel: slot s has 4(s+1) columns
    __host__ __device__ static constexpr int hidx(int s, int j) { return 2 * s * (s + 1) + j; }
    static constexpr int ST = 2 * SW * (SW + 1);  // same trimming for the Schur accumulator
    // ---- record layout. Words are placed in 16-word groups (64 bytes in fp32): every per-lane access of a sweep is
    // one 4-word chunk of a group, or single words of one group, at the group's start + a lane offset.
    // Wave-interleaved records (fp32, IL = 2): the records of instances 2i and 2i+1 at the same stage alternate in
    // 64-byte blocks (group g of instance 2i + h at word 32 g + 16 h of the pair's 2 RECW words), so the quad of one
    // instance and the quad of its partner fill whole 128-byte lines with one memory instruction where the
    // per-instance layout touched 16 half lines. fp64 (IL = 1) keeps one record after the other: a quad's 4 x 32
    // bytes already fill a line.
    static constexpr int BLK = 64 / (int)sizeof(real);      // reals of a 64-byte block
#ifndef ALQP_REC_IL_F32
#define ALQP_REC_IL_F32 2
#endif
    static constexpr int IL = sizeof(real) == 4 ? ALQP_REC_IL_F32 : 1;     // instances interleaved
    static_assert(IL == 1 || BLK == 16, "groups of 16 words are 64-byte blocks");
    // logical record word x -> word offset from the instance's record start (rec_base + t * RSTR)
    __host__ __device__ static constexpr int w(int x) { return (x / 16) * (16 * IL) + x % 16; }
    // L: slot s is s+1 chunks of 4 words per lane, the lanes of a quad interleaved (64 contiguous bytes per chunk);
    // in the last slot only the NLAST lanes that own a real row store anything (3 lanes: chunk stride 16, so
    // that no chunk crosses a group)
    static constexpr int NLAST = N - 4 * (SH - 1);                       // valid rows of the last slot (1..4)
    __host__ __device__ static constexpr int lanes_of(int s) { return s == SH - 1 ? NLAST : 4; }
    __host__ __device__ static constexpr int lstride(int s) { return lanes_of(s) == 3 ? 16 : 4 * lanes_of(s); }
    __host__ __device__ static constexpr int lbase(int s) {             // word offset of slot s
        int o = 0;
        for (int i = 0; i < s; ++i) o += (i + 1) * lstride(i);
        return o;
    }
    static constexpr int LW = lbase(SH);
    // fp32: the starting merit comes out of the first forward sweep; fp64 is short of registers
    // (it would spill 0.7 KB more) and keeps the residual pre-pass + a merit pass
    static constexpr bool PHI0_FWD = sizeof(real) == 4;   // (fp64, tried again with the W panel in LDS: 520 B of scratch come back)
#ifndef ALQP_S_AFTER_F32
#define ALQP_S_AFTER_F32 0   // experiment: 1 gives fp32 256 + 256 registers and 144 B of scratch (profiles/r02/experiments)
#endif
    static constexpr bool S_AFTER = sizeof(real) == 8 || ALQP_S_AFTER_F32;  // fp64: Schur accumulation after the panel (register pressure)
#ifndef ALQP_W_LDS_F32
#define ALQP_W_LDS_F32 0
#endif
    static constexpr bool W_LDS = ALQP_W_LDS && (sizeof(real) == 8 || ALQP_W_LDS_F32);   // the W rows live in LDS (WPanel)
    static constexpr int WLDS_WORDS = W_LDS ? SW * N * 64 : 1;          // reals of LDS per wavefront
    // the panel's multipliers are scaled by -1/p_j on the lane that owns the row, before the quad broadcast
    // (Quad::forward); -DALQP_PANEL_OWNER_SCALE=0 compiles the broadcast-then-multiply source (A/B builds)
#ifndef ALQP_PANEL_OWNER_SCALE
#define ALQP_PANEL_OWNER_SCALE 1
#endif
#ifndef ALQP_PANEL_OWNER_SCALE_F64
#define ALQP_PANEL_OWNER_SCALE_F64 ALQP_PANEL_OWNER_SCALE
#endif
    static constexpr bool OWNER_SCALE = sizeof(real) == 8 ? ALQP_PANEL_OWNER_SCALE_F64 : ALQP_PANEL_OWNER_SCALE;
    // ---- the factor of the first KL stages in LDS (fp32, fused solve only: Quad::forward / backward with FL). Between
    // the forward and the backward sweep's visit of stage t the chip moves (T - 1 - t) stages' worth of records, so
    // the factors of the first stages are the ones that go out to HBM and come back; the wavefront's LDS (one
    // wavefront per SIMD: a quarter of the CU's 160 KB) is otherwise unused in fp32. One chunk (slot s, c) of a
    // wavefront's 16 instances is lane-contiguous, 16 bytes per lane that owns a row: 64 lanes in a full slot,
    // 16 * NLAST in the last one (quad-major, the quad's owning lanes side by side).
    __host__ __device__ static constexpr int fl_chunk(int s) { return 16 * 4 * lanes_of(s); }   // words of one chunk of slot s
    __host__ __device__ static constexpr int fl_base(int s) {                                   // word offset of slot s
        int o = 0;
        for (int i = 0; i < s; ++i) o += (i + 1) * fl_chunk(i);
        return o;
    }
    static constexpr int FLW = fl_base(SH);            // words of one stage's factor, 16 instances
    static constexpr int FL_BUDGET = 36 * 1024 / 4;    // words per wavefront: leaves the CU's four wavefronts resident
    // stages held: as many whole stages as fit, at most 8 (a short horizon then crosses the boundary at every size);
    // -DALQP_FACTOR_LDS_F32=k sets it, 0 gives the kernel without any of this
#ifndef ALQP_FACTOR_LDS_F32
#define ALQP_FACTOR_LDS_F32 -1
#endif
    // n = 18 (14,4) keeps every stage in the records: with the LDS stores in its forward sweep hipcc spills 156 B per
    // lane there (8 B without; two stages would fit)
    static constexpr int KL = (sizeof(real) != 4 || W_LDS) ? 0
                              : ALQP_FACTOR_LDS_F32 >= 0   ? ALQP_FACTOR_LDS_F32
                              : N > 17                     ? 0
                              : (FL_BUDGET / FLW < 8 ? FL_BUDGET / FLW : 8);
    static_assert(KL * FLW <= 40 * 1024 / 4, "four wavefronts' factor stages fit a CU's LDS");
    __host__ __device__ static constexpr int p4(int x) { return (x + 3) & ~3; }
    // The record also carries the stage's slice of every small per-stage array (working copies
    // of z and lam, copies of diag Q, q, c and the bounds): in their own arrays these are 52-68
    // byte pieces, each costing one or two 128-byte lines per touch; side by side in the record
    // the sweeps and the line search touch a few whole lines. stage_in()/stage_out() copy them.
    //
    // Vector fields, lane-major: a field of S own slots per lane (S = SY for an n-vector, SW for an nx-vector, 4 for
    // the bound rows) is 4 S words. Slot m of lane q: for m < 4 (S / 4) in the HEAD, word 16 (m / 4) + 4 q + m % 4
    // (whole 16-word chunks, group-aligned: one 16-byte access per lane and chunk); the other S % 4 slots in the TAIL:
    // word t + 4 q + m - 4 (S / 4) of a tail group, where the tails of several fields share a group (field offsets t
    // within a lane's 4 words). Head and tail words of a lane are then the same lane offset (16 q bytes) from the
    // record's address: one address register pair per record. Padding words hold zeros.
    // Fields: y/d, z, r, s, lam (equality row block t), bound rows, diag Q, q, c. The heads of y and z come first, in
    // front of L: the sweeps read them from the NEXT stage's record too, and at the start of a record those reads stay
    // within the 4 KB immediate offset of the current stage's address (no second address register pair).
    static constexpr int NF = 9;
    __host__ __device__ static constexpr int fslots(int i) { return (i <= 1 || i == 6 || i == 7) ? SY : (i == 5 ? 4 : SW); }
    static constexpr int oL = 2 * 16 * (SY / 4);
    // the tail groups behind L (a field's tail slots never split over two groups); then the other heads
    __host__ __device__ static constexpr int tail_at(int i) {   // group start + the field's word within a lane's 4
        int g = (oL + LW + 15) & ~15, o = 0;
        for (int k = 0; k < NF; ++k) {
            const int r = fslots(k) % 4;
            if (r > 0 && o + r > 4) { g += 16; o = 0; }
            if (k == i) return g + o;
            o += r;
        }
        return o > 0 ? g + 16 : g;   // i == NF: end of the tail groups
    }
    __host__ __device__ static constexpr int head_at(int i) {
        if (i < 2) return i * 16 * (SY / 4);
        int o = tail_at(NF);
        for (int k = 2; k < i; ++k) o += 16 * (fslots(k) / 4);
        return o;
    }
    static constexpr FldT<head_at(0), tail_at(0)> oY{};    // y_t, later d_t (n)
    static constexpr FldT<head_at(1), tail_at(1)> oZ{};    // z_t (n)
    static constexpr FldT<head_at(2), tail_at(2)> oR{};    // r_t, eq residual of row block t (nx)
    static constexpr FldT<head_at(3), tail_at(3)> oS{};    // s_t = (J d)_eq (nx)
    static constexpr FldT<head_at(4), tail_at(4)> oLE{};   // lam, equality row block t (nx)
    // the bound rows of stage t: lane q's chunk = (lam_upper, lam_lower, u_upper, u_lower) of the ONE control lane q
    // owns (element NX + ju with (NX + ju) % 4 == q; zeros when it owns none)
    static_assert(NU <= 4, "the u-slot layout holds one control per lane");
    static constexpr FldT<head_at(5), tail_at(5)> oUS{};
    static constexpr FldT<head_at(6), tail_at(6)> oQ{};    // diag Q_t (n)
    static constexpr FldT<head_at(7), tail_at(7)> oq{};    // q_t (n)
    static constexpr FldT<head_at(8), tail_at(8)> oC{};    // c_t (nx)
    static constexpr int RECW = (head_at(NF) + 31) & ~31;  // whole 128-byte lines (fp32)
    static_assert(IL == 1 || RECW % 16 == 0, "whole groups per record");
    // position of slot m of lane q in a field read whole (ld_rep_*: head words, then tail words)
    template <int S>
    __host__ __device__ static constexpr int lp(int m, int q) {
        return m < 4 * (S / 4) ? 16 * (m / 4) + 4 * q + m % 4 : 16 * (S / 4) + q * (S % 4) + m - 4 * (S / 4);
    }
    // record word of position p of a field read whole (lp)
    template <int S>
    __host__ __device__ static constexpr int fw(Fld f, int p) {
        return p < 16 * (S / 4) ? w(f.h + p) : w(f.t + 4 * ((p - 16 * (S / 4)) / (S % 4)) + (p - 16 * (S / 4)) % (S % 4));
    }
    // element k of an n-vector field (k = 4m + q), row r of an nx-vector field
    __host__ __device__ static constexpr int pn(int k) { return lp<SY>(k >> 2, k & 3); }
    __host__ __device__ static constexpr int px(int r) { return lp<SW>(r >> 2, r & 3); }
    // word offset (from the record start, interleave included) of element k of n-vector field f
    __host__ __device__ static constexpr int wn(Fld f, int k) { return fw<SY>(f, pn(k)); }
    __host__ __device__ static constexpr int M(int T) { return T * NX + 2 * T * NU; }
    // ONE mapping from (instance, stage) to the workspace: every kernel addresses its records through rec_base()
    // (+ t * RSTR + w(word)), and the size the caller allocates is checked on the host against the highest word that
    // mapping can touch (ws_covers). Padding quads alias instance B - 1 (k_*_quad: `b = active ? b_raw : B - 1`); with
    // an odd B the last pair's second half is allocated and never touched.
    static constexpr int RSTR = RECW * IL;   // words from stage t to stage t + 1 of one instance
    __host__ __device__ static constexpr size_t rec_base(int b, int T) { return (size_t)(b / IL) * T * RSTR + (size_t)(b % IL) * 16; }
    __host__ __device__ static constexpr size_t ws_words(int B, int T) { return (size_t)((B + IL - 1) / IL) * T * RSTR; }
    __host__ static bool ws_covers(int B, int T) {
        return rec_base(B - 1, T) + (size_t)(T - 1) * RSTR + w(RECW - 1) + 1 <= ws_words(B, T);
    }
};

template <typename real, int NX, int NU>
struct Quad {
    using C = QCfg<real, NX, NU>;
    static constexpr int N = C::N, SH = C::SH, SW = C::SW, SY = C::SY, HT = C::HT, ST = C::ST, RECW = C::RECW;

    int q, T;
    bool active;
    const real *gQd, *gq, *gF, *gc, *gx0, *gulo, *guhi;
    long st_u;
#ifdef ALQP_SHDYN_UNIT
    int mt_F, mt_c;   // k_solve_lin_quad_shdyn only: masks on the stage stride of F / c, -1 per stage or 0 shared (ALQP_F_STAGE, ALQP_C_STAGE)
#endif
    real *gz, *glam, *rec;
    real rho;
    int info;
    real *wl;    // fp64: this lane's column of the W panel in LDS (WPanel), else unused
    using WT = WPanel<real, SW, N, C::W_LDS>;
    __device__ __forceinline__ WT wpanel() const {
        if constexpr (C::W_LDS) return WT{wl};
        else return WT{};
    }
    real *gFw;   // nonlinear fused solve: this instance's F_t linearisations (inside the workspace; gF points here too)
    real dyn_h;  //   step length of the dynamics model
    // caller-mode step kernel only (forward<EXT = true>): obstacle rows (Obstacle_MPC, al_utils.py:313-323, 351-388; as in
    // Team::forward_sweep) and the state-estimator variant's row set (al_utils_se.py:186-200, 300-310)
    const real *gobs;   // this instance's sphere centres [T][nobs][3] (global memory), nullptr without obstacles
    int nobs;
    real obs_r2;
    bool no_init;
    // fused solve, fp32 (QCfg::KL > 0; forward / backward with FL): the factor of the stages t < kl lives in the
    // wavefront's LDS, which starts at fl (one wavefront per block: lane = thread). kl = min(KL, T), or 0 under
    // ALQP_FACTOR_IN_WS; fl_ws: this forward sweep also stores those stages to the records (the launch's last Newton
    // step: the records a launch leaves behind hold every stage's factor)
    ALQP_LDS real *fl;
    int kl;
    bool fl_ws;
    // this stage's words of this lane (full chunks) and of this quad (last-slot chunks). The lane number is taken
    // afresh at every stage (two instructions, kept in the loop by `volatile`): an address register that lives through
    // the panel phase costs spills there (the kernel runs at 256 + 256 registers)
    __device__ __forceinline__ void fstage(int t, ALQP_LDS real *&pl, ALQP_LDS real *&pc) const {
        int lane;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane));
        pl = fl + t * C::FLW + 4 * lane;
        pc = fl + t * C::FLW + 4 * C::NLAST * (lane >> 2);
    }
    __device__ __forceinline__ ALQP_LDS real *fchunk(ALQP_LDS real *pl, ALQP_LDS real *pc, int s, int c, int ql) const {
        return (C::lanes_of(s) == 4 ? pl : pc + 4 * ql) + C::fl_base(s) + c * C::fl_chunk(s);
    }
    // the factor chunks of a stage between registers (H, trimmed panel) and the record / LDS
    __device__ __forceinline__ void st_factor_ws(real *rp, const real (&H)[HT]) const {
#pragma unroll
        for (int s = 0; s < SH; ++s)
#pragma unroll
            for (int c = 0; c <= s; ++c)
                if (C::lanes_of(s) == 4 || q < C::lanes_of(s))
                    gst4(lchunk(rp, s, c, q), H[C::hidx(s, 4 * c)],
                         H[C::hidx(s, 4 * c + 1)], H[C::hidx(s, 4 * c + 2)], H[C::hidx(s, 4 * c + 3)]);
    }
    __device__ __forceinline__ void st_factor_lds(int t, const real (&H)[HT]) const {
        ALQP_LDS real *pl, *pc;
        fstage(t, pl, pc);
#pragma unroll
        for (int s = 0; s < SH; ++s)
#pragma unroll
            for (int c = 0; c <= s; ++c)
                if (C::lanes_of(s) == 4 || q < C::lanes_of(s))
                    lst4<real>(fchunk(pl, pc, s, c, q), H[C::hidx(s, 4 * c)],
                         H[C::hidx(s, 4 * c + 1)], H[C::hidx(s, 4 * c + 2)], H[C::hidx(s, 4 * c + 3)]);
    }
    // lanes without a real row re-read lane 0's words (unconditional load, values unused)
    __device__ __forceinline__ void ld_factor_ws(real *rp, real (&H)[HT]) const {
#pragma unroll
        for (int s = 0; s < SH; ++s)
#pragma unroll
            for (int c = 0; c <= s; ++c) {
                const int ql = (C::lanes_of(s) == 4 || q < C::lanes_of(s)) ? q : 0;
                gld4(lchunk(rp, s, c, ql), H[C::hidx(s, 4 * c)],
                     H[C::hidx(s, 4 * c + 1)], H[C::hidx(s, 4 * c + 2)], H[C::hidx(s, 4 * c + 3)]);
            }
    }
    __device__ __forceinline__ void ld_factor_lds(int t, real (&H)[HT]) const {
        ALQP_LDS real *pl, *pc;
        fstage(t, pl, pc);
#pragma unroll
        for (int s = 0; s < SH; ++s)
#pragma unroll
            for (int c = 0; c <= s; ++c) {
                const int ql = (C::lanes_of(s) == 4 || q < C::lanes_of(s)) ? q : 0;
                lld4<real>(fchunk(pl, pc, s, c, ql), H[C::hidx(s, 4 * c)],
                     H[C::hidx(s, 4 * c + 1)], H[C::hidx(s, 4 * c + 2)], H[C::hidx(s, 4 * c + 3)]);
            }
    }

    __device__ __forceinline__ real uhi(int t, int j) const { return guhi[t * st_u + j]; }
    __device__ __forceinline__ real ulo(int t, int j) const { return gulo[t * st_u + j]; }
    __device__ __forceinline__ real *recp(int t) const { return rec + (size_t)t * C::RSTR; }
#ifdef ALQP_PHASE_TIMING
    // debug build only (tools/phase_timing.py): cycles per phase; a stamp drains the memory queue,
    // so "wait" buckets hold the exposed latency of the loads issued before them
    unsigned long long tacc[10], tlast;
    __device__ __forceinline__ void stamp(int bucket) {
        unsigned long long now;
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt vmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(now)::"memory");
        __builtin_amdgcn_sched_barrier(0);
        if (bucket >= 0) tacc[bucket] += now - tlast;
        tlast = now;
    }
#define ALQP_STAMP(b) stamp(b)
#else
#define ALQP_STAMP(b)
#endif

    // ---- lane-major vector fields of a record (QCfg: head chunks and tail; QCfg::pn / px) ----
    // own slots m < L of a field of S slots per lane: one 16-byte access per head chunk, single words in the tail
    template <int S, int L>
    __device__ __forceinline__ void ld_slots(FRef<real> f, real (&v)[L]) const {
        static_assert(L <= S, "slots of the field");
#pragma unroll
        for (int c = 0; 4 * c < L && c < S / 4; ++c) {
            const real *p = f.p + C::w(f.f.h + 16 * c) + 4 * q;
            if (4 * c + 3 < L) gld4(p, v[4 * c], v[4 * c + 1], v[4 * c + 2], v[4 * c + 3]);
            else
#pragma unroll
                for (int i = 0; 4 * c + i < L; ++i) v[4 * c + i] = p[i];
        }
        constexpr int H = 4 * (S / 4), R = S % 4;
        if constexpr (L > H) {
            const real *p = f.p + C::w(f.f.t) + 4 * q;
#pragma unroll
            for (int m = H; m < L; ++m) v[m] = p[m - H];
        }
    }
    // own slots L0 <= m < S of a field of S slots per lane into v[m]; v[m] for m < L0 is left alone. A head chunk that
    // holds slot L0 and slots in front of it is read whole (one 16-byte access) and only its slots >= L0 are taken.
    template <int S, int L0>
    __device__ __forceinline__ void ld_slots_from(FRef<real> f, real (&v)[S]) const {
        static_assert(L0 >= 0 && L0 <= S, "slots of the field");
#pragma unroll
        for (int c = L0 / 4; c < S / 4; ++c) {
            const real *p = f.p + C::w(f.f.h + 16 * c) + 4 * q;
            if (4 * c >= L0) gld4(p, v[4 * c], v[4 * c + 1], v[4 * c + 2], v[4 * c + 3]);
            else {
                real w[4];
                gld4(p, w[0], w[1], w[2], w[3]);
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (4 * c + i >= L0) v[4 * c + i] = w[i];
            }
        }
        constexpr int H = 4 * (S / 4);
        if constexpr (S > H) {
            const real *p = f.p + C::w(f.f.t) + 4 * q;
#pragma unroll
            for (int m = (L0 > H ? L0 : H); m < S; ++m) v[m] = p[m - H];
        }
    }
    template <int S>
    __device__ __forceinline__ void st_slots(FRef<real> f, const real (&v)[S]) const {
#pragma unroll
        for (int c = 0; c < S / 4; ++c) gst4(f.p + C::w(f.f.h + 16 * c) + 4 * q, v[4 * c], v[4 * c + 1], v[4 * c + 2], v[4 * c + 3]);
        constexpr int H = 4 * (S / 4), R = S % 4;
        if constexpr (R > 0) {
            real *p = f.p + C::w(f.f.t) + 4 * q;
#pragma unroll
            for (int m = H; m < S; ++m) p[m - H] = v[m];
        }
    }
    // the whole field (4 S words) into w[], positions QCfg::lp
    template <int S>
    __device__ __forceinline__ void ld_field(FRef<real> f, real (&w)[4 * S]) const {
        constexpr int H = 16 * (S / 4), R = S % 4;
#pragma unroll
        for (int c = 0; c < H; c += 4) gld4(f.p + C::w(f.f.h + c), w[c], w[c + 1], w[c + 2], w[c + 3]);
#pragma unroll
        for (int i = H; i < H + 4 * R; ++i) w[i] = f.p[C::template fw<S>(f.f, i)];
    }
    // own elements: k = 4m + q (m < SY) of an n-vector, rows r = 4s + q (s < SW) of an nx-vector;
    // slots without an element read / write the field's zero padding
    __device__ __forceinline__ void ld_own_n(FRef<real> f, real (&v)[SY]) const { ld_slots<SY, SY>(f, v); }
    __device__ __forceinline__ void ld_own_x(FRef<real> f, real (&v)[SW]) const { ld_slots<SW, SW>(f, v); }
    // x-part rows 4s + q of an n-vector (rows >= NX: whatever element 4s+q holds, finite)
    __device__ __forceinline__ void ld_ownx_of_n(FRef<real> f, real (&v)[SW]) const { ld_slots<SY, SW>(f, v); }
    template <int LEN>
    __device__ __forceinline__ void gstore(real *p, const real (&v)[LEN]) const {
#pragma unroll
        for (int c = 0; c + 4 <= LEN; c += 4) gst4(p + c, v[c], v[c + 1], v[c + 2], v[c + 3]);
#pragma unroll
        for (int c = (LEN / 4) * 4; c < LEN; ++c) p[c] = v[c];
    }
    __device__ __forceinline__ void st_own_n(FRef<real> f, const real (&v)[SY]) const { st_slots<SY>(f, v); }
    __device__ __forceinline__ void st_own_x(FRef<real> f, const real (&v)[SW]) const { st_slots<SW>(f, v); }
    // every lane gets the whole vector (the 4*SY / 4*SW words are read by all four lanes alike)
    __device__ __forceinline__ void ld_rep_n(FRef<real> f, real (&v)[N]) const {
        real w[4 * SY];
        ld_field<SY>(f, w);
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] = w[C::pn(k)];
    }
    __device__ __forceinline__ void ld_repx_of_n(FRef<real> f, real (&v)[NX]) const {   // x part of an n-vector
        real w[4 * SY];
        ld_field<SY>(f, w);
#pragma unroll
        for (int k = 0; k < NX; ++k) v[k] = w[C::pn(k)];
    }
    __device__ __forceinline__ void ld_rep_x(FRef<real> f, real (&v)[NX]) const {
        real w[4 * SW];
        ld_field<SW>(f, w);
#pragma unroll
        for (int r = 0; r < NX; ++r) v[r] = w[C::px(r)];
    }
    // slot c of L (QCfg::lbase) of this record, the chunk lane ql stores
    __device__ __forceinline__ real *lchunk(real *rp, int s, int c, int ql) const {
        return rp + C::w(C::oL + C::lbase(s) + c * C::lstride(s)) + 4 * ql;
    }
    // own elements out of a vector every lane holds (k = 4m + q; 0 where there is none)
    template <int LEN, int SL>
    __device__ __forceinline__ void own_of(const real (&full)[LEN], real (&v)[SL]) const {
#pragma unroll
        for (int m = 0; m < SL; ++m)
            v[m] = (4 * m < LEN) ? sel4(full[(4 * m < LEN) ? 4 * m : 0], (4 * m + 1 < LEN) ? full[(4 * m + 1 < LEN) ? 4 * m + 1 : 0] : real(0),
                                        (4 * m + 2 < LEN) ? full[(4 * m + 2 < LEN) ? 4 * m + 2 : 0] : real(0),
                                        (4 * m + 3 < LEN) ? full[(4 * m + 3 < LEN) ? 4 * m + 3 : 0] : real(0), q)
                                 : real(0);
    }
    // caller's contiguous array -> own elements (0 where there is none) and back
    template <int LEN, int SL>
    __device__ __forceinline__ void ld_own_ext(const real *src, real (&v)[SL]) const {
#pragma unroll
        for (int m = 0; m < SL; ++m) {
            const int k = 4 * m + q;
            const real x = src[(4 * m + 3 < LEN || k < LEN) ? k : LEN - 1];
            v[m] = (4 * m + 3 < LEN || k < LEN) ? x : real(0);
        }
    }
    template <int LEN, int SL>
    __device__ __forceinline__ void st_own_ext(real *dst, const real (&v)[SL]) const {
#pragma unroll
        for (int m = 0; m < SL; ++m)
            if (4 * m + 3 < LEN || 4 * m + q < LEN) dst[4 * m + q] = v[m];
    }

    // ---- bound rows (QCfg::oUS): the control this lane owns is ju = (q - NX) mod 4, if that is < NU
    __device__ __forceinline__ int own_ju() const { return (q - NX) & 3; }
    __device__ __forceinline__ void ld_own_us(const real *rp, real &lu, real &ll, real &bu, real &bl) const {
        gld4(rp + C::w(C::oUS.h) + 4 * q, lu, ll, bu, bl);
    }
    __device__ __forceinline__ void st_own_us(real *rp, real lu, real ll, real bu, real bl) const {
        gst4(rp + C::w(C::oUS.h) + 4 * q, lu, ll, bu, bl);
    }
    __device__ __forceinline__ void ld_rep_us(const real *rp, real (&lu)[NU], real (&ll)[NU], real (&bu)[NU], real (&bl)[NU]) const {
        real w[16];
        ld_field<4>(rp + C::oUS, w);
#pragma unroll
        for (int ju = 0; ju < NU; ++ju) {
            const int ql = (NX + ju) & 3;
            lu[ju] = w[4 * ql];
            ll[ju] = w[4 * ql + 1];
            bu[ju] = w[4 * ql + 2];
            bl[ju] = w[4 * ql + 3];
        }
    }

    // F_t rows of this lane: row 4s+q (zeros for rows >= NX). Loads are unconditional (row
    // index clamped, result masked) so that all of a stage's loads go out in one batch:
    // a load inside a divergent branch cannot be hoisted and costs its own round trip. That holds for a wave-uniform
    // branch too: the sweeps load F_{T-2} once more at the last stage, which has no dynamics rows, and discard it.
    // With the call under `dyn` hipcc splits the stage's loads into batches that wait for each other and spends ~100
    // more VALU instructions per stage on addresses (fp32 (13,4): +1.3 % launch time, 8 B more scratch in the
    // backward sweep; profiles/r22/README.md).
    __device__ __forceinline__ void load_F_rows(int t, WT &W) const {
        const real *Fg = gF + ALQP_F_STAGE(t);
#pragma unroll
        for (int s = 0; s < SW; ++s) {
            const int r = 4 * s + q;
            const int rc = (4 * s + 3 < NX) ? r : (r < NX ? r : NX - 1);
            gload<N>(Fg + rc * N, W[s]);
            if (4 * s + 3 >= NX) {
                const real m = r < NX ? real(1) : real(0);
#pragma unroll
                for (int k = 0; k < N; ++k) W[s][k] *= m;
            }
        }
    }
    // LEN contiguous words src -> dst, the quad's lanes taking 16-byte chunks in turn
    template <int LEN>
    __device__ __forceinline__ void copy_slice(const real *src, real *dst) const {
#pragma unroll
        for (int c = 0; 16 * c < LEN; ++c) {
            const int w0 = 16 * c + 4 * q;
            if (16 * c + 15 < LEN || w0 + 3 < LEN) {
                real a, b, cc, d;
                gld4(src + w0, a, b, cc, d);
                gst4(dst + w0, a, b, cc, d);
            } else {
#pragma unroll
                for (int w = 0; w < 4; ++w)
                    if (w0 + w < LEN) dst[w0 + w] = src[w0 + w];
            }
        }
    }
    // Kernel start: the stage's slice of z, lam, diag Q, q, c and the bounds -> its record, and
    // (when the launch starts with a merit evaluation or is a dual update only) the equality
    // residuals at the current z; a forward sweep recomputes them anyway.
    __device__ __forceinline__ void stage_in(bool with_residual, bool have_c = true) {
#pragma unroll 2
        for (int t = 0; t < T; ++t) {
            const bool dyn = t < T - 1;
            real *rp = recp(t);
            if (active) {
                real vn[SY], vx[SW];
                ld_own_ext<N>(gz + t * N, vn);
                st_own_n(rp + C::oZ, vn);
                ld_own_ext<N>(gQd + t * N, vn);
                st_own_n(rp + C::oQ, vn);
                ld_own_ext<N>(gq + t * N, vn);
                st_own_n(rp + C::oq, vn);
                ld_own_ext<NX>(glam + t * NX, vx);
                st_own_x(rp + C::oLE, vx);
                {
                    const int ju = own_ju(), jc = ju < NU ? ju : 0;
                    const real *lb = glam + T * NX + t * 2 * NU;
                    const real a0 = lb[jc], a1 = lb[NU + jc], a2 = guhi[t * st_u + jc], a3 = gulo[t * st_u + jc];
                    const bool has = ju < NU;
                    st_own_us(rp, has ? a0 : real(0), has ? a1 : real(0), has ? a2 : real(0), has ? a3 : real(0));
                }
                if (dyn && have_c) ld_own_ext<NX>(gc + ALQP_C_STAGE(t), vx);
                else {
#pragma unroll
                    for (int s = 0; s < SW; ++s) vx[s] = 0;
                }
                if (have_c) st_own_x(rp + C::oC, vx);
            }
            if (with_residual) {
                WT W = wpanel();
                real zt[N];
                load_F_rows(dyn ? t : (T > 1 ? T - 2 : 0), W);
                gload<N>(gz + t * N, zt);
                real rr[SW];
#pragma unroll
                for (int s = 0; s < SW; ++s) {
                    const int r = 4 * s + q;
                    rr[s] = 0;
                    if (4 * s + 3 < NX || r < NX) {
                        real xn = dyn ? gc[ALQP_C_STAGE(t) + r] : real(0);
#pragma unroll
                        for (int k = 0; k < N; ++k) xn = fma_(W[s][k], zt[k], xn);
                        // row block T-1 holds the initial-state rows x_0 - x_init (al_utils.py:274)
                        rr[s] = dyn ? gz[(t + 1) * N + r] - xn : gz[r] - gx0[r];
                    }
                }
                if (active) st_own_x(rp + C::oR, rr);
            }
        }
    }
    // Kernel end: the working copies of z and lam back to the caller's arrays.
    __device__ __forceinline__ void stage_out() {
        if (!active) return;
#pragma unroll 2
        for (int t = 0; t < T; ++t) {
            const real *rp = recp(t);
            real vn[SY], vx[SW];
            ld_own_n(rp + C::oZ, vn);
            st_own_ext<N>(gz + t * N, vn);
            ld_own_x(rp + C::oLE, vx);
            st_own_ext<NX>(glam + t * NX, vx);
            {
                real lu, ll, bu, bl;
                ld_own_us(rp, lu, ll, bu, bl);
                const int ju = own_ju();
                if (ju < NU) {
                    glam[T * NX + t * 2 * NU + ju] = lu;
                    glam[T * NX + t * 2 * NU + NU + ju] = ll;
                }
            }
        }
    }

    // ---- nonlinear fused solve (a dynamics model Dyn is inlined, alqp_dyn.hpp) -----------------
    // Linearisation pass of a Newton step (al_utils.py:233-248, dx_jac at the current iterate):
    // applies the pending line-search step, then per stage x+ = f(z_t) and J = df/dz by dual
    // numbers (the value in every lane, the n tangents split over the quad's four lanes),
    // F_t = J -> the workspace, c_t = f(z_t) - J z_t and r_t = x_{t+1} - f(z_t) -> the record. The
    // sweeps then run unchanged on (F_t, c_t).
    template <class Dyn>
    __device__ __forceinline__ void linearize(real alpha, bool pend) {
        static_assert(Dyn::NX == NX && Dyn::NU == NU, "model / kernel size mismatch");
        for (int t = 0; t < T; ++t) {
            const bool dyn = t < T - 1;
            real *rp = recp(t);
            const real *rn = recp(dyn ? t + 1 : t);
            real zt[N], dt[N], zn[SW], dn[SW];
            ld_rep_n(rp + C::oZ, zt);
            ld_rep_n(rp + C::oY, dt);
            ld_ownx_of_n(rn + C::oZ, zn);
            ld_ownx_of_n(rn + C::oY, dn);
            if (pend) {
#pragma unroll
                for (int k = 0; k < N; ++k) zt[k] = fma_(alpha, dt[k], zt[k]);
#pragma unroll
                for (int s = 0; s < SW; ++s) zn[s] = fma_(alpha, dn[s], zn[s]);
                if (active) {
                    real zo[SY];
                    own_of<N, SY>(zt, zo);
                    st_own_n(rp + C::oZ, zo);
                }
            }
            if (t == 0) {
                // initial-state rows x_0 - x_init live in row block T-1 (al_utils.py:274); a merit
                // evaluation may come before the first forward sweep rewrites them
                real r0[SW];
#pragma unroll
                for (int s = 0; s < SW; ++s) {
                    const int r = 4 * s + q;
                    const real z0r = sel4(zt[4 * s], (4 * s + 1 < NX) ? zt[(4 * s + 1 < NX) ? 4 * s + 1 : 0] : real(0),
                                          (4 * s + 2 < NX) ? zt[(4 * s + 2 < NX) ? 4 * s + 2 : 0] : real(0),
                                          (4 * s + 3 < NX) ? zt[(4 * s + 3 < NX) ? 4 * s + 3 : 0] : real(0), q);
                    r0[s] = (4 * s + 3 < NX || r < NX) ? z0r - gx0[(r < NX) ? r : NX - 1] : real(0);
                }
                if (active) st_own_x(recp(T - 1) + C::oR, r0);
            }
            if (dyn) {
                // the quad's lanes split the n tangents (lane q: columns 4i+q), then row 4s+q of J is
                // gathered: column k comes from lane k%4, the row index differs per destination lane
                constexpr int NTL = (N + 3) / 4;
                real xn[NX], Jl[NX][NTL];
                dyn_value_jac_split<Dyn, real>(zt, dyn_h, q, xn, Jl);
                real co[SW], ro[SW];
#pragma unroll
                for (int s = 0; s < SW; ++s) {
                    const int r = 4 * s + q;
                    real Jr[N];
#pragma unroll
                    for (int k = 0; k < N; ++k)
                        Jr[k] = sel4(qbv(Jl[4 * s][k >> 2], k),
                                     (4 * s + 1 < NX) ? qbv(Jl[(4 * s + 1 < NX) ? 4 * s + 1 : 0][k >> 2], k) : real(0),
                                     (4 * s + 2 < NX) ? qbv(Jl[(4 * s + 2 < NX) ? 4 * s + 2 : 0][k >> 2], k) : real(0),
                                     (4 * s + 3 < NX) ? qbv(Jl[(4 * s + 3 < NX) ? 4 * s + 3 : 0][k >> 2], k) : real(0), q);
                    const real xr = sel4(xn[4 * s], (4 * s + 1 < NX) ? xn[(4 * s + 1 < NX) ? 4 * s + 1 : 0] : real(0),
                                         (4 * s + 2 < NX) ? xn[(4 * s + 2 < NX) ? 4 * s + 2 : 0] : real(0),
                                         (4 * s + 3 < NX) ? xn[(4 * s + 3 < NX) ? 4 * s + 3 : 0] : real(0), q);
                    real c = xr;
#pragma unroll
                    for (int k = 0; k < N; ++k) c = fma_(-Jr[k], zt[k], c);
                    const bool okr = 4 * s + 3 < NX || r < NX;
                    if (okr && active) {
                        real *Fr = gFw + ((size_t)t * NX + r) * N;
#pragma unroll
                        for (int k = 0; k < N; ++k) Fr[k] = Jr[k];
                    }
                    co[s] = okr ? c : real(0);
                    ro[s] = okr ? zn[s] - xr : real(0);
                }
                if (active) {
                    st_own_x(rp + C::oC, co);
                    st_own_x(rp + C::oR, ro);
                }
            }
        }
    }
    // Merit of the 20 line-search candidates with the TRUE dynamics (al_utils.py:618-633): lane q of
    // the quad evaluates candidates k = 4i + q (i = 0..4) completely, then the values are exchanged.
    template <class Dyn>
    __device__ __forceinline__ void merit_nonlin(real (&phi)[20]) {
        real m[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) m[i] = 0;
        real x0v[NX], li[NX];
        gload<NX>(gx0, x0v);
        ld_rep_x(recp(T - 1) + C::oLE, li);
        const real a0 = sel4(real(1), real(0.5), real(0.25), real(0.125), q);
        for (int t = 0; t < T; ++t) {
            const bool dyn = t < T - 1;
            const real *rp = recp(t), *rn = recp(dyn ? t + 1 : t);
            real zt[N], dt[N], Qt[N], qt[N], zn[NX], dn[NX], le[NX], lu[NU], ll[NU], bu[NU], bl[NU];
            ld_rep_n(rp + C::oZ, zt);
            ld_rep_n(rp + C::oY, dt);
            ld_rep_n(rp + C::oQ, Qt);
            ld_rep_n(rp + C::oq, qt);
            ld_repx_of_n(rn + C::oZ, zn);
            ld_repx_of_n(rn + C::oY, dn);
            ld_rep_x(rp + C::oLE, le);
            ld_rep_us(rp, lu, ll, bu, bl);
            real alpha = a0;
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                real zc[N];
                real acc = 0;
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    zc[j] = fma_(alpha, dt[j], zt[j]);
                    acc = fma_(fma_(real(0.5) * Qt[j], zc[j], qt[j]), zc[j], acc);
                }
#pragma unroll
                for (int ju = 0; ju < NU; ++ju) {
                    const real vu = zc[NX + ju] - bu[ju], vl = bl[ju] - zc[NX + ju];
                    const real cu = fmax_(vu, real(0)), cl = fmax_(vl, real(0));
                    acc += fma_(lu[ju], vu, ll[ju] * vl) + real(0.5) * rho * fma_(cu, cu, cl * cl);
                }
                if (dyn) {
                    real xn[NX];
                    dyn_value<Dyn, real>(zc, dyn_h, xn);
#pragma unroll
                    for (int r = 0; r < NX; ++r) {
                        const real rr = fma_(alpha, dn[r], zn[r]) - xn[r];
                        acc = fma_(fma_(real(0.5) * rho, rr, le[r]), rr, acc);
                    }
                }
                if (t == 0) {
#pragma unroll
                    for (int r = 0; r < NX; ++r) {
                        const real rr = zc[r] - x0v[r];
                        acc = fma_(fma_(real(0.5) * rho, rr, li[r]), rr, acc);
                    }
                }
                m[i] += acc;
                alpha *= real(0.0625);
            }
        }
#pragma unroll
        for (int k = 0; k < 20; ++k) phi[k] = qbv(m[k >> 2], k);
    }

    // The panel's multiplier of row k at pivot j and the sign of the column operand that goes with it. OWNER_SCALE:
    // hs holds column j scaled by -1/p_j on the lanes that own its rows, the broadcast carries -l_kj and the updates
    // are fma(a, -l_kj, c). Otherwise l_kj = Hh[k][j] * (1/p_j) is formed behind the broadcast, on all four lanes,
    // and the updates are fma(-a, l_kj, c). The same operands reach every multiply and fma either way.
    template <int NHS>
    __device__ __forceinline__ static real panel_mult(const real (&H)[HT], const real (&hs)[NHS], real ip, int j, int k) {
        if constexpr (C::OWNER_SCALE) return qbv(hs[k >> 2], k);
        else return qbv(H[C::hidx(k >> 2, j)], k) * ip;
    }
    __device__ __forceinline__ static real pcol(real a) {
        if constexpr (C::OWNER_SCALE) return a;
        else return -a;
    }

    // ---- forward sweep: gradient, factorisation, forward substitution ------------------
    // With `pending`, the step alpha*d the previous line search chose (d is still in the
    // records) is applied on the fly: z_t is read, advanced, used and written back here, which
    // saves the separate pass (this sweep recomputes the equality residuals anyway).
    // With `phi0` the sweep also returns the merit at the z it linearises at (everything the
    // merit needs is in registers here): the starting merit of an AL iteration costs no pass of
    // its own and the launch needs no residual pre-pass.
    // EXT (one Newton direction for a caller-side line search, k_newton_step_quad): no record was filled - the
    // stage's vectors come straight from the caller's arrays (own elements, one word per instruction) and the
    // residual is z_{t+1}[x] - xnext_t with the caller's xnext = f(z_t) (gxn); nothing but the factor and y is
    // written. Saves the copy-in pass, the pass that formed c_t = xnext - F z (a third read of F) and the re-read.
    // FL (fused solve, QCfg::KL > 0): the factor of the stages t < kl goes to LDS (fchunk), and to the record as well
    // only under fl_ws
    template <bool EXT = false, bool FL = false>
    __device__ __forceinline__ void forward(real *g_out, real alpha, bool pending, real *phi0, const real *gxn = nullptr) {
        real mdist = 0;  // merit terms, per-lane parts (own elements and rows; summed over the quad at the end)
        real S[ST], Sy[SW];
        // carried from stage to stage, own rows / elements only (row 4s+q of block t-1 pins element 4s+q of x_t):
        // vpo = lam + rho r of the previous row block, Syo = (W y) of the previous stage
        real vpo[SW], Syo[SW];
        // own x-slots (m < SW) of z_t, pending step applied: stage t-1 needs them for its residual and hands them on,
        // so a stage reads only the slots m >= SW of its own z (and d) from the record. Not with EXT: the caller's
        // arrays are read element-wise and their x part is not a slot range of the n-vector.
        real zc[SW];
#pragma unroll
        for (int i = 0; i < ST; ++i) S[i] = 0;
#pragma unroll
        for (int s = 0; s < SW; ++s) Sy[s] = 0;
        // stage 0: x_0 is pinned by the initial-state rows (eq row block T-1), al_utils.py:274
        {
            real z0[SW], xi[SW], li[SW], r0[SW];
            if constexpr (EXT) {
                ld_own_ext<NX>(gz, z0);
                ld_own_ext<NX>(glam + (T - 1) * NX, li);
            } else {
                ld_ownx_of_n(recp(0) + C::oZ, z0);
                ld_own_x(recp(T - 1) + C::oLE, li);
            }
            ld_own_ext<NX>(gx0, xi);
            if (pending) {
                real d0[SW];
                ld_ownx_of_n(recp(0) + C::oY, d0);
#pragma unroll
                for (int s = 0; s < SW; ++s) z0[s] = fma_(alpha, d0[s], z0[s]);
            }
#pragma unroll
            for (int s = 0; s < SW; ++s) {
                bool valid = 4 * s + 3 < NX || 4 * s + q < NX;
                if constexpr (EXT) valid = valid && !no_init;   // state estimator: no initial-state rows
                const real r = valid ? z0[s] - xi[s] : real(0);
                vpo[s] = valid ? fma_(rho, r, li[s]) : real(0);
                if constexpr (C::PHI0_FWD) mdist += valid ? fma_(fma_(real(0.5) * rho, r, li[s]), r, real(0)) : real(0);  // initial-state rows
                Syo[s] = 0;
                r0[s] = r;
                zc[s] = z0[s];
            }
            if (!EXT && active) st_own_x(recp(T - 1) + C::oR, r0);
        }
        for (int t = 0; t < T; ++t) {
            const bool dyn = t < T - 1;
            WT W = wpanel();
            real Y[N];
            real dio[SY];   // diagonal of H_tt, own elements
            real v[SW];
            real zs[SY];
            real hob[3] = {0, 0, 0};   // obstacle rows (EXT): rho J_k'J_k entries (row q, columns 0..2) of the active rows
            real *rp = recp(t);
            // ---- loads (one batch) + residual + multiplier estimate. Everything per-stage is read as OWN
            // elements (one or two instructions per vector) and z_t is then broadcast inside the quad: loads
            // that return the same 80 bytes to all four lanes cost four times the L1 return bandwidth, which
            // is what the CU's four wavefronts queue on.
            {
                real zt[N];
                real Qo[SY], qo[SY];
                real cs[SW], zn[SW], lm[SW];
                real lu, ll, bu, bl;
                const int td = dyn ? t : (T > 1 ? T - 2 : 0);  // valid addresses for the last stage
                const real *rn = recp(td + 1);
                if constexpr (EXT) {
                    ld_own_ext<N>(gz + t * N, zs);
                    ld_own_ext<N>(gQd + t * N, Qo);
                    ld_own_ext<N>(gq + t * N, qo);
                    load_F_rows(td, W);
                    ld_own_ext<NX>(gxn + td * NX, cs);          // xnext_t = f(z_t): takes the place of F z + c
                    ld_own_ext<NX>(gz + (td + 1) * N, zn);
                    ld_own_ext<NX>(glam + td * NX, lm);
                    const int ju = own_ju(), jc = ju < NU ? ju : 0;
                    const real *lb = glam + T * NX + t * (2 * NU + nobs);   // obstacle rows sit behind the stage's bound rows
                    const bool has = ju < NU;
                    lu = has ? lb[jc] : real(0);
                    ll = has ? lb[NU + jc] : real(0);
                    bu = has ? guhi[t * st_u + jc] : real(0);
                    bl = has ? gulo[t * st_u + jc] : real(0);
                } else {
#pragma unroll
                    for (int s = 0; s < SW; ++s) zs[s] = zc[s];
                    ld_slots_from<SY, SW>(rp + C::oZ, zs);
                    if constexpr (ALQP_EXP_NOQ) { for (int m = 0; m < SY; ++m) Qo[m] = real(1); }
                    else ld_own_n(rp + C::oQ, Qo);
                    ld_own_n(rp + C::oq, qo);
                    load_F_rows(td, W);
                    ld_own_x(rp + C::oC, cs);
                    ld_ownx_of_n(rn + C::oZ, zn);
                    ld_own_x(rp + C::oLE, lm);
                    ld_own_us(rp, lu, ll, bu, bl);
                }
                if (pending) {  // wave-uniform: z_t += alpha d_t, z_{t+1}[x] += alpha d_{t+1}[x]
                    real dt[SY], dn[SW];
                    constexpr int M0 = EXT ? 0 : SW;   // the slots in front came advanced from the previous stage (zc)
                    ld_slots_from<SY, M0>(rp + C::oY, dt);
                    ld_ownx_of_n(rn + C::oY, dn);
#pragma unroll
                    for (int m = M0; m < SY; ++m) zs[m] = fma_(alpha, dt[m], zs[m]);   // written back with the stage results
#pragma unroll
                    for (int s = 0; s < SW; ++s) zn[s] = fma_(alpha, dn[s], zn[s]);
                }
#pragma unroll
                for (int s = 0; s < SW; ++s) zc[s] = zn[s];   // the next stage's zs[m < SW]: the same words, the same fma
                ALQP_STAMP(0);  // forward: exposed load latency
#pragma unroll
                for (int k = 0; k < N; ++k) zt[k] = qbv(zs[k >> 2], k);
                real rro[SW];
                if (!dyn) {
#pragma unroll
                    for (int s = 0; s < SW; ++s)
#pragma unroll
                        for (int k = 0; k < N; ++k) W[s][k] = 0;
                }
#pragma unroll
                for (int s = 0; s < SW; ++s) {
                    const int r = 4 * s + q;
                    real xn = cs[s];
                    if constexpr (!EXT) {
#pragma unroll
                        for (int k = 0; k < N; ++k) xn = fma_(W[s][k], zt[k], xn);
                    }
                    const real rr = zn[s] - xn;
                    const bool ok = dyn && r < NX;
                    v[s] = ok ? fma_(rho, rr, lm[s]) : real(0);
                    rro[s] = ok ? rr : real(0);
                    if constexpr (C::PHI0_FWD) mdist += ok ? fma_(fma_(real(0.5) * rho, rr, lm[s]), rr, real(0)) : real(0);
                }
                if (!ALQP_EXP_NORS && !EXT && dyn && active) st_own_x(rp + C::oR, rro);
                // ---- gradient and diagonal of H_tt, own elements (k = 4m + q)
                constexpr int MU0 = NX / 4;  // first element slot that can hold a control
                real zu = 0;                 // the control this lane owns (at most one: NU <= 4)
#pragma unroll
                for (int m = MU0; m < SY; ++m) zu = (4 * m + q >= NX && 4 * m + q < N) ? zs[m] : zu;
                const real vu = zu - bu, vl = bl - zu;
                const real au = vu >= 0 ? real(1) : real(0), al = vl >= 0 ? real(1) : real(0);
                const real cu = fmax_(vu, real(0)), cl = fmax_(vl, real(0));
                const real gu = fma_(rho, cu, lu) - fma_(rho, cl, ll);   // bound rows' part of the gradient on that control
                const real du = rho * (au + al);
                if constexpr (C::PHI0_FWD)
                    mdist += own_ju() < NU ? fma_(lu, vu, ll * vl) + real(0.5) * rho * fma_(cu, cu, cl * cl) : real(0);
                real go[SY];   // -(everything but the F'v term and the Schur carry), per own element
#pragma unroll
                for (int m = 0; m < SY; ++m) {
                    const int j = 4 * m + q;
                    const bool isx = (4 * m + 3 < NX) ? true : (4 * m >= NX ? false : j < NX);
                    const bool isu = (4 * m + 3 < NX) ? false : (j >= NX && j < N);
                    real g = fma_(Qo[m], zs[m], qo[m]);
                    real d = Qo[m];
                    if constexpr (C::PHI0_FWD) mdist = fma_(fma_(real(0.5) * Qo[m], zs[m], qo[m]), zs[m], mdist);   // padding: 0
                    g += isx ? vpo[m < SW ? m : 0] : (isu ? gu : real(0));
                    bool pinned = isx;
                    if constexpr (EXT) {
                        pinned = isx && !(no_init && t == 0);   // no E'E term on x_0 without initial-state rows
                        if (no_init && isu) g = 0;              // the given controls carry no gradient (al_utils_se.py:300-310)
                    }
                    d += pinned ? rho : (isu ? du : real(0));
                    dio[m] = d;
                    go[m] = g;
                }
                if constexpr (EXT && NX >= 3) {
                    if (nobs > 0) {
                        // J_k = -2 (p - o_k)' on x_t[0:3]: g += (lam_k + rho max(c_k, 0)) J_k', and for the rows with
                        // c_k >= 0 the Gauss-Newton term rho J_k'J_k on the position corner (al_utils.py:373-386, 113-120)
                        const real *lk = glam + T * NX + t * (2 * NU + nobs) + 2 * NU;
                        real gob = 0;
                        for (int k = 0; k < nobs; ++k) {
                            const real *o = gobs + (size_t)(t * nobs + k) * 3;
                            const real d0 = zt[0] - o[0], d1 = zt[1] - o[1], d2 = zt[2] - o[2];
                            const real ck = obs_r2 - fma_(d0, d0, fma_(d1, d1, d2 * d2));
                            const real dh = q == 0 ? d0 : (q == 1 ? d1 : d2);
                            gob = fma_(fma_(rho, ck > 0 ? ck : real(0), lk[k]), real(-2) * dh, gob);
                            if (ck >= 0) {
                                const real w4 = real(4) * rho * dh;
                                hob[0] = fma_(w4, d0, hob[0]); hob[1] = fma_(w4, d1, hob[1]); hob[2] = fma_(w4, d2, hob[2]);
                            }
                        }
                        go[0] += q < 3 ? gob : real(0);   // rows 0..2 of stage t are element slot 0 of lanes 0..2
                    }
                }
                // Y_j = -(g_j) - (W y)_{t-1,j}: broadcast of the own part plus the quad-reduced F'v term
#pragma unroll
                for (int m = 0; m < SY; ++m) {
                    const bool isx = (4 * m + 3 < NX) ? true : (4 * m >= NX ? false : 4 * m + q < NX);
                    go[m] = -go[m] - (isx ? Syo[m < SW ? m : 0] : real(0));
                }
                real fv[N];
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    real p = 0;
                    if (dyn) {
#pragma unroll
                        for (int s = 0; s < SW; ++s) p = fma_(W[s][j], v[s], p);
                        p = qsum(p);
                    }
                    fv[j] = p;
                    Y[j] = qbv(go[j >> 2], j) + p;
                }
                if (g_out) {   // trace only: g = -(Y + carry)
                    real fo[SY];
                    own_of<N, SY>(fv, fo);
#pragma unroll
                    for (int m = 0; m < SY; ++m) {
                        const bool isx = (4 * m + 3 < NX) ? true : (4 * m >= NX ? false : 4 * m + q < NX);
                        if (4 * m + 3 < N || 4 * m + q < N)
                            g_out[t * N + 4 * m + q] = -(go[m] + fo[m]) - (isx ? Syo[m < SW ? m : 0] : real(0));
                    }
                }
            }
            // ---- H_tt rows (lower part, trimmed): diag + (1/rho) w_i w_j - Schur
            real H[HT];
#pragma unroll
            for (int i = 0; i < HT; ++i) H[i] = 0;
#pragma unroll
            for (int s = 0; s < SH; ++s)
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (4 * s + c < N) H[C::hidx(s, 4 * s + c)] = (q == c) ? dio[s] : real(0);
            if constexpr (EXT && NX >= 3) {
                if (nobs > 0 && q < 3) {
#pragma unroll
                    for (int j = 0; j < 3; ++j) H[C::hidx(0, j)] += hob[j];
                }
            }
            // minus the Schur complement of stage t-1 (its registers are dead afterwards: keeps
            // the F'F phase below within the 256 architectural VGPRs)
            if (t > 0) {
#pragma unroll
                for (int s = 0; s < SW; ++s)
#pragma unroll
                    for (int b = 0; b < 4 * s + 4; ++b)
                        if (b < NX) H[C::hidx(s, b)] -= S[C::hidx(s, b)];
            }
#pragma unroll
            for (int i = 0; i < ST; ++i) S[i] = 0;
#pragma unroll
            for (int s = 0; s < SW; ++s) Sy[s] = 0;
            // W <- -rho F_t  (the F'F term is then (1/rho) W'W)
#pragma unroll
            for (int s = 0; s < SW; ++s)
#pragma unroll
                for (int k = 0; k < N; ++k) W[s][k] *= -rho;
            if (dyn) {
                const real irho = real(1) / rho;
#pragma unroll
                for (int r = 0; r < NX; ++r) {
                    real fr[N];
#pragma unroll
                    for (int j = 0; j < N; ++j) fr[j] = qbv(W[r >> 2][j], r);
#pragma unroll
                    for (int s = 0; s < SH; ++s) {
                        real fi = sel4(fr[4 * s], (4 * s + 1 < N) ? fr[(4 * s + 1 < N) ? 4 * s + 1 : 0] : real(0),
                                       (4 * s + 2 < N) ? fr[(4 * s + 2 < N) ? 4 * s + 2 : 0] : real(0),
                                       (4 * s + 3 < N) ? fr[(4 * s + 3 < N) ? 4 * s + 3 : 0] : real(0), q) * irho;
#pragma unroll
                        for (int j = 0; j < 4 * s + 4; ++j)
                            if (j < N) H[C::hidx(s, j)] = fma_(fi, fr[j], H[C::hidx(s, j)]);
                    }
                }
            }
            ALQP_STAMP(1);  // forward: residual, gradient, H assembly incl. F'F
            // ---- right-looking root-free panel factorisation: H = Lh D Lh' with D = diag(p_j) the
            // pivots and Lh unit lower. Column j is kept UNSCALED (Hh[k][j] = Lh[k][j] p_j) and
            // 1/p_j takes the pivot's place: no square root, no column scaling, and the solves
            // below use Hh[k][j] * (x_j / p_j).
            real ipv[C::S_AFTER ? N : 1];
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const real p = qbv(H[C::hidx(j >> 2, j)], j);
                if (!(p > 0) && info == 0) info = t * N + j + 1;
                // |p| (a free source modifier): on a non-positive pivot - rounding at rho*cond beyond the
                // dtype, flagged in info - the panel becomes a modified Cholesky (factor of H + E, E >= 0)
                // and the step stays a descent direction for the line search to judge; the reference's
                // half-finished cholesky_ex factor (al_utils.py:510-515) has nothing to restate
                const real ip = rcp_(fabs_(p));
                // The multiplier l_kj = Hh[k][j] / p_j, negated, is formed by the owner of row k BEFORE the quad
                // broadcast: 1/p_j is the same on every lane, so one multiply per slot of the column replaces one per
                // row k on all four lanes, and the broadcast carries the same 32 (64) bits the multiply behind it used
                // to make. Scaling by -1/p_j turns fma(-a, l, c) into fma(a, -l, c): the same product, the same
                // rounding, no sign flip to spend an instruction on. Words of hs above the diagonal and on row-less
                // lanes of the last slot are never the source lane of a broadcast and are not read otherwise.
                real hs[C::OWNER_SCALE ? SH : 1];
                if constexpr (C::OWNER_SCALE) {
                    const real nip = -ip;
#pragma unroll
                    for (int m = (j >> 2); m < SH; ++m) hs[m] = H[C::hidx(m, j)] * nip;
                }
                if constexpr (C::W_LDS) {
                    // W lives in LDS (fp64): its columns are read KB at a time, ALL reads of a group first, then the
                    // updates, then the writes. Element by element (read, 2-3 instructions, use, write - what hipcc makes
                    // of the plain loop below) every one of the 544 read-modify-writes of a stage exposes most of an LDS
                    // round trip to the one wavefront of the SIMD.
                    constexpr int KB = 8;
                    real wj[SW];
#pragma unroll
                    for (int s = 0; s < SW; ++s) wj[s] = W[s][j];
#pragma unroll
                    for (int k0 = j + 1; k0 < N; k0 += KB) {
                        real wv[KB][SW];
#pragma unroll
                        for (int kk = 0; kk < KB; ++kk)
#pragma unroll
                            for (int s = 0; s < SW; ++s)
                                if (k0 + kk < N) wv[kk][s] = W[s][k0 + kk];
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int kk = 0; kk < KB; ++kk) {
                            const int k = k0 + kk;
                            if (k < N) {
                                const real lkj = panel_mult(H, hs, ip, j, k);
#pragma unroll
                                for (int s = (k >> 2); s < SH; ++s) H[C::hidx(s, k)] = fma_(pcol(H[C::hidx(s, j)]), lkj, H[C::hidx(s, k)]);
#pragma unroll
                                for (int s = 0; s < SW; ++s) W[s][k] = fma_(pcol(wj[s]), lkj, wv[kk][s]);
                                Y[k] = fma_(pcol(Y[j]), lkj, Y[k]);
                            }
                        }
                    }
                } else {
#pragma unroll
                for (int k = j + 1; k < N; ++k) {
                    const real lkj = panel_mult(H, hs, ip, j, k);
#pragma unroll
                    for (int s = (k >> 2); s < SH; ++s) H[C::hidx(s, k)] = fma_(pcol(H[C::hidx(s, j)]), lkj, H[C::hidx(s, k)]);
#pragma unroll
                    for (int s = 0; s < SW; ++s) W[s][k] = fma_(pcol(W[s][j]), lkj, W[s][k]);
                    Y[k] = fma_(pcol(Y[j]), lkj, Y[k]);
                }
                }
                if constexpr (C::S_AFTER) ipv[j] = ip;
                if (!C::S_AFTER && dyn) {
                    real wsc[C::OWNER_SCALE ? SW : 1];   // W[b][j] / p_j on the owner of row b, as hs above
                    if constexpr (C::OWNER_SCALE) {
#pragma unroll
                        for (int s = 0; s < SW; ++s) wsc[s] = W[s][j] * ip;
                    }
#pragma unroll
                    for (int b = 0; b < NX; ++b) {
                        real wbj;
                        if constexpr (C::OWNER_SCALE) wbj = qbv(wsc[b >> 2], b);
                        else wbj = qbv(W[b >> 2][j], b) * ip;
#pragma unroll
                        for (int s = (b >> 2); s < SW; ++s) S[C::hidx(s, b)] = fma_(W[s][j], wbj, S[C::hidx(s, b)]);
                    }
                    const real yip = Y[j] * ip;
#pragma unroll
                    for (int s = 0; s < SW; ++s) Sy[s] = fma_(W[s][j], yip, Sy[s]);
                }
                H[C::hidx(j >> 2, j)] = (q == (j & 3)) ? ip : H[C::hidx(j >> 2, j)];
            }
            ALQP_STAMP(2);  // forward: panel
            // ---- stage results -> workspace (each lane its own words)
            if (active) {
                if constexpr (FL) {
                    if (t >= kl || fl_ws) st_factor_ws(rp, H);   // wave-uniform
                } else
                if (!(ALQP_EXP_NOL && t >= T - ALQP_EXP_NOL))
#pragma unroll
                for (int s = 0; s < SH; ++s)
#pragma unroll
                    for (int c = 0; c <= s; ++c)
                        if (C::lanes_of(s) == 4 || q < C::lanes_of(s))
                            gst4(lchunk(rp, s, c, q), H[C::hidx(s, 4 * c)],
                                 H[C::hidx(s, 4 * c + 1)], H[C::hidx(s, 4 * c + 2)], H[C::hidx(s, 4 * c + 3)]);
                real yo[SY];
                own_of<N, SY>(Y, yo);
                st_own_n(rp + C::oY, yo);
                if (pending) st_own_n(rp + C::oZ, zs);
            }
            if constexpr (FL) {
                // wave-uniform. Padding quads too: their backward sweep reads what they wrote, as it reads instance
                // B - 1's records. Behind the stores to the record: in front of them hipcc spills in the F'F phase
                // (16 B of scratch per lane, the launch 1 % slower than without any of this; profiles/r23/README.md)
                if (t < kl) st_factor_lds(t, H);
            }

            if constexpr (C::S_AFTER) {
                // fp64: the Schur complement of this stage once the factor's registers are free
                if (dyn) {
#pragma unroll
                    for (int j = 0; j < N; ++j) {
                        real wsc[C::OWNER_SCALE ? SW : 1];
                        if constexpr (C::OWNER_SCALE) {
#pragma unroll
                            for (int s = 0; s < SW; ++s) wsc[s] = W[s][j] * ipv[j];
                        }
#pragma unroll
                        for (int b = 0; b < NX; ++b) {
                            real wbj;
                            if constexpr (C::OWNER_SCALE) wbj = qbv(wsc[b >> 2], b);
                            else wbj = qbv(W[b >> 2][j], b) * ipv[j];
#pragma unroll
                            for (int s = (b >> 2); s < SW; ++s) S[C::hidx(s, b)] = fma_(W[s][j], wbj, S[C::hidx(s, b)]);
                        }
                        const real yip = Y[j] * ipv[j];
#pragma unroll
                        for (int s = 0; s < SW; ++s) Sy[s] = fma_(W[s][j], yip, Sy[s]);
                    }
                }
            }
            // ---- carry to the next stage (own rows): v = lam + rho r and W_t y_t
#pragma unroll
            for (int s = 0; s < SW; ++s) {
                vpo[s] = v[s];
                Syo[s] = Sy[s];
            }
            ALQP_STAMP(3);  // forward: stores drained
        }
        if constexpr (C::PHI0_FWD) { if (phi0) *phi0 = qsum(mdist); }
    }

    // ---- triangular solves with a stage's factor on OWN elements -------------------------
    // Lane q holds element 4m + q of an n-vector in slot m and row 4m + q of Hh in its own registers, so the owner of
    // a row updates it without fetching anything; one quad broadcast per step carries the finished element to the
    // other lanes. Lanes of slot m that may work at column j: lo <= q < hi. Rows on or above the diagonal of a 4 x 4
    // diagonal block hold whatever the forward sweep left there, and the lanes of the last slot without a row hold a
    // copy of lane 0's words: both are kept out with a select (a product with zero would let a NaN through).
    __host__ __device__ static constexpr int lane_lo(int m, int j) { return m == (j >> 2) ? (j & 3) + 1 : 0; }
    __device__ __forceinline__ bool in_lanes(int lo, int hi) const {
        return lo == 0 ? q < hi : (hi == 4 ? q >= lo : (q >= lo && q < hi));
    }
    // u <- Lh^{-1} u, column form (Lh[k][j] = Hh[k][j] / p_j, 1 / p_j on the diagonal): the owner of u_j scales it,
    // every row below takes its update. The same operations on the same operands as on replicated vectors.
    // PRECONDITION ON THE CALLER: in the last slot the lanes without a row (q >= NLAST) are not masked here; on return
    // u[SY - 1] of those lanes is arbitrary (accumulated from the copy of lane 0's words). A caller may read u only
    // through the owner of an element (qbv from lane k & 3, k < N) or must clear those lanes first, as solve_forward
    // does before its store; backward() feeds them only into ltsolve_own, which reads y through the owner.
    __device__ __forceinline__ void lsolve_own(const real (&H)[HT], real (&u)[SY]) const {
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const int mj = j >> 2;
            const real wj = qbv(u[mj] * H[C::hidx(mj, j)], j);
#pragma unroll
            for (int m = mj; m < SH; ++m) {
                const int lo = lane_lo(m, j);
                if (lo >= C::lanes_of(m)) continue;
                const real v = fma_(-H[C::hidx(m, j)], wj, u[m]);
                u[m] = lo == 0 ? v : (q >= lo ? v : u[m]);
            }
        }
    }
    // d <- Lh^{-T} D^{-1} y, dot form: d_i = (y_i - sum_{k>i} Hh[k][i] d_k) / p_i, every lane summing over its own rows
    // k > i; the owner finishes d_i and broadcasts it. d: own elements (0 where a lane has none), rep: the same vector
    // on every lane. Of y only the owner's copy of each element is read. (Other forms of this loop that were measured:
    // profiles/r08/README.md.)
    __device__ __forceinline__ void ltsolve_own(const real (&H)[HT], const real (&y)[SY], real (&d)[SY], real (&rep)[N]) const {
#pragma unroll
        for (int m = 0; m < SY; ++m) d[m] = 0;
#pragma unroll
        for (int i = N - 1; i >= 0; --i) {
            const int mi = i >> 2;
            real p = 0;
            bool any = false;
#pragma unroll
            for (int m = mi; m < SH; ++m) {
                const int lo = lane_lo(m, i), hi = C::lanes_of(m);
                if (lo >= hi) continue;
                const real h = (lo == 0 && hi == 4) ? H[C::hidx(m, i)] : (in_lanes(lo, hi) ? H[C::hidx(m, i)] : real(0));
                p = any ? fma_(h, d[m], p) : h * d[m];
                any = true;
            }
            real r = y[mi];
            if (any) r -= qsum(p);
            const real di = qbv(r * H[C::hidx(mi, i)], i);
            rep[i] = di;
            d[mi] = (q == (i & 3)) ? di : d[mi];
        }
    }

    // ---- backward sweep ---------------------------------------------------------------
    // LS: also accumulate the merit of the 20 line-search candidates z + 2^-k d while d_t and
    // s_t = (J d)_t are in registers (algebra: merit_candidates below; the sum runs over the
    // stages in sweep order T-1..0). The extra inputs sit in the record next to L and y.
    // d_ext (one Newton direction for the caller, k_newton_step_quad): d goes straight to the caller's array and
    // s = (J d)_eq, which only the fused line search reads, is not stored
    // store_s = false: s stays in registers, where the fused line search takes it from. Only iter_end() and
    // merit_candidates() read the record's s group, so a Newton step that another forward sweep follows need not
    // write it; k_backward_quad forms its s from F and w and does not rely on the group either.
    // FL: the factor of the stages t < kl is read from LDS, where this launch's forward<.., FL> left it
    template <bool LS, bool FL = false>
    __device__ __forceinline__ void backward(real (&phi)[20], real *d_ext = nullptr, bool store_s = true) {
        constexpr int MU0 = NX / 4;  // first element slot that can hold a control
        real c0 = 0, c1 = 0, c2 = 0;
        real acc[20];
        real rvT[SW], lvT[SW];
#pragma unroll
        for (int k = 0; k < 20; ++k) acc[k] = 0;
#pragma unroll
        for (int s = 0; s < SW; ++s) rvT[s] = lvT[s] = 0;
        real dxs[SW];   // own x rows of d_{t+1}, 0 where a lane has none
#pragma unroll
        for (int s = 0; s < SW; ++s) dxs[s] = 0;
        for (int t = T - 1; t >= 0; --t) {
            const bool dyn = t < T - 1;
            real *rp = recp(t);
            real H[HT];
            if constexpr (FL) {
                static_assert(!FL || !ALQP_EXP_NOL, "the no-factor experiment runs with the factor in the records");
                if (t < kl) ld_factor_lds(t, H);   // wave-uniform
                else ld_factor_ws(rp, H);
            } else
            if (ALQP_EXP_NOL && t >= T - ALQP_EXP_NOL) {
#pragma unroll
                for (int i = 0; i < HT; ++i) H[i] = real(1);
            } else
#pragma unroll
            for (int s = 0; s < SH; ++s)
#pragma unroll
                for (int c = 0; c <= s; ++c) {
                    // lanes without a real row re-read lane 0's words (unconditional load, values unused)
                    const int ql = (C::lanes_of(s) == 4 || q < C::lanes_of(s)) ? q : 0;
                    gld4(lchunk(rp, s, c, ql), H[C::hidx(s, 4 * c)],
                         H[C::hidx(s, 4 * c + 1)], H[C::hidx(s, 4 * c + 2)], H[C::hidx(s, 4 * c + 3)]);
                }
            real yo[SY];
            ld_own_n(rp + C::oY, yo);
            WT W = wpanel();
            load_F_rows(dyn ? t : (T > 1 ? T - 2 : 0), W);  // same batch as the record loads
            real zz[SY], QQ[SY], qq[SY], rv[SW], lv[SW];
            real lu = 0, ll = 0, bu = 0, bl = 0;
            if constexpr (LS) {
                ld_own_n(rp + C::oZ, zz);
                if constexpr (ALQP_EXP_NOQ) { for (int m = 0; m < SY; ++m) QQ[m] = real(1); }
                else ld_own_n(rp + C::oQ, QQ);
                ld_own_n(rp + C::oq, qq);
                ld_own_us(rp, lu, ll, bu, bl);
                if constexpr (ALQP_EXP_NORS) { for (int s = 0; s < SW; ++s) rv[s] = real(0); }
                else ld_own_x(rp + C::oR, rv);
                ld_own_x(rp + C::oLE, lv);
            }
            ALQP_STAMP(4);  // backward: exposed load latency
            if (dyn) {
                // v = F_t' dx_{t+1}
                real vv[N];
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    real p = 0;
#pragma unroll
                    for (int s = 0; s < SW; ++s) p = fma_(W[s][j], dxs[s], p);
                    vv[j] = qsum(p);
                }
                // u = Lh^{-1} v, rhs = y + rho u
                real uo[SY];
                own_of<N, SY>(vv, uo);
                lsolve_own(H, uo);
#pragma unroll
                for (int m = 0; m < SY; ++m) yo[m] = fma_(rho, uo[m], yo[m]);
            }
            // d = Lh^{-T} D^{-1} rhs: own elements for the stores, the line search and the next stage, Y on every lane
            // for s = dx_{t+1} - W d
            real down[SY], Y[N];
            ltsolve_own(H, yo, down, Y);
            if (active) {
                if (d_ext) st_own_ext<N>(d_ext + t * N, down);
                else st_own_n(rp + C::oY, down);
            }
            real sv[SW];
#pragma unroll
            for (int s = 0; s < SW; ++s) sv[s] = 0;
            if (dyn) {
#pragma unroll
                for (int s = 0; s < SW; ++s) {
                    const int r = 4 * s + q;
                    real p = 0;
#pragma unroll
                    for (int k = 0; k < N; ++k) p = fma_(W[s][k], Y[k], p);
                    sv[s] = (4 * s + 3 < NX || r < NX) ? dxs[s] - p : real(0);
                }
                if (!ALQP_EXP_NORS && active && !d_ext && store_s) st_own_x(rp + C::oS, sv);
            }
            if constexpr (LS) {
                real zu = 0, du = 0;   // the control this lane owns (at most one: NU <= 4)
#pragma unroll
                for (int m = 0; m < SY; ++m) {
                    const int j = 4 * m + q;
                    const real ok = (4 * m + 3 < N || j < N) ? real(1) : real(0);
                    const real z = zz[m], d = down[m], Qv = QQ[m] * ok, qv = qq[m] * ok;
                    c0 = fma_(fma_(real(0.5) * Qv, z, qv), z, c0);
                    c1 = fma_(fma_(Qv, z, qv), d, c1);
                    c2 = fma_(real(0.5) * Qv * d, d, c2);
                    if (m >= MU0) {
                        const bool mine = j >= NX && j < N;
                        zu = mine ? z : zu;
                        du = mine ? d : du;
                    }
                }
                {
                    const real isu = own_ju() < NU ? real(1) : real(0);
                    real alpha = 1;
#pragma unroll
                    for (int k = 0; k < 20; ++k) {
                        real zk = fma_(alpha, du, zu);
                        real vu = zk - bu, vl = bl - zk;
                        real cu = fmax_(vu, real(0)), cl = fmax_(vl, real(0));
                        acc[k] = fma_(isu, fma_(lu, vu, ll * vl) + real(0.5) * rho * fma_(cu, cu, cl * cl), acc[k]);
                        alpha *= real(0.5);
                    }
                }
                if (dyn) {
#pragma unroll
                    for (int s = 0; s < SW; ++s) {
                        const int r = 4 * s + q;
                        const real ok = (4 * s + 3 < NX || r < NX) ? real(1) : real(0);
                        const real rr = rv[s] * ok, ss = sv[s] * ok, lm = lv[s] * ok;
                        c0 = fma_(fma_(real(0.5) * rho, rr, lm), rr, c0);
                        c1 = fma_(fma_(rho, rr, lm), ss, c1);
                        c2 = fma_(real(0.5) * rho * ss, ss, c2);
                    }
                } else {
                    // row block T-1 holds the initial-state rows; their s = d_0[x] comes last
#pragma unroll
                    for (int s = 0; s < SW; ++s) {
                        rvT[s] = rv[s];
                        lvT[s] = lv[s];
                    }
                }
            }
#pragma unroll
            for (int s = 0; s < SW; ++s) dxs[s] = (4 * s + 3 < NX || 4 * s + q < NX) ? down[s] : real(0);
            ALQP_STAMP(5);  // backward: solves + stores
        }
        // initial-state rows: s = d_0[x]
        if (active && !d_ext && store_s) st_own_x(recp(T - 1) + C::oS, dxs);
        if constexpr (LS) {
#pragma unroll
            for (int s = 0; s < SW; ++s) {
                const int r = 4 * s + q;
                const real ok = (4 * s + 3 < NX || r < NX) ? real(1) : real(0);
                const real rr = rvT[s] * ok, ss = dxs[s], lm = lvT[s] * ok;
                c0 = fma_(fma_(real(0.5) * rho, rr, lm), rr, c0);
                c1 = fma_(fma_(rho, rr, lm), ss, c1);
                c2 = fma_(real(0.5) * rho * ss, ss, c2);
            }
            c0 = qsum(c0);
            c1 = qsum(c1);
            c2 = qsum(c2);
            real alpha = 1;
#pragma unroll
            for (int k = 0; k < 20; ++k) {
                phi[k] = qsum(acc[k]) + fma_(alpha, fma_(alpha, c2, c1), c0);
                alpha *= real(0.5);
            }
        }
    }

    // ---- forward substitution only, with the factor of a previous solve still in the workspace:
    //      y_t = L_t^{-1} ( rhs_t + rho F_{t-1} L_{t-1}^{-T} y_{t-1} [x rows] ), rhs_t = -gbar_t.
    //      Used by the backward pass of the implicit layer (NewtonAL.backward, al_utils.py:578-615);
    //      leaves y_t in the record's y slot, where backward() picks it up.
    __device__ __forceinline__ void solve_forward(const real *gbar) {
        real e[N];
#pragma unroll
        for (int j = 0; j < N; ++j) e[j] = 0;
        for (int t = 0; t < T; ++t) {
            real *rp = recp(t);
            real H[HT];
#pragma unroll
            for (int s = 0; s < SH; ++s)
#pragma unroll
                for (int c = 0; c <= s; ++c) {
                    const int ql = (C::lanes_of(s) == 4 || q < C::lanes_of(s)) ? q : 0;
                    gld4(lchunk(rp, s, c, ql), H[C::hidx(s, 4 * c)],
                         H[C::hidx(s, 4 * c + 1)], H[C::hidx(s, 4 * c + 2)], H[C::hidx(s, 4 * c + 3)]);
                }
            real yo[SY];
            ld_own_ext<N, SY>(gbar + t * N, yo);
            WT W = wpanel();
            load_F_rows(t > 0 ? t - 1 : 0, W);
#pragma unroll
            for (int m = 0; m < SY; ++m) yo[m] = -yo[m];
            if (t > 0) {
                // the x rows take rho (F_{t-1} e)[row]: row 4s + q is this lane's own
#pragma unroll
                for (int s = 0; s < SW; ++s) {
                    real p = 0;
#pragma unroll
                    for (int k = 0; k < N; ++k) p = fma_(W[s][k], e[k], p);
                    yo[s] = (4 * s + 3 < NX || 4 * s + q < NX) ? fma_(rho, p, yo[s]) : yo[s];
                }
            }
            // u = Lh^{-1} rhs
            lsolve_own(H, yo);
            if constexpr (C::NLAST < 4) yo[SY - 1] = q < C::NLAST ? yo[SY - 1] : real(0);   // lsolve_own's precondition
            if (active) st_own_n(rp + C::oY, yo);
            // e = Lh^{-T} D^{-1} u for the coupling of the next stage
            real eo[SY];
            ltsolve_own(H, yo, eo, e);
        }
    }

    // ---- merit of K candidates (see Team::merit_candidates for the algebra) ---------------
    // All loads of a stage are unconditional (clamped indices, masked contributions) so they
    // leave in one batch.
    template <int K>
    __device__ __forceinline__ void merit_candidates(real (&phi)[K], bool at_z) {
        real c0 = 0, c1 = 0, c2 = 0;
        real acc[K];
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] = 0;
        constexpr int MU0 = NX / 4;  // first element slot that can hold a control
#pragma unroll 4
        for (int t = 0; t < T; ++t) {  // 4 stages of loads in flight per round trip
            const real *rp = recp(t);
            real zz[SY], dd[SY], QQ[SY], qq[SY];
            real rv[SW], sv[SW], lv[SW];
            real lu, ll, bu, bl;
            ld_own_n(rp + C::oZ, zz);
            ld_own_n(rp + C::oY, dd);
            if constexpr (ALQP_EXP_NOQ) { for (int m = 0; m < SY; ++m) QQ[m] = real(1); }
            else ld_own_n(rp + C::oQ, QQ);
            ld_own_n(rp + C::oq, qq);
            ld_own_us(rp, lu, ll, bu, bl);
            if constexpr (ALQP_EXP_NORS) { for (int s = 0; s < SW; ++s) rv[s] = sv[s] = real(0); }
            else { ld_own_x(rp + C::oR, rv); ld_own_x(rp + C::oS, sv); }
            ld_own_x(rp + C::oLE, lv);
            real zu = 0, du = 0;   // the control this lane owns (at most one: NU <= 4)
#pragma unroll
            for (int m = 0; m < SY; ++m) {
                const int j = 4 * m + q;
                const real ok = (4 * m + 3 < N || j < N) ? real(1) : real(0);
                const real z = zz[m], d = at_z ? real(0) : dd[m] * ok, Qv = QQ[m] * ok, qv = qq[m] * ok;
                c0 = fma_(fma_(real(0.5) * Qv, z, qv), z, c0);
                c1 = fma_(fma_(Qv, z, qv), d, c1);
                c2 = fma_(real(0.5) * Qv * d, d, c2);
                if (m >= MU0) {
                    const bool mine = j >= NX && j < N;
                    zu = mine ? z : zu;
                    du = mine ? d : du;
                }
            }
            {
                const real isu = own_ju() < NU ? real(1) : real(0);
                real alpha = 1;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    real zk = fma_(alpha, du, zu);
                    real vu = zk - bu, vl = bl - zk;
                    real cu = fmax_(vu, real(0)), cl = fmax_(vl, real(0));
                    acc[k] = fma_(isu, fma_(lu, vu, ll * vl) + real(0.5) * rho * fma_(cu, cu, cl * cl), acc[k]);
                    alpha *= real(0.5);
                }
            }
#pragma unroll
            for (int s = 0; s < SW; ++s) {
                const int r = 4 * s + q;
                const real ok = (4 * s + 3 < NX || r < NX) ? real(1) : real(0);
                const real rr = rv[s] * ok, ss = at_z ? real(0) : sv[s] * ok, lm = lv[s] * ok;
                c0 = fma_(fma_(real(0.5) * rho, rr, lm), rr, c0);
                c1 = fma_(fma_(rho, rr, lm), ss, c1);
                c2 = fma_(real(0.5) * rho * ss, ss, c2);
            }
        }
        c0 = qsum(c0);
        c1 = qsum(c1);
        c2 = qsum(c2);
        real alpha = 1;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            phi[k] = qsum(acc[k]) + fma_(alpha, fma_(alpha, c2, c1), c0);
            alpha *= real(0.5);
        }
    }

    // End of an AL iteration in ONE pass over the records (own elements only): apply the pending
    // step (z += alpha d, r += alpha s), the dual update lam <- lam + rho r, bound rows clamped
    // at 0, rho <- rho * scale (AL_mpc.py:315-317,325), the merit at the new (z, lam, rho) = the
    // next iteration's starting merit (same expression order as merit_candidates<1>(., true)),
    // ||r_+||^2 and the finiteness flag (al_utils.py:545-549); on the last iteration also the
    // copy-out of z and lam.
    // With a dynamics model (Dyn::ID != 0) the residuals are re-evaluated with the TRUE dynamics at
    // the new z (AL_mpc.py:315: the dual update never uses the linearisation).
    template <class Dyn = NoDyn>
    __device__ __forceinline__ void iter_end(real alpha, bool pend, bool dual, real rho_scale, bool write_out,
                                             real &phi_next, real &rn2, int &bad) {
        constexpr int MU0 = NX / 4;
        const real rho_n = dual ? rho * rho_scale : rho;
        if (!pend) alpha = 0;
        real c0 = 0, acc0 = 0, r2 = 0;
#pragma unroll 2
        for (int t = 0; t < T; ++t) {
            real *rp = recp(t);
            real zz[SY], dd[SY], QQ[SY], qq[SY];
            real rv[SW], sv[SW], lv[SW];
            real lu, ll, bu, bl;
            ld_own_n(rp + C::oZ, zz);
            ld_own_n(rp + C::oY, dd);
            if constexpr (ALQP_EXP_NOQ) { for (int m = 0; m < SY; ++m) QQ[m] = real(1); }
            else ld_own_n(rp + C::oQ, QQ);
            ld_own_n(rp + C::oq, qq);
            ld_own_us(rp, lu, ll, bu, bl);
            if constexpr (ALQP_EXP_NORS) { for (int s = 0; s < SW; ++s) rv[s] = sv[s] = real(0); }
            else { ld_own_x(rp + C::oR, rv); ld_own_x(rp + C::oS, sv); }
            ld_own_x(rp + C::oLE, lv);
            real rtrue[SW];
#pragma unroll
            for (int s = 0; s < SW; ++s) rtrue[s] = 0;
            if constexpr (Dyn::ID != 0) {
                if (t < T - 1) {
                    const real *rn_ = recp(t + 1);
                    real zr[N], dr[N], xn[NX];
                    ld_rep_n(rp + C::oZ, zr);
                    ld_rep_n(rp + C::oY, dr);
                    if (pend) {
#pragma unroll
                        for (int k = 0; k < N; ++k) zr[k] = fma_(alpha, dr[k], zr[k]);
                    }
                    dyn_value<Dyn, real>(zr, dyn_h, xn);
                    real zno[SW], dno[SW];
                    ld_ownx_of_n(rn_ + C::oZ, zno);
                    ld_ownx_of_n(rn_ + C::oY, dno);
#pragma unroll
                    for (int s = 0; s < SW; ++s) {
                        real znn = zno[s];
                        const real dnn = dno[s];
                        if (pend) znn = fma_(alpha, dnn, znn);
                        const real xr = sel4(xn[4 * s], (4 * s + 1 < NX) ? xn[(4 * s + 1 < NX) ? 4 * s + 1 : 0] : real(0),
                                             (4 * s + 2 < NX) ? xn[(4 * s + 2 < NX) ? 4 * s + 2 : 0] : real(0),
                                             (4 * s + 3 < NX) ? xn[(4 * s + 3 < NX) ? 4 * s + 3 : 0] : real(0), q);
                        rtrue[s] = znn - xr;
                    }
                }
            }
            real zu = 0;   // the control this lane owns (at most one: NU <= 4)
#pragma unroll
            for (int m = 0; m < SY; ++m) {
                const int j = 4 * m + q;
                const bool valid = 4 * m + 3 < N || j < N;
                const real ok = valid ? real(1) : real(0);
                const real z = valid ? (pend ? fma_(alpha, dd[m], zz[m]) : zz[m]) : real(0);
                const real Qv = QQ[m] * ok, qv = qq[m] * ok;
                if (valid) bad |= !(z - z == real(0));
                zz[m] = z;
                if (valid && active) {
                    if (write_out) gz[t * N + j] = z;
                }
                c0 = fma_(fma_(real(0.5) * Qv, z, qv), z, c0);
                if (m >= MU0) zu = (j >= NX && j < N) ? z : zu;
            }
            {
                const int ju = own_ju();
                const bool isub = ju < NU;
                const real isu = isub ? real(1) : real(0);
                const real vu = zu - bu, vl = bl - zu;
                real lun = lu, lln = ll;
                if (dual) {
                    const real a = fma_(rho, vu, lu), c = fma_(rho, vl, ll);
                    lun = a < 0 ? real(0) : a;
                    lln = c < 0 ? real(0) : c;
                }
                if (isub && active) {
                    if (dual) st_own_us(rp, lun, lln, bu, bl);
                    if (write_out) {
                        glam[T * NX + t * 2 * NU + ju] = lun;
                        glam[T * NX + t * 2 * NU + NU + ju] = lln;
                    }
                }
                const real cu = fmax_(vu, real(0)), cl = fmax_(vl, real(0));
                acc0 = fma_(isu, fma_(lun, vu, lln * vl) + real(0.5) * rho_n * fma_(cu, cu, cl * cl), acc0);
                r2 = fma_(isu, fma_(cu, cu, cl * cl), r2);
            }
            if (pend && active) st_own_n(rp + C::oZ, zz);
#pragma unroll
            for (int s = 0; s < SW; ++s) {
                const int r = 4 * s + q;
                const bool valid = 4 * s + 3 < NX || r < NX;
                const real ok = valid ? real(1) : real(0);
                real rn = pend ? fma_(alpha, sv[s], rv[s]) : rv[s];
                if constexpr (Dyn::ID != 0) {
                    if (t < T - 1) rn = rtrue[s];
                }
                if (!valid) rn = 0;
                const real ln = valid ? (dual ? fma_(rho, rn, lv[s]) : lv[s]) : real(0);
                rv[s] = rn;
                lv[s] = ln;
                if (valid && active) {
                    if (write_out) glam[t * NX + r] = ln;
                }
                const real rr = rn * ok, lm = ln * ok;
                c0 = fma_(fma_(real(0.5) * rho_n, rr, lm), rr, c0);
                r2 = fma_(rr, rr, r2);
            }
            if (active) {
                if (pend || Dyn::ID != 0) st_own_x(rp + C::oR, rv);
                if (dual) st_own_x(rp + C::oLE, lv);
            }
        }
        rho = rho_n;
        c0 = qsum(c0);
        phi_next = qsum(acc0) + c0;
        rn2 = qsum(r2);
        bad = qor(bad);
    }

    __device__ __forceinline__ real rplus2(int &bad) {
        real acc = 0;
        for (int t = 0; t < T; ++t) {
            const real *rp = recp(t);
            real ro[SW], zo[SY];
            real ulu, ull, ubu, ubl;
            ld_own_x(rp + C::oR, ro);
            ld_own_n(rp + C::oZ, zo);
            ld_own_us(rp, ulu, ull, ubu, ubl);
#pragma unroll
            for (int s = 0; s < SW; ++s) {
                const int r = 4 * s + q;
                if (r < NX) { real rr = ro[s]; acc = fma_(rr, rr, acc); }
            }
#pragma unroll
            for (int m = 0; m < SY; ++m) {
                const int j = 4 * m + q;
                if (j < N) {
                    real z = zo[m];
                    bad |= !(z - z == real(0));
                    if (j >= NX) {
                        real cu = fmax_(z - ubu, real(0)), cl = fmax_(ubl - z, real(0));
                        acc += fma_(cu, cu, cl * cl);
                    }
                }
            }
        }
        bad = qor(bad);
        return qsum(acc);
    }
};

}  // namespace alqp
