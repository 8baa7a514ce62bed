"""Drop-in for the reference's ``qpth.AL_mpc`` module, MI355X-native.

``MPC`` keeps the surface the DEQ-MPC loop touches (callers are
``deqmpc/policies.py:1181-1216, 1236-1315`` of the reference):

  * ctor ``MPC(n_state, n_ctrl, T, u_lower, u_upper, ..., n_batch, dtype)``
    (qpth/AL_mpc.py:118-142; the kwargs the reference ignores are accepted and
    ignored here too),
  * ``__call__(x0, cost, dx, dx_jac, compute_Qq=None, u_init=None, x_init=None)
    -> (x[B,T,nx] f32, u[B,T,nu] f32, status)`` (qpth/AL_mpc.py:207-258),
  * ``reinitialize(x, mask)`` (must precede the first call, :569-579),
    ``warm_start_initialize(x, u, args)`` (:581-592),
  * attributes ``al_iter, x_init, u_init, lamda_prev, rho_prev`` and
    ``get_xu() / get_cost()`` (:560-567).

What runs where: this file is host logic only (state carry, dispatch, the
batch-global exit test that needs a host decision). All arithmetic of the AL
inner iteration - gradient, block-tridiagonal Cholesky, Newton step, 20-point
line search, dual update - is in the HIP kernels behind ``backend`` (csrc/).
There is no CPU path: without the built extension and a ROCm device it raises.

Two exit modes for the Newton loop:
  ``"reference"``  reproduces the reference's batch-global early exit
                   (al_utils.py:486,552,560-564): one kernel launch per Newton
                   step and a host read of sum_b |r+|^2 in between, exactly the
                   host syncs the reference has (its ``.item()`` calls);
  ``"fixed"``      always 4 Newton steps per AL iteration: the whole solve is one
                   kernel launch, no host sync, results do not depend on who else
                   is in the batch (so sharding the batch changes nothing).
"""
from __future__ import annotations

import math
import os
import sys

import torch
from torch.nn import Module

try:  # the package may be reached as top-level `qpth` (drop-in) or via the alias
    import deq_mpc_corl_amd  # noqa: F401
except ImportError:  # pragma: no cover
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    import deq_mpc_corl_amd  # noqa: F401

from deq_mpc_corl_amd import _lib as _abi
from deq_mpc_corl_amd.qpth import al_utils
from deq_mpc_corl_amd.qpth.al_utils import LinDx, QuadCost  # noqa: F401  (re-exported)

MAX_NEWTON = 4   # al_utils.py:485
N_LS = 20        # al_utils.py:619
RHO_SCALE = 10.0  # AL_mpc.py:325
SE_NO_BOUND = 1e20  # state estimator: |u| bound that is never active (rho_max * SE_NO_BOUND is finite in fp32)

# Two of diag_cost=False, x_lower / x_upper and ineqG / ineqh together need a backend with `solve_lin_gen` (the fused team
# kernel's combined instances); without it these are raised, in MPC.__init__ for a backend given
# there and in the guard block of the solve for the lazily resolved default
_NO_DENSE_XBOX = ("MPC: x_lower / x_upper with diag_cost=False: no kernel instance takes "
                  "both the dense cost and the state-bound rows")
_NO_DENSE_POLY = ("MPC: ineqG / ineqh with diag_cost=False: no kernel instance takes both the "
                  "dense cost and the general rows")
_NO_XBOX_POLY = ("MPC: ineqG / ineqh with x_lower / x_upper: no kernel instance takes both; write "
                 "the state box as rows of ineqG (G = [I 0; -I 0], h = [x_upper; -x_lower])")

# Models (fused_id) that take the one-launch route with state bounds / general rows BY DEFAULT: those whose median there is at
# or below the launch-per-step route's in every row of tools/bench_nonlin_rows.py. Every other compiled-in
# model takes it with prefer_fused=True only. Measured (profiles/r20/bench_nonlin_rows.jsonl): pendulum1l (1) and cartpole1l (2),
# 1.0-1.8 ms against 1.8-3.3 ms in every row; cartpole1l_v2 (4) was not timed.
ROWS_FUSED_DEFAULT_IDS = frozenset({1, 2})


def _detach_maybe(t):
    if t is None:
        return None
    return t.detach() if t.requires_grad else t


class _SolveState:
    """Everything the solve needs that autograd must not see."""

    __slots__ = ("mpc", "x0", "z", "lam", "rho", "dx", "dx_jac", "lin", "stream_mode",
                 "status_flag", "newton_per_al")


class _Launcher:
    """One solve's backend launches. The arguments every launch of the solve repeats are bound here once, so a call
    site states only what differs (al_iter, max_newton, flags, skip, newton_counts, workspace / variant). Also here:
    the backend's capabilities, each probed once with one default, and the scratch the launches share."""

    def __init__(self, be, st, dims, Qd, q, bnd, F, c, linearize_once, xbnd=None, poly=None, shdyn=None):
        self.be, self.st, self.dims, self.Qd, self.q, self.F, self.c = be, st, dims, Qd, q, F, c
        self.linearize_once = linearize_once   # F, c are the linearisation frozen at the warm start
        self.dense = Qd.dim() == 4             # Qd is all of C [B,T,n,n] (MPC(diag_cost=False)): solve_lin_dense, team kernel
        self.xbnd = xbnd                       # (xlo, xhi, sb_x, st_x) of MPC(x_lower=, x_upper=): solve_lin_xbox, team kernel
        self.poly = poly                       # (G, h, m, sb_g, st_g, sb_h, st_h) of MPC(ineqG=, ineqh=): solve_lin_poly, team kernel
        self.gen = self.dense + (xbnd is not None) + (poly is not None) >= 2   # two or three of them: solve_lin_gen, team kernel
        self.cached_ws = getattr(be, "_workspace", None)   # the quad kernels' cached scratch; None: no quad kernels
        self.has_backward_ws = hasattr(be, "backward_ws")
        self.has_solve_nonlin = hasattr(be, "solve_nonlin")
        self.rows_fused = False   # set by _run: the compiled-in model's one-launch route with state bounds / general rows
        self.has_solve_lin_shared = hasattr(be, "solve_lin_shared")
        # shdyn: (sb_F, st_F, sb_c, st_c) when F or c is shared by the batch (LinDx(F[T-1,nx,n] | F[nx,n]), f likewise), else
        # None. Shared data stays as given only for the plain problem on a backend that has solve_lin_shared; for a dense
        # cost, state bounds or general rows (their kernels read a per-instance F) and for any other backend it is
        # materialised here, once per solve.
        self.shdyn = shdyn
        if shdyn is not None and (not self.has_solve_lin_shared or self.dense or xbnd is not None or poly is not None):
            B, T, nx, nu = dims
            self.F = F.expand(B, T - 1, nx, nx + nu).contiguous()
            self.c = c.expand(B, T - 1, nx).contiguous()
            self.shdyn = None
        self.can_exit_in_kernel = getattr(be, "supports_exit_in_kernel", False)
        self.quad_min_batch = getattr(be, "QUAD_MIN_BATCH", 0)   # batch from which the quad kernels are the default
        B, dt, dev = dims[0], st.z.dtype, st.z.device
        # phi, rn2 and info out of ONE zeroed allocation (one fill kernel instead of three)
        esz = torch.empty((), dtype=dt).element_size()
        zb = torch.zeros(B * (2 * esz + 4), dtype=torch.uint8, device=dev)
        self.phi, self.rn2 = zb[:B * esz].view(dt), zb[B * esz:2 * B * esz].view(dt)
        self.info = zb[2 * B * esz:].view(torch.int32)
        self.status = torch.ones(B, dtype=torch.uint8, device=dev)
        self._x0_bounds = (st.x0, *bnd)   # x0, lo, hi, sb, stt
        self._problem = (st.x0, st.lam, st.rho, Qd, q, *bnd)
        self._out = dict(rnorm2=self.rn2, status=self.status, rho_scale=RHO_SCALE)
        # set by _run when a backward pass may follow: the private quad workspace (it IS the saved factor then) with
        # the arguments that select it, or the packed factor with ALQP_SAVE_FACTOR; nlws: the fused routes' workspace
        self.qws, self.private_kw, self.factor, self.save_flag, self.nlws = None, {}, None, 0, None
        self.d = self.k = self.acc = None   # Newton direction and line-search outputs of the PyTorch-dynamics steps
        self.primed = None                  # see lin_tracked
        self._cached = None

    def lin(self, info=True, **kw):
        st = self.st
        if self.gen:
            return self.be.solve_lin_gen(self.dims, self.Qd, self.q, self.F, self.c, *self._x0_bounds, self.xbnd, self.poly,
                                         st.z, st.lam, st.rho, self.phi, info=self.info if info else None, n_ls=N_LS,
                                         **self._out, **kw)
        if self.xbnd is not None:
            return self.be.solve_lin_xbox(self.dims, self.Qd, self.q, self.F, self.c, *self._x0_bounds, *self.xbnd, st.z,
                                          st.lam, st.rho, self.phi, info=self.info if info else None, n_ls=N_LS,
                                          **self._out, **kw)
        if self.poly is not None:
            return self.be.solve_lin_poly(self.dims, self.Qd, self.q, self.F, self.c, *self._x0_bounds, *self.poly, st.z,
                                          st.lam, st.rho, self.phi, info=self.info if info else None, n_ls=N_LS,
                                          **self._out, **kw)
        if self.shdyn is not None:
            return self.be.solve_lin_shared(self.dims, self.Qd, self.q, self.F, self.c, *self.shdyn, *self._x0_bounds, st.z,
                                            st.lam, st.rho, self.phi, info=self.info if info else None, n_ls=N_LS,
                                            **self._out, **kw)
        solve = self.be.solve_lin_dense if self.dense else self.be.solve_lin
        return solve(self.dims, self.Qd, self.q, self.F, self.c, *self._x0_bounds, st.z, st.lam, st.rho,
                     self.phi, info=self.info if info else None, n_ls=N_LS, **self._out, **kw)

    def lin_tracked(self, flags, private=True, **kw):
        """solve_lin with the ALQP_WS_PRIMED bookkeeping. `primed` is the workspace whose records hold THIS solve's
        current z / lam (written by the previous quad launch), else None: a launch on that workspace that saves no
        factor skips its copy-in pass. The launch goes to the solve's private workspace if it has one (and `private`),
        else to the cached scratch a quad launch will use. False: a refused cooperative launch, nothing done.
        The cached scratch is fetched once per solve: the backend hands out the same tensor for the same dims and
        dtype, and nothing between this solve's launches (dx / dx_jac included) may make it grow its cache."""
        on = self.private_kw if private else {}
        wsx = on.get("workspace")
        if wsx is None and self.cached_ws is not None and not self.dense and self.xbnd is None and self.poly is None:   # (no quad kernel reads a dense cost, state-bound or general rows)
            if self._cached is None:
                self._cached = self.cached_ws(self.dims, self.st.z)[0]
            wsx = self._cached
        if wsx is not None and self.primed is wsx and not flags & _abi.ALQP_SAVE_FACTOR:
            flags |= _abi.ALQP_WS_PRIMED
        ok = self.lin(flags=flags, **on, **kw)
        if ok is not False:
            self.primed = wsx if getattr(self.be, "last_variant", None) == "quad" else None
        return ok

    def nonlin(self, info=True, **kw):
        st = self.st
        if self.xbnd is not None or self.poly is not None:   # the team kernel with the model inlined
            return self.be.solve_nonlin_rows(self.dims, st.dx.fused_id, st.dx.dt, self.Qd, self.q, *self._x0_bounds,
                                             self.xbnd, self.poly, st.z, st.lam, st.rho, self.phi,
                                             info=self.info if info else None, workspace=self.nlws, **self._out, **kw)
        return self.be.solve_nonlin(self.dims, st.dx.fused_id, st.dx.dt, self.Qd, self.q, *self._x0_bounds, st.z, st.lam,
                                    st.rho, self.phi, info=self.info if info else None, workspace=self.nlws,
                                    **self._out, **kw)

    # The PyTorch-dynamics route's four launches. With state bounds (xbnd) each goes to its _xbox twin, which takes xbnd
    # behind the control bounds and knows no obstacle rows (the guards of MPC._run keep those apart). With general rows
    # (poly) each goes to its _rows twin, which takes xbnd (None: no state bounds) and poly behind the control bounds.
    # With a dense cost (Qd is all of C) merit, step and pick go to their _dense twins, which take both (None each); the
    # dual update reads no cost and keeps its route.
    def merit(self, z, xn, **okw):
        if self.dense:
            return self.be.merit_dense(self.dims, 1, z, xn, *self._problem, self.xbnd, self.poly, self.phi, self.rn2, **okw)
        if self.poly is not None:
            return self.be.merit_rows(self.dims, 1, z, xn, *self._problem, self.xbnd, self.poly, self.phi, self.rn2, **okw)
        if self.xbnd is not None:
            return self.be.merit_xbox(self.dims, 1, z, xn, *self._problem, self.xbnd, self.phi, self.rn2, **okw)
        self.be.merit(self.dims, 1, z, xn, *self._problem, self.phi, self.rn2, **okw)

    def newton_step(self, z, xn, F, **kw):
        if self.dense:
            return self.be.newton_step_dense(self.dims, z, xn, F, *self._problem, self.xbnd, self.poly, self.d, **kw)
        if self.poly is not None:
            return self.be.newton_step_rows(self.dims, z, xn, F, *self._problem, self.xbnd, self.poly, self.d, **kw)
        if self.xbnd is not None:
            return self.be.newton_step_xbox(self.dims, z, xn, F, *self._problem, self.xbnd, self.d, **kw)
        self.be.newton_step(self.dims, z, xn, F, *self._problem, self.d, **kw)

    def merit_pick(self, xn_all, z, **okw):
        if self.dense:
            return self.be.merit_pick_dense(self.dims, N_LS, self.d, xn_all, *self._problem, self.xbnd, self.poly, z,
                                            self.phi, rnorm2=self.rn2, k_out=self.k, accept_out=self.acc, **okw)
        if self.poly is not None:
            return self.be.merit_pick_rows(self.dims, N_LS, self.d, xn_all, *self._problem, self.xbnd, self.poly, z,
                                           self.phi, rnorm2=self.rn2, k_out=self.k, accept_out=self.acc, **okw)
        if self.xbnd is not None:
            return self.be.merit_pick_xbox(self.dims, N_LS, self.d, xn_all, *self._problem, self.xbnd, z, self.phi,
                                           rnorm2=self.rn2, k_out=self.k, accept_out=self.acc, **okw)
        self.be.merit_pick(self.dims, N_LS, self.d, xn_all, *self._problem, z, self.phi, rnorm2=self.rn2,
                           k_out=self.k, accept_out=self.acc, **okw)

    def dual_update(self, xn, **okw):
        st = self.st
        if self.poly is not None:
            return self.be.dual_update_rows(self.dims, st.z, xn, *self._x0_bounds, self.xbnd, self.poly, st.lam, st.rho,
                                            RHO_SCALE, **okw)
        if self.xbnd is not None:
            return self.be.dual_update_xbox(self.dims, st.z, xn, *self._x0_bounds, self.xbnd, st.lam, st.rho, RHO_SCALE,
                                            **okw)
        self.be.dual_update(self.dims, st.z, xn, *self._x0_bounds, st.lam, st.rho, RHO_SCALE, **okw)


class _ALSolve(torch.autograd.Function):
    """The whole AL solve as one differentiable node.

    Like the reference, only the LAST AL iteration is differentiated (earlier ones
    are cut by ``.detach().clone()``, AL_mpc.py:299) and w.r.t. q and diag(Q)
    (NewtonAL.backward, al_utils.py:578-615): w = -H^{-1} gbar with the factor saved
    at the last executed Newton step, q_grad = w, Q_grad = w * z_final.

    Beyond the reference, on the affine (``LinDx``) routes: when ``LinDx.F``, ``LinDx.f`` or ``x0`` requires grad they
    are the inputs ``dyn = (F, f, x0)`` and get dF, dc, dx0 of include/mi_alqp.h (alqp_backward_* with an AlqpBwdDyn) out
    of the same w (a batch-shared ``F`` / ``f`` gets the per-instance dF / dc summed over the axes it was broadcast over), with the same approximations (multipliers and active set held fixed, factor of the last executed Newton step);
    the multipliers in those formulas are the equality rows of the lam the solve returned, cloned here. With a callable
    ``dx`` nothing of this applies: ``x0.grad`` stays None there.

    Dense cost (``MPC(diag_cost=False)``): ``Qd`` is all of C, [B,T,n,n] and symmetric, and its gradient is
    0.5 (w z_final' + z_final w') per stage, formed here from the unchanged backward call's w = q_grad (its diagonal is
    the Qd_grad of the diagonal case).

    State bounds (``MPC(x_lower=, x_upper=)``): nothing changes here. The saved factor is that of the last Newton step's
    H, whose diagonal holds rho for every state-bound row active there, so w is taken with the active set held fixed,
    the approximation the control-bound rows already make.

    General rows (``MPC(ineqG=, ineqh=)``): the same holds, the active rows' rho G_k' G_k being in the saved factor. When
    ``ineqh`` requires grad it is one more input, behind ``dyn``: the rows enter g as G_k' (lam_k + rho max(G_k z - h_k, 0)),
    so with the active set and the multipliers held fixed dh[b,t,k] = -rho_last [G_k z_final,t - h_k >= 0] (G_k . w_t),
    formed here in PyTorch from w = q_grad and reduced over the axes ``ineqh`` broadcast over.

    The three together: the paragraphs above compose - one saved factor holds whatever went onto
    H_tt, and each gradient is formed from the same w as for its feature alone.
    """

    @staticmethod
    def forward(ctx, Qd, q, st, *extra):
        mpc = st.mpc
        n_h = 1 if len(extra) in (1, 4) else 0   # extra = [F, f, x0] [ineqh]
        dyn = extra[:len(extra) - n_h]
        ctx.n_h, ctx.poly = n_h, None
        need_grad = Qd.requires_grad or q.requires_grad or any(t.requires_grad for t in extra)
        with torch.no_grad():
            saved = mpc._run(st, Qd.detach().contiguous(), q.detach().contiguous(), need_grad)
        ctx.mpc = mpc
        ctx.has_factor = saved is not None
        ctx.n_dyn = len(dyn)
        ctx.dyn_dtypes = tuple(t.dtype for t in dyn)
        ctx.dyn_shapes = tuple(tuple(t.shape) for t in dyn)
        ctx.dense = Qd.dim() == 4
        if saved is not None:
            kind, factor, F_last, rho_last = saved
            ctx.factor_kind = kind  # "packed" (team kernels) or "workspace" (quad solve's workspace)
            lam_eq = ()
            if dyn and dyn[0].requires_grad:   # only dF reads the multipliers
                lam_eq = (st.lam[:, :(mpc.T - 1) * mpc.n_state].clone(),)
            if n_h:
                B = st.z.shape[0]
                G, h = mpc._poly_full(B, st.z.dtype, st.z.device)
                ctx.poly = (G, h, tuple(extra[-1].shape), extra[-1].dtype)
            ctx.save_for_backward(factor, F_last, rho_last, st.z, *lam_eq)
        ctx.dims = (st.z.shape[0], mpc.T, mpc.n_state, mpc.n_ctrl)
        return st.z.clone()

    @staticmethod
    def backward(ctx, gz):
        if not ctx.has_factor:
            return (None,) * (3 + ctx.n_dyn + ctx.n_h)
        factor, F_last, rho_last, z_final, *lam_eq = ctx.saved_tensors
        gbar = gz.to(z_final.dtype).contiguous()
        q_grad = torch.empty_like(z_final)
        Qd_grad = torch.empty_like(z_final)
        kw, outs = {}, ()
        want = ctx.needs_input_grad[3:3 + ctx.n_dyn]
        if any(want):
            from deq_mpc_corl_amd.backend import DynGrads
            B, T, nx, nu = ctx.dims
            new = lambda *shape: torch.empty(*shape, dtype=z_final.dtype, device=z_final.device)
            outs = (new(B, T - 1, nx, nx + nu) if want[0] else None, new(B, T - 1, nx) if want[1] else None,
                    new(B, nx) if want[2] else None)
            kw["dyn"] = DynGrads(lam_eq[0] if want[0] else None, *outs)   # passed only when asked for
        if ctx.factor_kind == "workspace":
            ctx.mpc.backend.backward_ws(ctx.dims, factor, F_last, rho_last, z_final, gbar, q_grad, Qd_grad, **kw)
        else:
            ctx.mpc.backend.backward(ctx.dims, factor, F_last, rho_last, z_final, gbar, q_grad, Qd_grad, **kw)
        if ctx.dense:
            wz = q_grad.unsqueeze(-1) * z_final.unsqueeze(-2)
            Qd_grad = 0.5 * (wz + wz.transpose(-1, -2))
        dh = ()
        if ctx.n_h:
            dh = (None,)
            if ctx.poly is not None and ctx.needs_input_grad[-1]:
                G, h, shape, hdt = ctx.poly
                act = (torch.einsum("btkj,btj->btk", G, z_final) - h >= 0).to(z_final.dtype)
                full = -rho_last.reshape(-1, 1, 1) * act * torch.einsum("btkj,btj->btk", G, q_grad)
                if len(shape) < 3:   # ineqh was [m] or [T,m]: every instance (and stage) it was broadcast over adds up
                    full = full.sum(dim=tuple(range(3 - len(shape))))
                dh = (full.reshape(shape).to(hdt),)
        if not ctx.n_dyn:
            return (Qd_grad, q_grad, None, *dh)
        if not outs:
            outs = (None,) * 3
        # a shared F / f ([T-1,nx,n], [nx,n] / [T-1,nx], [nx]) gets the per-instance gradient summed over the axes it was
        # broadcast over, like ineqh above (x0 is per instance: nothing to sum)
        full_dims = (4, 3, 2)
        outs = tuple(g if g is None or len(sh) == fd else g.sum(dim=tuple(range(fd - len(sh))))
                     for g, sh, fd in zip(outs, ctx.dyn_shapes, full_dims))
        return (Qd_grad, q_grad, None,
                *(None if g is None else g.to(d) for g, d in zip(outs, ctx.dyn_dtypes)), *dh)


class MPC(Module):
    """Batched box-constrained MPC solved by an augmented-Lagrangian method
    (same problem statement as qpth/AL_mpc.py:53-63):

        min_{x,u} sum_t 1/2 tau_t' C_t tau_t + c_t' tau_t     tau_t = [x_t; u_t]
        s.t.      x_{t+1} = f(x_t, u_t),  x_0 = x_init,  u_lower <= u <= u_upper
                  x_lower <= x_t <= x_upper  for all T stages (optional; stage 0 included)

    Differentiable w.r.t. the cost (diag C and c, as the reference). ``diag_cost=False``: C_t is a full matrix (cross
    terms, a Riccati terminal cost, a rotated frame); its symmetric part enters the solve and the gradient reaches all of
    C. With ``LinDx`` the fused team kernel runs; with a callable ``dx`` / ``dx_jac`` the
    PyTorch-dynamics route runs with the dense twins of its step, merit and pick kernels (``HipBackend.newton_step_dense``,
    ``merit_dense``, ``merit_pick_dense``), which take ``x_lower`` / ``x_upper`` and ``ineqG`` / ``ineqh`` too: the direction
    comes from the team kernel at any batch, a provider with a compiled-in model takes this route, and a backend without
    ``newton_step_dense`` raises ``NotImplementedError`` for a callable ``dx``. Not with ``linearize_once``,
    ``state_estimator`` or ``Obstacle_MPC``. With affine dynamics given as ``LinDx(F, f)`` the solve
    is also differentiable w.r.t. ``F``, ``f`` and ``x0`` (see ``_ALSolve``); not on the streaming route
    (``NotImplementedError``). With a callable ``dx`` there are no such gradients: ``x0.grad`` stays ``None``.

    ``LinDx(F, f)``: ``F`` is [B,T-1,nx,n] (per instance), [T-1,nx,n] (one sequence F_t for the whole
    batch, LTV) or [nx,n] (one model for the whole batch, LTI); ``f`` is [B,T-1,nx], [T-1,nx] or [nx], independently of
    ``F``. Shared forms are not copied B times: the kernels read the one copy (``HipBackend.solve_lin_shared``), on every
    LinDx route, and the result equals that of the expanded tensors bit for bit. Together with ``diag_cost=False``,
    ``x_lower`` / ``x_upper`` or ``ineqG`` / ``ineqh``, and on a backend without ``solve_lin_shared``, the shared forms are
    accepted and MATERIALISED (B copies) on the host once per solve; so is ``F`` for the backward pass when a gradient
    is asked for. A shared ``F`` / ``f`` that requires grad receives the sum of the per-instance gradients.

    ``x_lower`` / ``x_upper`` (both or neither): box constraints on the states, each a number, [nx], or
    anything that broadcasts to [B,T,nx] (per-stage bounds can relax stage 0, whose state is pinned to x0). A non-finite
    entry means "no bound". The reference carries the two arguments but never built their rows (al_utils.py:294-302
    are commented out). ``lamda_prev`` is then [B, T nx + T (2 nu + 2 nx)]: the equality rows, then per stage
    [u - u_upper | -u + u_lower | x - x_upper | -x + x_lower]. With ``LinDx`` the fused team kernel runs, at any batch.
    With a callable ``dx`` / ``dx_jac`` the PyTorch-dynamics route runs with the state-bound twins of
    its four kernels (``HipBackend.newton_step_xbox``, ``merit_xbox``, ``merit_pick_xbox``, ``dual_update_xbox``): the
    direction comes from the team kernel at any batch. A provider with a compiled-in model (``Pendulum1lDynamics``,
    ``Cartpole1lDynamics``, ``Cartpole1lV2Dynamics``) keeps its one launch per call: by default
    the models in ``ROWS_FUSED_DEFAULT_IDS`` (pendulum1l, cartpole1l), the third with ``prefer_fused=True``. That route
    is ``HipBackend.solve_nonlin_rows``, the team kernel with the model inlined and state bounds and / or general
    rows: ``exit_mode="fixed"`` one launch per solve, ``"reference"`` a launch per Newton step with the exit test on
    the device, gradients w.r.t. ``q``, ``diag(C)`` and ``ineqh`` from the packed factor. ``Cartpole2lDynamics`` (no
    instance of that kernel), a dense cost and a backend without ``solve_nonlin_rows`` take the launch-per-step
    route. A backend with neither ``newton_step_xbox`` nor that route raises ``NotImplementedError`` for a callable
    ``dx``. Not with ``linearize_once``, ``state_estimator`` or ``Obstacle_MPC``; with ``ineqG`` see below, with
    ``diag_cost=False`` above. The gradients of the route in use stay available (callable ``dx``: ``q`` and
    ``diag(C)``), taken with the active set held fixed.

    ``ineqG`` / ``ineqh`` (both or neither): m >= 1 general linear rows G_t tau_t <= h_t per stage, on all
    T stages next to the control bounds. ``ineqG`` is [m,n], [T,m,n] or [B,T,m,n], ``ineqh`` [m], [T,m] or [B,T,m]
    (independently); a non-finite ``ineqh`` entry means "no row". The reference carries the two arguments, but the code
    that reads them is never called (AL_mpc.py:496-498). ``lamda_prev`` is then [B, T nx + T (2 nu + m)]: the equality
    rows, then per stage [u - u_upper | -u + u_lower | G_t tau_t - h_t]. With ``LinDx`` the fused team kernel runs, at
    any batch. With a callable ``dx`` / ``dx_jac`` the PyTorch-dynamics route runs with the row twins
    of its four kernels (``HipBackend.newton_step_rows``, ``merit_rows``, ``merit_pick_rows``, ``dual_update_rows``),
    which take the state bounds too when both are given: the direction comes from the team kernel at any batch, a
    provider with a compiled-in model can take its one-launch route (see above), and a backend without ``newton_step_rows`` raises
    ``NotImplementedError`` for a callable ``dx``. Not with ``linearize_once``, ``state_estimator`` or ``Obstacle_MPC``. The
    gradients above stay available (callable ``dx``: ``q`` and ``diag(C)``), and the solve is also differentiable w.r.t. ``ineqh`` (active set held fixed); an
    ``ineqG`` that requires grad raises ``NotImplementedError``.

    ``diag_cost=False``, ``x_lower`` / ``x_upper`` and ``ineqG`` / ``ineqh`` go together, any two or all three (DESIGN
    section 23; ``HipBackend.solve_lin_gen``, the fused team kernel at any batch). ``lamda_prev`` is then
    [B, T nx + T (2 nu + [2 nx] + [m])]: the equality rows, then per stage
    [u - u_upper | -u + u_lower | x - x_upper | -x + x_lower | G_t tau_t - h_t]. Routes, guards and gradients are those
    of each feature alone. A backend without ``solve_lin_gen`` raises ``NotImplementedError`` for a combination.
    """

    def __init__(self, n_state, n_ctrl, T, u_lower=None, u_upper=None, u_init=None, x_init=None,
                 al_iter=2, verbose=0, eps=1e-7, back_eps=1e-7, n_batch=None,
                 linesearch_decay=0.2, max_linesearch_iter=10, exit_unconverged=True,
                 detach_unconverged=True, backprop=True, slew_rate_penalty=None,
                 solver_type="dense", add_goal_constraint=False, x_goal=None, diag_cost=True,
                 ineqG=None, ineqh=None, state_estimator=False, dtype=torch.float64,
                 exit_mode="reference", backend=None, process_group=None, prefer_fused=False,
                 check_numerics=None, exit_in_kernel="auto", x_lower=None, x_upper=None):
        super().__init__()
        if (u_lower is None) != (u_upper is None) or u_lower is None:
            raise ValueError("MPC: u_lower and u_upper are both required (AL_mpc.py:145,152)")
        if add_goal_constraint:
            raise NotImplementedError("goal constraints are not reachable from Tracking_MPC and are not built")
        if not diag_cost and state_estimator:
            raise NotImplementedError("MPC: diag_cost=False with state_estimator: that variant runs on the "
                                      "nonlinear-caller kernels, which read diag(C)")
        if exit_mode not in ("reference", "fixed"):
            raise ValueError("exit_mode must be 'reference' or 'fixed'")
        if (x_lower is None) != (x_upper is None):
            raise ValueError("MPC: x_lower and x_upper go together (pass +-inf for a side without a bound)")
        # combinations of the dense cost, the state bounds and the general rows run on solve_lin_gen; a backend given here
        # is asked now, the default one (resolved lazily) in the guard block of the solve
        # (with a callable dx the combinations with the dense cost run on the _dense twins of the launch-per-step kernels: a
        # backend that has them is asked again in the guard block of the solve, where the dynamics are known)
        no_gen = backend is not None and not hasattr(backend, "solve_lin_gen")
        no_dense_gen = no_gen and not hasattr(backend, "newton_step_dense")
        if x_lower is not None:
            # the state-bound rows live in the fused team kernel of the LinDx routes (alqp_solve_lin_xbox) and in the
            # _xbox twins of the launch-per-step kernels (a callable dx), which have no state-estimator row set
            if state_estimator:
                raise NotImplementedError("MPC: x_lower / x_upper with state_estimator: the state-bound variants of the "
                                          "nonlinear-caller kernels have no state-estimator row set")
            if not diag_cost and no_dense_gen:
                raise NotImplementedError(_NO_DENSE_XBOX)
        if ineqG is not None or ineqh is not None:
            # the general rows live in the fused team kernel of the LinDx routes (alqp_solve_lin_poly) and in the _rows
            # twins of the launch-per-step kernels (a callable dx), which have no state-estimator row set
            if not diag_cost and no_dense_gen:   # (before anything is asked of ineqG's shape or of ineqh)
                raise NotImplementedError(_NO_DENSE_POLY)
            if ineqG is None or ineqh is None:
                raise ValueError("MPC: ineqG and ineqh go together")
            if state_estimator:
                raise NotImplementedError("MPC: ineqG / ineqh with state_estimator: that variant runs on the "
                                          "nonlinear-caller kernels, which know no general rows")
            if x_lower is not None and no_gen:
                raise NotImplementedError(_NO_XBOX_POLY)
            ineqG, ineqh = torch.as_tensor(ineqG), torch.as_tensor(ineqh)
            if ineqG.requires_grad:
                raise NotImplementedError("MPC: a gradient w.r.t. ineqG is not built (it needs the multiplier estimate of "
                                          "the last Newton step, which the one-launch routes do not return); ineqh has one")
            n = n_state + n_ctrl
            if ineqG.dim() not in (2, 3, 4) or ineqG.shape[-1] != n or (ineqG.dim() >= 3 and ineqG.shape[-3] != T):
                raise ValueError(f"MPC: ineqG must be [m,n], [T,m,n] or [B,T,m,n] with n = {n}, T = {T}, got {tuple(ineqG.shape)}")
            m = ineqG.shape[-2]
            if ineqh.dim() not in (1, 2, 3) or ineqh.shape[-1] != m or (ineqh.dim() >= 2 and ineqh.shape[-2] != T):
                raise ValueError(f"MPC: ineqh must be [m], [T,m] or [B,T,m] with m = {m}, T = {T}, got {tuple(ineqh.shape)}")
            if not 1 <= m <= 64:
                raise ValueError(f"MPC: ineqG has {m} rows per stage, the kernel takes 1 to 64")
        self.dtype = dtype
        self.n_state, self.n_ctrl, self.T = n_state, n_ctrl, T
        self.ineqG = self.ineqh = None
        self.n_rows = 0
        if ineqG is not None:
            self.ineqG = ineqG.detach().to(dtype)
            self.ineqh = ineqh   # as given: it may require grad (_ALSolve); the solve reads _poly()'s finite copy
            self.n_rows = int(ineqG.shape[-2])
        self.u_lower = _detach_maybe(torch.as_tensor(u_lower).to(dtype))
        self.u_upper = _detach_maybe(torch.as_tensor(u_upper).to(dtype))
        self.x_lower = self.x_upper = None
        if x_lower is not None:
            # a non-finite entry is "no bound": a bound no state reaches, inert for every rho <= rho_max like the state
            # estimator's control rows (a literal infinity would make lam * r NaN in the merit)
            self.x_lower = torch.nan_to_num(_detach_maybe(torch.as_tensor(x_lower).to(dtype)), nan=-SE_NO_BOUND,
                                            posinf=SE_NO_BOUND, neginf=-SE_NO_BOUND)
            self.x_upper = torch.nan_to_num(_detach_maybe(torch.as_tensor(x_upper).to(dtype)), nan=SE_NO_BOUND,
                                            posinf=SE_NO_BOUND, neginf=-SE_NO_BOUND)
        self.u_init = _detach_maybe(u_init)
        self.x_init = _detach_maybe(x_init)
        self.al_iter = al_iter
        self.verbose = verbose
        self.n_batch = n_batch
        self.diag_cost = bool(diag_cost)
        self.linearize_once = False
        self.recompute_Qq = False
        # state_estimator=True (AL_mpc.py:179-199 -> qpth/al_utils_se.py): the controls are GIVEN and only the
        # states move; T-1 dynamics row blocks, no initial-state rows, no bound rows (lamda is [B, nx (T-1)]).
        self.state_estimator = bool(state_estimator)
        self.neq = n_state * (T - 1) if self.state_estimator else n_state * T
        self.nineq = 0 if self.state_estimator else 2 * n_ctrl * T
        if self.x_lower is not None:
            self.nineq += 2 * n_state * T   # AL_mpc.py:198-201
        self.nineq += self.n_rows * T       # AL_mpc.py:202-203
        self.rho_prev = 1.0
        self.rho_max = 1e8
        self.dyn_res_prev = 1000000
        self.exit_mode = exit_mode
        # None: numerical trouble is only recorded (last_info / last_status, no host read-back in the call);
        # "warn" / "raise": one read-back per call, warnings.warn / FloatingPointError when an instance met a
        # non-positive pivot (info) or holds a non-finite iterate (status). The reference has no such report:
        # its cholesky_ex `info` is dropped (al_utils.py:510).
        if check_numerics not in (None, "warn", "raise"):
            raise ValueError("check_numerics must be None, 'warn' or 'raise'")
        self.check_numerics = check_numerics
        # reference exit rule on an un-sharded batch: take the batch-global test inside one cooperative launch (True), or
        # between one-step launches (False; what a sharded batch always does - it needs the all-reduce in between).
        # "auto": inside the launch while the call is launch-bound, i.e. at most 512 wavefronts (half the SIMDs) - measured
        # at (20,13,4): bsz 200 (the reference's) 1.15 against 1.28 ms per call in fp32, 1.60 / 1.73 in fp64; B = 512
        # 1.29 / 1.39; from B = 1024 on the launches win (1.61 / 1.51; B = 2048: 2.41 / 1.68; B = 16384: 4.9 / 4.4): a grid
        # barrier per Newton step makes every wavefront wait for the slowest and spin next to working ones
        if exit_in_kernel not in (True, False, "auto"):
            raise ValueError("exit_in_kernel must be True, False or 'auto'")
        self.exit_in_kernel = exit_in_kernel
        self.prefer_fused = bool(prefer_fused)  # take the compiled-in dynamics model even where it is not the default
        self.process_group = process_group
        self._backend = backend
        self.warm_starting = None  # set by reinitialize(); forward() insists on it
        self.cost_hist_stream = [[], []]
        self.lamda_prev = None
        if n_batch is not None:
            self.lamda_prev = torch.zeros(n_batch, self.neq + self.nineq, dtype=dtype,
                                          device=self.u_upper.device)
        self.mask = None
        self.last_status = None
        self.last_info = None
        self.last_newton_per_al = None

    # -- backend -----------------------------------------------------------------
    @property
    def backend(self):
        if self._backend is None:
            from deq_mpc_corl_amd.backend import default_backend
            self._backend = default_backend()
        return self._backend

    # -- reference surface ---------------------------------------------------------
    def reinitialize(self, x, mask):
        """rho <- 1, lam <- 0, warm starts dropped (AL_mpc.py:569-579)."""
        self.u_init = None
        self.x_init = None
        self.n_batch = x.size(0)
        self.rho_prev = torch.ones((self.n_batch, 1), device=x.device, dtype=x.dtype)
        self.lamda_prev = torch.zeros(self.n_batch, self.neq + self.nineq, device=x.device, dtype=x.dtype)
        self.cost_hist_stream = [[], []]
        self.dyn_res_prev = 1000000
        self.just_initialized = True
        self.warm_starting = False
        self.mask = mask

    def warm_start_initialize(self, x, u, args):
        """Streaming warm start (AL_mpc.py:581-592): inits <- given, multipliers are
        shifted one stage and then zeroed (the reference multiplies by 0, :589),
        rho <- min(rho, args.rho_init_max)."""
        self.u_init = u
        self.x_init = x
        self.lamda_prev = torch.zeros_like(self.lamda_prev)
        self.rho_prev = torch.clamp(self.rho_prev, max=args.rho_init_max)
        self.just_initialized = True
        self.warm_starting = True

    @property
    def last_status(self):
        """Per-instance finiteness flag of the last solve (bool tensor), None before the first."""
        raw = getattr(self, "_status_raw", None)
        return None if raw is None else raw.bool()

    @last_status.setter
    def last_status(self, v):
        self._status_raw = v

    @property
    def dyn_res_prev(self):
        """||r+|| per instance after the last solve (AL_mpc.py's `dyn_res_prev`); the reference's initial 1000000 before."""
        raw = getattr(self, "_rn2_raw", None)
        return self._dyn_res_init if raw is None else raw.sqrt()

    @dyn_res_prev.setter
    def dyn_res_prev(self, v):
        self._dyn_res_init = v
        self._rn2_raw = None

    def get_xu(self):
        return torch.cat((self.x_init, self.u_init), dim=2)

    def get_cost(self, cost):
        xu = self.get_xu()
        f = cost.f.sum(dim=-1) if cost.f is not None else 0.0
        if not self.diag_cost:
            Cxu = (cost.C * xu.unsqueeze(-2)).sum(-1)   # (type-promoting like the diagonal form: xu is float32)
            return (0.5 * (xu * Cxu).sum(-1) + (cost.c * xu).sum(-1)).sum(dim=-1) + f
        Qd = cost.C.diagonal(dim1=-2, dim2=-1)
        return (0.5 * (xu * Qd * xu).sum(-1) + (cost.c * xu).sum(-1)).sum(dim=-1) + f

    def rollout(self, x, actions, dynamics):
        """x_{t+1} = f(x_t, u_t) from x_0 (AL_mpc.py:521-534)."""
        xs = [x]
        lin = self._as_lindx(dynamics, x.shape[0])
        for t in range(self.T - 1):
            xt, ut = xs[t], actions[:, t]
            if lin is not None:
                F = lin[0].expand(x.shape[0], self.T - 1, *lin[0].shape[-2:])   # views: a shared F / f is not copied
                c = lin[1].expand(x.shape[0], self.T - 1, lin[1].shape[-1])
                nxt = torch.einsum("bij,bj->bi", F[:, t].to(xt.dtype), torch.cat([xt, ut], -1)) + c[:, t].to(xt.dtype)
            else:
                nxt = dynamics(xt, ut)
            xs.append(nxt)
        return torch.stack(xs, 1)

    def forward(self, x0, cost, dx, dx_jac, compute_Qq=None, u_init=None, x_init=None):
        if self.warm_starting is None:
            raise RuntimeError("MPC.reinitialize(x, mask) must be called before the first solve "
                               "(the reference creates `warm_starting` there, AL_mpc.py:578)")
        self.compute_Qq = compute_Qq
        B = self.n_batch if self.n_batch is not None else cost.C.size(0)
        assert cost.C.ndimension() == 4
        assert x0.ndimension() == 2 and x0.size(0) == B

        def expand(v):
            return v.unsqueeze(0).expand(B, self.T, -1).clone() if v.ndimension() == 2 else v

        if u_init is not None:
            u = expand(u_init)
        elif self.u_init is None:
            u = torch.zeros(B, self.T, self.n_ctrl, dtype=x0.dtype, device=x0.device)
        else:
            u = expand(self.u_init)
        u = u.type_as(x0.data)
        if x_init is not None:
            x = expand(x_init)
        elif self.x_init is None:
            x = self.rollout(x0, u, dx)
        else:
            x = expand(self.x_init)
        x = x.type_as(x0.data)

        Qd = cost.C.diagonal(dim1=-2, dim2=-1) if self.diag_cost else self._sym(cost.C)
        x, u, status = self._al_solve(x, u, dx, dx_jac, x0, Qd, cost.c, bool(self.warm_starting))
        self.x_init = x.detach().clone()
        self.u_init = u.detach().clone()
        return x, u, status

    # the reference exposes both names; both end in the same machinery here
    def al_solve(self, x, u, dx, dx_jac, x0, cost, lamda_init=None, rho_init=None):
        if lamda_init is not None:
            self.lamda_prev = lamda_init
        if rho_init is not None:
            self.rho_prev = rho_init
        return self._al_solve(x, u, dx, dx_jac, x0, self._cost_C(cost), cost.c, False)

    def al_solve_stream(self, x, u, dx, dx_jac, x0, cost, lamda_init=None, rho_init=None):
        if lamda_init is not None:
            self.lamda_prev = lamda_init
        if rho_init is not None:
            self.rho_prev = rho_init
        return self._al_solve(x, u, dx, dx_jac, x0, self._cost_C(cost), cost.c, True)

    @staticmethod
    def _sym(Cm):
        """The symmetric part of C [B,T,n,n]: the quadratic form only sees it, and the dense kernel reads whole rows.
        Under autograd, so that the gradient reaches both halves of C."""
        return 0.5 * (Cm + Cm.transpose(-1, -2))

    def _cost_C(self, cost):
        """cost.C as al_solve / al_solve_stream hand it on: diag(C) [B,T,n] as given, or with diag_cost=False all of C
        [B,T,n,n], symmetrised."""
        if self.diag_cost:
            return cost.C
        if cost.C.dim() != 4:
            raise ValueError(f"MPC(diag_cost=False): cost.C must be [B,T,n,n], got {tuple(cost.C.shape)}")
        return self._sym(cost.C)

    # -- internals -------------------------------------------------------------------
    def _obs_kwargs(self, dtype, device):
        """Extra backend arguments describing the constraint-row set: obstacle rows (Obstacle_MPC), or the
        state-estimator variant's set without initial-state rows; the plain MPC has none."""
        return {"obs": "state_estimator"} if self.state_estimator else {}

    def _has_extra_rows(self):
        """True when the constraint-row set differs from the plain MPC's (obstacle rows, state estimator): a predicate
        that moves no tensor (`_obs_kwargs` would copy the obstacle centres and synchronise on every solve)."""
        return bool(self.state_estimator)

    def _as_lindx(self, dx, B):
        """(F, f, (sb_F, st_F), (sb_c, st_c)) if `dx` carries affine data, else None. F is [B,T-1,nx,n], [T-1,nx,n] or
        [nx,n], f [B,T-1,nx], [T-1,nx] or [nx]; the strides (words from one instance's / one stage's data to the next) are
        what alqp_solve_lin_shared takes: (0, 0) for one model, (0, w) for one sequence, ((T-1) w, w) per instance."""
        if self._has_extra_rows():
            return None   # obstacle rows exist only in the nonlinear-caller building blocks
        F = getattr(dx, "F", None)
        c = getattr(dx, "f", None)
        if F is None or c is None or not torch.is_tensor(F):
            return None
        n = self.n_state + self.n_ctrl
        Tm, nx = self.T - 1, self.n_state
        forms_F = {(B, Tm, nx, n): (Tm * nx * n, nx * n), (Tm, nx, n): (0, nx * n), (nx, n): (0, 0)}
        if tuple(F.shape) not in forms_F:
            raise ValueError(f"LinDx.F must be [B,T-1,nx,n]={B, Tm, nx, n}, [T-1,nx,n]={Tm, nx, n} (shared by the batch) "
                             f"or [nx,n]={nx, n} (shared by the batch and the stages), got {tuple(F.shape)}")
        forms_c = {(B, Tm, nx): (Tm * nx, nx), (Tm, nx): (0, nx), (nx,): (0, 0)}
        if not torch.is_tensor(c) or tuple(c.shape) not in forms_c:
            raise ValueError(f"LinDx.f must be [B,T-1,nx]={B, Tm, nx}, [T-1,nx]={Tm, nx} (shared by the batch) or "
                             f"[nx]={(nx,)} (shared by the batch and the stages), got "
                             f"{tuple(c.shape) if torch.is_tensor(c) else type(c).__name__}")
        return F, c, forms_F[tuple(F.shape)], forms_c[tuple(c.shape)]

    def _bounds(self, B, dtype, device):
        nu = self.n_ctrl
        if self.state_estimator:
            # no bound rows in this variant (AL_mpc.py:198): bounds no control reaches keep the kernels' bound
            # rows at residual 0 and multiplier 0 for every rho up to rho_max
            big = torch.full((nu,), SE_NO_BOUND, dtype=dtype, device=device)
            return -big, big, 0, 0
        lo = self.u_lower.to(device=device, dtype=dtype)
        hi = self.u_upper.to(device=device, dtype=dtype)
        if lo.dim() <= 1 and hi.dim() <= 1:
            lo = lo.reshape(-1).expand(nu).contiguous()
            hi = hi.reshape(-1).expand(nu).contiguous()
            return lo, hi, 0, 0
        lo = lo.expand(B, self.T, nu).contiguous()
        hi = hi.expand(B, self.T, nu).contiguous()
        return lo, hi, self.T * nu, nu

    def _xbounds(self, B, dtype, device):
        """(xlo, xhi, sb_x, st_x) as alqp_solve_lin_xbox takes them, or None without state bounds."""
        if self.x_lower is None:
            return None
        nx = self.n_state
        lo = self.x_lower.to(device=device, dtype=dtype)
        hi = self.x_upper.to(device=device, dtype=dtype)
        if lo.dim() <= 1 and hi.dim() <= 1:
            return lo.reshape(-1).expand(nx).contiguous(), hi.reshape(-1).expand(nx).contiguous(), 0, 0
        return lo.expand(B, self.T, nx).contiguous(), hi.expand(B, self.T, nx).contiguous(), self.T * nx, nx

    def _poly(self, B, dtype, device):
        """(G, h, m, sb_g, st_g, sb_h, st_h) as alqp_solve_lin_poly takes them, or None without general rows. A non-finite
        entry of ineqh is "no row": a right-hand side no stage reaches, inert for every rho <= rho_max."""
        if self.ineqG is None:
            return None
        m, n, T = self.n_rows, self.n_state + self.n_ctrl, self.T
        G = self.ineqG.to(device=device, dtype=dtype).contiguous()
        h = torch.nan_to_num(self.ineqh.detach().to(device=device, dtype=dtype), nan=SE_NO_BOUND, posinf=SE_NO_BOUND,
                             neginf=-SE_NO_BOUND).contiguous()
        for t, lead in ((G, G.dim() - 2), (h, h.dim() - 1)):
            if lead == 2 and t.shape[0] != B:
                raise ValueError(f"MPC: ineqG / ineqh given per instance for a batch of {t.shape[0]}, the solve has {B}")
        sg = {2: (0, 0), 3: (0, m * n), 4: (T * m * n, m * n)}[G.dim()]
        sh = {1: (0, 0), 2: (0, m), 3: (T * m, m)}[h.dim()]
        return (G, h, m, *sg, *sh)

    def _poly_full(self, B, dtype, device):
        """The rows as [B,T,m,n] and [B,T,m] (views), as the solve read them."""
        G, h = self._poly(B, dtype, device)[:2]
        return G.expand(B, self.T, self.n_rows, G.shape[-1]), h.expand(B, self.T, self.n_rows)

    def _rho_tensor(self, B, dtype, device):
        r = self.rho_prev
        if not torch.is_tensor(r):
            return torch.full((B,), float(r), dtype=dtype, device=device)
        return r.to(device=device, dtype=dtype).reshape(B).contiguous().clone()

    @staticmethod
    def _exit_terms(rn2, info):
        """Per-instance terms of the batch norm the Newton loop exits on. An instance whose factorisation hit a
        non-positive pivot (sticky info != 0) counts as +inf: the exit then never fires in this call. The reference's
        norm (torch.norm(dyn_res), al_utils.py:552) holds the UNDEFINED residuals of such instances (half-finished
        Cholesky factor, :510-515) and kept both recorded batches at the full 4 Newton steps
        (tests/golden/fail_*.npz: newton_per_al = [4]); without its garbage the healthy instances alone would stop
        after 3 and end 0.03 / 0.06 (fp64 / fp32) away from the reference's controls."""
        if info is None:
            return rn2
        return torch.where(info != 0, torch.full_like(rn2, float("inf")), rn2)

    def _global_sumsq(self, rn2, info=None):
        """sum_b sum_rows r+^2 as a 1-element float64 device tensor (all-reduced over the ranks
        of a sharded batch); nothing is synchronised with the host."""
        s = self._exit_terms(rn2, info).sum(dtype=torch.float64).reshape(1)
        if self._sharded():
            torch.distributed.all_reduce(s, group=self.process_group)
        return s

    def _global_norm(self, rn2, info=None):
        """sqrt(sum_b sum_rows r+^2): the batch-global quantity the reference exits on
        (torch.norm(dyn_res).item(), al_utils.py:486,552). With a sharded batch the
        partial sums are all-reduced (8 bytes over RCCL) so that every rank takes the
        same decision the un-sharded reference would."""
        s = self._exit_terms(rn2, info).sum(dtype=torch.float64)
        if self._sharded():
            torch.distributed.all_reduce(s, group=self.process_group)
        return math.sqrt(float(s.item()))

    def _sharded(self):
        return self.process_group is not None or (
            torch.distributed.is_available() and torch.distributed.is_initialized()
            and getattr(self, "sync_global_exit", False))

    def _global_mean(self, v):
        """Batch mean of a per-instance quantity (the stream loop's break test,
        `dyn_res_clamp.mean().item()`, AL_mpc.py:406-408); over ALL ranks of a sharded batch, so
        that every rank leaves the loop in the same iteration."""
        s = torch.stack((v.sum(dtype=torch.float64), torch.tensor(float(v.numel()), dtype=torch.float64, device=v.device)))
        if self._sharded():
            torch.distributed.all_reduce(s, group=self.process_group)
        s = s.tolist()
        return s[0] / s[1]

    def _global_max(self, v):
        """`rho.max().item()` (AL_mpc.py:412, 420), over all ranks of a sharded batch."""
        m = v.max().to(torch.float64).reshape(1)
        if self._sharded():
            torch.distributed.all_reduce(m, op=torch.distributed.ReduceOp.MAX, group=self.process_group)
        return float(m.item())

    def _al_solve(self, x, u, dx, dx_jac, x0, Qd, q, stream_mode):
        B = x.shape[0]
        dt = self.dtype
        dev = x0.device
        if self.lamda_prev is None:
            self.lamda_prev = torch.zeros(B, self.neq + self.nineq, dtype=dt, device=dev)
        nrows = self.n_state * self.T + 2 * self.n_ctrl * self.T   # the kernels' row layout
        st = _SolveState()
        st.mpc = self
        st.x0 = x0.detach().to(dt).contiguous()
        st.z = torch.cat((x, u), dim=2).detach().to(dt).contiguous()   # (cat made a fresh tensor: no clone)
        st.lam = self.lamda_prev.detach().to(device=dev, dtype=dt).contiguous().clone()
        if self.state_estimator:   # [B, nx (T-1)] -> the kernels' layout; the init and bound rows stay 0
            st.lam = torch.cat((st.lam, st.lam.new_zeros(B, nrows - self.neq)), dim=1).contiguous()
        st.rho = self._rho_tensor(B, dt, dev)
        st.dx, st.dx_jac = dx, dx_jac
        st.lin = self._as_lindx(dx, B)
        st.stream_mode = stream_mode
        st.status_flag = False
        z = _ALSolve.apply(Qd.to(dt), q.to(dt), st, *self._dyn_inputs(st, x0, stream_mode), *self._h_input())
        self.lamda_prev = st.lam[:, :self.neq].contiguous() if self.state_estimator else st.lam
        self.rho_prev = st.rho.reshape(B, 1)
        self.just_initialized = False
        self.last_newton_per_al = st.newton_per_al
        nx = self.n_state
        return z[..., :nx].float(), z[..., nx:].float(), st.status_flag

    def _dyn_inputs(self, st, x0, stream_mode):
        """(F, f, x0) as inputs of the autograd node when the affine dynamics or the initial state ask for a gradient
        (_ALSolve), else (): the node, and every launch, is then exactly what it is without this feature."""
        if st.lin is None or not torch.is_grad_enabled():
            return ()
        F, f = st.lin[:2]
        if not (F.requires_grad or (torch.is_tensor(f) and f.requires_grad) or x0.requires_grad):
            return ()
        if stream_mode or self.linearize_once:
            raise NotImplementedError("MPC: gradients w.r.t. LinDx.F / LinDx.f / x0 exist on the al_solve route only; the "
                                      "streaming route (al_solve_stream, linearize_once) carries lam and rho over "
                                      "its iterations on the host and saves no multipliers for them")
        return F, f, x0   # (each in one of _as_lindx's forms: _ALSolve.backward reduces the shared ones' gradients)

    def _h_input(self):
        """(ineqh,) as an input of the autograd node when it asks for a gradient (_ALSolve), else ()."""
        if self.ineqh is None or not torch.is_grad_enabled() or not self.ineqh.requires_grad:
            return ()
        return (self.ineqh,)

    def _linearize(self, st, z):
        """dx_jac at every (x_t, u_t), t < T-1 -> (f(z) [B,T-1,nx], F = [A|B] [B,T-1,nx,n]).
        Called the way the reference does (al_utils.py:501-503, 233-248): grad mode on and the
        iterate requiring grad, because the torch-coded environments differentiate through their own
        RK4 step inside `dx_jac` (rex_quadrotor.py:136-144)."""
        B, T, nx, nu = z.shape[0], self.T, self.n_state, self.n_ctrl
        with torch.enable_grad():
            zz = z.detach().requires_grad_(True)
            xn_j, (A, Bm) = st.dx_jac(zz[:, :-1, :nx].reshape(-1, nx), zz[:, :-1, nx:].reshape(-1, nu))
        Bm = Bm.detach().reshape(B, T - 1, nx, nu)
        if self.state_estimator:
            Bm = Bm * 0.0   # the controls do not move (al_utils_se.py:151)
        F = torch.cat((A.detach().reshape(B, T - 1, nx, nx), Bm), dim=-1).to(z.dtype).contiguous()
        return xn_j.detach().reshape(B, T - 1, nx).to(z.dtype).contiguous(), F

    def _true_next(self, st, zz):
        """f(x_t, u_t) of the TRUE dynamics, PyTorch-coded: zz [..., T, n] -> [..., T-1, nx]."""
        nx = self.n_state
        xn = st.dx(zz[..., :-1, :nx].reshape(-1, nx), zz[..., :-1, nx:].reshape(-1, self.n_ctrl))
        return xn.reshape(*zz.shape[:-2], self.T - 1, nx).to(zz.dtype).contiguous()

    def _fused_model(self, st):
        """True when the dynamics model is compiled into the library (dynamics.py) and this solve may take it: plain
        row set (the compiled-in models know no state-bound rows and no general rows: with x_lower / x_upper or
        ineqG / ineqh a provider such as PendulumDynamics takes the PyTorch-dynamics route), one call per solve (not the stream loop), the sizes it was
        compiled for, and the model's default route unless `prefer_fused`."""
        dx = st.dx
        return (st.lin is None and not st.stream_mode and not self._has_extra_rows() and self.x_lower is None
                and self.ineqG is None and self.diag_cost   # (nor do they read a dense cost)
                and getattr(dx, "fused_id", None) is not None
                and (getattr(dx, "fused_default", True) or self.prefer_fused)
                and (getattr(dx, "nx", None), getattr(dx, "nu", None)) == (self.n_state, self.n_ctrl))

    def _fused_rows_model(self, st, be, dims, dt):
        """True when this solve takes the compiled-in model's one-launch route WITH state bounds and / or general rows
        (HipBackend.solve_nonlin_rows; _fused_model above stays the plain row set's predicate): a
        compiled-in model of these sizes, one call per solve, a diagonal cost, state bounds and / or general rows present,
        a backend that has the method (and an instance of the model on that route), and `prefer_fused` or a model whose
        default this route is (ROWS_FUSED_DEFAULT_IDS, and `fused_default`)."""
        dx = st.dx
        if not (st.lin is None and not st.stream_mode and not self._has_extra_rows() and self.diag_cost
                and (self.x_lower is not None or self.ineqG is not None)
                and not self.linearize_once and not self.state_estimator
                and hasattr(be, "solve_nonlin_rows")
                and getattr(dx, "fused_id", None) is not None
                and (self.prefer_fused or (getattr(dx, "fused_default", True) and dx.fused_id in ROWS_FUSED_DEFAULT_IDS))
                and (getattr(dx, "nx", None), getattr(dx, "nu", None)) == (self.n_state, self.n_ctrl)):
            return False
        has = getattr(be, "nonlin_rows_workspace_bytes", None)   # 0: the library has no instance of this model there
        return has is None or has(dims, dt) > 0

    # ---- the Newton loop of one AL iteration (NewtonAL.forward, al_utils.py:451-576), per route ----
    def _newton_device_exit(self, L, launch, **step_kw):
        """Reference exit rule without a host round trip per Newton step: the batch-global test
        (al_utils.py:551-564) is taken on the device. All MAX_NEWTON one-step launches are enqueued, each one a
        no-op once ctl[0] is set, and the number of executed steps (ctl[1]) is read back once per solve."""
        launch(al_iter=1, max_newton=0, flags=_abi.ALQP_INIT_MERIT)
        ctl = torch.zeros(3, dtype=torch.float64, device=L.st.z.device)
        L.be.exit_test(self._global_sumsq(L.rn2, L.info), ctl, 0)
        for _ in range(MAX_NEWTON):
            launch(al_iter=1, max_newton=1, skip=ctl, **step_kw)
            L.be.exit_test(self._global_sumsq(L.rn2, L.info), ctl, 1)
        return ctl[1]

    def _newton_lin(self, L):
        """Affine data: every launch on the same workspace as the one before with nothing touched in between, so
        none but the first pays a copy-in pass (L.lin_tracked)."""
        if self.exit_mode == "fixed":
            L.lin_tracked(al_iter=1, max_newton=MAX_NEWTON, flags=_abi.ALQP_INIT_MERIT | L.save_flag, factor=L.factor)
            return MAX_NEWTON
        return self._newton_device_exit(L, L.lin_tracked, flags=L.save_flag, factor=L.factor)

    def _newton_torch(self, L):
        """`dx` / `dx_jac` as PyTorch calls between kernel launches. Returns (steps, F of the last one)."""
        st, z = L.st, L.st.z
        okw = self._obs_kwargs(z.dtype, z.device)   # {} or {"obs": (centres, radius)} (Obstacle_MPC)
        L.merit(z, self._true_next(st, z), **okw)
        old = self._global_norm(L.rn2, L.info) if self.exit_mode == "reference" else None
        alphas = (2.0 ** -torch.arange(N_LS, device=z.device, dtype=z.dtype)).view(N_LS, 1, 1, 1)
        # from B = QUAD_MIN_BATCH on the direction comes from the quad kernels (obstacle rows / the state-estimator
        # row set included), whose factor stays in the workspace records: the private one when backward follows
        # With state bounds, general rows or a dense cost the direction comes from the team kernel at any batch (no quad
        # step kernel knows those rows or reads a full C): no workspace is fetched, and the packed factor is the saved one.
        qws = L.qws   # (fetched once per solve, on the assumption L.lin_tracked states)
        if (qws is None and L.cached_ws is not None and L.dims[0] >= L.quad_min_batch and L.xbnd is None
                and L.poly is None and not L.dense):
            qws = L.cached_ws(L.dims, z)[0]
        steps = 0
        while steps < MAX_NEWTON:
            steps += 1
            xn, F = self._linearize(st, z)
            L.newton_step(z, xn, F, info=L.info, **(dict(workspace=qws) if qws is not None else dict(factor=L.factor)),
                          **okw)
            zc = (z.unsqueeze(0) + alphas * L.d.unsqueeze(0)).contiguous()
            # 20 merits + decision + update in one launch; rn2 <- the chosen candidate's when accepted
            L.merit_pick(self._true_next(st, zc), z, **okw)
            if self.exit_mode == "reference":
                new = self._global_norm(L.rn2, L.info)
                if new < 1e-3 or (math.isfinite(new) and abs(old - new) / new < 1e-3):   # inf: a tripped instance, no exit
                    break
                old = new
        return steps, F

    # ---- one AL iteration (Newton loop + dual update), per route: -> (Newton steps, F of the last one) ----
    # (one signature for all four, so that _solve_al_loop can pick the body once: only the fused one reads need_grad)
    def _al_iter_fused(self, L, need_grad):
        """Compiled-in model, reference exit: one launch per Newton step (the model inlined), the batch-global exit
        test on the device, then the dual update launch."""
        if need_grad and L.nlws is None:
            L.nlws = L.be.new_workspace_nonlin(L.dims, L.st.z)
        steps = self._newton_device_exit(L, L.nonlin, flags=0)
        L.nonlin(al_iter=1, max_newton=0, flags=_abi.ALQP_DUAL_UPDATE, info=False)
        # L and F of the last executed Newton step are still in the workspace
        return steps, (L.be.nonlin_F_view(L.nlws, L.dims) if need_grad else None)

    def _rows_F_last(self, L, need_grad):
        """The linearisation of the last executed Newton step out of the private workspace, as the packed backward reads it."""
        return L.be.nonlin_rows_F_view(L.nlws, L.dims).contiguous() if need_grad else None

    def _al_iter_fused_rows(self, L, need_grad):
        """_al_iter_fused's shape on the team kernel with rows: a merit launch, one launch per Newton step (each a no-op
        once the batch-global exit test on the device has fired), then the dual update launch. The packed factor is
        written by every launch that executes a Newton step."""
        if need_grad and L.nlws is None:
            L.nlws = L.be.new_workspace_nonlin_rows(L.dims, L.st.z)
        steps = self._newton_device_exit(L, L.nonlin, flags=L.save_flag, factor=L.factor)
        L.nonlin(al_iter=1, max_newton=0, flags=_abi.ALQP_DUAL_UPDATE, info=False)
        return steps, self._rows_F_last(L, need_grad)

    def _al_iter_coop(self, L, need_grad):
        """Affine data, reference exit: starting merit, Newton loop with the batch-global exit and dual update in one
        cooperative launch. None (nothing launched) when the grid cannot be co-resident."""
        cnt = torch.zeros(1, dtype=torch.int32, device=L.st.z.device)
        if not L.lin_tracked(al_iter=1, max_newton=MAX_NEWTON, factor=L.factor, newton_counts=cnt,
                             flags=_abi.ALQP_INIT_MERIT | _abi.ALQP_DUAL_UPDATE | L.save_flag):
            return None
        return cnt[0], L.F

    def _al_iter_lin(self, L, need_grad):
        """Affine data (given, or the frozen linearisation of `linearize_once`), a launch per Newton step."""
        steps = self._newton_lin(L)
        if L.linearize_once:
            self._dual_update_torch(L)
        else:
            # never on the private workspace: keep the saved factor's workspace out of later launches altogether
            L.lin_tracked(al_iter=1, max_newton=0, flags=_abi.ALQP_DUAL_UPDATE, private=False, info=False)
        return steps, L.F

    def _al_iter_torch(self, L, need_grad):
        out = self._newton_torch(L)
        self._dual_update_torch(L)
        return out

    def _dual_update_torch(self, L):
        """Dual update with the TRUE dynamics (AL_mpc.py:315-317 / :397-399)."""
        st = L.st
        xn = self._true_next(st, st.z)
        okw = self._obs_kwargs(st.z.dtype, st.z.device)
        L.merit(st.z, xn, **okw)
        L.dual_update(xn, **okw)
        L.primed = None   # lam/rho changed behind the workspace records' back

    # ---- the routes of a solve: each -> (newton_per_al, rho_last, F_last) ----
    def _solve_lin_one_launch(self, L, need_grad, coop):
        """Affine dynamics, the whole solve in ONE launch: 4 Newton steps per AL iteration (fixed exit), or with `coop`
        the reference's batch-global exit test taken INSIDE one cooperative launch (grid-wide barrier + ordered sum
        per Newton step, ALQP_EXIT_IN_KERNEL). None when that launch was refused."""
        counts = torch.zeros(self.al_iter, dtype=torch.int32, device=L.st.z.device) if coop else None
        ok = L.lin(al_iter=self.al_iter, max_newton=MAX_NEWTON, factor=L.factor, **L.private_kw,
                   flags=_abi.ALQP_INIT_MERIT | _abi.ALQP_DUAL_UPDATE | L.save_flag,
                   **(dict(newton_counts=counts) if coop else {}))
        if coop and not ok:
            return None
        npa = list(counts.unbind()) if coop else [MAX_NEWTON] * self.al_iter
        return npa, (L.st.rho / RHO_SCALE if need_grad or coop else None), L.F

    def _solve_fused_one_launch(self, L, need_grad, coop):
        """Dynamics model compiled into the library: the whole nonlinear solve in ONE launch, no PyTorch round trip
        between Newton steps; `coop` and None as in _solve_lin_one_launch."""
        if need_grad:   # private workspace: its records and F region are the saved factor
            L.nlws = L.be.new_workspace_nonlin(L.dims, L.st.z)
        counts = torch.zeros(self.al_iter, dtype=torch.int32, device=L.st.z.device) if coop else None
        ok = L.nonlin(al_iter=self.al_iter, max_newton=MAX_NEWTON, flags=_abi.ALQP_INIT_MERIT | _abi.ALQP_DUAL_UPDATE,
                      **(dict(newton_counts=counts) if coop else {}))
        if coop and not ok:
            return None
        npa = list(counts.unbind()) if coop else [MAX_NEWTON] * self.al_iter
        return npa, L.st.rho / RHO_SCALE, (L.be.nonlin_F_view(L.nlws, L.dims) if need_grad else None)

    def _solve_fused_rows_one_launch(self, L, need_grad):
        """Compiled-in model with state bounds and / or general rows, fixed exit: the whole nonlinear solve in ONE launch
        of the team kernel (no cooperative in-kernel exit on this route)."""
        if need_grad:   # private workspace: its F regions go with the packed factor
            L.nlws = L.be.new_workspace_nonlin_rows(L.dims, L.st.z)
        L.nonlin(al_iter=self.al_iter, max_newton=MAX_NEWTON, factor=L.factor,
                 flags=_abi.ALQP_INIT_MERIT | _abi.ALQP_DUAL_UPDATE | L.save_flag)
        return [MAX_NEWTON] * self.al_iter, L.st.rho / RHO_SCALE, self._rows_F_last(L, need_grad)

    def _solve_al_loop(self, L, need_grad, fused, coop):
        """The AL outer loop on the host (AL_mpc.py:260-339 / :342-423), one of four bodies per iteration."""
        st, stream = L.st, L.st.stream_mode
        prev_mean = None
        if L.linearize_once:  # dyn_res_clamp_prev starts at the residual of the warm start (:358-369)
            L.merit(st.z, self._true_next(st, st.z))
            prev_mean = self._global_mean(L.rn2.sqrt())
        body = (self._al_iter_fused_rows if L.rows_fused else self._al_iter_fused if fused else self._al_iter_coop if coop
                else self._al_iter_lin if L.F is not None else self._al_iter_torch)
        npa, rho_last, F_last = [], None, None
        for _ in range(100 if L.linearize_once else self.al_iter):
            rho_last = st.rho.clone()
            out = body(L, need_grad)
            if out is None:   # cooperative launch refused: a launch per Newton step from here on, no second try
                body = self._al_iter_lin
                out = body(L, need_grad)
            npa.append(out[0])
            F_last = out[1]
            if stream:
                if L.linearize_once:
                    mean = self._global_mean(L.rn2.sqrt())
                    if prev_mean is not None and not mean < prev_mean:
                        break
                    prev_mean = mean
                if self._global_max(st.rho) > self.rho_max:
                    break
        if stream and self._global_max(st.rho) > self.rho_max:
            st.status_flag = True
        return npa, rho_last, F_last

    def _run(self, st, Qd, q, need_grad):
        """One solve: the checks that raise, the allocation, then the route - the one-launch route that applies,
        else the AL loop. Mutates st.z/lam/rho. Returns (kind, factor, F_last, rho_last) when a backward pass may
        follow."""
        be = self.backend
        B, T, nx, nu = st.z.shape[0], self.T, self.n_state, self.n_ctrl
        n = nx + nu
        dt, dev = st.z.dtype, st.z.device
        dims = (B, T, nx, nu)
        stream = st.stream_mode
        if not be.supported(B, T, nx, nu, dt):
            raise RuntimeError(f"mi_alqp: no kernel instance for (nx={nx}, nu={nu}, T={T}, {dt}); "
                               "add it to ALQP_FOR_EACH_DIMS in csrc/alqp_dims.hpp")
        # a callable dx with a dense cost: the _dense twins of the launch-per-step kernels, which take
        # the state bounds and the general rows too
        dense_step = st.lin is None and hasattr(be, "newton_step_dense")
        # a compiled-in model on its one-launch route with state bounds / general rows needs none of the
        # launch-per-step twins the guards below ask a callable dx for
        rows_fused = self._fused_rows_model(st, be, dims, dt)
        if not hasattr(be, "solve_lin_gen"):
            # (a backend given to the constructor was refused there; this is the lazily resolved default's turn)
            if self.x_lower is not None and not self.diag_cost and not dense_step:
                raise NotImplementedError(_NO_DENSE_XBOX)
            if self.ineqG is not None and not self.diag_cost and not dense_step:
                raise NotImplementedError(_NO_DENSE_POLY)
            # (with a callable dx the two together run on the _rows twins of the launch-per-step kernels alone)
            if self.ineqG is not None and self.x_lower is not None and not (
                    st.lin is None and hasattr(be, "newton_step_rows")) and not (not self.diag_cost and dense_step):
                raise NotImplementedError(_NO_XBOX_POLY)
        if not self.diag_cost:
            # the dense cost lives in the fused team kernel (alqp_solve_lin_dense) and, for a callable dx, in the _dense
            # twins of the launch-per-step kernels: the plain nonlinear-caller kernels, the quad step
            # kernels, the obstacle / state-estimator row sets and the compiled-in models read diag(C)
            if self._has_extra_rows():
                raise NotImplementedError("MPC: diag_cost=False with obstacle rows / state_estimator: those run on the "
                                          "nonlinear-caller kernels, which read diag(C)")
            if self.linearize_once:
                raise NotImplementedError("MPC: diag_cost=False with linearize_once: the frozen-linearisation route "
                                          "evaluates merit and dual update with kernels that read diag(C)")
            if st.lin is None and not dense_step:
                raise NotImplementedError("MPC: diag_cost=False needs affine dynamics given as LinDx(F, f): the "
                                          "nonlinear-caller kernels and the compiled-in models read diag(C)")
        if self.x_lower is not None:
            # the state-bound rows live in the fused team kernel (alqp_solve_lin_xbox) and, for a callable dx, in the
            # launch-per-step kernels' _xbox twins, for a compiled-in model in the team kernel of DESIGN
            # section 28; the quad step kernels (the quad fused solve of the compiled-in models among them) and the obstacle /
            # state-estimator row sets know no such rows
            if self._has_extra_rows():
                raise NotImplementedError("MPC: x_lower / x_upper with obstacle rows (Obstacle_MPC): the state-bound "
                                          "variants of the nonlinear-caller kernels take no obstacle rows")
            if self.linearize_once:
                raise NotImplementedError("MPC: x_lower / x_upper with linearize_once: the frozen-linearisation route "
                                          "is not built with state-bound rows")
            if st.lin is None and not (rows_fused or hasattr(be, "newton_step_xbox")
                                       or (self.ineqG is not None and hasattr(be, "newton_step_rows"))
                                       or (not self.diag_cost and dense_step)):
                raise NotImplementedError("MPC: x_lower / x_upper need affine dynamics given as LinDx(F, f): the "
                                          "nonlinear-caller kernels and the compiled-in models know no state-bound rows")   # (wording pinned by tests: the models' quad solve)
            if st.lam.shape[1] != self.neq + self.nineq:
                raise ValueError(f"MPC: lamda has {st.lam.shape[1]} rows per instance, the state bounds need "
                                 f"{self.neq + self.nineq} = T nx + T (2 nu + 2 nx{' + m' if self.n_rows else ''})")
        if self.ineqG is not None:
            # the general rows live in the fused team kernel (alqp_solve_lin_poly) and, for a callable dx, in the
            # launch-per-step kernels' _rows twins, for a compiled-in model in the team kernel of DESIGN
            # section 28; the quad step kernels (the quad fused solve of the compiled-in models among them) and the obstacle /
            # state-estimator row sets know no such rows
            if self._has_extra_rows():
                raise NotImplementedError("MPC: ineqG / ineqh with obstacle rows (Obstacle_MPC): those run on the "
                                          "nonlinear-caller kernels, which know no general rows")
            if self.linearize_once:
                raise NotImplementedError("MPC: ineqG / ineqh with linearize_once: the frozen-linearisation route "
                                          "evaluates merit and dual update with kernels that know no general rows")
            if st.lin is None and not (rows_fused or hasattr(be, "newton_step_rows") or (not self.diag_cost and dense_step)):
                raise NotImplementedError("MPC: ineqG / ineqh need affine dynamics given as LinDx(F, f): the "
                                          "nonlinear-caller kernels and the compiled-in models know no general rows")   # (wording pinned by tests: the models' quad solve)
            if st.lam.shape[1] != self.neq + self.nineq:
                raise ValueError(f"MPC: lamda has {st.lam.shape[1]} rows per instance, the general rows need "
                                 f"{self.neq + self.nineq} = T nx + T (2 nu{' + 2 nx' if self.x_lower is not None else ''} + m)")
        if self.state_estimator:
            # cost gradient on the states only (al_utils_se.py:300-310) while the Hessian keeps diag(Q) on the
            # controls (:66-68): the kernels' `state_estimator` flag. Their merit still counts the controls' cost
            # terms, the same constant for every line-search candidate since du = 0 exactly (:31 leaves them out).
            if torch.is_tensor(getattr(st.dx, "F", None)) or self.linearize_once:
                raise NotImplementedError("state_estimator: only the callable dx / dx_jac route exists "
                                          "(al_utils_se.py has no LinDx or frozen-linearisation branch)")
        if need_grad and self.linearize_once and stream:
            # al_utils_lin.NewtonAL.backward returns 14 gradients for 15 inputs (al_utils_lin.py:444-459):
            # autograd rejects it, so the reference cannot differentiate this route. Same error type.
            raise RuntimeError("MPC: the linearize_once streaming route is not differentiable (the reference's "
                               "al_utils_lin.NewtonAL.backward returns an incorrect number of gradients)")
        if self.linearize_once and not stream:
            # The reference cannot run this combination either: al_solve (AL_mpc.py:292-306) hands the
            # frozen-linearisation dict to al_utils.merit_grad_hessian, which calls it
            # ("TypeError: 'dict' object is not callable", al_utils.py:237). Same error type here.
            raise TypeError("MPC: linearize_once is only defined for the streaming route (after "
                            "warm_start_initialize); the reference's al_solve raises TypeError on it as well")
        linearize_once = bool(self.linearize_once)
        if self._has_extra_rows() and linearize_once:
            raise NotImplementedError("Obstacle_MPC with linearize_once: the reference's frozen-linearisation "
                                      "module knows no obstacle rows (AL_mpc_custom.py:68, 75, 83)")

        F = c = shdyn = None
        if linearize_once:
            # frozen linearisation captured once per call (al_utils_lin.py:140-169)
            # note the offset: x_{t+1} of the WARM START minus F_t z_t, not f(z_t) - F_t z_t (:154)
            _, F = self._linearize(st, st.z)
            c = (st.z[:, 1:, :nx] - torch.einsum("btij,btj->bti", F, st.z[:, :-1])).contiguous()
        elif st.lin is not None:
            F = st.lin[0].detach().to(device=dev, dtype=dt).contiguous()
            c = st.lin[1].detach().to(device=dev, dtype=dt).contiguous()
            if F.dim() < 4 or c.dim() < 3:   # shared by the batch: the data as given, with its strides
                shdyn = (*st.lin[2], *st.lin[3])
        L = _Launcher(be, st, dims, Qd, q, self._bounds(B, dt, dev), F, c, linearize_once, self._xbounds(B, dt, dev),
                      self._poly(B, dt, dev), shdyn)
        F = L.F   # (materialised by the launcher where no kernel reads the shared form)
        # the quad kernels take the obstacle / state-estimator rows too, so their factor can stay in the records
        # (dense cost, state bounds, general rows: team kernel, packed factor)
        use_qws = (need_grad and L.has_backward_ws and B >= L.quad_min_batch and not L.dense and L.xbnd is None
                   and L.poly is None)
        if use_qws:
            L.qws = be.new_workspace(dims, st.z)
            L.private_kw = dict(workspace=L.qws, variant="quad")
        elif need_grad:
            L.factor = torch.empty(B, T, n * (n + 1) // 2, dtype=dt, device=dev)
            L.save_flag = _abi.ALQP_SAVE_FACTOR
        if st.lin is None or linearize_once:
            L.d = torch.empty(B, T, n, dtype=dt, device=dev)
            L.k = torch.zeros(B, dtype=torch.int32, device=dev)
            L.acc = torch.zeros(B, dtype=torch.int32, device=dev)

        # Reference exit rule on an un-sharded batch: the batch-global test of the Newton loop may be taken inside a
        # cooperative launch instead of between one-step launches (see `exit_in_kernel` in __init__)
        in_kernel = self.exit_mode == "reference" and not self._sharded() and L.can_exit_in_kernel
        auto = self.exit_in_kernel == "auto"
        coop = (in_kernel and F is not None and not linearize_once and (self.exit_in_kernel is True or (
            auto and B < L.quad_min_batch and -(-B // max(1, be.qps_per_wave(B, T, nx, nu, dt))) <= 512)))
        fused = L.has_solve_nonlin and self._fused_model(st)
        coop_nl = in_kernel and fused and (self.exit_in_kernel is True or (auto and -(-B // 16) <= 512))
        fixed = self.exit_mode == "fixed"
        L.rows_fused = rows_fused
        res = None
        if F is not None and not stream and (coop or fixed):
            res = self._solve_lin_one_launch(L, need_grad, coop)
        elif fused and (coop_nl or fixed):
            res = self._solve_fused_one_launch(L, need_grad, coop_nl)
        elif L.rows_fused and fixed:
            res = self._solve_fused_rows_one_launch(L, need_grad)
        if res is None:
            res = self._solve_al_loop(L, need_grad, fused, coop)
        npa, rho_last, F_last = res

        # device-side exit counters (one read-back for the whole solve)
        on_dev = [i for i, v in enumerate(npa) if torch.is_tensor(v)]
        if on_dev:
            for i, v in zip(on_dev, torch.stack([npa[i].to(torch.float64) for i in on_dev]).tolist()):
                npa[i] = int(round(v))
            if min(npa) < 0:
                raise RuntimeError("mi_alqp: a grid barrier of the in-kernel exit test timed out (ALQP_EXIT_IN_KERNEL); "
                                   "construct the MPC with exit_in_kernel=False")
        st.newton_per_al = npa
        # (kept raw: `last_status` / `dyn_res_prev` are formed when read - two device kernels per call that a
        #  solve whose caller never looks at them does not pay for; at the reference's batch size a call is ~0.6 ms)
        self._status_raw = L.status
        self.last_info = L.info
        self._rn2_raw = L.rn2
        if self.check_numerics is not None:
            n_piv = int((L.info != 0).sum().item())
            n_bad = int((L.status == 0).sum().item())
            if n_piv or n_bad:
                msg = (f"mi_alqp: {n_piv} of {B} instances met a non-positive pivot (penalty x conditioning beyond "
                       f"{dt}; modified-Cholesky step taken, see MPC.last_info), {n_bad} hold a non-finite iterate "
                       "(MPC.last_status)")
                if self.check_numerics == "raise":
                    raise FloatingPointError(msg)
                import warnings
                warnings.warn(msg, RuntimeWarning, stacklevel=3)
        if need_grad and F_last is not None:
            if F_last.dim() < 4:   # the backward kernels read a per-instance F: materialised only here, for them
                F_last = F_last.expand(B, T - 1, nx, n).contiguous()
            if L.nlws is not None and not L.rows_fused:
                return "workspace", L.nlws, F_last, rho_last
            if use_qws:
                return "workspace", L.qws, F_last, rho_last
            return "packed", L.factor, F_last, rho_last
        return None
