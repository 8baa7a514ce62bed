"""Device backend: torch tensors -> raw device pointers -> libmi_alqp.so.

PyTorch is plumbing here (allocator, streams); every number is produced by the
hand-written gfx950 kernels in csrc/. All methods enqueue on torch's current HIP
stream and never synchronise.
"""
from __future__ import annotations

import ctypes as C

import os

import torch

from . import _lib


def _dt(t):
    if t.dtype == torch.float32:
        return "f32"
    if t.dtype == torch.float64:
        return "f64"
    raise TypeError(f"mi_alqp: unsupported dtype {t.dtype}")


def _ptr(t, name, dtype=None, allow_none=False):
    if t is None:
        if allow_none:
            return None
        raise ValueError(f"mi_alqp: {name} is required")
    if not t.is_cuda:
        raise RuntimeError(
            f"mi_alqp: {name} lives on {t.device}; the solver only runs on a ROCm device "
            "(no CPU fallback)")
    if not t.is_contiguous():
        raise ValueError(f"mi_alqp: {name} must be contiguous")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"mi_alqp: {name} has dtype {t.dtype}, expected {dtype}")
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# experiments only (profiles/r02/experiments): bits 24-31 of AlqpParams.flags reach the quad kernel untouched
_DEBUG_FLAGS = ((int(os.environ.get("ALQP_DEBUG_STAGGER", "0")) & 0xff) << 24) | ((int(os.environ.get("ALQP_DEBUG_STAGGER_CU", "0")) & 0xf) << 20)


class DynGrads:
    """What `backward` / `backward_ws` take as `dyn=`: the outputs for the gradients w.r.t. the affine dynamics
    x_{t+1} = F_t z_t + c_t and the initial state (include/mi_alqp.h, AlqpBwdDyn). `lam` [B, >= (T-1) nx]
    holds the multipliers the solve returned (rows may be a view of the full lam: only a unit inner stride is
    needed; required with dF). dF [B, T-1, nx, n], dc [B, T-1, nx], dx0 [B, nx]: a tensor to fill, or None."""

    __slots__ = ("lam", "dF", "dc", "dx0")

    def __init__(self, lam=None, dF=None, dc=None, dx0=None):
        self.lam, self.dF, self.dc, self.dx0 = lam, dF, dc, dx0


def _dyn_args(dyn, dims, dt):
    """A DynGrads (or None) -> the AlqpBwdDyn of alqp_backward_* (or None: the plain kernels)."""
    if dyn is None:
        return None
    B, T, nx, nu = dims
    lam = dyn.lam
    if lam is None:
        if dyn.dF is not None:
            raise ValueError("mi_alqp: dyn.dF needs dyn.lam (the multipliers the solve returned)")
        lam_p, sb = None, 0
    else:
        if (not lam.is_cuda or lam.dtype != dt or lam.dim() != 2 or lam.shape[0] != B or lam.shape[1] < (T - 1) * nx
                or lam.stride(1) != 1 or (B > 1 and lam.stride(0) < (T - 1) * nx)):
            raise ValueError(f"mi_alqp: dyn.lam must be a [B, >= (T-1) nx] {dt} device tensor with unit inner stride")
        lam_p, sb = lam.data_ptr(), max(int(lam.stride(0)), (T - 1) * nx)
    outs = []
    for t, name, shape in ((dyn.dF, "dF", (B, T - 1, nx, nx + nu)), (dyn.dc, "dc", (B, T - 1, nx)),
                           (dyn.dx0, "dx0", (B, nx))):
        if t is not None and tuple(t.shape) != shape:
            raise ValueError(f"mi_alqp: dyn.{name} has shape {tuple(t.shape)}, expected {shape}")
        outs.append(None if t is None else _ptr(t, "dyn." + name, dt).value)
    return _lib.AlqpBwdDyn(lam_p, sb, *outs)


def _step_length(h, K, dt):
    """Step length of the CasADi dynamics providers -> (h, h_pt): a number, or one value per point (a [K] tensor)."""
    if not torch.is_tensor(h):
        return float(h), None
    hpt = h.to(dt).reshape(-1).contiguous()
    if hpt.numel() != K:
        raise ValueError("mi_alqp: h must be a number or one value per point")
    return 0.0, hpt


class HipBackend:
    """The product backend: thin argument marshalling over the C ABI."""

    name = "hip"
    supports_exit_in_kernel = True   # solve_lin(newton_counts=...): ALQP_EXIT_IN_KERNEL, cooperative launch
    default_variant = "auto"
    # "auto": the quad variant (16 instances per wavefront, factor streamed through HBM) once the batch fills the chip,
    # the team variant (one instance per lane team, factor in LDS) below. This number is the batch from which the
    # launch-per-step routes take the quad kernels; the fused solve asks the library (_pick_variant), whose table
    # (csrc/alqp_abi.hip, with the measurements) this value overrides only when it is changed
    QUAD_MIN_BATCH = 4096

    def __init__(self):
        self.lib = _lib.load()
        self._ws = {}  # key -> cached scratch tensor (_scratch)
        if os.environ.get("ALQP_QUAD_STAGGER") is not None:   # -1 auto (default), 0 off, > 0 units of ~1024 clocks
            self.set_quad_stagger(int(os.environ["ALQP_QUAD_STAGGER"]))

    quad_stagger = -1   # -1 automatic, 0 off, > 0 explicit units of ~1024 clocks (passed per call in AlqpParams.quad_stagger)

    def set_quad_stagger(self, mode):
        """Start offset between the four wavefronts of a CU in the quad solve (AlqpParams.quad_stagger, include/mi_alqp.h):
        -1 automatic, 0 off, > 0 explicit. Returns the previous mode. Timing only - results do not depend on it.
        State of THIS backend object; the library keeps none."""
        prev, self.quad_stagger = self.quad_stagger, (-1 if int(mode) < 0 else int(mode))
        return prev

    def workspace_bytes(self, B, T, nx, nu, dtype):
        d = _lib.AlqpDims(B, T, nx, nu)
        return int(self.lib.alqp_workspace_bytes(C.byref(d), int(dtype == torch.float64)))

    def _workspace(self, dims, like):
        """Device scratch for the quad variant, cached per (device, dtype). Contents need
        not survive between calls; stream order protects reuse on one stream."""
        need = self.workspace_bytes(*dims, like.dtype)
        return self._scratch((like.device, like.dtype), need // like.element_size(), like.dtype, like.device, 16), need

    def _scratch(self, key, numel, dtype, device, spare=0):
        """self._ws[key]: the cached scratch tensor under `key`; allocated anew, with `numel + spare` elements, when it
        is missing or holds fewer than `numel`."""
        t = self._ws.get(key)
        if t is None or t.numel() < numel:
            t = self._ws[key] = torch.empty(numel + spare, dtype=dtype, device=device)
        return t

    # -- queries ---------------------------------------------------------------
    def supported(self, B, T, nx, nu, dtype):
        d = _lib.AlqpDims(B, T, nx, nu)
        return bool(self.lib.alqp_supported(C.byref(d), int(dtype == torch.float64)))

    def lds_bytes(self, B, T, nx, nu, dtype):
        d = _lib.AlqpDims(B, T, nx, nu)
        return int(self.lib.alqp_lds_bytes(C.byref(d), int(dtype == torch.float64)))

    def qps_per_wave(self, B, T, nx, nu, dtype):
        d = _lib.AlqpDims(B, T, nx, nu)
        return int(self.lib.alqp_qps_per_wave(C.byref(d), int(dtype == torch.float64)))

    def _pick_variant(self, dims, dtype, flags):
        """What "auto" resolves to in solve_lin (alqp_pick_variant): 1 team, 2 quad, 0 no instance of (nx, nu). The
        library's table, unless QUAD_MIN_BATCH was changed: then quad from that batch on."""
        qmin = -1 if self.QUAD_MIN_BATCH == HipBackend.QUAD_MIN_BATCH else self.QUAD_MIN_BATCH
        return int(self.lib.alqp_pick_variant(C.byref(_lib.AlqpDims(*dims)), int(dtype == torch.float64), flags, qmin))

    # -- kernels -----------------------------------------------------------------
    def solve_lin(self, dims, Qd, q, F, c, x0, ulo, uhi, sb_u, st_u, z, lam, rho, phi,
                  rnorm2=None, info=None, status=None, factor=None, al_iter=2, max_newton=4,
                  n_ls=20, flags=_lib.ALQP_INIT_MERIT | _lib.ALQP_DUAL_UPDATE, rho_scale=10.0,
                  trace=None, variant=None, workspace=None, skip=None, newton_counts=None, exit_tol=1e-3):
        """variant: None/"auto" (quad unless a factor must be saved), "team", "quad".
        workspace: a dedicated scratch tensor for the quad variant (kept by the caller when
        the factor it holds afterwards is needed for `backward_ws`); default: a cached one.
        newton_counts (int32 [al_iter], device): with it the reference's batch-global exit test of the Newton loop
        runs INSIDE the launch (ALQP_EXIT_IN_KERNEL, one cooperative launch); returns False - nothing launched - when
        the grid cannot be co-resident (the caller then takes the launch-per-step route), True otherwise."""
        return self._solve_lin("alqp_solve_lin_", dims, _ptr(Qd, "Qd", z.dtype), q, F, c, x0, ulo, uhi, sb_u, st_u, z, lam,
                               rho, phi, rnorm2, info, status, factor, al_iter, max_newton, n_ls, flags, rho_scale, trace,
                               variant, skip, newton_counts, exit_tol, quad=True, workspace=workspace)

    def solve_lin_shared(self, dims, Qd, q, F, c, sb_F, st_F, sb_c, st_c, x0, ulo, uhi, sb_u, st_u, z, lam, rho, phi,
                         rnorm2=None, info=None, status=None, factor=None, al_iter=2, max_newton=4,
                         n_ls=20, flags=_lib.ALQP_INIT_MERIT | _lib.ALQP_DUAL_UPDATE, rho_scale=10.0,
                         trace=None, variant=None, workspace=None, skip=None, newton_counts=None, exit_tol=1e-3):
        """solve_lin on batch-shared dynamics (alqp_solve_lin_shared): F and c addressed with an instance stride and a
        stage stride in words. F [nx,n] (sb_F = st_F = 0), [T-1,nx,n] (0, nx n) or [B,T-1,nx,n] ((T-1) nx n, nx n); c
        likewise without the last axis (0, 0 / 0, nx / (T-1) nx, nx), independently of F. Keywords, kernel choice,
        workspace and return value as solve_lin; the numbers are those of solve_lin on the expanded tensors, bit for bit."""
        B, T, nx, nu = dims
        for t, name, sb, st, w in ((F, "F", sb_F, st_F, nx * (nx + nu)), (c, "c", sb_c, st_c, nx)):
            if t is not None and min(sb, st) >= 0 and t.numel() < (B - 1) * sb + (T - 2) * st + w:
                raise ValueError(f"mi_alqp: {name} has {t.numel()} elements, too few for strides ({sb}, {st})")
        return self._solve_lin("alqp_solve_lin_shared_", dims, _ptr(Qd, "Qd", z.dtype), q, F, c, x0, ulo, uhi, sb_u, st_u, z,
                               lam, rho, phi, rnorm2, info, status, factor, al_iter, max_newton, n_ls, flags, rho_scale,
                               trace, variant, skip, newton_counts, exit_tol, quad=True, workspace=workspace,
                               after_c=(sb_F, st_F, sb_c, st_c))

    def _solve_lin(self, entry, dims, cost, q, F, c, x0, ulo, uhi, sb_u, st_u, z, lam, rho, phi, rnorm2, info, status,
                   factor, al_iter, max_newton, n_ls, flags, rho_scale, trace, variant, skip, newton_counts, exit_tol,
                   quad=False, workspace=None, after_c=(), after_u=(), after_stream=()):
        """What the six solve_lin* methods share: the params struct, the exit-in-kernel set-up, the trace struct, the call and
        the cooperative-launch fallback. entry: the entry point's name without its dtype suffix; cost: its third argument
        (the pointer to Qd or C, or None); after_c / after_u / after_stream: what it takes behind c, behind st_u and behind
        the stream. quad: alqp_solve_lin and alqp_solve_lin_shared, the entry points with quad kernels: kernel choice,
        workspace, debug flags and stagger; the others run the team kernels only."""
        B, T, nx, nu = dims
        dt = z.dtype
        name = entry + _dt(z)
        d = _lib.AlqpDims(B, T, nx, nu)
        if quad:
            if variant is None:
                variant = self.default_variant
            vnum = {"auto": 0, "team": 1, "quad": 2}[variant]
            if vnum == 0:
                vnum = self._pick_variant(dims, dt, flags)   # 0 (no such instance) goes through: the library refuses it
            ws, ws_bytes = (None, 0)
            if vnum == 2:
                if workspace is not None:
                    ws, ws_bytes = workspace, self.workspace_bytes(*dims, z.dtype)
                    if ws.numel() * ws.element_size() < ws_bytes:
                        raise ValueError("mi_alqp: workspace too small")
                else:
                    ws, ws_bytes = self._workspace(dims, z)
            self.last_variant = "quad" if vnum == 2 else "team"
            flags |= _DEBUG_FLAGS
            ws_args = (_ptr(ws, "workspace", dt, True), ws_bytes)
        else:
            vnum = {"auto": 0, "team": 1, "quad": 2}[variant or "auto"]   # quad goes through: the library refuses it
            self.last_variant = "team"
            ws_args = (None, 0) if after_stream else ()   # alqp_solve_lin_gen: alqp_solve_lin's arguments, then its own
        skp = _ptr(skip, "skip", torch.float64, True)
        p = _lib.AlqpParams(al_iter, max_newton, n_ls, flags, rho_scale, vnum, skp.value if skp is not None else None)
        if quad:
            p.quad_stagger = {-1: 0, 0: -1}.get(self.quad_stagger, self.quad_stagger)   # ABI: 0 automatic, < 0 off
        if newton_counts is not None:
            self._exit_in_kernel(p, B, z.device, newton_counts, exit_tol)
        tr = None
        if trace is not None:
            tr = _lib.AlqpTrace(*[
                (trace[k].data_ptr() if trace.get(k) is not None else None)
                for k in ("g", "d", "phi", "phi_prev", "k", "accept")])
        rc = getattr(self.lib, name)(
            C.byref(d), C.byref(p), cost, _ptr(q, "q", dt), _ptr(F, "F", dt),
            _ptr(c, "c", dt), *after_c, _ptr(x0, "x0", dt), _ptr(ulo, "u_lower", dt), _ptr(uhi, "u_upper", dt),
            sb_u, st_u, *after_u, _ptr(z, "z", dt), _ptr(lam, "lam", dt), _ptr(rho, "rho", dt),
            _ptr(phi, "phi", dt), _ptr(rnorm2, "rnorm2", dt, True),
            _ptr(info, "info", torch.int32, True), _ptr(status, "status", torch.uint8, True),
            _ptr(factor, "factor", dt, True), C.byref(tr) if tr is not None else None, *ws_args, _stream(), *after_stream)
        if rc == _lib.ALQP_E_COOP and newton_counts is not None:
            return False
        _lib.check(rc, name)
        return True

    @staticmethod
    def _row_checks(dims, lam, dense_C, xbnd, poly, need=None):
        """The host-side checks of every method that takes a dense cost, state bounds or general rows. dense_C: C or None;
        xbnd: (xlo, xhi, sb_x, st_x) or None; poly: (G, h, m, sb_g, st_g, sb_h, st_h) or None. C is [B,T,n,n], lam (when
        given) at least M = T nx + T (2 nu + [2 nx] + [m]) wide, bounds and rows as long as their strides reach. need: how
        the message names the rows lam is too narrow for, where the method has a wording of its own.
        -> (xlo, xhi, sb_x, st_x, G, h, m, sb_g, st_g, sb_h, st_h), None / 0 for what is absent."""
        B, T, nx, nu = dims
        n = nx + nu
        if dense_C is not None and tuple(dense_C.shape) != (B, T, n, n):
            raise ValueError(f"mi_alqp: C has shape {tuple(dense_C.shape)}, expected {(B, T, n, n)}")
        xlo, xhi, sb_x, st_x = xbnd if xbnd is not None else (None, None, 0, 0)
        G, h, m, sb_g, st_g, sb_h, st_h = poly if poly is not None else (None, None, 0, 0, 0, 0, 0)
        M = T * nx + T * (2 * nu + (2 * nx if xbnd is not None else 0) + (max(int(m), 0) if poly is not None else 0))
        if lam is not None and (lam.dim() != 2 or lam.shape[0] != B or lam.shape[1] < M):
            if need is None:
                need = "these rows need" if poly is not None else "the state-bound rows need" if xbnd is not None else "expected"
            raise ValueError(f"mi_alqp: lam has shape {tuple(lam.shape)}, {need} [B, {M}]")
        if xbnd is not None:
            for t, name in ((xlo, "x_lower"), (xhi, "x_upper")):
                if t is None:
                    raise ValueError(f"mi_alqp: {name} is required")
                if min(sb_x, st_x) >= 0 and t.numel() < (B - 1) * sb_x + (T - 1) * st_x + nx:
                    raise ValueError(f"mi_alqp: {name} has {t.numel()} elements, too few for strides ({sb_x}, {st_x})")
        for t, name, sb, st, w in ((G, "ineqG", sb_g, st_g, m * n), (h, "ineqh", sb_h, st_h, m)):
            if t is not None and m >= 1 and min(sb, st) >= 0 and t.numel() < (B - 1) * sb + (T - 1) * st + w:
                raise ValueError(f"mi_alqp: {name} has {t.numel()} elements, too few for strides ({sb}, {st})")
        return xlo, xhi, sb_x, st_x, G, h, m, sb_g, st_g, sb_h, st_h

    @staticmethod
    def _rows_cargs(rows, dt):
        """_row_checks' tuple as the C arguments from x_lo to st_h."""
        xlo, xhi, sb_x, st_x, G, h, *rest = rows
        return (_ptr(xlo, "x_lower", dt, True), _ptr(xhi, "x_upper", dt, True), sb_x, st_x,
                _ptr(G, "ineqG", dt, True), _ptr(h, "ineqh", dt, True), *rest)

    def solve_lin_dense(self, dims, Cs, q, F, c, x0, ulo, uhi, sb_u, st_u, z, lam, rho, phi,
                        rnorm2=None, info=None, status=None, factor=None, al_iter=2, max_newton=4,
                        n_ls=20, flags=_lib.ALQP_INIT_MERIT | _lib.ALQP_DUAL_UPDATE, rho_scale=10.0,
                        trace=None, variant=None, skip=None, newton_counts=None, exit_tol=1e-3):
        """solve_lin with a dense stage cost (alqp_solve_lin_dense): Cs [B,T,n,n], symmetric, in place of Qd. Team
        kernel only (variant None / "auto" / "team"), no workspace; everything else as solve_lin."""
        self._row_checks(dims, None, Cs, None, None)
        return self._solve_lin("alqp_solve_lin_dense_", dims, _ptr(Cs, "C", z.dtype), q, F, c, x0, ulo, uhi, sb_u, st_u, z,
                               lam, rho, phi, rnorm2, info, status, factor, al_iter, max_newton, n_ls, flags, rho_scale,
                               trace, variant, skip, newton_counts, exit_tol)

    def solve_lin_xbox(self, dims, Qd, q, F, c, x0, ulo, uhi, sb_u, st_u, xlo, xhi, sb_x, st_x, z, lam, rho, phi,
                       rnorm2=None, info=None, status=None, factor=None, al_iter=2, max_newton=4,
                       n_ls=20, flags=_lib.ALQP_INIT_MERIT | _lib.ALQP_DUAL_UPDATE, rho_scale=10.0,
                       trace=None, variant=None, skip=None, newton_counts=None, exit_tol=1e-3):
        """solve_lin with state box rows xlo[t] <= x_t <= xhi[t] (alqp_solve_lin_xbox): xlo / xhi [nx] (sb_x = st_x = 0)
        or [B,T,nx] (sb_x = T nx, st_x = nx), finite. lam is [B, T nx + T (2 nu + 2 nx)]: per stage
        [u - uhi | -u + ulo | x - xhi | -x + xlo] behind the equality rows. Team kernel only (variant None / "auto" /
        "team"), no workspace; everything else as solve_lin."""
        rows = self._row_checks(dims, lam, None, (xlo, xhi, sb_x, st_x), None)
        return self._solve_lin("alqp_solve_lin_xbox_", dims, _ptr(Qd, "Qd", z.dtype), q, F, c, x0, ulo, uhi, sb_u, st_u, z,
                               lam, rho, phi, rnorm2, info, status, factor, al_iter, max_newton, n_ls, flags, rho_scale,
                               trace, variant, skip, newton_counts, exit_tol, after_u=self._rows_cargs(rows, z.dtype)[:4])

    def solve_lin_poly(self, dims, Qd, q, F, c, x0, ulo, uhi, sb_u, st_u, G, h, m, sb_g, st_g, sb_h, st_h, z, lam, rho, phi,
                       rnorm2=None, info=None, status=None, factor=None, al_iter=2, max_newton=4,
                       n_ls=20, flags=_lib.ALQP_INIT_MERIT | _lib.ALQP_DUAL_UPDATE, rho_scale=10.0,
                       trace=None, variant=None, skip=None, newton_counts=None, exit_tol=1e-3):
        """solve_lin with m general rows G_t z_t <= h_t per stage, z_t = [x_t; u_t] (alqp_solve_lin_poly): G [m,n] (sb_g =
        st_g = 0), [T,m,n] (0, m n) or [B,T,m,n] (T m n, m n), h likewise without the last axis, finite. lam is
        [B, T nx + T (2 nu + m)]: per stage [u - uhi | -u + ulo | G_t z_t - h_t] behind the equality rows. Team kernel
        only (variant None / "auto" / "team"), no workspace; everything else as solve_lin."""
        rows = self._row_checks(dims, lam, None, None, (G, h, m, sb_g, st_g, sb_h, st_h), "the general rows need")
        return self._solve_lin("alqp_solve_lin_poly_", dims, _ptr(Qd, "Qd", z.dtype), q, F, c, x0, ulo, uhi, sb_u, st_u, z,
                               lam, rho, phi, rnorm2, info, status, factor, al_iter, max_newton, n_ls, flags, rho_scale,
                               trace, variant, skip, newton_counts, exit_tol, after_u=self._rows_cargs(rows, z.dtype)[4:])

    def solve_lin_gen(self, dims, Qd_or_C, q, F, c, x0, ulo, uhi, sb_u, st_u, xbnd, poly, z, lam, rho, phi,
                      rnorm2=None, info=None, status=None, factor=None, al_iter=2, max_newton=4,
                      n_ls=20, flags=_lib.ALQP_INIT_MERIT | _lib.ALQP_DUAL_UPDATE, rho_scale=10.0,
                      trace=None, variant=None, skip=None, newton_counts=None, exit_tol=1e-3):
        """solve_lin with two or three of a dense cost, state bounds and general rows together (alqp_solve_lin_gen).
        Qd_or_C: C [B,T,n,n] (a dense cost) or Qd [B,T,n]; xbnd: (xlo, xhi, sb_x, st_x) as solve_lin_xbox takes them,
        or None; poly: (G, h, m, sb_g, st_g, sb_h, st_h) as solve_lin_poly takes them, or None. lam is
        [B, T nx + T (2 nu + [2 nx] + [m])]: per stage [u - uhi | -u + ulo | x - xhi | -x + xlo | G_t z_t - h_t] behind the
        equality rows. Team kernel only (variant None / "auto" / "team"), no workspace; everything else as solve_lin."""
        dt = z.dtype
        dense = Qd_or_C is not None and Qd_or_C.dim() == 4
        rows = self._row_checks(dims, lam, Qd_or_C if dense else None, xbnd, poly, "these rows need")
        return self._solve_lin("alqp_solve_lin_gen_", dims, None if dense else _ptr(Qd_or_C, "Qd", dt), q, F, c, x0, ulo, uhi,
                               sb_u, st_u, z, lam, rho, phi, rnorm2, info, status, factor, al_iter, max_newton, n_ls, flags,
                               rho_scale, trace, variant, skip, newton_counts, exit_tol,
                               after_stream=(_ptr(Qd_or_C, "C", dt) if dense else None, *self._rows_cargs(rows, dt)))

    def _exit_in_kernel(self, p, B, device, newton_counts, exit_tol):
        """AlqpParams fields of ALQP_EXIT_IN_KERNEL: the cached scratch (arrival counter + 2 x B partial sums)."""
        scr = self._scratch(("exit", device), 2 * B + 2, torch.float64, device)
        scr.zero_()   # arrival counter, partial sums, time-out flag
        p.flags |= _lib.ALQP_EXIT_IN_KERNEL
        p.exit_tol = float(exit_tol)
        p.newton_counts = _ptr(newton_counts, "newton_counts", torch.int32).value
        p.exit_scratch = scr.data_ptr()

    def solve_nonlin(self, dims, dyn_id, dyn_h, Qd, q, x0, ulo, uhi, sb_u, st_u, z, lam, rho, phi, rnorm2=None,
                     info=None, status=None, al_iter=2, max_newton=4,
                     flags=_lib.ALQP_INIT_MERIT | _lib.ALQP_DUAL_UPDATE, rho_scale=10.0, skip=None, workspace=None,
                     newton_counts=None, exit_tol=1e-3):
        """Nonlinear fused solve (alqp_solve_nonlin): the dynamics model `dyn_id` is inlined.
        workspace: a private one (new_workspace_nonlin) when the factor and linearisation it holds
        afterwards are needed by backward_ws; default: a cached one."""
        B, T, nx, nu = dims
        dt = z.dtype
        sfx = _dt(z)
        d = _lib.AlqpDims(B, T, nx, nu)
        need = int(self.lib.alqp_workspace_bytes_nonlin(C.byref(d), int(dt == torch.float64)))
        if need == 0:
            raise RuntimeError("mi_alqp: nonlinear fused solve not available for these sizes")
        if workspace is not None:
            ws = workspace
            if ws.numel() * ws.element_size() < need:
                raise ValueError("mi_alqp: workspace too small")
        else:
            ws = self._scratch(("nl", z.device, dt), need // z.element_size(), dt, z.device, 16)
        skp = _ptr(skip, "skip", torch.float64, True)
        p = _lib.AlqpParams(al_iter, max_newton, 20, flags, rho_scale, 2, skp.value if skp is not None else None)
        if newton_counts is not None:   # the reference's exit test inside one cooperative launch, see solve_lin
            self._exit_in_kernel(p, B, z.device, newton_counts, exit_tol)
        fn = getattr(self.lib, "alqp_solve_nonlin_" + sfx)
        rc = fn(C.byref(d), C.byref(p), int(dyn_id), float(dyn_h), _ptr(Qd, "Qd", dt), _ptr(q, "q", dt), _ptr(x0, "x0", dt),
                _ptr(ulo, "u_lower", dt), _ptr(uhi, "u_upper", dt), sb_u, st_u, _ptr(z, "z", dt), _ptr(lam, "lam", dt),
                _ptr(rho, "rho", dt), _ptr(phi, "phi", dt), _ptr(rnorm2, "rnorm2", dt, True),
                _ptr(info, "info", torch.int32, True), _ptr(status, "status", torch.uint8, True),
                _ptr(ws, "workspace", dt), need, _stream())
        if rc == _lib.ALQP_E_COOP and newton_counts is not None:
            return False
        _lib.check(rc, "alqp_solve_nonlin_" + sfx)
        self.last_variant = "quad"
        return True

    def nonlin_rows_workspace_bytes(self, dims, dtype):
        """alqp_workspace_bytes_nonlin_rows: 0 when no compiled-in model of this (nx, nu) runs on the team route."""
        return int(self.lib.alqp_workspace_bytes_nonlin_rows(C.byref(_lib.AlqpDims(*dims)), int(dtype == torch.float64)))

    def solve_nonlin_rows(self, dims, dyn_id, dyn_h, Qd, q, x0, ulo, uhi, sb_u, st_u, xbnd, poly, z, lam, rho, phi,
                          rnorm2=None, info=None, status=None, factor=None, al_iter=2, max_newton=4,
                          flags=_lib.ALQP_INIT_MERIT | _lib.ALQP_DUAL_UPDATE, rho_scale=10.0, trace=None, skip=None,
                          workspace=None):
        """Nonlinear fused solve with state bounds and / or general rows (alqp_solve_nonlin_rows): solve_nonlin's problem,
        the model `dyn_id` inlined, plus xbnd = (xlo, xhi, sb_x, st_x) and / or poly = (G, h, m, sb_g, st_g, sb_h, st_h) as
        solve_lin_gen takes them (None: absent; at least one must be given). One launch of the team kernel, any batch.
        lam is [B, T nx + T (2 nu + [2 nx] + [m])], per stage [u | x | G] behind the equality rows. factor (with
        ALQP_SAVE_FACTOR): the packed factor of the last executed Newton step, for `backward` together with
        nonlin_rows_F_view(workspace). workspace: a private one (new_workspace_nonlin_rows) when the linearisation it
        holds afterwards is needed; default: a cached one."""
        B, T, nx, nu = dims
        dt = z.dtype
        name = "alqp_solve_nonlin_rows_" + _dt(z)
        if xbnd is None and poly is None:
            raise ValueError("mi_alqp: solve_nonlin_rows needs state bounds or general rows (the plain problem is solve_nonlin's)")
        rows = self._row_checks(dims, lam, None, xbnd, poly, "these rows need")
        need = self.nonlin_rows_workspace_bytes(dims, dt)
        if need == 0:
            raise RuntimeError("mi_alqp: nonlinear fused solve with rows not available for these sizes")
        if workspace is not None:
            ws = workspace
            if ws.numel() * ws.element_size() < need:
                raise ValueError("mi_alqp: workspace too small")
        else:
            ws = self._scratch(("nlr", z.device, dt), need // z.element_size(), dt, z.device)
        skp = _ptr(skip, "skip", torch.float64, True)
        p = _lib.AlqpParams(al_iter, max_newton, 20, flags, rho_scale, 1, skp.value if skp is not None else None)
        tr = None
        if trace is not None:
            tr = _lib.AlqpTrace(*[
                (trace[k].data_ptr() if trace.get(k) is not None else None)
                for k in ("g", "d", "phi", "phi_prev", "k", "accept")])
        rc = getattr(self.lib, name)(
            C.byref(_lib.AlqpDims(B, T, nx, nu)), C.byref(p), int(dyn_id), float(dyn_h), _ptr(Qd, "Qd", dt),
            _ptr(q, "q", dt), _ptr(x0, "x0", dt), _ptr(ulo, "u_lower", dt), _ptr(uhi, "u_upper", dt), sb_u, st_u,
            *self._rows_cargs(rows, dt), _ptr(z, "z", dt), _ptr(lam, "lam", dt), _ptr(rho, "rho", dt),
            _ptr(phi, "phi", dt), _ptr(rnorm2, "rnorm2", dt, True), _ptr(info, "info", torch.int32, True),
            _ptr(status, "status", torch.uint8, True), _ptr(factor, "factor", dt, True),
            C.byref(tr) if tr is not None else None, _ptr(ws, "workspace", dt), need, _stream())
        _lib.check(rc, name)
        self.last_variant = "team"
        return True

    def new_workspace_nonlin_rows(self, dims, like):
        """A private workspace for solve_nonlin_rows: per instance F [T-1,nx,n], then xnext [T-1,nx]."""
        need = self.nonlin_rows_workspace_bytes(dims, like.dtype)
        if need == 0:
            raise RuntimeError("mi_alqp: nonlinear fused solve with rows not available for these sizes")
        return torch.empty(need // like.element_size(), dtype=like.dtype, device=like.device)

    def nonlin_rows_F_view(self, ws, dims):
        """The F regions of a solve_nonlin_rows workspace as a [B, T-1, nx, n] tensor (a strided view: the linearisation of
        the last executed Newton step of every instance)."""
        B, T, nx, nu = dims
        n = nx + nu
        per = (T - 1) * nx * (n + 1)
        return ws[:B * per].view(B, per)[:, :(T - 1) * nx * n].view(B, T - 1, nx, n)

    def dyn_pendulum1l(self, x, u, h, want_jac=True):
        """pendulum1l provider (alqp_dyn_pendulum1l): x [K,2], u [K,1], h float or [K(,1)] tensor
        -> xnext [K,2], F [K,2,3] or None."""
        K = x.shape[0]
        dt = x.dtype
        xn = torch.empty(K, 2, dtype=dt, device=x.device)
        F = torch.empty(K, 2, 3, dtype=dt, device=x.device) if want_jac else None
        h, hpt = _step_length(h, K, dt)
        fn = getattr(self.lib, "alqp_dyn_pendulum1l_" + _dt(x))
        rc = fn(K, _ptr(x, "x", dt), _ptr(u, "u", dt), h, _ptr(hpt, "h", dt, True),
                _ptr(xn, "xnext", dt), _ptr(F, "F", dt, True), _stream())
        _lib.check(rc, "alqp_dyn_pendulum1l")
        return xn, F

    def dyn_cartpole1l(self, x, tau, h, want_jac=True, version=1):
        """cartpole1l provider (alqp_dyn_cartpole1l; version=2: alqp_dyn_cartpole1l_v2, the cartpole1l_v2 package's
        constants): x [K,4], tau [K,2], h float or per-point tensor -> xnext [K,4], J [K,4,6] (d xnext / d(q, qdot, tau))
        or None."""
        K = x.shape[0]
        dt = x.dtype
        xn = torch.empty(K, 4, dtype=dt, device=x.device)
        J = torch.empty(K, 4, 6, dtype=dt, device=x.device) if want_jac else None
        h, hpt = _step_length(h, K, dt)
        fn = getattr(self.lib, ("alqp_dyn_cartpole1l_v2_" if version == 2 else "alqp_dyn_cartpole1l_") + _dt(x))
        rc = fn(K, _ptr(x, "x", dt), _ptr(tau, "tau", dt), h, _ptr(hpt, "h", dt, True),
                _ptr(xn, "xnext", dt), _ptr(J, "J", dt, True), _stream())
        _lib.check(rc, "alqp_dyn_cartpole1l")
        return xn, J

    def dyn_cartpole2l(self, x, tau, h, want_jac=True):
        """cartpole2l provider (alqp_dyn_cartpole2l): x [K,6], tau [K,3] -> xnext [K,6], J [K,6,9] or None."""
        K = x.shape[0]
        dt = x.dtype
        xn = torch.empty(K, 6, dtype=dt, device=x.device)
        J = torch.empty(K, 6, 9, dtype=dt, device=x.device) if want_jac else None
        h, hpt = _step_length(h, K, dt)
        fn = getattr(self.lib, "alqp_dyn_cartpole2l_" + _dt(x))
        rc = fn(K, _ptr(x, "x", dt), _ptr(tau, "tau", dt), h, _ptr(hpt, "h", dt, True),
                _ptr(xn, "xnext", dt), _ptr(J, "J", dt, True), _stream())
        _lib.check(rc, "alqp_dyn_cartpole2l")
        return xn, J

    def dyn_rigid(self, model, params, x, u, h, want_jac=True):
        """Quadrotor / flying-cartpole provider (alqp_dyn_rexquadrotor / alqp_dyn_flyingcartpole): model "rex" (x [K,12])
        or "flycart" (x [K,14]), u [K,4], params an _lib.AlqpRigidParams -> xnext [K,nx], F = [A | B] [K,nx,nx+4] or None."""
        K, nx = x.shape
        dt = x.dtype
        xn = torch.empty(K, nx, dtype=dt, device=x.device)
        F = torch.empty(K, nx, nx + 4, dtype=dt, device=x.device) if want_jac else None
        name = {"rex": "alqp_dyn_rexquadrotor_", "flycart": "alqp_dyn_flyingcartpole_"}[model]
        if nx != {"rex": 12, "flycart": 14}[model] or u.shape != (K, 4):
            raise ValueError(f"mi_alqp: {model} dynamics take x [K,{ {'rex': 12, 'flycart': 14}[model] }] and u [K,4]")
        rc = getattr(self.lib, name + _dt(x))(K, C.byref(params), _ptr(x, "x", dt), _ptr(u, "u", dt), float(h),
                                             _ptr(xn, "xnext", dt), _ptr(F, "F", dt, True), _stream())
        _lib.check(rc, name)
        return xn, F

    def exit_test(self, sumsq, ctl, mode, tol=1e-3):
        """Device-side batch-global exit test (alqp_exit_test): sumsq 0-d/1-elem float64 tensor,
        ctl float64[3] = {done, steps, old_norm}; nothing is synchronised."""
        rc = self.lib.alqp_exit_test(_ptr(sumsq, "sumsq", torch.float64), _ptr(ctl, "ctl", torch.float64),
                                     int(mode), float(tol), _stream())
        _lib.check(rc, "alqp_exit_test")

    @staticmethod
    def _obs_struct(obs, dims, dt):
        """obs = (pos [B,T,nobs,3] tensor, radius float) -> AlqpObstacles (Obstacle_MPC rows)."""
        if isinstance(obs, str) and obs == "state_estimator":     # that variant's row set and gradient, no obstacle rows
            return _lib.AlqpObstacles(None, 0.0, 0, 1)
        pos, radius = obs
        B, T = dims[0], dims[1]
        if pos.dim() != 4 or pos.shape[0] != B or pos.shape[1] != T or pos.shape[3] != 3:
            raise ValueError(f"mi_alqp: obstacle centres must be [B,T,nobs,3], got {tuple(pos.shape)}")
        return _lib.AlqpObstacles(_ptr(pos, "obstacle centres", dt).value, float(radius), int(pos.shape[2]), 0)

    def newton_step(self, dims, z, xnext, F, x0, lam, rho, Qd, q, ulo, uhi, sb_u, st_u, d_out,
                    g_out=None, factor=None, info=None, obs=None, workspace=None):
        """workspace: a quad-variant workspace tensor -> the quad kernels (16 instances per wavefront,
        the factor stays in the workspace records for backward_ws); None -> the team kernel
        (one instance per lane team, optional packed `factor`). obs: obstacle rows / the state-estimator row set."""
        B, T, nx, nu = dims
        dt = z.dtype
        sfx = _dt(z)
        d = _lib.AlqpDims(B, T, nx, nu)
        need = 0
        if workspace is not None:
            if factor is not None:
                raise ValueError("mi_alqp: the quad Newton step leaves its factor in the workspace records (no packed factor)")
            need = self.workspace_bytes(*dims, dt)
            if workspace.numel() * workspace.element_size() < need:
                raise ValueError("mi_alqp: workspace too small")
        o = self._obs_struct(obs, dims, dt) if obs is not None else None
        rc = getattr(self.lib, "alqp_newton_step_" + sfx)(
            C.byref(d), _ptr(z, "z", dt), _ptr(xnext, "xnext", dt), _ptr(F, "F", dt), _ptr(x0, "x0", dt),
            _ptr(lam, "lam", dt), _ptr(rho, "rho", dt), _ptr(Qd, "Qd", dt), _ptr(q, "q", dt),
            _ptr(ulo, "u_lower", dt), _ptr(uhi, "u_upper", dt), sb_u, st_u, C.byref(o) if o is not None else None,
            _ptr(workspace, "workspace", dt, True), need, _ptr(d_out, "d_out", dt), _ptr(g_out, "g_out", dt, True),
            _ptr(factor, "factor", dt, True), _ptr(info, "info", torch.int32, True), _stream())
        _lib.check(rc, "alqp_newton_step_" + sfx)
        self.last_step_kernel = "k_newton_step" if workspace is None else "k_newton_step_quad"

    def merit(self, dims, K, zc, xnext, x0, lam, rho, Qd, q, ulo, uhi, sb_u, st_u, phi, rnorm2=None, obs=None):
        B, T, nx, nu = dims
        dt = zc.dtype
        sfx = _dt(zc)
        d = _lib.AlqpDims(B, T, nx, nu)
        o = self._obs_struct(obs, dims, dt) if obs is not None else None
        rc = getattr(self.lib, "alqp_merit_" + sfx)(
            C.byref(d), K, _ptr(zc, "zc", dt), _ptr(xnext, "xnext", dt), _ptr(x0, "x0", dt),
            _ptr(lam, "lam", dt), _ptr(rho, "rho", dt), _ptr(Qd, "Qd", dt), _ptr(q, "q", dt),
            _ptr(ulo, "u_lower", dt), _ptr(uhi, "u_upper", dt), sb_u, st_u, C.byref(o) if o is not None else None,
            _ptr(phi, "phi", dt), _ptr(rnorm2, "rnorm2", dt, True), _stream())
        _lib.check(rc, "alqp_merit_" + sfx)

    def merit_pick(self, dims, n_ls, d, xnext_all, x0, lam, rho, Qd, q, ulo, uhi, sb_u, st_u, z, phi_prev,
                   rnorm2=None, phi_all=None, k_out=None, accept_out=None, obs=None):
        """The line search of one Newton step in one launch (alqp_merit_pick): merits of z + 2^-k d from the
        caller's x_next of every candidate, decision, z and phi_prev updated in place."""
        B, T, nx, nu = dims
        dt = z.dtype
        sfx = _dt(z)
        dd = _lib.AlqpDims(B, T, nx, nu)
        o = self._obs_struct(obs, dims, dt) if obs is not None else None
        rc = getattr(self.lib, "alqp_merit_pick_" + sfx)(
            C.byref(dd), n_ls, _ptr(d, "d", dt), _ptr(xnext_all, "xnext_all", dt), _ptr(x0, "x0", dt),
            _ptr(lam, "lam", dt), _ptr(rho, "rho", dt), _ptr(Qd, "Qd", dt), _ptr(q, "q", dt),
            _ptr(ulo, "u_lower", dt), _ptr(uhi, "u_upper", dt), sb_u, st_u, C.byref(o) if o is not None else None,
            _ptr(z, "z", dt), _ptr(phi_prev, "phi_prev", dt), _ptr(rnorm2, "rnorm2", dt, True),
            _ptr(phi_all, "phi_all", dt, True), _ptr(k_out, "k_out", torch.int32, True),
            _ptr(accept_out, "accept_out", torch.int32, True), _stream())
        _lib.check(rc, "alqp_merit_pick_" + sfx)

    def linesearch_pick(self, dims, n_ls, phi, phi_prev, d, z, k_out=None, accept_out=None):
        B, T, nx, nu = dims
        dt = z.dtype
        sfx = _dt(z)
        dd = _lib.AlqpDims(B, T, nx, nu)
        fn = getattr(self.lib, "alqp_linesearch_pick_" + sfx)
        rc = fn(C.byref(dd), n_ls, _ptr(phi, "phi", dt), _ptr(phi_prev, "phi_prev", dt),
                _ptr(d, "d", dt), _ptr(z, "z", dt), _ptr(k_out, "k_out", torch.int32, True),
                _ptr(accept_out, "accept_out", torch.int32, True), _stream())
        _lib.check(rc, "alqp_linesearch_pick_" + sfx)

    def dual_update(self, dims, z, xnext, x0, ulo, uhi, sb_u, st_u, lam, rho, rho_scale=10.0, obs=None):
        B, T, nx, nu = dims
        dt = z.dtype
        sfx = _dt(z)
        d = _lib.AlqpDims(B, T, nx, nu)
        o = self._obs_struct(obs, dims, dt) if obs is not None else None
        rc = getattr(self.lib, "alqp_dual_update_" + sfx)(
            C.byref(d), _ptr(z, "z", dt), _ptr(xnext, "xnext", dt), _ptr(x0, "x0", dt), _ptr(ulo, "u_lower", dt),
            _ptr(uhi, "u_upper", dt), sb_u, st_u, C.byref(o) if o is not None else None, _ptr(lam, "lam", dt),
            _ptr(rho, "rho", dt), rho_scale, _stream())
        _lib.check(rc, "alqp_dual_update_" + sfx)

    # -- the same four with more rows per stage and / or a dense stage cost, for MPC with a callable dx. Three families of
    # entry points: alqp_*_xbox (state box rows; x_lower=, x_upper=), alqp_*_rows (general rows, with or without state box
    # rows; ineqG=, ineqh=) and alqp_*_dense (a dense stage cost, with or without either; diag_cost=False). One private method
    # per call shape, the named methods below are its callers. fam: "xbox", "rows" or "dense"; cost: Qd, or C for "dense";
    # xbnd = (xlo, xhi, sb_x, st_x) or None; poly = (G, h, m, sb_g, st_g, sb_h, st_h) or None. The dual update reads no
    # cost: dual_update, _xbox or _rows ------------------------------------------------------------------------------------
    def _fam_cargs(self, fam, dims, lam, cost, xbnd, poly, dt):
        """_row_checks, then the family's C arguments behind st_u: from x_lo to st_x (xbox) or to st_h."""
        rows = self._rows_cargs(self._row_checks(dims, lam, cost if fam == "dense" else None, xbnd, poly), dt)
        return rows[:4] if fam == "xbox" else rows

    def _step_fam(self, fam, dims, z, xnext, F, x0, lam, rho, cost, q, ulo, uhi, sb_u, st_u, xbnd, poly, d_out, g_out, factor,
                  info):
        dt = z.dtype
        name = f"alqp_newton_step_{fam}_" + _dt(z)
        rows = self._fam_cargs(fam, dims, lam, cost, xbnd, poly, dt)
        d = _lib.AlqpDims(*dims)
        rc = getattr(self.lib, name)(
            C.byref(d), _ptr(z, "z", dt), _ptr(xnext, "xnext", dt), _ptr(F, "F", dt), _ptr(x0, "x0", dt),
            _ptr(lam, "lam", dt), _ptr(rho, "rho", dt),
            _ptr(cost, "C" if fam == "dense" else "Qd", dt), _ptr(q, "q", dt),
            _ptr(ulo, "u_lower", dt), _ptr(uhi, "u_upper", dt), sb_u, st_u, *rows, _ptr(d_out, "d_out", dt),
            _ptr(g_out, "g_out", dt, True), _ptr(factor, "factor", dt, True), _ptr(info, "info", torch.int32, True),
            _stream())
        _lib.check(rc, name)
        self.last_step_kernel = "k_newton_step_" + fam

    def _merit_fam(self, fam, dims, K, zc, xnext, x0, lam, rho, cost, q, ulo, uhi, sb_u, st_u, xbnd, poly, phi, rnorm2):
        dt = zc.dtype
        name = f"alqp_merit_{fam}_" + _dt(zc)
        rows = self._fam_cargs(fam, dims, lam, cost, xbnd, poly, dt)
        d = _lib.AlqpDims(*dims)
        rc = getattr(self.lib, name)(
            C.byref(d), K, _ptr(zc, "zc", dt), _ptr(xnext, "xnext", dt), _ptr(x0, "x0", dt),
            _ptr(lam, "lam", dt), _ptr(rho, "rho", dt),
            _ptr(cost, "C" if fam == "dense" else "Qd", dt), _ptr(q, "q", dt),
            _ptr(ulo, "u_lower", dt), _ptr(uhi, "u_upper", dt), sb_u, st_u, *rows, _ptr(phi, "phi", dt),
            _ptr(rnorm2, "rnorm2", dt, True), _stream())
        _lib.check(rc, name)

    def _merit_pick_fam(self, fam, dims, n_ls, d, xnext_all, x0, lam, rho, cost, q, ulo, uhi, sb_u, st_u, xbnd, poly, z,
                        phi_prev, rnorm2, phi_all, k_out, accept_out):
        dt = z.dtype
        name = f"alqp_merit_pick_{fam}_" + _dt(z)
        rows = self._fam_cargs(fam, dims, lam, cost, xbnd, poly, dt)
        dd = _lib.AlqpDims(*dims)
        rc = getattr(self.lib, name)(
            C.byref(dd), n_ls, _ptr(d, "d", dt), _ptr(xnext_all, "xnext_all", dt), _ptr(x0, "x0", dt),
            _ptr(lam, "lam", dt), _ptr(rho, "rho", dt),
            _ptr(cost, "C" if fam == "dense" else "Qd", dt), _ptr(q, "q", dt),
            _ptr(ulo, "u_lower", dt), _ptr(uhi, "u_upper", dt), sb_u, st_u, *rows, _ptr(z, "z", dt),
            _ptr(phi_prev, "phi_prev", dt), _ptr(rnorm2, "rnorm2", dt, True), _ptr(phi_all, "phi_all", dt, True),
            _ptr(k_out, "k_out", torch.int32, True), _ptr(accept_out, "accept_out", torch.int32, True), _stream())
        _lib.check(rc, name)

    def _dual_fam(self, fam, dims, z, xnext, x0, ulo, uhi, sb_u, st_u, xbnd, poly, lam, rho, rho_scale):
        dt = z.dtype
        name = f"alqp_dual_update_{fam}_" + _dt(z)
        rows = self._fam_cargs(fam, dims, lam, None, xbnd, poly, dt)
        d = _lib.AlqpDims(*dims)
        rc = getattr(self.lib, name)(
            C.byref(d), _ptr(z, "z", dt), _ptr(xnext, "xnext", dt), _ptr(x0, "x0", dt), _ptr(ulo, "u_lower", dt),
            _ptr(uhi, "u_upper", dt), sb_u, st_u, *rows, _ptr(lam, "lam", dt), _ptr(rho, "rho", dt), rho_scale,
            _stream())
        _lib.check(rc, name)

    def newton_step_xbox(self, dims, z, xnext, F, x0, lam, rho, Qd, q, ulo, uhi, sb_u, st_u, xbnd, d_out,
                         g_out=None, factor=None, info=None):
        """newton_step with state box rows (alqp_newton_step_xbox): xbnd = (xlo, xhi, sb_x, st_x) as solve_lin_xbox takes
        them, lam [B, T nx + T (2 nu + 2 nx)]. The team kernel at any batch (no workspace), optional packed `factor`."""
        self._step_fam("xbox", dims, z, xnext, F, x0, lam, rho, Qd, q, ulo, uhi, sb_u, st_u, xbnd, None, d_out, g_out,
                       factor, info)

    def merit_xbox(self, dims, K, zc, xnext, x0, lam, rho, Qd, q, ulo, uhi, sb_u, st_u, xbnd, phi, rnorm2=None):
        """merit with state box rows (alqp_merit_xbox); xbnd and lam as newton_step_xbox."""
        self._merit_fam("xbox", dims, K, zc, xnext, x0, lam, rho, Qd, q, ulo, uhi, sb_u, st_u, xbnd, None, phi, rnorm2)

    def merit_pick_xbox(self, dims, n_ls, d, xnext_all, x0, lam, rho, Qd, q, ulo, uhi, sb_u, st_u, xbnd, z, phi_prev,
                        rnorm2=None, phi_all=None, k_out=None, accept_out=None):
        """merit_pick with state box rows (alqp_merit_pick_xbox); xbnd and lam as newton_step_xbox."""
        self._merit_pick_fam("xbox", dims, n_ls, d, xnext_all, x0, lam, rho, Qd, q, ulo, uhi, sb_u, st_u, xbnd, None, z,
                             phi_prev, rnorm2, phi_all, k_out, accept_out)

    def dual_update_xbox(self, dims, z, xnext, x0, ulo, uhi, sb_u, st_u, xbnd, lam, rho, rho_scale=10.0):
        """dual_update with state box rows (alqp_dual_update_xbox); xbnd and lam as newton_step_xbox."""
        self._dual_fam("xbox", dims, z, xnext, x0, ulo, uhi, sb_u, st_u, xbnd, None, lam, rho, rho_scale)

    def newton_step_rows(self, dims, z, xnext, F, x0, lam, rho, Qd, q, ulo, uhi, sb_u, st_u, xbnd, poly, d_out,
                         g_out=None, factor=None, info=None):
        """newton_step with general rows (alqp_newton_step_rows): poly = (G, h, m, sb_g, st_g, sb_h, st_h) as
        solve_lin_poly takes them, xbnd = (xlo, xhi, sb_x, st_x) or None (no state bounds),
        lam [B, T nx + T (2 nu + [2 nx] + m)]. The team kernel at any batch (no workspace), optional packed `factor`."""
        self._step_fam("rows", dims, z, xnext, F, x0, lam, rho, Qd, q, ulo, uhi, sb_u, st_u, xbnd, poly, d_out, g_out,
                       factor, info)

    def merit_rows(self, dims, K, zc, xnext, x0, lam, rho, Qd, q, ulo, uhi, sb_u, st_u, xbnd, poly, phi, rnorm2=None):
        """merit with general rows (alqp_merit_rows); xbnd, poly and lam as newton_step_rows."""
        self._merit_fam("rows", dims, K, zc, xnext, x0, lam, rho, Qd, q, ulo, uhi, sb_u, st_u, xbnd, poly, phi, rnorm2)

    def merit_pick_rows(self, dims, n_ls, d, xnext_all, x0, lam, rho, Qd, q, ulo, uhi, sb_u, st_u, xbnd, poly, z,
                        phi_prev, rnorm2=None, phi_all=None, k_out=None, accept_out=None):
        """merit_pick with general rows (alqp_merit_pick_rows); xbnd, poly and lam as newton_step_rows."""
        self._merit_pick_fam("rows", dims, n_ls, d, xnext_all, x0, lam, rho, Qd, q, ulo, uhi, sb_u, st_u, xbnd, poly, z,
                             phi_prev, rnorm2, phi_all, k_out, accept_out)

    def dual_update_rows(self, dims, z, xnext, x0, ulo, uhi, sb_u, st_u, xbnd, poly, lam, rho, rho_scale=10.0):
        """dual_update with general rows (alqp_dual_update_rows); xbnd, poly and lam as newton_step_rows."""
        self._dual_fam("rows", dims, z, xnext, x0, ulo, uhi, sb_u, st_u, xbnd, poly, lam, rho, rho_scale)

    def newton_step_dense(self, dims, z, xnext, F, x0, lam, rho, Cs, q, ulo, uhi, sb_u, st_u, xbnd, poly, d_out,
                          g_out=None, factor=None, info=None):
        """newton_step with a dense stage cost (alqp_newton_step_dense): Cs [B,T,n,n], symmetric, in place of Qd;
        xbnd = (xlo, xhi, sb_x, st_x) or None, poly = (G, h, m, sb_g, st_g, sb_h, st_h) or None,
        lam [B, T nx + T (2 nu + [2 nx] + [m])]. The team kernel at any batch (no workspace), optional packed `factor`."""
        self._step_fam("dense", dims, z, xnext, F, x0, lam, rho, Cs, q, ulo, uhi, sb_u, st_u, xbnd, poly, d_out, g_out,
                       factor, info)

    def merit_dense(self, dims, K, zc, xnext, x0, lam, rho, Cs, q, ulo, uhi, sb_u, st_u, xbnd, poly, phi, rnorm2=None):
        """merit with a dense stage cost (alqp_merit_dense); Cs, xbnd, poly and lam as newton_step_dense."""
        self._merit_fam("dense", dims, K, zc, xnext, x0, lam, rho, Cs, q, ulo, uhi, sb_u, st_u, xbnd, poly, phi, rnorm2)

    def merit_pick_dense(self, dims, n_ls, d, xnext_all, x0, lam, rho, Cs, q, ulo, uhi, sb_u, st_u, xbnd, poly, z,
                         phi_prev, rnorm2=None, phi_all=None, k_out=None, accept_out=None):
        """merit_pick with a dense stage cost (alqp_merit_pick_dense); Cs, xbnd, poly and lam as newton_step_dense."""
        self._merit_pick_fam("dense", dims, n_ls, d, xnext_all, x0, lam, rho, Cs, q, ulo, uhi, sb_u, st_u, xbnd, poly, z,
                             phi_prev, rnorm2, phi_all, k_out, accept_out)

    def _backward(self, dims, factor, workspace, ws_bytes, F, rho, z_final, gbar, q_grad, Qd_grad, dyn):
        """alqp_backward_*: `factor` or `workspace` is a device pointer, the other None."""
        dt = gbar.dtype
        name = "alqp_backward_" + _dt(gbar)
        d = _lib.AlqpDims(*dims)
        dy = _dyn_args(dyn, dims, dt)
        rc = getattr(self.lib, name)(
            C.byref(d), factor, workspace, ws_bytes, _ptr(F, "F", dt), _ptr(rho, "rho", dt),
            _ptr(z_final, "z_final", dt), _ptr(gbar, "gbar", dt), _ptr(q_grad, "q_grad", dt),
            _ptr(Qd_grad, "Qd_grad", dt), C.byref(dy) if dy is not None else None, _stream())
        _lib.check(rc, name)

    def backward(self, dims, factor, F, rho, z_final, gbar, q_grad, Qd_grad, dyn=None):
        """w = -H^{-1} gbar with the packed factor -> q_grad, Qd_grad; with dyn (a DynGrads) also dF / dc / dx0."""
        self._backward(dims, _ptr(factor, "factor", gbar.dtype), None, 0, F, rho, z_final, gbar, q_grad, Qd_grad, dyn)

    def new_workspace_nonlin(self, dims, like):
        """A private workspace for nonlinear fused solves: [records | F linearisations]."""
        B, T, nx, nu = dims
        d = _lib.AlqpDims(B, T, nx, nu)
        need = int(self.lib.alqp_workspace_bytes_nonlin(C.byref(d), int(like.dtype == torch.float64)))
        return torch.empty(need // like.element_size() + 16, dtype=like.dtype, device=like.device)

    def nonlin_F_view(self, ws, dims):
        """The F region of a nonlinear workspace as a [B, T-1, nx, n] tensor (the linearisation of the
        last executed Newton step, next to its factor in the records)."""
        B, T, nx, nu = dims
        off = self.workspace_bytes(B, T, nx, nu, ws.dtype) // ws.element_size()
        return ws[off:off + B * (T - 1) * nx * (nx + nu)].view(B, T - 1, nx, nx + nu)

    def new_workspace(self, dims, like):
        """A private workspace for one quad solve whose factor will be used by backward_ws."""
        need = self.workspace_bytes(*dims, like.dtype)
        return torch.empty(need // like.element_size() + 16, dtype=like.dtype, device=like.device)

    def backward_ws(self, dims, workspace, F, rho, z_final, gbar, q_grad, Qd_grad, dyn=None):
        """The same with the factor a quad solve or quad Newton step left in `workspace`."""
        self._backward(dims, None, _ptr(workspace, "workspace", gbar.dtype), self.workspace_bytes(*dims, gbar.dtype),
                       F, rho, z_final, gbar, q_grad, Qd_grad, dyn)

    # ---- interior-point path (csrc/alqp_ipm.hip) -------------------------------------------------
    def _ipm_ws(self, dims, like):
        d = _lib.AlqpDims(*dims)
        need = int(self.lib.alqp_ipm_workspace_bytes(C.byref(d), int(like.dtype == torch.float64)))
        if need == 0:
            raise RuntimeError(f"mi_alqp: no interior-point kernel instance for (nx={dims[2]}, nu={dims[3]})")
        return self._scratch(("ipm", like.device, like.dtype), need // like.element_size(), like.dtype, like.device, 16), need

    ipm_variant = "auto"   # default kernel of ipm_solve / ipm_backward: a key of _lib.IPM_VARIANTS (include/mi_alqp.h)

    def ipm_solve(self, dims, Cd, c, F, f, x0, uhi, ulo, exit_mode="reference", eps=1e-12, not_improved_lim=3,
                  max_iter=20, ry_fn=None, kkt_eps=1e-7, process_group=None, sharded=False, variant=None):
        """pdipm_b_LU.forward (batch_LU.py:29-197) on time-major data: Cd, c [T,B,n]; F [T-1,B,nx,n];
        f [T-1,B,nx]; x0 [B,nx]; uhi, ulo [nu]. ry_fn(z [B,T*n]) -> [B,T*nx]: equality residual of the TRUE
        dynamics (one launch per iteration, PyTorch call in between), or None for A z - b.
        exit_mode "fixed" (and no ry_fn): ONE launch for the whole solve. "reference": the reference's
        batch-global exit rule, one host read per iteration (the reference syncs there as well); with `sharded`
        the three batch-global quantities are max-reduced over the ranks of `process_group` first.
        variant: "auto" (the register/LDS-resident kernel when T <= 20, else the generic one), "generic_lds",
        "generic_ws", "resident" (AlqpIpmParams.variant); None: self.ipm_variant."""
        vnum = _lib.IPM_VARIANTS[variant or self.ipm_variant]
        B, T, nx, nu = dims
        n = nx + nu
        dt, dev = c.dtype, c.device
        sfx = _dt(c)
        d = _lib.AlqpDims(B, T, nx, nu)
        ws, need = self._ipm_ws(dims, c)
        out = {"zhat": torch.empty(B, T * n, dtype=dt, device=dev), "nus": torch.empty(B, T * nx, dtype=dt, device=dev),
               "lams": torch.empty(B, 2 * T * nu, dtype=dt, device=dev),
               "slacks": torch.empty(B, 2 * T * nu, dtype=dt, device=dev),
               "resid": torch.empty(B, dtype=dt, device=dev), "info": torch.zeros(B, dtype=torch.int32, device=dev)}
        mu = torch.empty(B, dtype=dt, device=dev)
        improved = torch.zeros(B, dtype=torch.int32, device=dev)
        fn = getattr(self.lib, "alqp_ipm_solve_" + sfx)
        ptrs = (_ptr(Cd, "Cd", dt), _ptr(c, "c", dt), _ptr(F, "F", dt), _ptr(f, "f", dt), _ptr(x0, "x0", dt),
                _ptr(uhi, "u_upper", dt), _ptr(ulo, "u_lower", dt), B * n, n, B * nx * n, nx * n, B * nx, nx)

        def launch(flags, iters=0, it0=0, ry=None):
            p = _lib.AlqpIpmParams(flags, iters, it0, kkt_eps, vnum)
            rc = fn(C.byref(d), C.byref(p), *ptrs, _ptr(ws, "workspace", dt), need, _ptr(ry, "ry", dt, True),
                    _ptr(out["zhat"], "zhat", dt), _ptr(out["nus"], "nus", dt), _ptr(out["lams"], "lams", dt),
                    _ptr(out["slacks"], "slacks", dt), _ptr(out["resid"], "resid", dt), _ptr(mu, "mu", dt), None,
                    _ptr(improved, "improved", torch.int32), _ptr(out["info"], "info", torch.int32), _stream())
            _lib.check(rc, "alqp_ipm_solve_" + sfx)

        if exit_mode == "fixed" and ry_fn is None:
            launch(_lib.ALQP_IPM_INIT | _lib.ALQP_IPM_LOOP | _lib.ALQP_IPM_FINAL, max_iter)
            out["iters"] = max_iter
            return out
        launch(_lib.ALQP_IPM_INIT)
        ws_words = need // c.element_size() // B
        cur_x = ws[:B * ws_words].view(B, ws_words)[:, :T * n]      # the iterate's x block of every instance
        n_not_improved, done = 0, max_iter
        for it in range(max_iter):
            ry = ry_fn(cur_x.contiguous()).to(dt).contiguous() if ry_fn is not None else None
            launch(_lib.ALQP_IPM_RESID, 0, it, ry)
            if exit_mode == "reference":
                # batch_LU.py:120-151: nNotImproved counts iterations in which NO instance improved
                glob = torch.stack((improved.max().to(torch.float64), out["resid"].max().to(torch.float64),
                                    -mu.min().to(torch.float64)))
                if sharded:
                    torch.distributed.all_reduce(glob, op=torch.distributed.ReduceOp.MAX, group=process_group)
                any_imp, best_max, mu_min = glob.tolist()
                mu_min = -mu_min
                n_not_improved = 0 if (it == 0 or any_imp > 0) else n_not_improved + 1
                if n_not_improved == not_improved_lim or best_max < eps or mu_min > 1e32:
                    done = it
                    break
            launch(_lib.ALQP_IPM_STEP, 0, it)
        launch(_lib.ALQP_IPM_FINAL)
        out["iters"] = done
        return out

    def ipm_backward(self, dims, Cd, F, lams, slacks, g, variant=None):
        """DenseQPFunction.backward's KKT solve (qp.py:243-252) -> dx [B,T*n], dlam [B,2*T*nu], dnu [B,T*nx]."""
        vnum = _lib.IPM_VARIANTS[variant or self.ipm_variant]
        B, T, nx, nu = dims
        n = nx + nu
        dt, dev = g.dtype, g.device
        sfx = _dt(g)
        d = _lib.AlqpDims(B, T, nx, nu)
        ws, need = self._ipm_ws(dims, g)
        dx = torch.empty(B, T * n, dtype=dt, device=dev)
        dlam = torch.empty(B, 2 * T * nu, dtype=dt, device=dev)
        dnu = torch.empty(B, T * nx, dtype=dt, device=dev)
        fn = getattr(self.lib, "alqp_ipm_backward_" + sfx)
        rc = fn(C.byref(d), _ptr(Cd, "Cd", dt), _ptr(F, "F", dt), B * n, n, B * nx * n, nx * n, _ptr(lams, "lams", dt),
                _ptr(slacks, "slacks", dt), _ptr(g, "gbar", dt), _ptr(ws, "workspace", dt), need, _ptr(dx, "dx", dt),
                _ptr(dlam, "dlam", dt), _ptr(dnu, "dnu", dt), None, vnum, _stream())
        _lib.check(rc, "alqp_ipm_backward_" + sfx)
        return dx, dlam, dnu


_default = None


def default_backend():
    global _default
    if _default is None:
        _default = HipBackend()
    return _default
