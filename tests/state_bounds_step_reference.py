"""TEST-ONLY reference for the state box rows on the callable-dynamics route (MPC(x_lower=, x_upper=) with a callable
dx; alqp_newton_step_xbox, alqp_merit_xbox, alqp_merit_pick_xbox, alqp_dual_update_xbox): XboxOracleBackend plus the four
`_xbox` methods, composed the way its `solve_lin_xbox` is. The oracle sees the plain problem and the plain part of lam
(OracleBackend.merit / dual_update / linesearch_pick, orc.grad_hess + orc.newton_dir as OracleBackend.newton_step calls
them); the state rows' terms come from state_bounds_reference.box_rows, and the only arithmetic here is the sum of the two.

Also here: a small nonlinear plant usable at any (nx, nu) with its analytic Jacobian, and the problems the CPU and GPU
tests of the route share."""
import numpy as np
import torch

from oracle import oracle_py as orc
from tests import state_bounds_reference as sbr
from tests.oracle_backend import OracleBackend, _bounds, _n, _sfx
from tests.state_bounds_reference import XboxOracleBackend, box_rows, join_lam, lam_width, split_lam


def _t(a, like):
    return torch.from_numpy(np.ascontiguousarray(a)).to(like.dtype)


class XboxStepOracleBackend(XboxOracleBackend):
    name = "oracle-test-xbox-step"

    @staticmethod
    def _split(dims, lam, xbnd):
        """-> plain lam (tensor, CPU), lam_xu, lam_xl (numpy [B,T,nx]), xlo, xhi (numpy, broadcastable to [B,T,nx])."""
        B, T, nx, nu = dims
        assert tuple(lam.shape) == (B, lam_width(T, nx, nu)), tuple(lam.shape)
        xlo, xhi, sb_x, st_x = xbnd
        plain, lxu, lxl = split_lam(_n(lam), T, nx, nu)
        xl, xh = sbr._xbounds(xlo, xhi, sb_x, st_x, B, T, nx)
        assert np.isfinite(xl).all() and np.isfinite(xh).all(), "the host hands the kernels finite bounds"
        return torch.from_numpy(plain), lxu, lxl, xl, xh

    def newton_step_xbox(self, dims, z, xnext, F, x0, lam, rho, Qd, q, ulo, uhi, sb_u, st_u, xbnd, d_out, g_out=None,
                         factor=None, info=None):
        self.calls.append("newton_step_xbox")
        B, T, nx, nu = dims
        s = _sfx(z)
        lo, hi = _bounds(ulo, uhi, sb_u, st_u, B, T, nu)
        plain, lxu, lxl, xl, xh = self._split(dims, lam, xbnd)
        g, Hd, Hs = sbr.grad_hess_xbox(s, _n(z), _n(xnext), _n(F), _n(x0), _n(plain), lxu, lxl, _n(rho), _n(Qd), _n(q),
                                       lo, hi, xl, xh)
        d, inf, L, _ = orc.newton_dir(s, g, Hd, Hs, nx, want_factor=True)
        self.last_hessian = (Hd, Hs)
        d_out.copy_(torch.from_numpy(d))
        if g_out is not None:
            g_out.copy_(torch.from_numpy(g))
        if factor is not None:
            factor.copy_(torch.from_numpy(self._pack_X(L)))
        if info is not None:
            cur = _n(info)
            info.copy_(torch.from_numpy(np.where(cur == 0, inf, cur).astype(np.int32)))

    def merit_xbox(self, dims, K, zc, xnext, x0, lam, rho, Qd, q, ulo, uhi, sb_u, st_u, xbnd, phi, rnorm2=None):
        self.calls.append("merit_xbox")
        B, T, nx, nu = dims
        plain, lxu, lxl, xl, xh = self._split(dims, lam, xbnd)
        r2 = torch.empty(K, B, dtype=zc.dtype)
        OracleBackend.merit(self, dims, K, zc, xnext, x0, plain, rho, Qd, q, ulo, uhi, sb_u, st_u, phi, r2)
        zc_ = _n(zc).reshape(K, B, T, nx + nu)
        for k in range(K):
            _, _, px, rx, _ = box_rows(zc_[k][..., :nx], xl, xh, lxu, lxl, _n(rho))
            phi.view(K, B)[k].add_(_t(px, phi))
            r2[k].add_(_t(rx, r2))
        if rnorm2 is not None:
            rnorm2.view(K, B).copy_(r2)

    def merit_pick_xbox(self, dims, n_ls, d, xnext_all, x0, lam, rho, Qd, q, ulo, uhi, sb_u, st_u, xbnd, z, phi_prev,
                        rnorm2=None, phi_all=None, k_out=None, accept_out=None):
        """OracleBackend.merit_pick with merit_xbox in place of merit."""
        self.calls.append("merit_pick_xbox")
        B, T, nx, nu = dims
        alphas = (2.0 ** -torch.arange(n_ls, dtype=z.dtype)).view(n_ls, 1, 1, 1)
        zc = (z.unsqueeze(0) + alphas * d.unsqueeze(0)).contiguous()
        phis = torch.empty(n_ls, B, dtype=z.dtype)
        rn2s = torch.empty(n_ls, B, dtype=z.dtype)
        self.merit_xbox(dims, n_ls, zc, xnext_all, x0, lam, rho, Qd, q, ulo, uhi, sb_u, st_u, xbnd, phis, rn2s)
        self.calls.pop()
        kk = torch.zeros(B, dtype=torch.int32)
        acc = torch.zeros(B, dtype=torch.int32)
        self.linesearch_pick(dims, n_ls, phis, phi_prev, d, z, kk, acc)
        if rnorm2 is not None:
            rnorm2.copy_(torch.where(acc.bool(), rn2s.gather(0, kk.long().unsqueeze(0)).squeeze(0), rnorm2))
        if phi_all is not None:
            phi_all.copy_(phis)
        if k_out is not None:
            k_out.copy_(kk)
        if accept_out is not None:
            accept_out.copy_(acc)

    def dual_update_xbox(self, dims, z, xnext, x0, ulo, uhi, sb_u, st_u, xbnd, lam, rho, rho_scale=10.0):
        self.calls.append("dual_update_xbox")
        B, T, nx, nu = dims
        plain, lxu, lxl, xl, xh = self._split(dims, lam, xbnd)
        _, _, _, _, (nxu, nxl) = box_rows(_n(z)[..., :nx], xl, xh, lxu, lxl, _n(rho))   # (with the rho before its growth)
        OracleBackend.dual_update(self, dims, z, xnext, x0, ulo, uhi, sb_u, st_u, plain, rho, rho_scale)
        lam.copy_(_t(join_lam(_n(plain), nxu, nxl, T, nx, nu), lam))


# ---- a nonlinear plant at any (nx, nu) -------------------------------------------------------------------------------

class SinPlant:
    """x+ = x + h (A x + B u + 0.3 sin x) with seeded A [nx,nx], B [nx,nu]; `jac` returns (x+, (dx+/dx, dx+/du)), the form
    MPC's dx_jac has. Works on tensors of any device and dtype (A, B are moved to the argument's)."""

    def __init__(self, nx, nu, seed=0, h=0.1):
        g = torch.Generator().manual_seed(1000 + seed)
        self.nx, self.nu, self.h = nx, nu, h
        self.A = torch.randn(nx, nx, generator=g, dtype=torch.float64) / np.sqrt(nx) - 0.5 * torch.eye(nx, dtype=torch.float64)
        self.B = torch.randn(nx, nu, generator=g, dtype=torch.float64)

    def _ab(self, x):
        return self.A.to(device=x.device, dtype=x.dtype), self.B.to(device=x.device, dtype=x.dtype)

    def __call__(self, x, u):
        A, B = self._ab(x)
        return x + self.h * (x @ A.T + u @ B.T + 0.3 * torch.sin(x))

    def jac(self, x, u):
        A, B = self._ab(x)
        eye = torch.eye(self.nx, dtype=x.dtype, device=x.device)
        Jx = eye + self.h * (A + 0.3 * torch.diag_embed(torch.cos(x)))
        Ju = (self.h * B).expand(x.shape[0], self.nx, self.nu)
        return self(x, u), (Jx, Ju)


class AffineCallable:
    """An affine (F, f) [B,T-1,nx,n], [B,T-1,nx] wrapped as a callable dx / dx_jac: the route twin of LinDx(F, f). MPC
    calls dx on points flattened as [..., B, T-1]: the stage data are tiled over the leading candidates axis."""

    def __init__(self, F, f):
        self.Fm, self.fv = F, f
        self.B, self.Tm, self.nx, n = F.shape
        self.nu = n - self.nx

    def _at(self, K):
        reps = K // (self.B * self.Tm)
        F = self.Fm.reshape(-1, self.nx, self.nx + self.nu).repeat(reps, 1, 1)
        f = self.fv.reshape(-1, self.nx).repeat(reps, 1)
        return F, f

    def __call__(self, x, u):
        F, f = self._at(x.shape[0])
        return torch.einsum("kij,kj->ki", F.to(x.dtype), torch.cat([x, u], -1)) + f.to(x.dtype)

    def jac(self, x, u):
        F, _ = self._at(x.shape[0])
        F = F.to(x.dtype)
        return self(x, u), (F[..., :self.nx], F[..., self.nx:])


# ---- shared problems ---------------------------------------------------------------------------------------------------

def step_problem(B, T, nx, nu, dtype, per_stage=False, seed=5, width=0.6):
    """The active-bound synthetic problem with state bounds that bind on both sides in every instance (xbox_problem with
    `push`), and the SinPlant of this size: CPU tensors. -> (pr, plant)."""
    pr = sbr.xbox_problem(B, T, nx, nu, dtype, per_stage=per_stage, seed=seed, width=width, push=True)
    return pr, SinPlant(nx, nu, seed=seed)


def bounded_plant_problem(B, T, nx, nu, dtype, width=0.4, seed=5):
    """A problem the SinPlant can satisfy: xbox_problem's cost with state 0 pulled above and state 1 below the box
    |x| <= width on every stage, x0 inside the box, controls |u| <= 2, and the plant's own rollout from x0 under u = 0 as
    the start. -> (pr, plant)."""
    pr = sbr.xbox_problem(B, T, nx, nu, dtype, seed=seed, width=width, push=True)
    plant = SinPlant(nx, nu, seed=seed)
    pr["x0"] = (0.3 * torch.tanh(pr["x0"])).contiguous()
    pr["lo"], pr["hi"] = torch.full((nu,), -2.0, dtype=dtype), torch.full((nu,), 2.0, dtype=dtype)
    z0 = torch.zeros(B, T, nx + nu, dtype=dtype)
    z0[:, 0, :nx] = pr["x0"]
    for t in range(T - 1):
        z0[:, t + 1, :nx] = plant(z0[:, t, :nx], z0[:, t, nx:])
    pr["z0"] = z0
    return pr, plant


def strides(pr):
    B, T, nx, nu = pr["dims"]
    sb_u, st_u = (0, 0) if pr["lo"].dim() == 1 else (T * nu, nu)
    sb_x, st_x = (0, 0) if pr["xlo"].dim() == 1 else (T * nx, nx)
    return sb_u, st_u, sb_x, st_x


def true_next(plant, z, nx):
    """f(x_t, u_t), t < T-1, for z [..., T, n] -> [..., T-1, nx]."""
    xn = plant(z[..., :-1, :nx].reshape(-1, nx), z[..., :-1, nx:].reshape(-1, z.shape[-1] - nx))
    return xn.reshape(*z.shape[:-2], z.shape[-2] - 1, nx).contiguous()


def linearize(plant, z, nx):
    B, T, n = z.shape
    xn, (A, Bm) = plant.jac(z[:, :-1, :nx].reshape(-1, nx), z[:, :-1, nx:].reshape(-1, n - nx))
    F = torch.cat((A.reshape(B, T - 1, nx, nx), Bm.reshape(B, T - 1, nx, n - nx)), -1).contiguous()
    return xn.reshape(B, T - 1, nx).contiguous(), F


def al_iteration(be, pr, plant, z, lam, rho, n_newton=4, n_ls=20, dual=True):
    """One AL iteration of the PyTorch-dynamics route through `be`'s four _xbox methods on tensors of be's device (the
    reference backend: CPU), in place on z, lam, rho: merit, n_newton x (step, pick), dual update."""
    dims = pr["dims"]
    B, T, nx, nu = dims
    sb_u, st_u, sb_x, st_x = strides(pr)
    xb = (pr["xlo"], pr["xhi"], sb_x, st_x)
    prob = (pr["x0"], lam, rho, pr["Qd"], pr["q"], pr["lo"], pr["hi"], sb_u, st_u)
    phi = torch.zeros(B, dtype=z.dtype, device=z.device)
    rn2 = torch.zeros(B, dtype=z.dtype, device=z.device)
    d = torch.empty_like(z)
    be.merit_xbox(dims, 1, z, true_next(plant, z, nx), *prob, xb, phi, rn2)
    alphas = (2.0 ** -torch.arange(n_ls, dtype=z.dtype, device=z.device)).view(n_ls, 1, 1, 1)
    for _ in range(n_newton):
        xn, F = linearize(plant, z, nx)
        be.newton_step_xbox(dims, z, xn, F, *prob, xb, d)
        zc = (z.unsqueeze(0) + alphas * d.unsqueeze(0)).contiguous()
        be.merit_pick_xbox(dims, n_ls, d, true_next(plant, zc, nx), *prob, xb, z, phi, rnorm2=rn2)
    if dual:
        be.dual_update_xbox(dims, z, true_next(plant, z, nx), pr["x0"], pr["lo"], pr["hi"], sb_u, st_u, xb, lam, rho)
    return phi, rn2


def kernel_inputs(pr, plant):
    """lam, rho after ONE reference AL iteration from the problem's start, with the iterate it left: what the GPU tests feed
    every kernel. -> dict(z, lam, rho, xn, F, d) of CPU tensors in the problem's dtype (d: the reference's next direction)."""
    B, T, nx, nu = pr["dims"]
    be = XboxStepOracleBackend()
    z = pr["z0"].clone()
    lam = torch.zeros(B, lam_width(T, nx, nu), dtype=z.dtype)
    rho = torch.ones(B, dtype=z.dtype)
    al_iteration(be, pr, plant, z, lam, rho)
    xn, F = linearize(plant, z, nx)
    sb_u, st_u, sb_x, st_x = strides(pr)
    d = torch.empty_like(z)
    g = torch.empty_like(z)
    be.newton_step_xbox(pr["dims"], z, xn, F, pr["x0"], lam, rho, pr["Qd"], pr["q"], pr["lo"], pr["hi"], sb_u, st_u,
                        (pr["xlo"], pr["xhi"], sb_x, st_x), d, g_out=g)
    return dict(z=z, lam=lam, rho=rho, xn=xn, F=F, d=d, g=g, hessian=be.last_hessian)


def state_rows_active(pr, z, lam):
    """Per instance: (an upper state row active, a lower state row active, a nonzero state-row multiplier)."""
    B, T, nx, nu = pr["dims"]
    ru, rl = sbr.xbox_residuals(pr, z)
    _, lxu, lxl = split_lam(_n(lam), T, nx, nu)
    return ((ru > 0).reshape(B, -1).any(1), (rl > 0).reshape(B, -1).any(1),
            ((lxu > 0) | (lxl > 0)).reshape(B, -1).any(1))


# ---- the GPU tests' cases (tests/test_gpu_state_bounds_step.py; their fp64 reference is checked on the CPU too) ----------
# (nx, nu, T, B, per_stage): the smallest team; NROWS 15 of 16 lanes; pad4(N) == N twice; (13,4); (14,4); the workload's
# horizon. B odd and no multiple of the teams per wavefront at the two sizes with four 16-lane teams per wavefront ((2,1):
# B = 5, a ragged second wavefront; (4,1): B = 3, one padding team). Bounds [nx] in three shapes, [B,T,nx] in four.
GPU_CASES = [(2, 1, 2, 5, False), (4, 1, 3, 3, True), (6, 2, 3, 2, False), (12, 4, 3, 2, True), (13, 4, 3, 2, True),
             (14, 4, 3, 2, False), (13, 4, 20, 2, True)]
GPU_SEED = 5


def gpu_case(nx, nu, T, B, per_stage, dtype):
    """-> (pr, plant, inp): the problem, its plant and kernel_inputs of the case, CPU tensors in `dtype`."""
    pr, plant = step_problem(B, T, nx, nu, dtype, per_stage=per_stage, seed=GPU_SEED)
    return pr, plant, kernel_inputs(pr, plant)


def merit_magnitude_xbox(pr, z, xn, lam, rho, zmag=None):
    """aux_cases.merit_magnitude with the state rows' terms: -> (phi, A, rp2, A2) per instance in float64, A / A2 the
    magnitudes the rounding bound of k_merit_xbox / k_merit_pick_xbox scales with (tests/aux_cases.py: every a - b counts
    |a| + |b|). The state elements add what the control elements add: one bound pair per element of the T*n loop."""
    from tests import aux_cases as ax
    B, T, nx, nu = pr["dims"]
    f = lambda t: t.detach().cpu().double().numpy() if torch.is_tensor(t) else np.asarray(t, np.float64)
    z, xn, lam, rho = f(z), f(xn), f(lam), f(rho).reshape(B)
    plain, lxu, lxl = split_lam(lam, T, nx, nu)
    ulo, uhi = np.broadcast_to(f(pr["lo"]), (B, T, nu)), np.broadcast_to(f(pr["hi"]), (B, T, nu))
    xlo, xhi = np.broadcast_to(f(pr["xlo"]), (B, T, nx)), np.broadcast_to(f(pr["xhi"]), (B, T, nx))
    m = ax.merit_magnitude(z, xn, f(pr["x0"]), plain, rho, f(pr["Qd"]), f(pr["q"]), ulo, uhi, zmag=zmag)
    x = z[..., :nx]
    xm = np.abs(x) if zmag is None else zmag[..., :nx]
    ru, rl = x - xhi, -x + xlo
    um, lm = xm + np.abs(xhi), xm + np.abs(xlo)
    s = lambda a: a.reshape(B, -1).sum(1)
    rp2 = s(np.maximum(ru, 0) ** 2 + np.maximum(rl, 0) ** 2)
    A2 = s(um ** 2 + lm ** 2)
    phi = m.phi + s(lxu * ru + lxl * rl) + 0.5 * rho * rp2
    A = m.A + s(np.abs(lxu) * um + np.abs(lxl) * lm) + 0.5 * np.abs(rho) * A2
    return phi, A, m.rp2 + rp2, m.A2 + A2


def row_terms_numpy(pr, z, xn, lam, rho):
    """A direct float64 statement of the five row terms at (z, xnext, lam, rho), independent of the oracle and of
    box_rows: -> dict(phi [B], rp2 [B], lam_new [B,M])."""
    B, T, nx, nu = pr["dims"]
    n = nx + nu
    f = lambda t: t.detach().cpu().double().numpy()
    z, xn, lam, rho = f(z), f(xn), f(lam), f(rho).reshape(B)
    Qd, q, x0 = f(pr["Qd"]), f(pr["q"]), f(pr["x0"])
    ulo, uhi = np.broadcast_to(f(pr["lo"]), (B, T, nu)), np.broadcast_to(f(pr["hi"]), (B, T, nu))
    xlo, xhi = np.broadcast_to(f(pr["xlo"]), (B, T, nx)), np.broadcast_to(f(pr["xhi"]), (B, T, nx))
    neq, nit = T * nx, 2 * nu + 2 * nx
    phi = np.zeros(B)
    rp2 = np.zeros(B)
    new = lam.copy()
    for b in range(B):
        phi[b] = (0.5 * Qd[b] * z[b] * z[b] + q[b] * z[b]).sum()
        for t in range(T):
            for i in range(nx):
                r = z[b, t + 1, i] - xn[b, t, i] if t < T - 1 else z[b, 0, i] - x0[b, i]
                phi[b] += lam[b, t * nx + i] * r
                rp2[b] += r * r
                new[b, t * nx + i] = lam[b, t * nx + i] + rho[b] * r
            rows = [(j, z[b, t, nx + j] - uhi[b, t, j]) for j in range(nu)]
            rows += [(nu + j, -z[b, t, nx + j] + ulo[b, t, j]) for j in range(nu)]
            rows += [(2 * nu + i, z[b, t, i] - xhi[b, t, i]) for i in range(nx)]
            rows += [(2 * nu + nx + i, -z[b, t, i] + xlo[b, t, i]) for i in range(nx)]
            for k, r in rows:
                m = neq + t * nit + k
                phi[b] += lam[b, m] * r
                rp2[b] += max(r, 0.0) ** 2
                new[b, m] = max(0.0, lam[b, m] + rho[b] * r)
        phi[b] += 0.5 * rho[b] * rp2[b]
    return dict(phi=phi, rp2=rp2, lam_new=new)
