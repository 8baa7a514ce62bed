"""TEST-ONLY helpers for the compiled-in models' one-launch route with state bounds and / or general rows
(alqp_solve_nonlin_rows, HipBackend.solve_nonlin_rows).

The oracle is the CPU route the project already pins: rows_step_reference.RowsStepOracleBackend (which is also the
state-bound backend, XboxStepOracleBackend) driven with `dx` / `dx_jac` that are the model restatements of oracle/dyn_py.py
wrapped as torch callables (OraclePlant). The second yardstick is the launch-per-step GPU route: the same kernels the
parent runs for a provider, reached here through the backend's four launch-per-step methods (al_iteration below with
HipBackend and the provider) or through MPC with the provider wrapped so that it has no fused_id (Plain).

Row mask: 2 state bounds, 4 general rows, 6 both (the library's objects)."""
import numpy as np
import torch

from oracle import dyn_py
from tests import state_bounds_step_reference as ssr
from tests.gen_rows_reference import lam_width
from tests.poly_rows_reference import strides as poly_strides

H_STEP = 0.05
MODELS = {"pendulum1l": (2, 1, 1), "cartpole1l": (4, 1, 2), "cartpole1l_v2": (4, 1, 4)}   # nx, nu, dyn_id
MASKS = (2, 4, 6)
# how far beyond the start the cost pulls every state: far enough that the Newton loop of an AL iteration is still moving at its
# fourth step in float64 (at 0.8 it has converged by then and the oracle's own line search of that step is a tie)
PULL = 10.0


class OraclePlant:
    """x+ = f(x, u) of oracle/dyn_py.py's restatement of the model, as MPC's dx / dx_jac: float64 arithmetic on the CPU,
    results in the arguments' dtype."""

    def __init__(self, model, h=H_STEP):
        self.model, self.h = model, h
        self.nx, self.nu, _ = MODELS[model]

    def _eval(self, x, u):
        xx, uu = x.detach().double().numpy(), u.detach().double().numpy()
        if self.model == "pendulum1l":
            return dyn_py.pendulum1l(xx, uu, self.h)
        fn = dyn_py.cartpole1l if self.model == "cartpole1l" else dyn_py.cartpole1l_v2
        xn, J = fn(xx, np.concatenate([uu, np.zeros_like(uu)], 1), self.h)   # tau = (u, 0)
        return xn, J[:, :, :4], J[:, :, 4:5]

    def __call__(self, x, u):
        return torch.from_numpy(self._eval(x, u)[0]).to(x.dtype)

    def jac(self, x, u):
        xn, A, B = self._eval(x, u)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(x.dtype)
        return t(xn), (t(A), t(B))


def provider(model, h=H_STEP):
    from deq_mpc_corl_amd import dynamics as dy
    return {"pendulum1l": dy.Pendulum1lDynamics, "cartpole1l": dy.Cartpole1lDynamics,
            "cartpole1l_v2": dy.Cartpole1lV2Dynamics}[model](h)


class Plain:
    """A provider without its fused_id: the launch-per-step route (the `Plain` of tests/test_dynamics_provider.py)."""

    def __init__(self, prov):
        self.prov = prov

    def __call__(self, x, u):
        return self.prov(x, u)

    def jac(self, x, u):
        return self.prov.jac(x, u)


def problem(model, B, T, m, per_instance, dtype, seed=11, pull=PULL, h_step=H_STEP):
    """A problem in which every instance stays constrained: the rate state nx-1 starts ABOVE its upper bound (stage 0 is
    pinned to x0, so that state row is active at every iterate and its multiplier grows), the first general row is the
    same bound written as a row, and the further rows (m > 1) are dense, placed around the start like rows_problem's
    (even k violated at the start, odd k slack). The cost pulls every state outward and the control bound is tight, so
    that control rows become active too. Bounds [nx] and rows [m,n], or with `per_instance` [B,T,nx] and [B,T,m,n]. The
    start is the model's own rollout from x0 under small random controls. CPU tensors in `dtype`; -> (pr, plant)."""
    nx, nu, _ = MODELS[model]
    n = nx + nu
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    plant = OraclePlant(model, h_step)
    x0 = 0.4 * rnd(B, nx) - 0.2
    x0[:, nx - 1] = 0.25 + 0.1 * rnd(B)                      # above the bound 0.2 below
    ub = 0.15   # tight: control rows end active in some instance of every case (checked on the oracle)
    z0 = torch.zeros(B, T, n, dtype=torch.float64)
    z0[:, 0, :nx] = x0
    z0[..., nx:] = 0.2 * rnd(B, T, nu) - 0.1
    for t in range(T - 1):
        z0[:, t + 1, :nx] = plant(z0[:, t, :nx], z0[:, t, nx:])
    Qd = torch.ones(B, T, n, dtype=torch.float64)
    Qd[..., :nx] += rnd(B, T, nx)
    Qd[..., nx:] = 0.1
    xref = torch.zeros(B, T, n, dtype=torch.float64)
    xref[..., :nx] = z0[..., :nx] + pull * torch.sign(rnd(B, T, nx) - 0.5)
    xref[..., nx - 1] = z0[..., nx - 1] + pull   # the rate state is pulled UP, against its upper bound, on every stage
    q = -Qd * xref
    q[..., nx:] = 0.3 * (rnd(B, T, nu) - 0.5)
    xhi = torch.full((nx,), 0.6, dtype=torch.float64)
    xhi[nx - 1] = 0.2
    xlo = -xhi.clone()
    xlo[nx - 1] = -0.6
    G = torch.randn(m, n, generator=g, dtype=torch.float64) / n ** 0.5
    G[0] = 0
    G[0, nx - 1] = 1.0
    if per_instance:
        xhi = (xhi + 0.02 * rnd(B, T, nx)).contiguous()
        xlo = (xlo - 0.02 * rnd(B, T, nx)).contiguous()
        G = (G + 0.05 * torch.randn(B, T, m, n, generator=g, dtype=torch.float64) * (torch.arange(m) > 0).view(m, 1)).contiguous()
    gz = torch.einsum("btkj,btj->btk", G.expand(B, T, m, n), z0)
    u_ = rnd(m)
    even = torch.arange(m) % 2 == 0
    s = torch.where(even, 0.05 + 0.1 * u_, -0.3 - 0.3 * u_)
    if per_instance:
        h = (gz - s).contiguous()
    else:
        h = torch.where(even, gz.amin((0, 1)), gz.amax((0, 1))) - s
    h = h.clone()
    h[..., 0] = 0.2 if not per_instance else h[..., 0] * 0 + 0.2 + 0.01 * rnd(B, T)
    c = lambda v: v.to(dtype).contiguous()
    pr = dict(dims=(B, T, nx, nu), x0=c(x0), z0=c(z0), Qd=c(Qd), q=c(q), lo=torch.full((nu,), -ub, dtype=dtype),
              hi=torch.full((nu,), ub, dtype=dtype), xlo=c(xlo), xhi=c(xhi), G=c(G), h=c(h), m=m, model=model, h_step=h_step)
    return pr, plant


def row_args(pr, mask):
    """(sb_u, st_u, xbnd or None, poly or None) for `mask`."""
    B, T, nx, nu = pr["dims"]
    sb_u, st_u, sb_x, st_x = ssr.strides(pr)
    xbnd = (pr["xlo"], pr["xhi"], sb_x, st_x) if mask & 2 else None
    poly = (pr["G"], pr["h"], pr["m"], *poly_strides(pr["G"], pr["h"], T, pr["m"], nx + nu)) if mask & 4 else None
    return sb_u, st_u, xbnd, poly


def lam_cols(pr, mask):
    B, T, nx, nu = pr["dims"]
    return lam_width(T, nx, nu, bool(mask & 2), pr["m"] if mask & 4 else 0)


def to_dev(pr, dev):
    return {k: (v.to(dev).contiguous() if torch.is_tensor(v) else v) for k, v in pr.items()}


def al_iteration(be, pr, plant, mask, z, lam, rho, phi=None, n_newton=4, init=True, dual=True):
    """One AL iteration of the launch-per-step route through `be`'s four methods of the mask (_xbox for 2, _rows for 4 and
    6), in place on z, lam, rho, on the tensors' device. -> dict(g, d [S,B,T,n], phi [S,20,B], phi_prev, k, accept [S,B],
    phi_end, rn2 [B]): what the kernel's trace holds, step by step."""
    dims = pr["dims"]
    B, T, nx, nu = dims
    sb_u, st_u, xb, poly = row_args(pr, mask)
    prob = (pr["x0"], lam, rho, pr["Qd"], pr["q"], pr["lo"], pr["hi"], sb_u, st_u)
    rows = (xb, poly) if poly is not None else (xb,)
    sfx = "rows" if poly is not None else "xbox"
    merit, step = getattr(be, "merit_" + sfx), getattr(be, "newton_step_" + sfx)
    pick, dual_update = getattr(be, "merit_pick_" + sfx), getattr(be, "dual_update_" + sfx)
    new = lambda *s, dt=z.dtype: torch.zeros(*s, dtype=dt, device=z.device)
    phi = new(B) if phi is None else phi
    rn2, d, g = new(B), new(B, T, nx + nu), new(B, T, nx + nu)
    tr = dict(g=[], d=[], phi=[], phi_prev=[], k=[], accept=[])
    if init:
        merit(dims, 1, z, ssr.true_next(plant, z, nx), *prob, *rows, phi, rn2)
    alphas = (2.0 ** -torch.arange(20, dtype=z.dtype, device=z.device)).view(20, 1, 1, 1)
    for _ in range(n_newton):
        xn, F = ssr.linearize(plant, z, nx)
        step(dims, z, xn, F, *prob, *rows, d, g_out=g)
        zc = (z.unsqueeze(0) + alphas * d.unsqueeze(0)).contiguous()
        pa, kk, acc = new(20, B), new(B, dt=torch.int32), new(B, dt=torch.int32)
        tr["phi_prev"].append(phi.clone())
        pick(dims, 20, d, ssr.true_next(plant, zc, nx), *prob, *rows, z, phi, rnorm2=rn2, phi_all=pa, k_out=kk, accept_out=acc)
        for key, v in (("g", g), ("d", d), ("phi", pa), ("k", kk), ("accept", acc)):
            tr[key].append(v.clone())
    xn = ssr.true_next(plant, z, nx)
    merit(dims, 1, z, xn, *prob, *rows, new(B), rn2)   # the true residual at the iterate the iteration ends on
    if dual:
        dual_update(dims, z, xn, pr["x0"], pr["lo"], pr["hi"], sb_u, st_u, *rows, lam, rho)
    out = {k: torch.stack(v) for k, v in tr.items()} if n_newton else {}
    out.update(phi_end=phi.clone(), rn2=rn2.clone())
    return out


def start(pr, mask):
    B = pr["dims"][0]
    dt = pr["z0"].dtype
    return pr["z0"].clone(), torch.zeros(B, lam_cols(pr, mask), dtype=dt), torch.ones(B, dtype=dt)


def near_ties(tr, tol_rel):
    """Instances whose line search the oracle does not decide at some step: its two best candidate merits, or the best
    and phi_prev, within tol_rel of the merit's size. -> bool [B]."""
    ph = tr["phi"].double()
    srt = ph.sort(1).values
    size = ph.abs().amax(1).clamp(min=1.0)
    und = (srt[:, 1] - srt[:, 0] <= tol_rel * size) | ((srt[:, 0] - tr["phi_prev"].double()).abs() <= tol_rel * size)
    return und.any(0)


def tie_oracle_backend(tol_rel):
    """RowsStepOracleBackend that marks, per instance, every line search of a solve the oracle's own arithmetic does not
    decide (near_ties with tol_rel, on the 20 merits and the previous merit of each pick, state-bound and row methods
    alike): `undecided` [B] bool after the solve. Two correct solvers may take different candidates at such a step and part ways
    there by up to that step's |d|: `tied_step` [B], the largest |d| of an instance's undecided picks (what
    rows_step_reference.TieBackend records for the row methods)."""
    from tests.rows_step_reference import RowsStepOracleBackend

    class TieOracleBackend(RowsStepOracleBackend):
        undecided = tied_step = None   # [B]: any pick undecided; the largest |d| of an instance's undecided picks

        def _pick(self, name, args, kw, n_ls, phi_prev, d):
            B = phi_prev.shape[0]
            prev = phi_prev.clone()
            pa = torch.empty(n_ls, B, dtype=phi_prev.dtype)
            want = kw.get("phi_all")
            getattr(super(), name)(*args, **{**kw, "phi_all": pa})
            if want is not None:
                want.copy_(pa)
            und = near_ties(dict(phi=pa.unsqueeze(0), phi_prev=prev.unsqueeze(0)), tol_rel).numpy()
            step = d.double().abs().reshape(B, -1).max(1).values.numpy()
            if self.undecided is None:
                self.undecided, self.tied_step = np.zeros(B, bool), np.zeros(B)
            self.undecided |= und
            self.tied_step = np.where(und, np.maximum(self.tied_step, step), self.tied_step)

        def merit_pick_rows(self, dims, n_ls, d, xnext_all, x0, lam, rho, Qd, q, ulo, uhi, sb_u, st_u, xbnd, poly, z, phi_prev, **kw):
            self._pick("merit_pick_rows", (dims, n_ls, d, xnext_all, x0, lam, rho, Qd, q, ulo, uhi, sb_u, st_u, xbnd, poly, z,
                                           phi_prev), kw, n_ls, phi_prev, d)

        def merit_pick_xbox(self, dims, n_ls, d, xnext_all, x0, lam, rho, Qd, q, ulo, uhi, sb_u, st_u, xbnd, z, phi_prev, **kw):
            self._pick("merit_pick_xbox", (dims, n_ls, d, xnext_all, x0, lam, rho, Qd, q, ulo, uhi, sb_u, st_u, xbnd, z,
                                           phi_prev), kw, n_ls, phi_prev, d)

    return TieOracleBackend()
