"""TEST-ONLY helpers for the compiled-in models' one-launch route on the plain row set (alqp_solve_nonlin,
HipBackend.solve_nonlin: the four `Dyn` instantiations of k_solve_lin_quad), all four models.

The oracle is the CPU route the project already pins against the reference's own goldens
(test_host_logic_with_restated_dynamics_vs_reference_mpc): tests/oracle_backend.OracleBackend's launch-per-step methods
(merit, newton_step, merit_pick, dual_update) driven with state_bounds_step_reference.linearize / true_next on the model
restatements of oracle/dyn_py.py wrapped as torch callables (OraclePlant). The second yardstick is the launch-per-step GPU
route: the same driver (al_iteration) over HipBackend's four methods with the provider's kernels, the route the parent runs
for a plain callable. Nothing of the solver is restated here."""
import functools

import numpy as np
import torch

from oracle import dyn_py
from oracle import oracle_py as orc
from tests import nonlin_rows_reference as nr
from tests import state_bounds_step_reference as ssr
from tests.oracle_backend import OracleBackend, _bounds

H_STEP = nr.H_STEP
PULL = nr.PULL
MODELS = {"pendulum1l": (2, 1, 1), "cartpole1l": (4, 1, 2), "cartpole1l_v2": (4, 1, 4), "cartpole2l": (6, 1, 3)}   # nx, nu, dyn_id
U_BOUND = 0.15   # tight: control rows end active (asserted on the oracle, tests/test_nonlin_reference_cpu.py)
SEEDS = tuple(range(11, 19))
TD = {"f64": torch.float64, "f32": torch.float32}
EPS = {"f64": 2.0 ** -52, "f32": 2.0 ** -23}

# (model, T, B, per_bt). Shapes from the kernel's structure: every model (NX = 2, 4, 6: the sel4 paddings of
# Quad::linearize), T = 2 (one dynamics stage, T < KL), 5, 9 (above the KL cap of 8), B = 1, 17 (a wavefront of quads plus
# one, the last fp32 record pair half used), 33; per_bt: control bounds [B,T,nu] (sb_u, st_u nonzero). SEED is the first of
# SEEDS at which, in every case, the fp64 oracle decides every line search of the case's two AL iterations and the fp32
# oracle keeps the caps of tie_caps_ok (choose_seed, on the CPU; tests/test_nonlin_reference_cpu.py asserts it).
SEED = 11
CASES = [("pendulum1l", 2, 1, False), ("pendulum1l", 5, 17, True), ("pendulum1l", 9, 33, False),
         ("cartpole1l", 5, 1, False), ("cartpole1l", 9, 17, False),
         ("cartpole1l_v2", 2, 33, True), ("cartpole1l_v2", 5, 17, False),
         ("cartpole2l", 2, 17, False), ("cartpole2l", 5, 33, True), ("cartpole2l", 9, 1, False)]


# one small case per model for the gradients through MPC, shared bounds (MPC takes them as [nu])
GRAD_CASES = [CASES[2], CASES[4], CASES[6], CASES[7]]


def case_id(c):
    mo, T, B, pbt = c
    return f"{mo}-T{T}-B{B}-{'bt' if pbt else 'shared'}"


class OraclePlant(nr.OraclePlant):
    """nonlin_rows_reference.OraclePlant with cartpole2l: tau = (u, 0, 0), as Cartpole2lDynamics pads it."""

    def __init__(self, model, h=H_STEP):
        self.model, self.h = model, h
        self.nx, self.nu, _ = MODELS[model]

    def _eval(self, x, u):
        if self.model != "cartpole2l":
            return super()._eval(x, u)
        xx, uu = x.detach().double().numpy(), u.detach().double().numpy()
        xn, J = dyn_py.cartpole2l(xx, np.concatenate([uu, np.zeros_like(uu), np.zeros_like(uu)], 1), self.h)
        return xn, J[:, :, :6], J[:, :, 6:7]


def provider(model, h=H_STEP):
    from deq_mpc_corl_amd import dynamics as dy
    return {"pendulum1l": dy.Pendulum1lDynamics, "cartpole1l": dy.Cartpole1lDynamics, "cartpole1l_v2": dy.Cartpole1lV2Dynamics,
            "cartpole2l": dy.Cartpole2lDynamics}[model](h)


def problem(model, B, T, per_bt, dtype, seed=SEED, pull=PULL, h_step=H_STEP):
    """nonlin_rows_reference.problem's recipe without its state bounds and rows, at any of the four models: the start is the
    model's own rollout from x0 under small random controls, the cost pulls every state `pull` beyond the start and the
    control bound is tight (U_BOUND), so that control rows become active. Control bounds [nu], or with `per_bt` [B,T,nu],
    each entry widened by its own amount. CPU tensors in `dtype`; -> (pr, plant)."""
    nx, nu, _ = MODELS[model]
    n = nx + nu
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    plant = OraclePlant(model, h_step)
    x0 = 0.4 * rnd(B, nx) - 0.2
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
    q = -Qd * xref
    q[..., nx:] = 0.3 * (rnd(B, T, nu) - 0.5)
    if per_bt:
        lo, hi = -(U_BOUND + 0.02 * rnd(B, T, nu)), U_BOUND + 0.02 * rnd(B, T, nu)
    else:
        lo, hi = torch.full((nu,), -U_BOUND, dtype=torch.float64), torch.full((nu,), U_BOUND, dtype=torch.float64)
    c = lambda v: v.to(dtype).contiguous()
    pr = dict(dims=(B, T, nx, nu), x0=c(x0), z0=c(z0), Qd=c(Qd), q=c(q), lo=c(lo), hi=c(hi), model=model, h_step=h_step,
              dyn_id=MODELS[model][2])
    return pr, plant


def strides(pr):
    """(sb_u, st_u) of the problem's control bounds, in elements."""
    B, T, nx, nu = pr["dims"]
    return (0, 0) if pr["lo"].dim() == 1 else (T * nu, nu)


def lam_cols(pr):
    B, T, nx, nu = pr["dims"]
    return T * nx + 2 * T * nu


def start(pr):
    B = pr["dims"][0]
    dt = pr["z0"].dtype
    return pr["z0"].clone(), torch.zeros(B, lam_cols(pr), dtype=dt), torch.ones(B, dtype=dt)


def to_dev(pr, dev):
    return nr.to_dev(pr, dev)


def al_iteration(be, pr, plant, z, lam, rho, phi=None, n_newton=4, init=True, dual=True, hessian=False):
    """One AL iteration of the launch-per-step route through `be`'s four plain methods, in place on z, lam, rho (and phi,
    when given), on the tensors' device: nonlin_rows_reference.al_iteration without rows. -> dict(g, d [S,B,T,n], phi
    [S,20,B], phi_prev, k, accept [S,B], F [S,B,T-1,nx,n], phi_end, rn2 [B]); with `hessian` (the CPU oracle only) also Hd
    [S,B,T,n,n], Hs [S,B,T-1,n,n] and L [S,B,T,n,n]: the Hessian blocks and the factor of every step."""
    dims = pr["dims"]
    B, T, nx, nu = dims
    sb_u, st_u = strides(pr)
    prob = (pr["x0"], lam, rho, pr["Qd"], pr["q"], pr["lo"], pr["hi"], sb_u, st_u)
    new = lambda *s, dt=z.dtype: torch.zeros(*s, dtype=dt, device=z.device)
    phi = new(B) if phi is None else phi
    rn2, d, g = new(B), new(B, T, nx + nu), new(B, T, nx + nu)
    tr = dict(g=[], d=[], phi=[], phi_prev=[], k=[], accept=[], F=[])
    hs = dict(Hd=[], Hs=[], L=[])
    if init:
        be.merit(dims, 1, z, ssr.true_next(plant, z, nx), *prob, phi, rn2)
    alphas = (2.0 ** -torch.arange(20, dtype=z.dtype, device=z.device)).view(20, 1, 1, 1)
    for _ in range(n_newton):
        xn, F = ssr.linearize(plant, z, nx)
        if hessian:
            for key, v in zip(("Hd", "Hs", "L"), step_hessian(pr, z, xn, F, lam, rho)):
                hs[key].append(torch.from_numpy(v))
        be.newton_step(dims, z, xn, F, *prob, d, g_out=g)
        zc = (z.unsqueeze(0) + alphas * d.unsqueeze(0)).contiguous()
        pa, kk, acc = new(20, B), new(B, dt=torch.int32), new(B, dt=torch.int32)
        tr["phi_prev"].append(phi.clone())
        be.merit_pick(dims, 20, d, ssr.true_next(plant, zc, nx), *prob, z, phi, rnorm2=rn2, phi_all=pa, k_out=kk, accept_out=acc)
        for key, v in (("g", g), ("d", d), ("phi", pa), ("k", kk), ("accept", acc), ("F", F)):
            tr[key].append(v.clone())
    xn = ssr.true_next(plant, z, nx)
    be.merit(dims, 1, z, xn, *prob, new(B), rn2)   # the true residual at the iterate the iteration ends on
    if dual:
        be.dual_update(dims, z, xn, pr["x0"], pr["lo"], pr["hi"], sb_u, st_u, lam, rho)
    out = {k: torch.stack(v) for k, v in {**tr, **(hs if hessian else {})}.items()} if n_newton else {}
    out.update(phi_end=phi.clone(), rn2=rn2.clone())
    return out


def step_hessian(pr, z, xn, F, lam, rho, dtype=None):
    """The oracle's Hessian blocks and factor of the Newton step at (z, lam, rho) with the linearisation (xn, F): what
    OracleBackend.newton_step forms (orc.grad_hess, orc.newton_dir). dtype "f64": on the inputs upcast. -> (Hd, Hs, L)."""
    B, T, nx, nu = pr["dims"]
    s = dtype or ("f64" if z.dtype == torch.float64 else "f32")
    npdt = np.float64 if s == "f64" else np.float32
    c = lambda t: np.ascontiguousarray(t.detach().cpu().numpy().astype(npdt))
    lo, hi = _bounds(pr["lo"].cpu(), pr["hi"].cpu(), *strides(pr), B, T, nu)
    g, Hd, Hs = orc.grad_hess(s, c(z), c(xn), c(F), c(pr["x0"]), c(lam), c(rho), c(pr["Qd"]), c(pr["q"]),
                              lo.astype(npdt), hi.astype(npdt))
    _, _, L, _ = orc.newton_dir(s, g, Hd, Hs, nx, want_factor=True)
    return Hd, Hs, L


def backward_f64(pr, plant, z_pre, lam, rho, z_final, gbar):
    """The backward pass of the implicit layer for a Newton step taken at z_pre: the fp64 oracle's Hessian of that step
    (the plant's Jacobian at z_pre, orc.grad_hess) factored and solved by orc.backward, on the inputs upcast.
    -> (q_grad, Qd_grad) [B,T,n] float64."""
    d = lambda t: t.detach().cpu().double()
    pr64 = {k: (d(v) if torch.is_tensor(v) else v) for k, v in pr.items()}
    nx = pr["dims"][2]
    xn, F = ssr.linearize(plant, d(z_pre), nx)
    _, _, L = step_hessian(pr64, d(z_pre), xn, F, d(lam), d(rho), "f64")
    return orc.backward("f64", L, F.numpy(), d(rho).numpy(), d(z_final).numpy(), d(gbar).numpy())


def tie_tol(pr, dtype):
    """The merit tolerance of tests/aux_cases.py for a candidate's merit, relative to the merit's size (near_ties)."""
    from tests import aux_cases as ax
    B, T, nx, nu = pr["dims"]
    return ax.gamma_merit(T, nx, nu, 0, cand=True) * EPS[dtype]


def undecided_steps(tr, tol):
    """-> bool [S,B]: the oracle does not decide step s's line search (nonlin_rows_reference.near_ties, step by step)."""
    S = tr["phi"].shape[0]
    return np.stack([nr.near_ties({k: tr[k][s:s + 1] for k in ("phi", "phi_prev")}, tol).numpy() for s in range(S)])


def compared(und):
    """-> bool [S,B]: the instances whose EARLIER picks the oracle decides (an undecided pick is held to the achieved merit
    at its own step; only the steps after it lose the instance)."""
    ok = np.ones_like(und)
    for s in range(und.shape[0] - 1):
        ok[s + 1:] &= ~und[s]
    return ok


def tie_caps_ok(und, B):
    """The caps of a case: at every step at least three quarters of the batch compared, a one-instance case in full."""
    ok = compared(und)
    return bool((ok.mean(1) >= 0.75).all() and (B > 1 or ok.all()))


def oracle_solve(model, T, B, per_bt, dtype, seed=SEED, al_iter=2):
    """The oracle's whole solve from the problem's start: `al_iter` AL iterations of four Newton steps with the dual update.
    -> (pr, plant, list of per-iteration (state before, trace with Hessians), final (z, lam, rho), phi, rn2)."""
    pr, plant = problem(model, B, T, per_bt, TD[dtype], seed)
    z, lam, rho = start(pr)
    be = OracleBackend()
    its = []
    phi = torch.zeros(B, dtype=TD[dtype])
    for _ in range(al_iter):
        before = (z.clone(), lam.clone(), rho.clone())
        tr = al_iteration(be, pr, plant, z, lam, rho, phi=phi, hessian=True)
        its.append((before, tr))
    return pr, plant, its, (z, lam, rho), its[-1][1]["phi_end"], its[-1][1]["rn2"]


def solve_ties(its, pr, dtype):
    """Over the line searches of a whole solve -> (und [S_total,B], undecided [B], tied_step [B]: the largest |d| of an
    instance's undecided picks, what nonlin_rows_reference.tie_oracle_backend records)."""
    B = pr["dims"][0]
    tol = tie_tol(pr, dtype)
    und = np.concatenate([undecided_steps(tr, tol) for _, tr in its])
    dmax = np.concatenate([tr["d"].double().abs().reshape(tr["d"].shape[0], B, -1).amax(2).numpy() for _, tr in its])
    return und, und.any(0), np.where(und, dmax, 0.0).max(0)


def choose_seed(model, T, B, per_bt):
    """The first of SEEDS at which the fp64 oracle decides every line search of the case's two AL iterations and the fp32
    oracle keeps tie_caps_ok in each of them (the per-step test runs the second from the oracle's state after the
    first); None when no seed does."""
    for seed in SEEDS:
        good = True
        for dtype in ("f64", "f32"):
            pr, _, its, _, _, _ = oracle_solve(model, T, B, per_bt, dtype, seed)
            for _, tr in its:
                und = undecided_steps(tr, tie_tol(pr, dtype))
                good &= (not und.any()) if dtype == "f64" else tie_caps_ok(und, B)
        if good:
            return seed
    return None


def controls_active(pr, z, lam):
    """Per instance: (a control row violated or at its bound at z, a nonzero control-row multiplier)."""
    B, T, nx, nu = pr["dims"]
    lo, hi = _bounds(pr["lo"], pr["hi"], *strides(pr), B, T, nu)
    u = z[..., nx:].double().numpy()
    act = ((u >= np.broadcast_to(hi, u.shape)) | (u <= np.broadcast_to(lo, u.shape))).reshape(B, -1).any(1)
    return act, (lam[:, T * nx:] > 0).reshape(B, -1).any(1).numpy()


class TieOracleBackend(OracleBackend):
    """OracleBackend that marks, per instance, every line search of a solve the oracle's own arithmetic does not decide
    (nonlin_rows_reference.tie_oracle_backend for the plain merit_pick): `undecided`, `tied_step` [B] after the solve."""

    def __init__(self, tol_rel):
        self.tol_rel, self.undecided, self.tied_step = tol_rel, None, None

    def merit_pick(self, dims, n_ls, d, xnext_all, x0, lam, rho, Qd, q, ulo, uhi, sb_u, st_u, z, phi_prev, **kw):
        B = phi_prev.shape[0]
        prev = phi_prev.clone()
        pa = torch.empty(n_ls, B, dtype=phi_prev.dtype)
        want = kw.get("phi_all")
        super().merit_pick(dims, n_ls, d, xnext_all, x0, lam, rho, Qd, q, ulo, uhi, sb_u, st_u, z, phi_prev, **{**kw, "phi_all": pa})
        if want is not None:
            want.copy_(pa)
        und = nr.near_ties(dict(phi=pa.unsqueeze(0), phi_prev=prev.unsqueeze(0)), self.tol_rel).numpy()
        step = d.double().abs().reshape(B, -1).max(1).values.numpy()
        if self.undecided is None:
            self.undecided, self.tied_step = np.zeros(B, bool), np.zeros(B)
        self.undecided |= und
        self.tied_step = np.where(und, np.maximum(self.tied_step, step), self.tied_step)


def mpc_grads(pr, mode, dyn, backend, dtype, dev):
    """MPC (al_iter = 2, prefer_fused) on the problem with `dyn` as dx / dx_jac, then d/dq and d/dQd of a seeded weighted sum
    of (x, u). backend None: the product's. -> (dict(z, dq, dQd) float64 numpy, Newton steps per AL iteration, the MPC)."""
    from deq_mpc_corl_amd import MPC, QuadCost
    B, T, nx, nu = pr["dims"]
    t = lambda v: v.to(dev).clone()
    Qd, q = t(pr["Qd"]).requires_grad_(True), t(pr["q"]).requires_grad_(True)
    mpc = MPC(nx, nu, T, u_lower=pr["lo"].to(dev), u_upper=pr["hi"].to(dev), n_batch=B, dtype=dtype, exit_mode=mode, al_iter=2,
              prefer_fused=True, **({"backend": backend} if backend is not None else {}))
    mpc.reinitialize(t(pr["x0"]), None)
    x, u, _ = mpc(t(pr["x0"]), QuadCost(torch.diag_embed(Qd), q), dyn, dyn.jac, x_init=t(pr["z0"][..., :nx]),
                  u_init=t(pr["z0"][..., nx:]))
    gw = torch.Generator().manual_seed(3)
    wx, wu = torch.randn(B, T, nx, generator=gw).to(dev), torch.randn(B, T, nu, generator=gw).to(dev)
    ((x * wx).sum() + (u * wu).sum()).backward()
    out = dict(z=torch.cat((x, u), -1), dq=q.grad, dQd=Qd.grad)
    return ({k: v.detach().cpu().double().numpy() for k, v in out.items()}, [int(k) for k in mpc.last_newton_per_al], mpc)


@functools.lru_cache(maxsize=None)
def oracle_grads(model, T, B, per_bt, mode, dtype):
    """mpc_grads on TieOracleBackend with the plant on the CPU: once per session, never modified.
    -> (pr, dict(z, dq, dQd), Newton counts, undecided [B], tied_step [B])."""
    pr, plant = problem(model, B, T, per_bt, TD[dtype], SEED)
    be = TieOracleBackend(tie_tol(pr, dtype))
    ref, newton, _ = mpc_grads(pr, mode, plant, be, TD[dtype], "cpu")
    return pr, ref, newton, be.undecided, be.tied_step
