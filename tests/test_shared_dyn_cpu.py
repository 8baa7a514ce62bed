"""Batch-shared affine dynamics, LinDx(F[T-1,nx,n] | F[nx,n], f[T-1,nx] | f[nx]), without a GPU.

The host side only: what MPC accepts, what it hands to the backend (the shared data as given, with its strides, when the
backend has solve_lin_shared; materialised otherwise and for the dense-cost / state-bound / general-row kernels), that
every route computes what it computes on the expanded tensors, and that a shared F / f gets the per-instance gradient
summed over the axes it was broadcast over. The kernels are pinned on the GPU (tests/test_gpu_shared_dyn.py)."""
import numpy as np
import pytest
import torch

from oracle import oracle_py as orc
from tests.oracle_backend import OracleBackend
from tests.test_dyn_grad_cpu import FD_H, FD_TOL, _DynOracleBackend

NX, NU, B, T = 2, 1, 3, 4
N = NX + NU


def _problem(nx=NX, nu=NU, b=B, t=T, seed=7):
    from deq_mpc_corl_amd import synthetic_problem
    return synthetic_problem(b, t, nx, nu, seed=seed, dtype=torch.float64, active=True)


def _forms(p):
    """name -> (F, f) as the caller gives them; instance 0's model is the shared one."""
    lti, ltv = p.F[0, 0].clone(), p.F[0].clone()
    f_lti, f_ltv = p.c[0, 0].clone(), p.c[0].clone()
    return {"lti": (lti, f_lti), "ltv_fB": (ltv, p.c.clone()), "lti_fT": (lti, f_ltv), "FB_flti": (p.F.clone(), f_lti),
            "ltv": (ltv, f_ltv)}


def _expanded(p, F, f):
    return (F.expand(p.B, p.T - 1, p.nx, p.nx + p.nu).contiguous(), f.expand(p.B, p.T - 1, p.nx).contiguous())


def _run(be, p, F, f, route, exit_mode, **mpc_kw):
    """One MPC solve -> (x, u, lamda_prev, rho_prev)."""
    from deq_mpc_corl_amd import MPC, QuadCost
    from deq_mpc_corl_amd.qpth.al_utils import LinDx
    mpc = MPC(p.nx, p.nu, p.T, u_lower=p.u_lo, u_upper=p.u_hi, n_batch=p.B, dtype=torch.float64, exit_mode=exit_mode,
              al_iter=2, backend=be, **mpc_kw)
    mpc.reinitialize(p.x0, None)
    xi, ui = p.z0[..., :p.nx].clone(), p.z0[..., p.nx:].clone()
    dx = LinDx(F, f)
    if route == "forward":
        x, u, _ = mpc(p.x0, QuadCost(torch.diag_embed(p.Qd), p.q), dx, None, x_init=xi, u_init=ui)
    elif route == "al_solve":
        x, u, _ = mpc.al_solve(xi, ui, dx, None, p.x0, QuadCost(p.Qd, p.q))
    else:
        x, u, _ = mpc.al_solve_stream(xi, ui, dx, None, p.x0, QuadCost(p.Qd, p.q))
    return x, u, mpc.lamda_prev, mpc.rho_prev


@pytest.mark.parametrize("form", ["lti", "ltv_fB", "lti_fT", "FB_flti"])
@pytest.mark.parametrize("route,exit_mode", [("forward", "fixed"), ("forward", "reference"), ("al_solve", "fixed"),
                                             ("al_solve", "reference"), ("stream", "fixed"), ("stream", "reference")])
def test_fallback_equals_expanded_bitwise(form, route, exit_mode):
    """OracleBackend has no solve_lin_shared: MPC materialises the shared forms and every route returns what it returns
    for the expanded tensors, bit for bit. (On the parent commit the first case raises ValueError from _as_lindx.)"""
    p = _problem()
    F, f = _forms(p)[form]
    assert not hasattr(OracleBackend, "solve_lin_shared")
    got = _run(OracleBackend(), p, F, f, route, exit_mode)
    want = _run(OracleBackend(), p, *_expanded(p, F, f), route, exit_mode)
    for name, a, b in zip(("x", "u", "lamda_prev", "rho_prev"), got, want):
        assert torch.equal(a, b), name


class _SharedOracleBackend(_DynOracleBackend):
    """A backend WITH solve_lin_shared: expands, calls solve_lin, records what it was handed. The dense-cost,
    state-bound and general-row entry points record the dynamics' shapes and do nothing else."""

    def __init__(self):
        super().__init__()
        self.calls = []

    def solve_lin(self, dims, Qd, q, F, c, *a, **kw):
        if not getattr(self, "_inside", False):
            self.calls.append(("solve_lin", tuple(F.shape), tuple(c.shape)))
        return super().solve_lin(dims, Qd, q, F, c, *a, **kw)

    def solve_lin_shared(self, dims, Qd, q, F, c, sb_F, st_F, sb_c, st_c, *a, **kw):
        self.calls.append(("solve_lin_shared", tuple(F.shape), tuple(c.shape), sb_F, st_F, sb_c, st_c))
        Bb, Tt, nx, nu = dims
        self._inside = True
        try:
            return self.solve_lin(dims, Qd, q, F.expand(Bb, Tt - 1, nx, nx + nu).contiguous(),
                                  c.expand(Bb, Tt - 1, nx).contiguous(), *a, **kw)
        finally:
            self._inside = False

    def _other(name):
        def f(self, dims, Qd, q, F, c, *a, **kw):
            self.calls.append((name, tuple(F.shape), tuple(c.shape)))
            return True
        return f

    solve_lin_dense, solve_lin_xbox, solve_lin_poly = _other("solve_lin_dense"), _other("solve_lin_xbox"), _other("solve_lin_poly")


WF, WC = NX * N, NX
STRIDES = {"lti": (0, 0, 0, 0), "ltv_fB": (0, WF, (T - 1) * WC, WC), "lti_fT": (0, 0, 0, WC),
           "FB_flti": ((T - 1) * WF, WF, 0, 0), "ltv": (0, WF, 0, WC)}


@pytest.mark.parametrize("form", sorted(STRIDES))
@pytest.mark.parametrize("route,exit_mode", [("forward", "fixed"), ("forward", "reference"), ("stream", "reference")])
def test_backend_gets_unexpanded_tensors_and_strides(form, route, exit_mode):
    p = _problem()
    F, f = _forms(p)[form]
    be = _SharedOracleBackend()
    got = _run(be, p, F, f, route, exit_mode)
    assert be.calls and all(c == ("solve_lin_shared", tuple(F.shape), tuple(f.shape), *STRIDES[form]) for c in be.calls), be.calls
    want = _run(OracleBackend(), p, *_expanded(p, F, f), route, exit_mode)
    for name, a, b in zip(("x", "u", "lamda_prev", "rho_prev"), got, want):
        assert torch.equal(a, b), name


def test_per_instance_still_reaches_solve_lin():
    p = _problem()
    be = _SharedOracleBackend()
    _run(be, p, p.F.clone(), p.c.clone(), "forward", "fixed")
    assert be.calls == [("solve_lin", (B, T - 1, NX, N), (B, T - 1, NX))]


@pytest.mark.parametrize("kind", ["dense", "xbox", "poly"])
def test_other_kernels_get_expanded_dynamics(kind):
    """diag_cost=False, x_lower / x_upper and ineqG / ineqh: their kernels read a per-instance F, the host materialises."""
    from deq_mpc_corl_amd import MPC, QuadCost
    from deq_mpc_corl_amd.qpth.al_utils import LinDx
    p = _problem()
    F, f = _forms(p)["lti"]
    kw = {"dense": dict(diag_cost=False), "xbox": dict(x_lower=-5.0, x_upper=5.0),
          "poly": dict(ineqG=torch.eye(N, dtype=torch.float64)[:2], ineqh=torch.full((2,), 3.0, dtype=torch.float64))}[kind]
    be = _SharedOracleBackend()
    mpc = MPC(p.nx, p.nu, p.T, u_lower=p.u_lo, u_upper=p.u_hi, n_batch=p.B, dtype=torch.float64, exit_mode="fixed",
              al_iter=2, backend=be, **kw)
    mpc.reinitialize(p.x0, None)
    mpc(p.x0, QuadCost(torch.diag_embed(p.Qd), p.q), LinDx(F, f), None, x_init=p.z0[..., :p.nx].clone(),
        u_init=p.z0[..., p.nx:].clone())
    assert be.calls == [("solve_lin_" + kind, (B, T - 1, NX, N), (B, T - 1, NX))]


@pytest.mark.parametrize("form", sorted(STRIDES))
def test_rollout_equals_expanded(form):
    from deq_mpc_corl_amd import MPC
    from deq_mpc_corl_amd.qpth.al_utils import LinDx
    p = _problem()
    F, f = _forms(p)[form]
    mpc = MPC(p.nx, p.nu, p.T, u_lower=p.u_lo, u_upper=p.u_hi, n_batch=p.B, dtype=torch.float64, backend=OracleBackend())
    u = torch.randn(p.B, p.T, p.nu, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    got = mpc.rollout(p.x0, u, LinDx(F, f))
    want = mpc.rollout(p.x0, u, LinDx(*_expanded(p, F, f)))
    assert got.shape == (p.B, p.T, p.nx) and torch.equal(got, want)


def test_forward_without_x_init_rolls_out_shared_dynamics():
    from deq_mpc_corl_amd import MPC, QuadCost
    from deq_mpc_corl_amd.qpth.al_utils import LinDx
    p = _problem()
    F, f = _forms(p)["lti"]
    outs = []
    for Fx, fx in ((F, f), _expanded(p, F, f)):
        mpc = MPC(p.nx, p.nu, p.T, u_lower=p.u_lo, u_upper=p.u_hi, n_batch=p.B, dtype=torch.float64, exit_mode="fixed",
                  backend=OracleBackend())
        mpc.reinitialize(p.x0, None)
        outs.append(mpc(p.x0, QuadCost(torch.diag_embed(p.Qd), p.q), LinDx(Fx, fx), None)[:2])
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def _grad_run(be, p, F, f, exit_mode):
    from deq_mpc_corl_amd import MPC, QuadCost
    from deq_mpc_corl_amd.qpth.al_utils import LinDx
    mpc = MPC(p.nx, p.nu, p.T, u_lower=p.u_lo, u_upper=p.u_hi, n_batch=p.B, dtype=torch.float64, exit_mode=exit_mode,
              al_iter=2, backend=be)
    mpc.reinitialize(p.x0, None)
    F, f = F.clone().requires_grad_(True), f.clone().requires_grad_(True)
    x, u, _ = mpc(p.x0, QuadCost(torch.diag_embed(p.Qd), p.q), LinDx(F, f), None, x_init=p.z0[..., :p.nx].clone(),
                  u_init=p.z0[..., p.nx:].clone())
    gen = torch.Generator().manual_seed(5)
    gx = torch.randn(x.shape, generator=gen, dtype=torch.float64).to(x.dtype)
    gu = torch.randn(u.shape, generator=gen, dtype=torch.float64).to(u.dtype)
    ((x * gx).sum() + (u * gu).sum()).backward()
    return F.grad, f.grad


@pytest.mark.parametrize("backend", [_DynOracleBackend, _SharedOracleBackend])
@pytest.mark.parametrize("exit_mode", ["fixed", "reference"])
@pytest.mark.parametrize("form", sorted(STRIDES))
def test_shared_gradients_are_the_expanded_ones_summed(form, exit_mode, backend):
    p = _problem()
    F, f = _forms(p)[form]
    gF, gf = _grad_run(backend(), p, F, f, exit_mode)
    eF, ef = _grad_run(_DynOracleBackend(), p, *_expanded(p, F, f), exit_mode)
    assert gF.shape == F.shape and gf.shape == f.shape and gF.dtype == F.dtype
    wantF = eF if F.dim() == 4 else eF.sum(dim=tuple(range(4 - F.dim())))
    wantf = ef if f.dim() == 3 else ef.sum(dim=tuple(range(3 - f.dim())))
    assert torch.equal(gF, wantF) and torch.equal(gf, wantf)


@pytest.mark.parametrize("nx,nu", [(2, 1), (4, 2)])
def test_shared_gradients_vs_central_differences(nx, nu):
    """tests/test_dyn_grad_cpu.py's construction (seed-3 problem, a warm stage, then ONE AL iteration run to
    stationarity from (z1, lam1, rho1)), its step FD_H and its bound FD_TOL. MPC differentiates that AL iteration started
    at its own stationary point zf (its four Newton steps stay there), with LinDx(F[nx,n], f[nx]); the finite differences
    move the ONE shared entry, i.e. every instance's and stage's copy together, through the oracle's solve."""
    from deq_mpc_corl_amd import MPC, QuadCost, synthetic_problem
    from deq_mpc_corl_amd.qpth.al_utils import LinDx
    Bb, Tt = 4, 5
    p = synthetic_problem(Bb, Tt, nx, nu, seed=3, dtype=torch.float64, active=True)
    c = lambda a: a.numpy().copy()
    Qd, q, x0, lo, hi, z0 = (c(a) for a in (p.Qd, p.q, p.x0, p.u_lo, p.u_hi, p.z0))
    F1, f1 = c(p.F[0, 0]), c(p.c[0, 0])
    ex = lambda F_, f_: (np.broadcast_to(F_, (Bb, Tt - 1, nx, nx + nu)).copy(), np.broadcast_to(f_, (Bb, Tt - 1, nx)).copy())
    o1 = orc.solve_lin("f64", Qd, q, *ex(F1, f1), x0, lo, hi, z0, al_iter=2, max_newton=4)
    z1, lam1, rho1 = o1["z"], o1["lam"], o1["rho"]

    def stage(F_, f_):
        return orc.solve_lin("f64", Qd, q, *ex(F_, f_), x0, lo, hi, z1, lam0=lam1, rho0=rho1, al_iter=1, max_newton=8,
                             exit_mode="fixed")

    zf = stage(F1, f1)["z"]
    mpc = MPC(nx, nu, Tt, u_lower=p.u_lo, u_upper=p.u_hi, n_batch=Bb, dtype=torch.float64, exit_mode="fixed", al_iter=1,
              backend=_DynOracleBackend())
    mpc.reinitialize(p.x0, None)
    Ft, ft = torch.from_numpy(F1).requires_grad_(True), torch.from_numpy(f1).requires_grad_(True)
    zt = torch.from_numpy(zf)
    x, u, _ = mpc.al_solve(zt[..., :nx].clone(), zt[..., nx:].clone(), LinDx(Ft, ft), None, p.x0, QuadCost(p.Qd, p.q),
                           lamda_init=torch.from_numpy(lam1), rho_init=torch.from_numpy(rho1).reshape(Bb, 1))
    moved = np.abs(np.concatenate((x.detach().numpy(), u.detach().numpy()), -1) - zf).max()
    print(f"({nx},{nu}): MPC's four Newton steps from zf moved z by {moved:.2e} (float32 outputs)")
    assert moved < 1e-6 * max(1.0, np.abs(zf).max())
    # MPC returns x, u as float32, so autograd hands the solve a float32 gbar: weights that float32 holds exactly make
    # the loss MPC differentiates and the loss the differences evaluate the same function
    gbar = np.random.default_rng(1).standard_normal(zf.shape).astype(np.float32).astype(np.float64)
    gt = torch.from_numpy(gbar)
    ((x.double() * gt[..., :nx]).sum() + (u.double() * gt[..., nx:]).sum()).backward()
    assert Ft.grad.shape == (nx, nx + nu) and ft.grad.shape == (nx,)
    loss = lambda oo: float((gbar * oo["z"]).sum())
    rng = np.random.default_rng(2)
    probes = []
    for name, arr, grad in (("F", F1, Ft.grad.numpy()), ("f", f1, ft.grad.numpy())):
        for _ in range(4):
            idx = tuple(int(rng.integers(0, s)) for s in arr.shape)
            vals = []
            for sgn in (1.0, -1.0):
                a = arr.copy()
                a[idx] += sgn * FD_H
                vals.append(loss(stage(*((a, f1) if name == "F" else (F1, a)))))
            probes.append((name, grad[idx], (vals[0] - vals[1]) / (2 * FD_H)))
    scale = max(abs(a) for _, a, _ in probes)
    err = max(abs(a - fd) for _, a, fd in probes) / scale
    print(f"({nx},{nu}): shared dF, df vs central differences: {err:.2e} (relative to the largest probed gradient {scale:.3g})")
    assert err < FD_TOL, (err, probes)


@pytest.mark.parametrize("bad", ["F_B+1", "F_T", "F_n+1", "f_T"])
def test_shape_errors(bad):
    from deq_mpc_corl_amd import MPC, QuadCost
    from deq_mpc_corl_amd.qpth.al_utils import LinDx
    p = _problem()
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    F, f = {"F_B+1": (z(B + 1, T - 1, NX, N), p.c), "F_T": (z(T, NX, N), p.c), "F_n+1": (z(NX, N + 1), p.c),
            "f_T": (p.F, z(T, NX))}[bad]
    mpc = MPC(p.nx, p.nu, p.T, u_lower=p.u_lo, u_upper=p.u_hi, n_batch=p.B, dtype=torch.float64, backend=OracleBackend())
    mpc.reinitialize(p.x0, None)
    with pytest.raises(ValueError) as e:
        mpc(p.x0, QuadCost(torch.diag_embed(p.Qd), p.q), LinDx(F, f), None, x_init=p.z0[..., :p.nx].clone(),
            u_init=p.z0[..., p.nx:].clone())
    msg = str(e.value)
    lead = "[B,T-1,nx,n]" if bad.startswith("F") else "[B,T-1,nx]"
    assert lead in msg and "[T-1,nx" in msg and "[nx" in msg, msg   # the three accepted forms
