"""Dense (non-diagonal) stage cost through MPC(diag_cost=False), without a GPU: the host wiring on the test backend of
tests/dense_cost_reference.py, and that backend itself pinned to the reference-pinned oracle.

The reference cannot run a dense cost (al_utils.merit_grad_hessian leaves `Qfull` undefined on that branch), so there is
no golden. The pins are: the diagonal twin (diag_embed(Qd) through the dense path reproduces the reference-generated
goldens), the rotated-states test (a diagonal problem in rotated state coordinates IS a dense problem, and the AL
iteration is equivariant under that rotation, so OracleBackend on the diagonal problem is the reference), and central
finite differences for the gradient w.r.t. C."""
import numpy as np
import pytest
import torch

from tests import golden_util as gu
from tests.dense_cost_reference import DenseOracleBackend, dense_w, run_solve
from tests.test_dyn_grad_cpu import dyn_grads

F64 = torch.float64


def t64(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(F64)


def _mpc(p_dims, lo, hi, be, diag_cost, exit_mode="reference", al_iter=2, **kw):
    from deq_mpc_corl_amd import MPC
    B, T, nx, nu = p_dims
    return MPC(nx, nu, T, u_lower=lo, u_upper=hi, n_batch=B, dtype=F64, exit_mode=exit_mode, al_iter=al_iter,
               backend=be, diag_cost=diag_cost, **kw)


def _solve(mpc, C, q, F, c, x0, z0, nx):
    from deq_mpc_corl_amd import QuadCost
    from deq_mpc_corl_amd.qpth.al_utils import LinDx
    mpc.reinitialize(x0, None)
    return mpc(x0, QuadCost(C, q), LinDx(F, c), None, x_init=z0[..., :nx].clone(), u_init=z0[..., nx:].clone())


# ---- 1. diagonal twin on the reference-generated goldens -----------------------------------------------------------
@pytest.mark.parametrize("name", ["pend_f64_al2", "cart_f64_al2", "pend_active_f64_al6"])
def test_diagonal_twin_reproduces_goldens(name):
    g = gu.load(name)
    B, T, nx, nu = g["B"], g["T"], g["nx"], g["nu"]
    C = torch.diag_embed(t64(g["Qd"]))
    out = {}
    for diag_cost in (True, False):
        be = DenseOracleBackend()
        mpc = _mpc((B, T, nx, nu), t64(g["u_lo"]), t64(g["u_hi"]), be, diag_cost, al_iter=g["al_iter"])
        x, u, _ = _solve(mpc, C, t64(g["q"]), t64(g["F"]), t64(g["c"]), t64(g["x0"]), t64(g["z0"]), nx)
        out[diag_cost] = (x.numpy(), u.numpy(), list(mpc.last_newton_per_al))
        assert set(be.calls) == {"solve_lin" if diag_cost else "solve_lin_dense"}
    assert out[False][2] == out[True][2] == list(g["newton_per_al"])
    for x, u, _ in out.values():   # tests/test_host_logic.py's tolerance for the fp64 goldens
        assert np.abs(x - g["x"]).max() < 2e-5 and np.abs(u - g["u"]).max() < 2e-5
    dev = max(np.abs(out[False][i] - out[True][i]).max() for i in (0, 1))
    print(f"{name}: dense path vs diagonal path on diag_embed(Qd): {dev:.2e}")


# ---- 2. rotated states ---------------------------------------------------------------------------------------------
def _rotated_pair(B, T, nx, nu, seed):
    """A diagonal problem (tilde) and the same problem in rotated state coordinates z = blockdiag(P, I) z~ (dense)."""
    from deq_mpc_corl_amd import synthetic_problem
    p = synthetic_problem(B, T, nx, nu, seed=seed, dtype=F64, active=True)
    n = nx + nu
    gen = torch.Generator().manual_seed(seed + 100)
    D = torch.cat((1.0 + 19.0 * torch.rand(B, T, nx, generator=gen, dtype=F64),   # distinct: else P D P' stays diagonal
                   torch.full((B, T, nu), 1e-3, dtype=F64)), -1)
    qt = -D * p.xref
    P, _ = torch.linalg.qr(torch.randn(B, nx, nx, generator=gen, dtype=F64))
    Pn = torch.zeros(B, n, n, dtype=F64)
    Pn[:, :nx, :nx] = P
    Pn[:, nx:, nx:] = torch.eye(nu, dtype=F64)
    tilde = dict(C=torch.diag_embed(D), q=qt, F=p.F, c=p.c, x0=p.x0, z0=p.z0)
    dense = dict(C=torch.einsum("bij,btj,bkj->btik", Pn, D, Pn), q=torch.einsum("bij,btj->bti", Pn, qt),
                 F=torch.einsum("bij,btjk,blk->btil", P, p.F, Pn), c=torch.einsum("bij,btj->bti", P, p.c),
                 x0=torch.einsum("bij,bj->bi", P, p.x0), z0=torch.einsum("bij,btj->bti", Pn, p.z0))
    return p, P, tilde, dense


@pytest.mark.parametrize("exit_mode", ["reference", "fixed"])
@pytest.mark.parametrize("nx,nu,T,B", [(2, 1, 5, 6), (4, 2, 6, 5), (13, 4, 20, 3), (13, 4, 2, 3)])
def test_rotated_states_match_the_diagonal_oracle(nx, nu, T, B, exit_mode):
    p, P, tilde, dense = _rotated_pair(B, T, nx, nu, seed=11)
    off = dense["C"] - torch.diag_embed(dense["C"].diagonal(dim1=-2, dim2=-1))
    assert off.abs().max() > 1.0   # a dense problem indeed
    from tests.oracle_backend import OracleBackend
    m0 = _mpc((B, T, nx, nu), p.u_lo, p.u_hi, OracleBackend(), True, exit_mode)
    x0_, u0_, _ = _solve(m0, nx=nx, **tilde)
    be = DenseOracleBackend()
    m1 = _mpc((B, T, nx, nu), p.u_lo, p.u_hi, be, False, exit_mode)
    x1, u1, _ = _solve(m1, nx=nx, **dense)
    assert set(be.calls) == {"solve_lin_dense"}
    assert list(m1.last_newton_per_al) == list(m0.last_newton_per_al)
    back = torch.einsum("bji,btj->bti", P, x1.to(F64))   # P' x
    dev = max((back - x0_.to(F64)).abs().max().item(), (u1.to(F64) - u0_.to(F64)).abs().max().item())
    print(f"({nx},{nu}) T={T} {exit_mode}: Newton counts {list(m1.last_newton_per_al)}, rotated-back deviation {dev:.2e}, "
          f"largest off-diagonal {off.abs().max().item():.2f}")
    assert dev < 1e-6


# ---- 3. C_grad against central finite differences -------------------------------------------------------------------
FD_H = 1e-5
# relative to the largest probed analytic gradient. Measured on the reference backend (fp64, these probes):
# (2,1) 8.8e-10, (4,2) 7.0e-9, (13,4) 7.9e-9, max |g(z_final)| 9.0e-14; the bound is 20x the largest.
FD_TOL = 1.6e-7


def _stationary_stage(nx, nu, B=4, T=5, seed=3, cost_seed=1):
    """synthetic_dense_cost problem, warm stage (2 AL iterations), then `stage(C)`: one AL iteration of 8 Newton steps
    from the warm stage's (z, lam, rho), as tests/test_dyn_grad_cpu.py does it. (cost_seed 1: with 0, 2 or 3 one
    instance of one of the three sizes still changes its active set in the 8th Newton step, |g| ~ 0.05-0.4, and finite
    differences through a solve that is not stationary pin nothing.)"""
    from deq_mpc_corl_amd import synthetic_dense_cost, synthetic_problem
    p = synthetic_problem(B, T, nx, nu, seed=seed, dtype=F64, active=True)
    C, q = synthetic_dense_cost(p, cost_seed)
    be = DenseOracleBackend()
    o1 = run_solve(be, C, q, p.F, p.c, p.x0, p.u_lo, p.u_hi, p.z0, al_iter=2, max_newton=4)
    assert torch.allclose(o1["rho"], torch.full_like(o1["rho"], 100.0))

    def stage(C_, **kw):
        Cs = 0.5 * (C_ + C_.transpose(-1, -2))   # what MPC.forward does
        return run_solve(be, Cs, q, p.F, p.c, p.x0, p.u_lo, p.u_hi, o1["z"], o1["lam"], o1["rho"], al_iter=1,
                         max_newton=8, **kw)
    return p, C, q, o1, stage


@pytest.mark.parametrize("nx,nu", [(2, 1), (4, 2), (13, 4)])
def test_C_grad_vs_finite_differences(nx, nu):
    p, C, q, o1, stage = _stationary_stage(nx, nu)
    B, T = p.B, p.T
    tr = {}
    zf = stage(C, trace=tr)["z"].numpy()
    # stationary: the merit gradient at z_final with the stage's (lam, rho)
    be = DenseOracleBackend()
    from tests.dense_cost_reference import split_cost
    Cd, off = split_cost(C.numpy())
    xn = np.einsum("btij,btj->bti", p.F.numpy(), zf[:, :-1]) + p.c.numpy()
    g, Hd, Hs = be.grad_hess_dense("f64", zf, xn, p.F.numpy(), p.x0.numpy(), o1["lam"].numpy(), o1["rho"].numpy(), Cd, off,
                                   q.numpy(), p.u_lo.numpy(), p.u_hi.numpy())
    gmax = np.abs(g).reshape(B, -1).max(1)
    print(f"({nx},{nu}): max |g(z_final)| per instance {gmax}")
    assert (gmax < 1e-10).all(), gmax
    gbar = np.random.default_rng(1).standard_normal(zf.shape)
    w = dense_w(Hd, Hs, gbar)
    Cg = 0.5 * (w[..., :, None] * zf[..., None, :] + zf[..., :, None] * w[..., None, :])
    rng = np.random.default_rng(2)
    probes = []
    for _ in range(8):
        idx = tuple(int(rng.integers(0, s)) for s in C.shape)
        vals = []
        for sgn in (1.0, -1.0):
            Cp = C.clone()
            Cp[idx] += sgn * FD_H
            vals.append(float((gbar * stage(Cp)["z"].numpy()).sum()))
        probes.append((Cg[idx], (vals[0] - vals[1]) / (2 * FD_H)))
    scale = max(abs(a) for a, _ in probes)
    err = max(abs(a - fd) for a, fd in probes) / scale
    print(f"({nx},{nu}): dC vs central differences: {err:.2e} (relative to the largest probed gradient {scale:.3g})")
    assert err < FD_TOL, (err, probes)


# ---- 4. host wiring -------------------------------------------------------------------------------------------------
class _WiringBackend(DenseOracleBackend):
    """backward with `dyn=` as HipBackend's takes it (tests/test_dyn_grad_cpu.py's _DynOracleBackend, on this backend)."""

    def backward(self, dims, factor, F, rho, z_final, gbar, q_grad, Qd_grad, **kw):
        self.z_final = z_final.detach().clone()
        super().backward(dims, factor, F, rho, z_final, gbar, q_grad, Qd_grad)
        dyn = kw.get("dyn")
        if dyn is not None:
            n = lambda a: a.detach().numpy()
            for out, ref in zip((dyn.dF, dyn.dc, dyn.dx0), dyn_grads(n(q_grad), n(F), n(z_final), n(dyn.lam), n(rho))):
                if out is not None:
                    out.copy_(torch.from_numpy(ref))


@pytest.mark.parametrize("exit_mode", ["fixed", "reference"])
def test_mpc_dense_cost_end_to_end(exit_mode):
    from deq_mpc_corl_amd import QuadCost, synthetic_dense_cost, synthetic_problem
    from deq_mpc_corl_amd.qpth.al_utils import LinDx
    nx, nu, B, T = 4, 2, 5, 5
    p = synthetic_problem(B, T, nx, nu, seed=7, dtype=F64, active=True)
    C0, q0 = synthetic_dense_cost(p, 7)
    # an unsymmetric C with the same symmetric part: the solve must see only that part, the gradient both halves
    skew = torch.randn(C0.shape, generator=torch.Generator().manual_seed(1), dtype=F64)
    C = (C0 + 0.1 * (skew - skew.transpose(-1, -2))).requires_grad_(True)
    q = q0.clone().requires_grad_(True)
    F, f, x0 = (a.clone().requires_grad_(True) for a in (p.F, p.c, p.x0))
    be = _WiringBackend()
    mpc = _mpc((B, T, nx, nu), p.u_lo, p.u_hi, be, False, exit_mode)
    mpc.reinitialize(p.x0, None)
    x, u, _ = mpc(x0, QuadCost(C, q), LinDx(F, f), None, x_init=p.z0[..., :nx].clone(), u_init=p.z0[..., nx:].clone())
    assert set(be.calls) == {"solve_lin_dense"}   # never solve_lin
    gen = torch.Generator().manual_seed(5)
    gx, gu_ = torch.randn(x.shape, generator=gen), torch.randn(u.shape, generator=gen)
    ((x * gx).sum() + (u * gu_).sum()).backward()
    n = lambda a: a.detach().numpy().astype(np.float64)
    w, zf = n(q.grad), n(be.z_final)
    assert C.grad is not None and C.grad.shape == C.shape and np.abs(w).max() > 0
    assert torch.equal(C.grad, C.grad.transpose(-1, -2))
    want = 0.5 * (w[..., :, None] * zf[..., None, :] + zf[..., :, None] * w[..., None, :])
    assert np.abs(n(C.grad) - want).max() <= 1e-14 * np.abs(want).max()
    ref = dyn_grads(w, n(F), zf, n(mpc.lamda_prev), n(mpc.rho_prev).reshape(-1) / 10.0)
    for k, got, wnt in zip(("F", "f", "x0"), (F.grad, f.grad, x0.grad), ref):
        err = np.abs(n(got) - wnt).max() / np.abs(wnt).max()
        print(f"{exit_mode}: d{k} next to the dense cost vs dyn_grads on the MPC's outputs: {err:.2e}")
        assert err < 1e-10, (k, err)
    # the solve saw the symmetric part only: the same iterate from C0
    be2 = _WiringBackend()
    m2 = _mpc((B, T, nx, nu), p.u_lo, p.u_hi, be2, False, exit_mode)
    x2, u2, _ = _solve(m2, C0, q0, p.F, p.c, p.x0, p.z0, nx)
    assert (x2 - x.detach()).abs().max() < 1e-6 and (u2 - u.detach()).abs().max() < 1e-6
    # get_cost evaluates the full quadratic form at the returned iterate
    z = torch.cat((x2, u2), -1).to(F64)
    full = (0.5 * torch.einsum("bti,btij,btj->b", z, C0, z) + (q0 * z).sum((-1, -2)))
    assert torch.allclose(m2.get_cost(QuadCost(C0, q0)).to(F64), full, rtol=1e-6)


def test_stream_route_takes_the_dense_cost():
    from deq_mpc_corl_amd import QuadCost, synthetic_dense_cost, synthetic_problem
    from deq_mpc_corl_amd.qpth.al_utils import LinDx
    nx, nu, B, T = 2, 1, 3, 4
    p = synthetic_problem(B, T, nx, nu, seed=2, dtype=F64, active=True)
    C, q = synthetic_dense_cost(p, 2)
    outs = []
    for stream in (False, True):
        be = DenseOracleBackend()
        mpc = _mpc((B, T, nx, nu), p.u_lo, p.u_hi, be, False, "fixed")
        mpc.reinitialize(p.x0, None)
        solve = mpc.al_solve_stream if stream else mpc.al_solve
        x, u, _ = solve(p.z0[..., :nx].clone(), p.z0[..., nx:].clone(), LinDx(p.F, p.c), None, p.x0, QuadCost(C, q))
        assert set(be.calls) == {"solve_lin_dense"}
        outs.append(torch.cat((x, u), -1))
    assert torch.equal(outs[0], outs[1])   # al_iter = 2 on both routes, rho stays below rho_max


def test_guarded_combinations_raise():
    from deq_mpc_corl_amd import MPC, PendulumDynamics, QuadCost, synthetic_dense_cost, synthetic_problem
    from deq_mpc_corl_amd.qpth.al_utils import LinDx
    from deq_mpc_corl_amd.qpth.AL_mpc_custom import Obstacle_MPC
    nx, nu, B, T = 2, 1, 3, 4
    p = synthetic_problem(B, T, nx, nu, seed=2, dtype=F64, active=True)
    C, q = synthetic_dense_cost(p, 2)
    kw = dict(u_lower=p.u_lo, u_upper=p.u_hi, n_batch=B, dtype=F64, backend=DenseOracleBackend(), diag_cost=False)
    with pytest.raises(NotImplementedError, match="state_estimator"):
        MPC(nx, nu, T, state_estimator=True, **kw)
    with pytest.raises(NotImplementedError, match="Obstacle_MPC"):
        Obstacle_MPC(3, nu, T, **kw)
    dyn = PendulumDynamics()
    mpc = MPC(nx, nu, T, **kw)
    mpc.reinitialize(p.x0, None)
    with pytest.raises(NotImplementedError, match="LinDx"):   # a callable dx
        mpc(p.x0, QuadCost(C, q), dyn, dyn.jac, x_init=p.z0[..., :nx].clone(), u_init=p.z0[..., nx:].clone())
    mpc = MPC(nx, nu, T, **kw)
    mpc.reinitialize(p.x0, None)
    mpc.linearize_once = True
    with pytest.raises(NotImplementedError, match="linearize_once"):
        mpc.al_solve_stream(p.z0[..., :nx].clone(), p.z0[..., nx:].clone(), LinDx(p.F, p.c), dyn.jac, p.x0, QuadCost(C, q))
    for bad in (dict(add_goal_constraint=True), dict(ineqG=torch.zeros(1))):   # still not built
        with pytest.raises(NotImplementedError):
            MPC(nx, nu, T, **kw, **bad)


# ---- 5. generator ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,nu", [(13, 4), (4, 2), (2, 1)])
def test_generator_conditions(nx, nu):
    p, C, q, o1, stage = _stationary_stage(nx, nu)
    assert torch.equal(C, C.transpose(-1, -2))
    ev = torch.linalg.eigvalsh(C)
    off = (C - torch.diag_embed(C.diagonal(dim1=-2, dim2=-1))).abs().max().item()
    assert ev.min() > 0
    xref_q = -torch.einsum("btij,btj->bti", C, p.xref)
    assert torch.allclose(q, xref_q)
    u = stage(C)["z"][..., nx:]
    on = int((u.abs() >= p.u_hi.reshape(-1)[0] - 1e-9).sum())
    print(f"({nx},{nu}): smallest eigenvalue {ev.min().item():.3g}, largest off-diagonal {off:.2f}, "
          f"controls on a bound {on} of {u.numel()}")
    assert on > u.numel() // 2
