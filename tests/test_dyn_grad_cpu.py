"""Gradients w.r.t. the affine dynamics (F, c) and the initial state x0 through the AL solve, without a GPU.

With w = -H^{-1} gbar (H: Hessian of the last executed Newton step, rho: the penalty it was built with), v_t the
dynamics rows of the multipliers the solve RETURNED and s_t = w_{t+1}[0:nx] - F_t w_t (include/mi_alqp.h,
alqp_backward_* with an AlqpBwdDyn):

    dF_t[i][j] = -v_t[i] w_t[j] - rho s_t[i] z_final,t[j]      dc_t[i] = -rho s_t[i]      dx0[i] = -rho w_0[i]

`dyn_grads` below is those three lines in numpy; the GPU tests (tests/test_gpu_dyn_grad.py) import it as their
reference. Here it is pinned by central finite differences through the CPU oracle's solve, and the host wiring of MPC
(which inputs join the autograd node, what reaches the backend) runs on an oracle-backed test backend."""
import numpy as np
import pytest
import torch

from oracle import oracle_py as orc
from tests.oracle_backend import OracleBackend


def dyn_grads(w, F, z, lam_eq, rho):
    """w, z [B,T,n]; F [B,T-1,nx,n]; lam_eq [B, >= (T-1) nx] (returned multipliers, dynamics rows first); rho [B]
    -> dF [B,T-1,nx,n], dc [B,T-1,nx], dx0 [B,nx] (float64)."""
    w, F, z, lam_eq = (np.asarray(a, np.float64) for a in (w, F, z, lam_eq))
    B, Tm1, nx, n = F.shape
    rho = np.asarray(rho, np.float64).reshape(B)
    v = lam_eq[:, :Tm1 * nx].reshape(B, Tm1, nx)
    s = w[:, 1:, :nx] - np.einsum("btij,btj->bti", F, w[:, :-1])
    r3, r2 = rho[:, None, None], rho[:, None]
    dF = -v[..., None] * w[:, :-1, None, :] - r3[..., None] * s[..., None] * z[:, :-1, None, :]
    return dF, -r3 * s, -r2 * w[:, 0, :nx]


def _dense_w(Hd, Hs, gbar):
    """w = -H^{-1} gbar with H assembled from grad_hess's blocks."""
    B, T, n = gbar.shape
    w = np.empty_like(gbar)
    for b in range(B):
        H = np.zeros((T * n, T * n))
        for t in range(T):
            H[t * n:(t + 1) * n, t * n:(t + 1) * n] = Hd[b, t]
        for t in range(T - 1):
            H[(t + 1) * n:(t + 2) * n, t * n:(t + 1) * n] = Hs[b, t]
            H[t * n:(t + 1) * n, (t + 1) * n:(t + 2) * n] = Hs[b, t].T
        w[b] = -np.linalg.solve(H, gbar[b].reshape(-1)).reshape(T, n)
    return w


FD_H = 1e-5
# central differences against the formulas, relative to the largest probed analytic gradient. Measured on the oracle
# (fp64, these probes): (4,2) 1.1e-10, (13,4) 1.5e-10, (2,1) 4.4e-11, (6,1) 3.4e-11; the bound is ~100x the largest.
FD_TOL = 1e-8


@pytest.mark.parametrize("nx,nu", [(4, 2), (13, 4), (2, 1), (6, 1)])
def test_formulas_vs_finite_differences(nx, nu):
    from deq_mpc_corl_amd import synthetic_problem
    B, T = 4, 5
    p = synthetic_problem(B, T, nx, nu, seed=3, dtype=torch.float64, active=True)
    c = lambda a: a.numpy().copy()
    Qd, q, F, cc, x0, lo, hi, z0 = (c(a) for a in (p.Qd, p.q, p.F, p.c, p.x0, p.u_lo, p.u_hi, p.z0))
    # warm stage, then the tested stage: one AL iteration of 8 Newton steps from (z1, lam1, rho1), stationary at its end
    o1 = orc.solve_lin("f64", Qd, q, F, cc, x0, lo, hi, z0, al_iter=2, max_newton=4)
    z1, lam1, rho1 = o1["z"], o1["lam"], o1["rho"]
    assert np.allclose(rho1, 100.0)

    def stage(F_, c_, x0_):
        return orc.solve_lin("f64", Qd, q, F_, c_, x0_, lo, hi, z1, lam0=lam1, rho0=rho1, al_iter=1, max_newton=8,
                             exit_mode="fixed")

    o = stage(F, cc, x0)
    zf, lam_out = o["z"], o["lam"]
    gbar = np.random.default_rng(1).standard_normal(zf.shape)
    loss = lambda oo: float((gbar * oo["z"]).sum())

    xn = np.einsum("btij,btj->bti", F, zf[:, :-1]) + cc
    g, Hd, Hs = orc.grad_hess("f64", zf, xn, F, x0, lam1, rho1, Qd, q, lo, hi)
    gmax = np.abs(g).reshape(B, -1).max(1)
    print(f"({nx},{nu}): max |g(z_final)| per instance {gmax}")
    assert (gmax < 1e-10).all(), gmax   # every instance, no exclusions

    # what the kernels rely on: after the dual update the returned lam holds lam_in + rho r(z_final) on the equality rows
    # (dynamics rows t nx + i, then the initial-state rows), unclamped
    neq = T * nx
    r = np.concatenate(((zf[:, 1:, :nx] - xn).reshape(B, -1), zf[:, 0, :nx] - x0), axis=1)
    id_err = np.abs(lam_out[:, :neq] - (lam1[:, :neq] + rho1[:, None] * r)).max()
    print(f"({nx},{nu}): returned lam vs lam_in + rho r(z_final): {id_err:.2e}")
    assert id_err < 1e-12
    nact = int((np.abs(zf[..., nx:]) >= hi.reshape(-1)[0] - 1e-12).sum())
    print(f"({nx},{nu}): controls on or beyond a bound at z_final: {nact} of {B * T * nu}")

    w = _dense_w(Hd, Hs, gbar)
    dF, dc, dx0 = dyn_grads(w, F, zf, lam_out, rho1)

    rng = np.random.default_rng(2)
    probes = []   # (name, analytic, finite difference)
    for name, arr, grad in (("F", F, dF), ("c", cc, dc), ("x0", x0, dx0)):
        for _ in range(4):
            idx = tuple(int(rng.integers(0, s)) for s in arr.shape)
            vals = []
            for sgn in (1.0, -1.0):
                a = arr.copy()
                a[idx] += sgn * FD_H
                args = {"F": (a, cc, x0), "c": (F, a, x0), "x0": (F, cc, a)}[name]
                vals.append(loss(stage(*args)))
            probes.append((name, grad[idx], (vals[0] - vals[1]) / (2 * FD_H)))
    scale = max(abs(a) for _, a, _ in probes)
    for name in ("F", "c", "x0"):
        e = max(abs(a - fd) for nm, a, fd in probes if nm == name) / scale
        print(f"({nx},{nu}): d{name} vs central differences: {e:.2e} (relative to the largest probed gradient {scale:.3g})")
    err = max(abs(a - fd) for _, a, fd in probes) / scale
    assert err < FD_TOL, (err, probes)


class _DynOracleBackend(OracleBackend):
    """OracleBackend whose backward takes `dyn=` as HipBackend's does: w from orc.backward (it is q_grad), the three
    outputs from dyn_grads. Records whether each call carried the argument."""

    def __init__(self):
        self.dyn_seen = []

    def backward(self, dims, factor, F, rho, z_final, gbar, q_grad, Qd_grad, **kw):
        self.dyn_seen.append("dyn" in kw)
        self.z_final = z_final.detach().clone()
        super().backward(dims, factor, F, rho, z_final, gbar, q_grad, Qd_grad)
        dyn = kw.get("dyn")
        if dyn is None:
            return
        n = lambda t: t.detach().numpy()
        lam = n(dyn.lam) if dyn.lam is not None else np.zeros((dims[0], (dims[1] - 1) * dims[2]))
        for out, ref in zip((dyn.dF, dyn.dc, dyn.dx0), dyn_grads(n(q_grad), n(F), n(z_final), lam, n(rho))):
            if out is not None:
                out.copy_(torch.from_numpy(ref))


def _mpc_run(exit_mode, dyn_grad, seed=7):
    from deq_mpc_corl_amd import MPC, QuadCost, synthetic_problem
    from deq_mpc_corl_amd.qpth.al_utils import LinDx
    nx, nu, B, T = 4, 2, 5, 5
    p = synthetic_problem(B, T, nx, nu, seed=seed, dtype=torch.float64, active=True)
    be = _DynOracleBackend()
    mpc = MPC(nx, nu, T, u_lower=p.u_lo, u_upper=p.u_hi, n_batch=B, dtype=torch.float64, exit_mode=exit_mode, al_iter=2,
              backend=be)
    mpc.reinitialize(p.x0, None)
    C = torch.diag_embed(p.Qd).requires_grad_(True)
    cq = p.q.clone().requires_grad_(True)
    F, f, x0 = (t.clone().requires_grad_(dyn_grad) for t in (p.F, p.c, p.x0))
    x, u, _ = mpc(x0, QuadCost(C, cq), LinDx(F, f), None, x_init=p.z0[..., :nx].clone(), u_init=p.z0[..., nx:].clone())
    gen = torch.Generator().manual_seed(5)
    gx = torch.randn(x.shape, generator=gen, dtype=torch.float64).to(x.dtype)
    gu = torch.randn(u.shape, generator=gen, dtype=torch.float64).to(u.dtype)
    ((x * gx).sum() + (u * gu).sum()).backward()
    return dict(mpc=mpc, be=be, C=C, c=cq, F=F, f=f, x0=x0, x=x, u=u, gbar=torch.cat((gx, gu), -1))


@pytest.mark.parametrize("exit_mode", ["fixed", "reference"])
def test_mpc_returns_dynamics_gradients(exit_mode):
    r = _mpc_run(exit_mode, True)
    assert r["be"].dyn_seen == [True]
    for k in ("F", "f", "x0"):
        assert r[k].grad is not None, f"{k}.grad is None"
        assert r[k].grad.dtype == r[k].dtype and r[k].grad.shape == r[k].shape
    # the same chain by hand on the MPC's own results: its float64 z_final (x, u are returned as float32; the backend
    # kept what backward was handed), the lam it returned and rho_prev / 10; w is the gradient w.r.t. the cost's c
    mpc = r["mpc"]
    n = lambda t: t.detach().numpy().astype(np.float64)
    zf = n(r["be"].z_final)
    assert np.abs(zf - np.concatenate((n(r["x"]), n(r["u"])), -1)).max() < 1e-6 * np.abs(zf).max()
    ref = dyn_grads(n(r["c"].grad), n(r["F"]), zf, n(mpc.lamda_prev), n(mpc.rho_prev).reshape(-1) / 10.0)
    for k, want in zip(("F", "f", "x0"), ref):
        err = np.abs(n(r[k].grad) - want).max() / np.abs(want).max()
        print(f"{exit_mode}: d{k} vs helper on the MPC's outputs: {err:.2e}")
        assert err < 1e-10, (k, err)
    # without the new inputs: the same C / c gradients, and no `dyn` at the backend
    r0 = _mpc_run(exit_mode, False)
    assert r0["be"].dyn_seen == [False]
    assert all(r0[k].grad is None for k in ("F", "f", "x0"))
    assert torch.equal(r0["C"].grad, r["C"].grad) and torch.equal(r0["c"].grad, r["c"].grad)
