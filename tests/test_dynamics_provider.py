"""pendulum1l dynamics provider: the oracle restatement against vectors
produced by the reference's own CasADi-generated code (tests/golden/dyn_pendulum1l.npz,
tools/gen_dyn_golden.py), and the HIP kernel against both."""
import os

import numpy as np
import pytest
import torch

from oracle import dyn_py

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "dyn_pendulum1l.npz"))
GOLDC = np.load(os.path.join(os.path.dirname(__file__), "golden", "dyn_cartpole1l.npz"))
GOLDC2 = np.load(os.path.join(os.path.dirname(__file__), "golden", "dyn_cartpole2l.npz"))


@pytest.mark.parametrize("tag", ["h05", "h01"])
def test_restatement_matches_reference_vectors(tag):
    xn, A, B = dyn_py.pendulum1l(GOLD["x"], GOLD["u"], float(GOLD[tag + "_h"]))
    assert np.abs(xn - GOLD[tag + "_xn"]).max() < 5e-14   # omega reaches 25: relative 2e-15
    assert np.abs(A - GOLD[tag + "_A"]).max() < 1e-14
    assert np.abs(B - GOLD[tag + "_B"]).max() < 1e-14


def test_restatement_jacobian_is_the_derivative_of_the_step():
    """Independent of the goldens: central differences of the step itself."""
    x, u, h = GOLD["x"][:64], GOLD["u"][:64], 0.05
    _, A, B = dyn_py.pendulum1l(x, u, h)
    eps = 1e-6
    for j in range(2):
        dx = np.zeros_like(x); dx[:, j] = eps
        num = (dyn_py.pendulum1l(x + dx, u, h)[0] - dyn_py.pendulum1l(x - dx, u, h)[0]) / (2 * eps)
        assert np.abs(num - A[:, :, j]).max() < 1e-7
    du = np.full_like(u, eps)
    num = (dyn_py.pendulum1l(x, u + du, h)[0] - dyn_py.pendulum1l(x, u - du, h)[0]) / (2 * eps)
    assert np.abs(num - B[:, :, 0]).max() < 1e-7


@pytest.mark.skipif(not dyn_py.have_ref(), reason="oracle/_ref not built (the reference sources were not available to build())")
def test_compiled_reference_reproduces_its_fixture():
    xn, A, B = dyn_py.pendulum1l_ref(GOLD["x"][:32], GOLD["u"][:32], 0.05)
    assert np.array_equal(xn, GOLD["h05_xn"][:32]) and np.array_equal(A, GOLD["h05_A"][:32])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,tol", [(torch.float64, 5e-13), (torch.float32, 2e-5)])
@pytest.mark.parametrize("tag", ["h05", "h01"])
def test_hip_provider_matches_reference_vectors(dtype, tol, tag):
    from deq_mpc_corl_amd import Pendulum1lDynamics
    dev = "cuda:0"
    x = torch.tensor(GOLD["x"], dtype=dtype, device=dev)
    u = torch.tensor(GOLD["u"], dtype=dtype, device=dev)
    dyn = Pendulum1lDynamics(dt=float(GOLD[tag + "_h"]))
    xn, (A, B) = dyn.jac(x, u)
    xo = dyn(x, u)
    torch.cuda.synchronize()
    scale = 1.0 + np.abs(GOLD[tag + "_xn"])
    assert (np.abs(xn.cpu().numpy() - GOLD[tag + "_xn"]) / scale).max() < tol
    assert np.abs(A.cpu().numpy() - GOLD[tag + "_A"]).max() < tol
    assert np.abs(B.cpu().numpy() - GOLD[tag + "_B"]).max() < tol
    assert torch.equal(xo, xn)


@pytest.mark.gpu
def test_hip_provider_ragged_sizes_and_cpu_tensors_fail_loudly():
    from deq_mpc_corl_amd import Pendulum1lDynamics
    dyn = Pendulum1lDynamics(dt=0.05)
    for K in (1, 255, 257, 1000):
        x = torch.randn(K, 2, dtype=torch.float64, device="cuda:0")
        u = torch.randn(K, 1, dtype=torch.float64, device="cuda:0")
        xn, (A, B) = dyn.jac(x, u)
        o = dyn_py.pendulum1l(x.cpu().numpy(), u.cpu().numpy(), 0.05)
        assert np.abs(xn.cpu().numpy() - o[0]).max() < 1e-12 and np.abs(A.cpu().numpy() - o[1]).max() < 1e-12
        assert A.shape == (K, 2, 2) and B.shape == (K, 2, 1)
    with pytest.raises(RuntimeError):
        dyn(torch.zeros(4, 2, dtype=torch.float64), torch.zeros(4, 1, dtype=torch.float64))


@pytest.mark.gpu
def test_package_twin_has_the_reference_signature():
    """dynamics(q, qdot, tau, h[bsz,1]) -> [q', qdot'], derivatives(...) -> six [bsz,1,1] blocks in
    the order of my_envs/pendulum1l/src/dynamics_cpu.cpp:81-107."""
    from deq_mpc_corl_amd.dynamics import pendulum1l
    dev = "cuda:0"
    x = torch.tensor(GOLD["x"], dtype=torch.float64, device=dev)
    u = torch.tensor(GOLD["u"], dtype=torch.float64, device=dev)
    h = torch.full((x.shape[0], 1), 0.05, dtype=torch.float64, device=dev)
    qn, qdn = pendulum1l.dynamics(x[:, :1].contiguous(), x[:, 1:].contiguous(), u, h)
    assert qn.shape == (x.shape[0], 1)
    assert np.abs(torch.cat((qn, qdn), 1).cpu().numpy() - GOLD["h05_xn"]).max() < 5e-13
    J = pendulum1l.derivatives(x[:, :1].contiguous(), x[:, 1:].contiguous(), u, h)
    assert len(J) == 6 and all(j.shape == (x.shape[0], 1, 1) for j in J)
    assert np.abs(J[1].cpu().numpy()[:, 0, 0] - GOLD["h05_A"][:, 0, 1]).max() < 5e-13   # dq'/dqdot
    assert np.abs(J[5].cpu().numpy()[:, 0, 0] - GOLD["h05_B"][:, 1, 0]).max() < 5e-13   # dqdot'/dtau


@pytest.mark.gpu
def test_mpc_nonlinear_mode_with_the_hip_provider():
    """The drop-in MPC in nonlinear-caller mode driven by the kernel provider: same result as
    with an equivalent PyTorch implementation of the same dynamics (autograd Jacobians)."""
    from deq_mpc_corl_amd import MPC, QuadCost, Pendulum1lDynamics
    dev, dt = "cuda:0", torch.float64
    B, T = 48, 8
    g = torch.Generator().manual_seed(5)
    x0 = torch.stack([torch.rand(B, generator=g) * 2 - 1, torch.randn(B, generator=g)], 1).to(dt).to(dev)
    Qd = torch.tensor([10.0, 1.0, 0.1], dtype=dt, device=dev).expand(B, T, 3).contiguous()
    q = torch.zeros(B, T, 3, dtype=dt, device=dev)
    h = 0.05

    def f_torch(x, u):
        def acc(th):
            return 4.0 * u[:, 0] - 19.62 * torch.sin(th)
        th, om = x[:, 0], x[:, 1]
        k1t, k1o = om, acc(th)
        k2t, k2o = om + 0.5 * h * k1o, acc(th + 0.5 * h * k1t)
        k3t, k3o = om + 0.5 * h * k2o, acc(th + 0.5 * h * k2t)
        k4t, k4o = om + h * k3o, acc(th + h * k3t)
        return torch.stack([th + h / 6 * (k1t + 2 * k2t + 2 * k3t + k4t), om + h / 6 * (k1o + 2 * k2o + 2 * k3o + k4o)], 1)

    def f_torch_jac(x, u):
        with torch.enable_grad():   # the MPC evaluates dynamics under no_grad
            xr, ur = x.detach().requires_grad_(True), u.detach().requires_grad_(True)
            xn = f_torch(xr, ur)
            rows = [torch.autograd.grad(xn[:, i].sum(), (xr, ur), retain_graph=True) for i in range(2)]
        A = torch.stack([r[0] for r in rows], 1)
        Bm = torch.stack([r[1] for r in rows], 1)
        return xn.detach(), (A, Bm)

    res = {}
    for name, dx, dxj in (("hip", None, None), ("torch", f_torch, f_torch_jac)):
        if name == "hip":
            prov = Pendulum1lDynamics(dt=h)
            dx, dxj = prov, prov.jac
        mpc = MPC(2, 1, T, u_lower=-2.0, u_upper=2.0, n_batch=B, dtype=dt)
        mpc.reinitialize(x0, None)
        mpc.al_iter = 2
        cost = QuadCost(torch.diag_embed(Qd), q, torch.zeros(B, T, dtype=dt, device=dev))
        x, u, _ = mpc(x0, cost, dx, dxj)
        res[name] = (x.cpu(), u.cpu(), list(mpc.last_newton_per_al))
    assert res["hip"][2] == res["torch"][2]
    assert torch.allclose(res["hip"][0], res["torch"][0], atol=1e-6)
    assert torch.allclose(res["hip"][1], res["torch"][1], atol=1e-6)


# ---- cartpole1l ------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["h05", "h01"])
def test_cartpole_restatement_matches_reference_vectors(tag):
    xn, J = dyn_py.cartpole1l(GOLDC["x"], GOLDC["tau"], float(GOLDC[tag + "_h"]))
    assert np.abs(xn - GOLDC[tag + "_xn"]).max() < 5e-14
    assert np.abs(J - GOLDC[tag + "_J"]).max() < 1e-14


def test_cartpole_restatement_jacobian_is_the_derivative_of_the_step():
    x, tau, h = GOLDC["x"][:64], GOLDC["tau"][:64], 0.05
    _, J = dyn_py.cartpole1l(x, tau, h)
    eps = 1e-6
    for j in range(6):
        dx, dt_ = np.zeros_like(x), np.zeros_like(tau)
        if j < 4:
            dx[:, j] = eps
        else:
            dt_[:, j - 4] = eps
        num = (dyn_py.cartpole1l(x + dx, tau + dt_, h)[0] - dyn_py.cartpole1l(x - dx, tau - dt_, h)[0]) / (2 * eps)
        assert np.abs(num - J[:, :, j]).max() < 2e-6


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,tol", [(torch.float64, 5e-13), (torch.float32, 5e-5)])
@pytest.mark.parametrize("tag", ["h05", "h01"])
def test_hip_cartpole_matches_reference_vectors(dtype, tol, tag):
    from deq_mpc_corl_amd.backend import default_backend
    be = default_backend()
    dev = "cuda:0"
    x = torch.tensor(GOLDC["x"], dtype=dtype, device=dev)
    tau = torch.tensor(GOLDC["tau"], dtype=dtype, device=dev)
    xn, J = be.dyn_cartpole1l(x, tau, float(GOLDC[tag + "_h"]))
    torch.cuda.synchronize()
    scale = 1.0 + np.abs(GOLDC[tag + "_xn"])
    assert (np.abs(xn.cpu().numpy() - GOLDC[tag + "_xn"]) / scale).max() < tol
    assert np.abs(J.cpu().numpy() - GOLDC[tag + "_J"]).max() < tol


@pytest.mark.gpu
def test_hip_cartpole_class_and_package_twin():
    from deq_mpc_corl_amd import Cartpole1lDynamics
    from deq_mpc_corl_amd.dynamics import cartpole1l
    dev, dt = "cuda:0", torch.float64
    sel = GOLDC["tau"][:, 1] == 0          # the rows the environments can produce: tau = (u, 0)
    x = torch.tensor(GOLDC["x"][sel], dtype=dt, device=dev)
    u = torch.tensor(GOLDC["tau"][sel][:, :1], dtype=dt, device=dev)
    dyn = Cartpole1lDynamics(dt=0.05)
    xn, (A, B) = dyn.jac(x, u)
    assert A.shape == (x.shape[0], 4, 4) and B.shape == (x.shape[0], 4, 1)
    assert np.abs(xn.cpu().numpy() - GOLDC["h05_xn"][sel]).max() < 5e-13
    assert np.abs(A.cpu().numpy() - GOLDC["h05_J"][sel][:, :, :4]).max() < 5e-13
    assert np.abs(B.cpu().numpy() - GOLDC["h05_J"][sel][:, :, 4:5]).max() < 5e-13
    assert torch.equal(dyn(x, u), xn)
    xa = torch.tensor(GOLDC["x"], dtype=dt, device=dev)
    ta = torch.tensor(GOLDC["tau"], dtype=dt, device=dev)
    h = torch.full((xa.shape[0], 1), 0.05, dtype=dt, device=dev)
    qn, qdn = cartpole1l.dynamics(xa[:, :2].contiguous(), xa[:, 2:].contiguous(), ta, h)
    assert np.abs(torch.cat((qn, qdn), 1).cpu().numpy() - GOLDC["h05_xn"]).max() < 5e-13
    blocks = cartpole1l.derivatives(xa[:, :2].contiguous(), xa[:, 2:].contiguous(), ta, h)
    assert len(blocks) == 6 and all(b.shape == (xa.shape[0], 2, 2) for b in blocks)
    assert np.abs(blocks[4].cpu().numpy() - GOLDC["h05_J"][:, 2:, 2:4]).max() < 5e-13   # dqdot'/dqdot


# ---- cartpole1l_v2 (the reference's second one-link package: same model, lighter cart and pole) ----
GOLDV2 = np.load(os.path.join(os.path.dirname(__file__), "golden", "dyn_cartpole1l_v2.npz"))


@pytest.mark.parametrize("tag", ["h05", "h01"])
def test_cartpole_v2_restatement_matches_reference_vectors(tag):
    xn, J = dyn_py.cartpole1l_v2(GOLDV2["x"], GOLDV2["tau"], float(GOLDV2[tag + "_h"]))
    assert np.abs(xn - GOLDV2[tag + "_xn"]).max() < 5e-13      # accelerations are ~15x those of cartpole1l at the same force
    assert np.abs(J - GOLDV2[tag + "_J"]).max() < 5e-13
    # and it is NOT the first package's model: the two fixtures differ by far more than any tolerance here
    assert np.abs(GOLDV2[tag + "_xn"] - GOLDC[tag + "_xn"]).max() > 1e-2


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,tol", [(torch.float64, 5e-12), (torch.float32, 5e-4)])
@pytest.mark.parametrize("tag", ["h05", "h01"])
def test_hip_cartpole_v2_matches_reference_vectors(dtype, tol, tag):
    from deq_mpc_corl_amd.backend import default_backend
    be = default_backend()
    dev = "cuda:0"
    x = torch.tensor(GOLDV2["x"], dtype=dtype, device=dev)
    tau = torch.tensor(GOLDV2["tau"], dtype=dtype, device=dev)
    xn, J = be.dyn_cartpole1l(x, tau, float(GOLDV2[tag + "_h"]), version=2)
    torch.cuda.synchronize()
    scale = 1.0 + np.abs(GOLDV2[tag + "_xn"])
    assert (np.abs(xn.cpu().numpy() - GOLDV2[tag + "_xn"]) / scale).max() < tol
    assert (np.abs(J.cpu().numpy() - GOLDV2[tag + "_J"]) / (1.0 + np.abs(GOLDV2[tag + "_J"]))).max() < tol


@pytest.mark.gpu
def test_hip_cartpole_v2_class_package_twin_and_mpc():
    """`Cartpole1lV2Dynamics` / `dynamics.cartpole1l_v2` against the fixture, and an MPC on that model (provider kernels
    between the solver's launches, nonlinear-caller mode) against the same MPC driven by the CPU restatement."""
    from deq_mpc_corl_amd import MPC, Cartpole1lV2Dynamics, QuadCost
    from deq_mpc_corl_amd.dynamics import cartpole1l_v2
    dev, dt = "cuda:0", torch.float64
    sel = GOLDV2["tau"][:, 1] == 0
    x = torch.tensor(GOLDV2["x"][sel], dtype=dt, device=dev)
    u = torch.tensor(GOLDV2["tau"][sel][:, :1], dtype=dt, device=dev)
    dyn = Cartpole1lV2Dynamics(dt=0.05)
    xn, (A, B) = dyn.jac(x, u)
    assert np.abs(xn.cpu().numpy() - GOLDV2["h05_xn"][sel]).max() < 5e-12
    assert np.abs(A.cpu().numpy() - GOLDV2["h05_J"][sel][:, :, :4]).max() < 5e-11
    assert np.abs(B.cpu().numpy() - GOLDV2["h05_J"][sel][:, :, 4:5]).max() < 5e-11
    xa = torch.tensor(GOLDV2["x"], dtype=dt, device=dev)
    ta = torch.tensor(GOLDV2["tau"], dtype=dt, device=dev)
    h = torch.full((xa.shape[0], 1), 0.05, dtype=dt, device=dev)
    qn, qdn = cartpole1l_v2.dynamics(xa[:, :2].contiguous(), xa[:, 2:].contiguous(), ta, h)
    assert np.abs(torch.cat((qn, qdn), 1).cpu().numpy() - GOLDV2["h05_xn"]).max() < 5e-12
    assert len(cartpole1l_v2.derivatives(xa[:, :2].contiguous(), xa[:, 2:].contiguous(), ta, h)) == 6

    class CpuDyn:   # the same model through the CPU restatement (test infrastructure)
        def __call__(self, xx, uu):
            o = dyn_py.cartpole1l_v2(xx.detach().cpu().numpy(), np.concatenate([uu.detach().cpu().numpy(), np.zeros((uu.shape[0], 1))], 1), 0.05)[0]
            return torch.as_tensor(o, dtype=dt, device=xx.device)

        def jac(self, xx, uu):
            o, Jn = dyn_py.cartpole1l_v2(xx.detach().cpu().numpy(), np.concatenate([uu.detach().cpu().numpy(), np.zeros((uu.shape[0], 1))], 1), 0.05)
            Jt = torch.as_tensor(Jn, dtype=dt, device=xx.device)
            return torch.as_tensor(o, dtype=dt, device=xx.device), (Jt[..., :4], Jt[..., 4:5])

    B_, T = 12, 8
    g = torch.Generator().manual_seed(3)
    x0 = (0.3 * torch.randn(B_, 4, generator=g, dtype=dt)).to(dev)
    Qd = torch.cat((torch.full((B_, T, 4), 5.0, dtype=dt), torch.full((B_, T, 1), 1e-2, dtype=dt)), -1).to(dev)
    q = (0.1 * torch.randn(B_, T, 5, generator=g, dtype=dt)).to(dev)
    out = []
    for prov in (dyn, CpuDyn()):
        mpc = MPC(4, 1, T, u_lower=torch.tensor([-2.0], dtype=dt, device=dev), u_upper=torch.tensor([2.0], dtype=dt, device=dev),
                  n_batch=B_, dtype=dt)
        mpc.reinitialize(x0, None)
        mpc.al_iter = 2
        xs, us, _ = mpc(x0, QuadCost(torch.diag_embed(Qd), q, torch.zeros(B_, T, dtype=dt, device=dev)), prov, prov.jac)
        out.append((xs.cpu(), us.cpu(), list(mpc.last_newton_per_al)))
    assert out[0][2] == out[1][2]
    assert torch.allclose(out[0][0], out[1][0], atol=1e-6) and torch.allclose(out[0][1], out[1][1], atol=1e-6)


# ---- nonlinear fused solve (alqp_solve_nonlin) ----------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("env", ["pendulum1l", "cartpole1l", "cartpole1l_v2", "cartpole2l"])
@pytest.mark.parametrize("dtype,tol", [(torch.float64, 5e-7), (torch.float32, 2e-3)])
def test_fused_nonlinear_solve_equals_the_launch_per_step_path(env, dtype, tol):
    """One launch with the model inlined against the host-driven nonlinear-caller mode (kernel per
    Newton-step phase, provider kernels for dx / dx_jac - the path that is validated against the
    reference's nonlinear goldens), both with exit_mode='fixed'. Active bounds included."""
    from deq_mpc_corl_amd import MPC, QuadCost, Pendulum1lDynamics, Cartpole1lDynamics, Cartpole1lV2Dynamics, Cartpole2lDynamics
    dev = "cuda:0"
    prov = {"pendulum1l": Pendulum1lDynamics, "cartpole1l": Cartpole1lDynamics, "cartpole1l_v2": Cartpole1lV2Dynamics,
            "cartpole2l": Cartpole2lDynamics}[env](0.05)
    nx, T, B = prov.nx, (6 if env == "pendulum1l" else 9), 70
    n = nx + 1
    g = torch.Generator().manual_seed(11)
    x0 = (0.6 * torch.randn(B, nx, generator=g)).to(dtype).to(dev)
    Qd = (0.5 + torch.rand(B, T, n, generator=g)).to(dtype).to(dev)
    Qd[..., -1] = 0.05
    q = (0.3 * torch.randn(B, T, n, generator=g)).to(dtype).to(dev)
    ub = {"pendulum1l": 0.4, "cartpole1l_v2": 0.3}.get(env, 3.0)   # tight: the bound rows become active

    class Plain:                                        # same kernels, but no fused_id: launch-per-step path
        def __call__(self, x, u):
            return prov(x, u)

        def jac(self, x, u):
            return prov.jac(x, u)

    res = {}
    for name, dyn in (("fused", prov), ("stepwise", Plain())):
        mpc = MPC(nx, 1, T, u_lower=-ub, u_upper=ub, n_batch=B, dtype=dtype, exit_mode="fixed", prefer_fused=True)
        mpc.reinitialize(x0, None)
        mpc.al_iter = 3
        cost = QuadCost(torch.diag_embed(Qd), q, torch.zeros(B, T, dtype=dtype, device=dev))
        x, u, _ = mpc(x0, cost, dyn, dyn.jac)
        res[name] = (x.double().cpu(), u.double().cpu(), mpc.lamda_prev.double().cpu(), mpc.rho_prev.double().cpu())
    assert float(res["fused"][2][:, T * nx:].max()) > 0                      # bounds were active
    if dtype == torch.float64:
        # identical after one AL iteration (1e-16); afterwards the two factorisations (root-free LDL'
        # here, Cholesky in the step kernel) differ by rounding, which rho = 10, 100 amplifies in lam,
        # and x, u are returned in fp32 (AL_mpc.py:337-338): one fp32 ulp
        assert torch.allclose(res["fused"][0], res["stepwise"][0], atol=5e-7)
        assert torch.allclose(res["fused"][1], res["stepwise"][1], atol=5e-7)
        # (cartpole1l_v2: the light cart makes the same force 15x the acceleration - the rounding difference of the two
        #  factorisations shows up an order of magnitude larger in lam)
        la, lr = (5e-4, 1e-5) if env == "cartpole1l_v2" else (2e-5, 1e-6)
        dl = (res["fused"][2] - res["stepwise"][2]).abs()
        assert bool((dl <= la + lr * res["stepwise"][2].abs()).all()), float(dl.max())
    else:
        # fp32: a near-tie in a 20-point line search may pick another candidate for single instances
        err = (res["fused"][0] - res["stepwise"][0]).abs().reshape(B, -1).max(1).values
        assert float(err.median()) < 1e-4 and float((err < tol).float().mean()) >= 0.9
    assert torch.equal(res["fused"][3], res["stepwise"][3])


# ---- against the REFERENCE MPC driving its own compiled pendulum1l package ------------------
import tests.golden_util as gu  # noqa: E402

CASADI_GOLDENS = ["pend1l_casadi_f64_al2", "pend1l_casadi_active_f64_al3",
                  "cart1l_casadi_f64_al2", "cart1l_casadi_active_f64_al3"]


@pytest.mark.parametrize("name", CASADI_GOLDENS)
def test_host_logic_with_restated_dynamics_vs_reference_mpc(name):
    """CPU: the drop-in MPC (test-only oracle backend) in nonlinear-caller mode with the RESTATED
    pendulum dynamics against qpth.AL_mpc.MPC run on the reference's compiled CasADi package
    (tools/gen_golden.py `CasadiPendulum1l`): same Newton-step counts, same x, u, lam, rho."""
    from deq_mpc_corl_amd import MPC, QuadCost
    from tests.oracle_backend import OracleBackend
    g = gu.load(name)
    dt = torch.float64
    B, T, nx = g["B"], g["T"], g["nx"]

    class Dyn:
        def __call__(self, x, u):
            return self.jac(x, u)[0]

        def jac(self, x, u):
            if name.startswith("pend"):
                xn, A, Bm = dyn_py.pendulum1l(x.detach().numpy(), u.detach().numpy(), 0.05)
            else:
                xn, J = dyn_py.cartpole1l(x.detach().numpy(), np.concatenate([u.detach().numpy(), np.zeros((u.shape[0], 1))], 1), 0.05)
                A, Bm = J[:, :, :4].copy(), J[:, :, 4:5].copy()
            return torch.from_numpy(xn), (torch.from_numpy(A), torch.from_numpy(Bm))

    tt = lambda a: torch.tensor(a, dtype=dt)
    mpc = MPC(nx, 1, T, u_lower=tt(g["u_lo"]), u_upper=tt(g["u_hi"]), n_batch=B, dtype=dt, backend=OracleBackend())
    x0 = tt(g["x0"])
    mpc.reinitialize(x0, None)
    mpc.al_iter = g["al_iter"]
    z0 = tt(g["z0"])
    Qd = tt(g["Qd"]).requires_grad_(True)
    q = tt(g["q"]).requires_grad_(True)
    cost = QuadCost(torch.diag_embed(Qd), q, torch.zeros(B, T, dtype=dt))
    dyn = Dyn()
    x, u, _ = mpc(x0, cost, dyn, dyn.jac, x_init=z0[..., :nx].clone(), u_init=z0[..., nx:].clone())
    assert list(mpc.last_newton_per_al) == list(g["newton_per_al"])
    ((x * torch.tensor(g["bwd_wx"])).sum() + (u * torch.tensor(g["bwd_wu"])).sum()).backward()
    assert np.abs(q.grad.numpy() - g["bwd_q_grad"]).max() < 1e-5 * np.abs(g["bwd_q_grad"]).max()
    assert np.abs(Qd.grad.numpy() - g["bwd_Qd_grad"]).max() < 1e-5 * np.abs(g["bwd_Qd_grad"]).max()
    x, u = x.detach(), u.detach()
    assert np.abs(x.numpy() - g["x"]).max() < 2e-5 and np.abs(u.numpy() - g["u"]).max() < 2e-5
    assert np.abs(mpc.lamda_prev.numpy() - g["lam_final"]).max() < 1e-6 * max(1.0, np.abs(g["lam_final"]).max())
    assert np.array_equal(mpc.rho_prev.numpy().reshape(-1), g["rho_final"].reshape(-1))


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASADI_GOLDENS)
@pytest.mark.parametrize("path", ["one launch (alqp_solve_nonlin)", "one launch per Newton step, reference exit",
                                  "provider kernels, launch per phase, reference exit"])
@pytest.mark.parametrize("with_grad", [False, True])
def test_gpu_nonlinear_paths_vs_reference_mpc(name, path, with_grad):
    """Both GPU routes of the nonlinear MPC against the reference MPC run on its own compiled
    pendulum1l / cartpole1l package. Where the reference executed all 4 Newton steps in every AL
    iteration (the pendulum fixtures) the fixed-4-step fused launch is comparable as well; the
    cartpole fixtures (early batch-global exits: [2,1] and [1,1,4] steps) pin the reference-exit
    route and its step counts."""
    from deq_mpc_corl_amd import MPC, QuadCost, Pendulum1lDynamics, Cartpole1lDynamics
    g = gu.load(name)
    if path.startswith("one launch (") and not all(k == 4 for k in g["newton_per_al"]):
        pytest.skip("the reference left its Newton loop early in this fixture: only the reference-exit route is comparable")
    dt, dev = torch.float64, "cuda:0"
    B, T, nx = g["B"], g["T"], g["nx"]
    tt = lambda a: torch.tensor(a, dtype=dt, device=dev)
    prov = Pendulum1lDynamics(0.05) if name.startswith("pend") else Cartpole1lDynamics(0.05)
    mode = "fixed" if path.startswith("one launch (") else "reference"
    if path.startswith("provider kernels"):
        class Plain:            # no fused_id: dx / dx_jac as plain callables between kernel launches
            def __call__(self, x, u):
                return prov_k(x, u)

            def jac(self, x, u):
                return prov_k.jac(x, u)

        prov_k, prov = prov, None
        prov = Plain()
    mpc = MPC(nx, 1, T, u_lower=tt(g["u_lo"]), u_upper=tt(g["u_hi"]), n_batch=B, dtype=dt, exit_mode=mode)
    x0 = tt(g["x0"])
    mpc.reinitialize(x0, None)
    mpc.al_iter = g["al_iter"]
    z0 = tt(g["z0"])
    Qd, q = tt(g["Qd"]), tt(g["q"])
    if with_grad:   # NewtonAL.backward (al_utils.py:578-615): gradients w.r.t. q and diag Q from the saved factor
        Qd.requires_grad_(True)
        q.requires_grad_(True)
    cost = QuadCost(torch.diag_embed(Qd), q, torch.zeros(B, T, dtype=dt, device=dev))
    x, u, _ = mpc(x0, cost, prov, prov.jac, x_init=z0[..., :nx].clone(), u_init=z0[..., nx:].clone())
    assert list(mpc.last_newton_per_al) == list(g["newton_per_al"])
    if with_grad:
        ((x * torch.tensor(g["bwd_wx"], device=dev)).sum() + (u * torch.tensor(g["bwd_wu"], device=dev)).sum()).backward()
        assert np.abs(q.grad.cpu().numpy() - g["bwd_q_grad"]).max() < 1e-5 * np.abs(g["bwd_q_grad"]).max()
        assert np.abs(Qd.grad.cpu().numpy() - g["bwd_Qd_grad"]).max() < 1e-5 * np.abs(g["bwd_Qd_grad"]).max()
        x, u = x.detach(), u.detach()
    assert np.abs(x.cpu().numpy() - g["x"]).max() < 2e-5 and np.abs(u.cpu().numpy() - g["u"]).max() < 2e-5
    assert np.abs(mpc.lamda_prev.cpu().numpy() - g["lam_final"]).max() < 1e-6 * max(1.0, np.abs(g["lam_final"]).max())
    assert np.array_equal(mpc.rho_prev.cpu().numpy().reshape(-1), g["rho_final"].reshape(-1))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_fused_nonlinear_solve_does_not_depend_on_workspace_contents(dtype):
    """The bug class the reference-MPC fixture caught (a residual block read before it was written,
    masked by a previous identical run's leftovers): NaN-poisoned, zeroed and huge-valued workspaces
    must give bit-identical results."""
    from deq_mpc_corl_amd import MPC, QuadCost, Cartpole1lDynamics
    from deq_mpc_corl_amd.backend import default_backend
    be = default_backend()
    dev = "cuda:0"
    prov = Cartpole1lDynamics(0.05)
    B, T, nx = 21, 7, 4
    g = torch.Generator().manual_seed(3)
    x0 = (0.5 * torch.randn(B, nx, generator=g)).to(dtype).to(dev)
    Qd = (0.5 + torch.rand(B, T, 5, generator=g)).to(dtype).to(dev)
    q = (0.3 * torch.randn(B, T, 5, generator=g)).to(dtype).to(dev)
    xi = (0.4 * torch.randn(B, T, nx, generator=g)).to(dtype).to(dev)     # NOT a rollout: residuals != 0
    ui = (0.4 * torch.randn(B, T, 1, generator=g)).to(dtype).to(dev)
    outs = []
    for fill in (float("nan"), 0.0, 1e30):
        for ws in be._ws.values():
            ws.fill_(fill)
        mpc = MPC(nx, 1, T, u_lower=-1.0, u_upper=1.0, n_batch=B, dtype=dtype, exit_mode="fixed")
        mpc.reinitialize(x0, None)
        mpc.al_iter = 2
        cost = QuadCost(torch.diag_embed(Qd), q, torch.zeros(B, T, dtype=dtype, device=dev))
        x, u, _ = mpc(x0, cost, prov, prov.jac, x_init=xi.clone(), u_init=ui.clone())
        if not outs:                                   # first pass allocates the workspace: poison it and redo
            for ws in be._ws.values():
                ws.fill_(fill)
            mpc = MPC(nx, 1, T, u_lower=-1.0, u_upper=1.0, n_batch=B, dtype=dtype, exit_mode="fixed")
            mpc.reinitialize(x0, None)
            mpc.al_iter = 2
            x, u, _ = mpc(x0, cost, prov, prov.jac, x_init=xi.clone(), u_init=ui.clone())
        outs.append((x.clone(), u.clone(), mpc.lamda_prev.clone()))
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert torch.equal(a, b)
    assert bool(torch.isfinite(outs[0][0]).all())


# ---- cartpole2l ------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["h05", "h01"])
def test_cartpole2l_restatement_matches_reference_vectors(tag):
    xn, J = dyn_py.cartpole2l(GOLDC2["x"], GOLDC2["tau"], float(GOLDC2[tag + "_h"]))
    assert np.abs(xn - GOLDC2[tag + "_xn"]).max() < 5e-14
    assert np.abs(J - GOLDC2[tag + "_J"]).max() < 2e-14


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,tol", [(torch.float64, 2e-12), (torch.float32, 2e-4)])
@pytest.mark.parametrize("tag", ["h05", "h01"])
def test_hip_cartpole2l_matches_reference_vectors(dtype, tol, tag):
    from deq_mpc_corl_amd.backend import default_backend
    be = default_backend()
    dev = "cuda:0"
    x = torch.tensor(GOLDC2["x"], dtype=dtype, device=dev)
    tau = torch.tensor(GOLDC2["tau"], dtype=dtype, device=dev)
    xn, J = be.dyn_cartpole2l(x, tau, float(GOLDC2[tag + "_h"]))
    xo, _ = be.dyn_cartpole2l(x, tau, float(GOLDC2[tag + "_h"]), want_jac=False)
    torch.cuda.synchronize()
    scale = 1.0 + np.abs(GOLDC2[tag + "_xn"])
    assert (np.abs(xn.cpu().numpy() - GOLDC2[tag + "_xn"]) / scale).max() < tol
    assert (np.abs(J.cpu().numpy() - GOLDC2[tag + "_J"]) / (1.0 + np.abs(GOLDC2[tag + "_J"]))).max() < tol
    assert torch.allclose(xo, xn, rtol=0, atol=1e-12 if dtype == torch.float64 else 1e-5)


@pytest.mark.gpu
def test_hip_cartpole2l_class_and_package_twin():
    from deq_mpc_corl_amd import Cartpole2lDynamics
    from deq_mpc_corl_amd.dynamics import cartpole2l
    dev, dt = "cuda:0", torch.float64
    sel = (GOLDC2["tau"][:, 1] == 0) & (GOLDC2["tau"][:, 2] == 0)
    x = torch.tensor(GOLDC2["x"][sel], dtype=dt, device=dev)
    u = torch.tensor(GOLDC2["tau"][sel][:, :1], dtype=dt, device=dev)
    dyn = Cartpole2lDynamics(dt=0.05)
    xn, (A, B) = dyn.jac(x, u)
    assert A.shape == (x.shape[0], 6, 6) and B.shape == (x.shape[0], 6, 1)
    assert np.abs(xn.cpu().numpy() - GOLDC2["h05_xn"][sel]).max() < 2e-12
    assert np.abs(A.cpu().numpy() - GOLDC2["h05_J"][sel][:, :, :6]).max() < 2e-12
    assert np.abs(B.cpu().numpy() - GOLDC2["h05_J"][sel][:, :, 6:7]).max() < 2e-12
    xa = torch.tensor(GOLDC2["x"], dtype=dt, device=dev)
    ta = torch.tensor(GOLDC2["tau"], dtype=dt, device=dev)
    h = torch.full((xa.shape[0], 1), 0.05, dtype=dt, device=dev)
    qn, qdn = cartpole2l.dynamics(xa[:, :3].contiguous(), xa[:, 3:].contiguous(), ta, h)
    assert np.abs(torch.cat((qn, qdn), 1).cpu().numpy() - GOLDC2["h05_xn"]).max() < 2e-12
    blocks = cartpole2l.derivatives(xa[:, :3].contiguous(), xa[:, 3:].contiguous(), ta, h)
    assert len(blocks) == 6 and all(b.shape == (xa.shape[0], 3, 3) for b in blocks)
    assert np.abs(blocks[5].cpu().numpy() - GOLDC2["h05_J"][:, 3:, 6:9]).max() < 2e-12   # dqdot'/dtau
