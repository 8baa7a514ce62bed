"""The quad kernels' triangular solves on own elements (csrc/alqp_quad.hpp: lsolve_own, ltsolve_own; emulated on the
CPU in test_quad_own_solves_emulation.py) at the smallest shapes at which their slot arithmetic can go wrong:

* dims (2,1), (4,2), (6,1), (12,4), (13,4), (14,4): n % 4 = 3, 2, 3, 0, 1, 2 and nx % 4 = 2, 0, 2, 0, 1, 2 - a last slot
  with 1, 2, 3 and 4 rows, an x / u boundary inside and at the end of a slot;
* T = 2 (one dynamics stage, and the clamp on the last stage's F) and T = 5;
* B = 1 (a lone quad in the wavefront) and B = 17 (odd: the last fp32 record pair is half used);
* fp32 and fp64 (the fp64 W panel lives in LDS and is only read by these solves).

T = 1 cannot be computed: the C ABI's minimum horizon is 2 (mi_alqp.h, AlqpDims.T; tests/test_cabi.py pins
alqp_supported == 0 for T < 2), so no kernel can be asked for a problem without a dynamics stage. One test of its own,
test_horizon_one_is_refused, holds that the entry points say so; the grids below start at T = 2. The stage without
dynamics rows that every sweep has (t = T - 1) runs in every case.

Nothing here depends on which form of the solves the library holds: the file passes with the library built from the
commit before the own-element solves as well (MI_ALQP_LIB selects the library)."""
import numpy as np
import pytest
import torch

from oracle import oracle_py as orc
from tests.test_gpu_nonlin_scale import _problem
from tests.test_gpu_parity import FP32_QUAD_TEAM_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TD = {"f32": torch.float32, "f64": torch.float64}
DIMS = [(2, 1), (4, 2), (6, 1), (12, 4), (13, 4), (14, 4)]
HORIZONS = [2, 5]
BATCHES = [1, 17]
# quad against team Newton direction, relative to max(1, |d|max): the tolerances of
# test_newton_step_quad_with_extra_rows_equals_team. Largest measured at these shapes on the MI355X, with the library
# before the own-element solves / with them: fp64 7.8e-16 / 9.0e-16, fp32 5.6e-7 / 5.6e-7
STEP_TOL = {"f64": 1e-9, "f32": 2e-3}
SOLVE_SEED = 11

grid = pytest.mark.parametrize("nx,nu,T,B,dtype", [(nx, nu, T, B, dt) for (nx, nu) in DIMS for T in HORIZONS
                                                   for B in BATCHES for dt in ("f32", "f64")])


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("nx,nu", DIMS)
def test_horizon_one_is_refused(nx, nu, dtype):
    """T = 1 is below the ABI's minimum horizon: the Newton step (with a workspace) and the fused quad solve return
    their error instead of launching."""
    from deq_mpc_corl_amd.backend import default_backend
    be = default_backend()
    dt, B, T = TD[dtype], 17, 1
    dims = (B, T, nx, nu)
    assert not be.supported(B, T, nx, nu, dt)
    new = lambda *shape: torch.zeros(*shape, dtype=dt, device=DEV)
    z, lam, rho = new(B, T, nx + nu), new(B, T * nx + 2 * T * nu), torch.ones(B, dtype=dt, device=DEV)
    F, c, x0 = new(B, 1, nx, nx + nu), new(B, 1, nx), new(B, nx)
    Qd, q, ulo, uhi = torch.ones_like(z), new(B, T, nx + nu), -torch.ones(nu, dtype=dt, device=DEV), torch.ones(nu, dtype=dt, device=DEV)
    with pytest.raises(RuntimeError, match="bad argument|unsupported"):
        be.newton_step(dims, z, c, F, x0, lam, rho, Qd, q, ulo, uhi, 0, 0, torch.empty_like(z), workspace=new(1 << 16))
    with pytest.raises(RuntimeError, match="bad argument|unsupported"):
        be.solve_lin(dims, Qd, q, F, c, x0, ulo, uhi, 0, 0, z, lam, rho, new(B), new(B),
                     torch.zeros(B, dtype=torch.int32, device=DEV), torch.zeros(B, dtype=torch.uint8, device=DEV),
                     al_iter=2, max_newton=4, n_ls=20, flags=3, variant="quad", workspace=new(1 << 16))
    assert float(z.abs().max()) == 0.0   # nothing ran


def _step_inputs(dims, dt, with_obs):
    B, T, nx, nu = dims
    p, z, xn, lam, rho = _problem(B, T, nx, nu, dt, seed=nx * 10 + nu, active=True)
    obs = None
    if with_obs:
        nobs = 4
        g = torch.Generator(device="cpu").manual_seed(11)
        pos = (z[:, :, None, :3].cpu().double() + 0.25 * torch.randn(B, T, nobs, 3, generator=g, dtype=torch.float64)).to(dt).to(DEV).contiguous()
        obs = (pos, 0.3)
        lam_o = (0.2 * torch.rand(B, T, nobs, generator=g, dtype=torch.float64)).to(dt).to(DEV)
        lam = torch.cat([lam[:, :T * nx], torch.cat([lam[:, T * nx:].reshape(B, T, 2 * nu), lam_o], 2).reshape(B, -1)], 1).contiguous()
    return p, z, xn, lam, rho, obs


def _step(be, dims, inp, ws):
    p, z, xn, lam, rho, obs = inp
    d = torch.full_like(z, float("nan"))
    info = torch.zeros(dims[0], dtype=torch.int32, device=DEV)
    be.newton_step(dims, z, xn, p.F, p.x0, lam, rho, p.Qd, p.q, p.u_lo, p.u_hi, 0, 0, d, info=info, obs=obs, workspace=ws)
    torch.cuda.synchronize()
    assert int(info.abs().max()) == 0
    return d


def _row_sets(nx):
    # obstacle rows constrain the position x[0:3]
    return (False, True) if nx >= 3 else (False,)


@grid
def test_quad_step_equals_team_step(nx, nu, T, B, dtype):
    """One Newton direction through the quad kernels (forward sweep, then the backward sweep's two solves per stage,
    d straight to the caller) against the team kernel, on the same problem without and with obstacle rows."""
    from deq_mpc_corl_amd.backend import default_backend
    be = default_backend()
    dt, dims = TD[dtype], (B, T, nx, nu)
    for with_obs in _row_sets(nx):
        inp = _step_inputs(dims, dt, with_obs)
        d_team = _step(be, dims, inp, None).cpu().numpy()
        d_quad = _step(be, dims, inp, be.new_workspace(dims, inp[1])).cpu().numpy()
        err = np.abs(d_quad - d_team).max() / max(1.0, float(np.abs(d_team).max()))
        print(f"quad vs team step ({nx},{nu}) T={T} B={B} {dtype} obs={with_obs}: {err:.3e}")
        assert np.isfinite(d_quad).all()
        assert err < STEP_TOL[dtype], (with_obs, err)


@grid
def test_quad_step_reads_nothing_unwritten(nx, nu, T, B, dtype):
    """The same step on a workspace full of NaN: every record word a sweep reads was written by that launch, so d is
    finite and the same bits as on a zeroed workspace."""
    from deq_mpc_corl_amd.backend import default_backend
    be = default_backend()
    dt, dims = TD[dtype], (B, T, nx, nu)
    for with_obs in _row_sets(nx):
        inp = _step_inputs(dims, dt, with_obs)
        ws = be.new_workspace(dims, inp[1])
        d_clean = _step(be, dims, inp, ws.zero_())
        d_poison = _step(be, dims, inp, ws.fill_(float("nan")))
        assert bool(torch.isfinite(d_poison).all()), with_obs
        assert torch.equal(d_clean, d_poison), with_obs


@grid
def test_quad_fused_solve_against_oracle(nx, nu, T, B, dtype):
    """The fused solve (two AL iterations of four Newton steps: forward and backward sweep per step, line search on the
    backward sweep's own elements in fp32) against the CPU oracle. fp32 by the rule of test_gpu_quad_record_layout.py
    scaled to the batch: median below 1e-5, at most one instance in 17 at or above 2e-3 (a line-search near-tie)."""
    from deq_mpc_corl_amd import synthetic_problem
    from deq_mpc_corl_amd.backend import default_backend
    be = default_backend()
    dt, dims = TD[dtype], (B, T, nx, nu)
    p = synthetic_problem(B, T, nx, nu, seed=SOLVE_SEED, dtype=dt, device=DEV)
    z = p.z0.clone()
    lam = torch.zeros(B, T * nx + 2 * T * nu, dtype=dt, device=DEV)
    rho = torch.ones(B, dtype=dt, device=DEV)
    phi = torch.zeros(B, dtype=dt, device=DEV)
    rn2 = torch.zeros(B, dtype=dt, device=DEV)
    info = torch.zeros(B, dtype=torch.int32, device=DEV)
    st = torch.zeros(B, dtype=torch.uint8, device=DEV)
    be.solve_lin(dims, p.Qd, p.q, p.F, p.c, p.x0, p.u_lo, p.u_hi, 0, 0, z, lam, rho, phi, rn2, info, st,
                 al_iter=2, max_newton=4, n_ls=20, flags=3, variant="quad")
    torch.cuda.synchronize()
    assert be.last_variant == "quad"
    c = lambda a: a.cpu().numpy()
    o = orc.solve_lin(dtype, c(p.Qd), c(p.q), c(p.F), c(p.c), c(p.x0), c(p.u_lo), c(p.u_hi), c(p.z0), al_iter=2,
                      exit_mode="fixed")
    assert int(info.abs().sum()) == 0 and bool(st.all())
    assert np.isfinite(c(z)).all() and np.isfinite(c(lam)).all()
    err = np.abs(c(z) - o["z"]).reshape(B, -1).max(1)
    print(f"quad fused solve ({nx},{nu}) T={T} B={B} {dtype}: median {np.median(err):.3e}, max {err.max():.3e}, "
          f"{int((err >= 2e-3).sum())} at or above 2e-3")
    if dtype == "f64":
        assert err.max() < 1e-9, err
    else:
        assert np.median(err) < 1e-5 and (err >= 2e-3).sum() <= B // 17, np.sort(err)[-4:]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("nx,nu", [(13, 4), (6, 1)])
def test_quad_backward_pass_equals_team_factor(nx, nu, dtype):
    """Gradients w.r.t. q and diag(Q) through k_backward_quad (forward substitution over the horizon, then the backward
    sweep, on the factor the quad solve left in its workspace) against the team kernels' packed factor, as
    test_backward_quad_workspace_equals_team_factor does at (13,4), B = 37, T = 9, and at its tolerances."""
    from deq_mpc_corl_amd import MPC, AffineDynamics, QuadCost, synthetic_problem
    from deq_mpc_corl_amd.backend import HipBackend

    dt = TD[dtype]
    B, T = 17, 5
    p = synthetic_problem(B, T, nx, nu, seed=31, dtype=dt, device=DEV, active=True)
    g = torch.Generator(device="cpu").manual_seed(2)
    wx = torch.randn(B, T, nx, generator=g).to(DEV)
    wu = torch.randn(B, T, nu, generator=g).to(DEV)
    grads = {}
    for name in ("quad", "team"):
        be = HipBackend()
        calls = []
        if name == "quad":
            be.QUAD_MIN_BATCH = 0   # below 4096 the host logic would keep the packed factor of the team kernels
            bw_ws = be.backward_ws
            be.backward_ws = lambda *a, _f=bw_ws, _c=calls: (_c.append(1), _f(*a))[1]
        else:
            be.default_variant = "team"
        mpc = MPC(nx, nu, T, u_lower=p.u_lo, u_upper=p.u_hi, n_batch=B, dtype=dt, exit_mode="fixed", backend=be)
        if name == "team":
            class _NoWs:   # hides the workspace route from the host logic (hasattr check)
                def __init__(self, inner): self._i = inner
                def __getattr__(self, k):
                    if k == "backward_ws": raise AttributeError(k)
                    return getattr(self._i, k)
            mpc._backend = _NoWs(be)
        mpc.reinitialize(p.x0, None)
        mpc.al_iter = 2
        Qd = p.Qd.clone().requires_grad_(True)
        q = p.q.clone().requires_grad_(True)
        dyn = AffineDynamics(p.F, p.c)
        cost = QuadCost(torch.diag_embed(Qd), q, torch.zeros(B, T, device=DEV, dtype=dt))
        x, u, _ = mpc(p.x0, cost, dyn, dyn.jac, x_init=p.z0[..., :nx].clone(), u_init=p.z0[..., nx:].clone())
        ((x * wx).sum() + (u * wu).sum()).backward()
        assert bool(calls) == (name == "quad")
        grads[name] = (q.grad.clone(), Qd.grad.clone(), x.detach().clone())
    eq = float((grads["quad"][0] - grads["team"][0]).abs().max()) / float(grads["team"][0].abs().max())
    eQ = float((grads["quad"][1] - grads["team"][1]).abs().max()) / float(grads["team"][1].abs().max())
    ex = float((grads["quad"][2] - grads["team"][2]).abs().max())
    print(f"quad vs team backward ({nx},{nu}) {dtype}: x {ex:.2e}, q_grad {eq:.2e}, Qd_grad {eQ:.2e}")
    if dtype == "f64":
        assert ex <= 1e-5 and eq < 1e-6 and eQ < 1e-6
    else:
        assert ex < FP32_QUAD_TEAM_TOL["x"] and eq < FP32_QUAD_TEAM_TOL["grad"] and eQ < FP32_QUAD_TEAM_TOL["grad"]
