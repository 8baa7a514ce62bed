"""CPU checks of tests/nonlin_reference.py, the helpers of tests/test_gpu_nonlin_quad.py (alqp_solve_nonlin against the CPU
oracle): the plant of all four models, the problem generator (the model's own rollout as the start, control rows that end
active, bounds [nu] and [B,T,nu]), the driver (it is MPC's route on OracleBackend), the Hessian / backward reference, and the
line-search conditions of every case on the oracle alone: the fp64 oracle decides every line search, the fp32 oracle leaves
at every step at least three quarters of a batch compared and a one-instance case in full. Nothing here touches a GPU."""
import numpy as np
import pytest
import torch

from oracle import dyn_py
from tests import nonlin_reference as nl
from tests import nonlin_rows_reference as nr
from tests.dense_cost_reference import dense_w
from tests.oracle_backend import OracleBackend

IDS = [nl.case_id(c) for c in nl.CASES]
cases = pytest.mark.parametrize("model,T,B,pbt", nl.CASES, ids=IDS)


def test_case_list_covers_every_model_horizon_and_batch():
    assert {c[0] for c in nl.CASES} == set(nl.MODELS) and len(nl.CASES) <= 12
    assert {c[1] for c in nl.CASES} == {2, 5, 9} and {c[2] for c in nl.CASES} == {1, 17, 33}
    assert any(c[3] for c in nl.CASES) and {c[0] for c in nl.GRAD_CASES} == set(nl.MODELS)
    assert nr.MODELS == {"pendulum1l": (2, 1, 1), "cartpole1l": (4, 1, 2), "cartpole1l_v2": (4, 1, 4)}   # left as it was
    from deq_mpc_corl_amd import dynamics as dy
    for model, (nx, nu, dyn_id) in nl.MODELS.items():
        prov = nl.provider(model)
        assert (prov.nx, prov.nu, prov.fused_id, prov.dt) == (nx, nu, dyn_id, nl.H_STEP)
    assert isinstance(nl.provider("cartpole2l"), dy.Cartpole2lDynamics)


@pytest.mark.parametrize("model", list(nl.MODELS))
def test_plant_is_the_restatement(model):
    nx, nu, _ = nl.MODELS[model]
    g = torch.Generator().manual_seed(2)
    x = 0.5 * torch.randn(9, nx, generator=g, dtype=torch.float64)
    u = 0.5 * torch.randn(9, nu, generator=g, dtype=torch.float64)
    plant = nl.OraclePlant(model)
    xn, (A, Bm) = plant.jac(x, u)
    assert torch.equal(plant(x, u), xn) and A.shape == (9, nx, nx) and Bm.shape == (9, nx, nu)
    if model == "cartpole2l":   # tau = (u, 0, 0), as Cartpole2lDynamics._tau pads it
        tau = np.concatenate([u.numpy(), np.zeros((9, 2))], 1)
        ro, J = dyn_py.cartpole2l(x.numpy(), tau, nl.H_STEP)
        assert np.array_equal(xn.numpy(), ro) and np.array_equal(A.numpy(), J[..., :6]) and np.array_equal(Bm.numpy(), J[..., 6:7])
    else:
        ro, (Ao, Bo) = nr.OraclePlant(model).jac(x, u)
        assert torch.equal(xn, ro) and torch.equal(A, Ao) and torch.equal(Bm, Bo)
    eps = 1e-6   # the Jacobian is the derivative of the step: central differences
    J = torch.cat((A, Bm), -1)
    for j in range(nx + nu):
        dx, du = torch.zeros_like(x), torch.zeros_like(u)
        (dx if j < nx else du)[:, j if j < nx else j - nx] = eps
        num = (plant(x + dx, u + du) - plant(x - dx, u - du)) / (2 * eps)
        assert float((num - J[..., j]).abs().max()) < 2e-6
    # results in the arguments' dtype
    assert plant(x.float(), u.float()).dtype == torch.float32


@cases
def test_problem_generator(model, T, B, pbt):
    pr, plant = nl.problem(model, B, T, pbt, torch.float64)
    nx, nu, dyn_id = nl.MODELS[model]
    assert pr["dims"] == (B, T, nx, nu) and pr["dyn_id"] == dyn_id
    z0 = pr["z0"]
    assert torch.equal(z0[:, 0, :nx], pr["x0"])
    assert torch.equal(nl.ssr.true_next(plant, z0, nx), z0[:, 1:, :nx])   # the start is the model's own rollout
    assert float((pr["q"][..., :nx] / pr["Qd"][..., :nx] + z0[..., :nx]).abs().min()) == pytest.approx(nl.PULL)
    if pbt:
        assert pr["lo"].shape == (B, T, nu) and nl.strides(pr) == (T * nu, nu)
        assert len(torch.unique(pr["hi"])) == B * T * nu
    else:
        assert pr["lo"].shape == (nu,) and nl.strides(pr) == (0, 0)
    assert float(pr["hi"].max()) <= nl.U_BOUND + 0.02 and float(pr["lo"].min()) >= -nl.U_BOUND - 0.02
    z, lam, rho = nl.start(pr)
    assert lam.shape == (B, T * nx + 2 * T * nu) and not lam.any() and bool((rho == 1).all())
    p32, _ = nl.problem(model, B, T, pbt, torch.float32)
    assert p32["z0"].dtype == torch.float32 and torch.equal(p32["z0"], z0.float())


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@cases
def test_control_rows_end_active_and_ties_stay_within_the_caps(model, T, B, pbt, dtype):
    """On the oracle alone, for the seed the GPU tests use: control rows active at the solve's end in at least three
    quarters of the instances (a one-instance case: in it) with multipliers > 0; the fp64 oracle decides every line search
    of both AL iterations; the fp32 oracle keeps the caps in each."""
    pr, plant, its, (z, lam, rho), _, _ = nl.oracle_solve(model, T, B, pbt, dtype)
    act, lam_pos = nl.controls_active(pr, z, lam)
    assert act.mean() >= 0.75 and lam_pos.mean() >= 0.75 and (B > 1 or (act.all() and lam_pos.all())), (act.sum(), lam_pos.sum())
    assert bool((rho == 100).all()) and torch.isfinite(z).all()
    counts = []
    for _, tr in its:
        und = nl.undecided_steps(tr, nl.tie_tol(pr, dtype))
        counts.append(und.sum(1).tolist())
        if dtype == "f64":
            assert not und.any(), counts
        else:
            assert nl.tie_caps_ok(und, B), counts
        assert (tr["accept"] == 1).any() and float(tr["d"].abs().max()) > 0
    print(f"{nl.case_id((model, T, B, pbt))} {dtype}: undecided picks per step {counts}")
    und, undecided, tied = nl.solve_ties(its, pr, dtype)
    assert und.shape == (8, B) and np.array_equal(undecided, und.any(0)) and ((tied > 0) == undecided).all()


def test_seed_is_the_first_that_meets_the_caps():
    for c in (nl.CASES[0], nl.CASES[5], nl.CASES[7]):   # a one-instance case and the two with the most fp32 ties
        assert nl.choose_seed(*c) == nl.SEED


def test_tie_helpers():
    phi = torch.tensor([[[3.0, 1.0], [1.0, 1.0 + 1e-9], [2.0, 5.0]]]).expand(2, 3, 2).contiguous()   # [S=2, 3 candidates, B=2]
    tr = dict(phi=phi, phi_prev=torch.full((2, 2), 9.0))
    und = nl.undecided_steps(tr, 1e-6)
    assert und.tolist() == [[False, True], [False, True]]
    assert nl.compared(und).tolist() == [[True, True], [True, False]]
    assert not nl.tie_caps_ok(und, 2) and nl.tie_caps_ok(und[:1], 2) and nl.tie_caps_ok(np.zeros((4, 1), bool), 1)
    assert not nl.tie_caps_ok(np.array([[True], [False]]), 1)
    tr["phi_prev"][0, 0] = 1.0   # the best merit within the tolerance of the previous one: undecided accept
    assert nl.undecided_steps(tr, 1e-6)[0].tolist() == [True, True]


@pytest.mark.parametrize("mode", ["fixed", "reference"])
@pytest.mark.parametrize("model,T,B,pbt", nl.GRAD_CASES, ids=[nl.case_id(c) for c in nl.GRAD_CASES])
def test_driver_is_mpcs_route_and_fp64_decides_the_gradient_cases(model, T, B, pbt, mode):
    """MPC on OracleBackend with the plant (the route the reference's goldens pin) marks no undecided line search in fp64, in
    either exit mode; with the fixed exit it is the driver's solve, bit for bit."""
    pr, ref, newton, und, tied = nl.oracle_grads(model, T, B, pbt, mode, "f64")
    assert not und.any() and len(newton) == 2 and 1 <= min(newton) and max(newton) <= 4
    assert np.abs(ref["dq"]).max() > 0 and np.abs(ref["dQd"]).max() > 0
    if mode == "fixed":
        _, _, _, (z, lam, rho), _, _ = nl.oracle_solve(model, T, B, pbt, "f64")
        assert newton == [4, 4] and np.array_equal(ref["z"], z.float().double().numpy())   # (MPC returns x, u in fp32)


def test_backward_reference_is_the_dense_solve():
    model, T, B, pbt = nl.CASES[1]
    pr, plant, its, (z, lam, rho), _, _ = nl.oracle_solve(model, T, B, pbt, "f32")
    (zb, lb, rb), tr = its[1]
    gbar = torch.randn(B, T, 3, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    qg, Qg = nl.backward_f64(pr, plant, zb, lb, rb, z, gbar)
    xn, F = nl.ssr.linearize(plant, zb.double(), 2)
    pr64 = {k: (v.double() if torch.is_tensor(v) else v) for k, v in pr.items()}
    Hd, Hs, L = nl.step_hessian(pr64, zb.double(), xn, F, lb.double(), rb.double(), "f64")
    w = dense_w(Hd, Hs, gbar.numpy())
    assert np.abs(qg - w).max() < 1e-12 * np.abs(w).max()
    assert np.abs(Qg - w * z.double().numpy()).max() < 1e-12 * np.abs(Qg).max()
    assert np.abs(L @ L.transpose(0, 1, 3, 2) - Hd).max() > 0   # (L is the banded factor, not the blocks' own)
    # and the driver's recorded Hessian of that step is the same object in the case's precision
    assert np.abs(tr["Hd"][0].numpy() - Hd).max() < 1e-4 * np.abs(Hd).max()


def test_driver_returns_what_its_docstring_says():
    model, T, B, pbt = nl.CASES[1]
    pr, plant = nl.problem(model, B, T, pbt, torch.float64)
    z, lam, rho = nl.start(pr)
    tr = nl.al_iteration(OracleBackend(), pr, plant, z, lam, rho, hessian=True)
    n = 3
    assert tr["g"].shape == tr["d"].shape == (4, B, T, n) and tr["phi"].shape == (4, 20, B) and tr["F"].shape == (4, B, T - 1, 2, n)
    assert tr["Hd"].shape == (4, B, T, n, n) and tr["Hs"].shape == (4, B, T - 1, n, n) and tr["L"].shape == (4, B, T, n, n)
    assert torch.equal(tr["phi"].min(1).values[-1], tr["phi_end"]) and bool((rho == 10).all())
    # a step taken alone from a state of the trace is that step
    z2, lam2, rho2 = nl.start(pr)
    one = nl.al_iteration(OracleBackend(), pr, plant, z2, lam2, rho2, n_newton=1, dual=False)
    assert torch.equal(one["d"][0], tr["d"][0]) and torch.equal(one["k"][0], tr["k"][0]) and not lam2.any()
