"""Backward through the quad workspace records (alqp_backward on a workspace / k_backward_quad) against a float64 reference, on
every compiled (nx, nu) and both dtypes. The backward pass reads the factor (L chunks) and the y / d field of every
record; in fp32 those records are interleaved in pairs of instances (QCfg::IL = 2), so an odd B leaves the last pair
half used and puts a single real instance into the last wavefront.

Step route: one quad Newton step (newton_step with a workspace) leaves the factor of H at (z, lam, rho) in the records;
the reference is the C oracle in float64 on the same inputs (grad_hess -> newton_dir(want_factor) -> backward), so the
comparison sees only the backward's reading of the records and can be tight.
Solve route: the quad fused solve (solve_lin, variant "quad") and then backward_ws, against the oracle's solve with the
factor saved plus its backward; fp32 instances whose line search met a near-tie are accounted for as in
test_gpu_parity.py."""
import numpy as np
import pytest
import torch

from oracle import oracle_py as orc
from tests.test_gpu_nonlin_scale import _problem
from tests.test_gpu_parity import check_excluded, near_tie_instances
from tests.test_quad_record_layout_cpu import _dims

DEV = "cuda:0"
TD = {"f32": torch.float32, "f64": torch.float64}
DIMS = _dims()   # every (nx, nu) compiled into the library
RHO_SCALE = 10.0   # the fused solve's dual update (solve_lin rho_scale): the factor it leaves belongs to rho / 10

# step route, relative to max |grad|. Largest measured on the MI355X over all dims and both B: fp64 2.4e-16, fp32 7.4e-8
STEP_TOL = {"f64": 1e-12, "f32": 1e-6}


def _dense_backward(go, Hd, Hs, gbar, z):
    """w = -H^-1 gbar with H assembled from grad_hess's blocks (Hd: diagonal, Hs: block (t+1, t))."""
    B, T, n = go.shape
    qg, Qg = np.empty_like(gbar), np.empty_like(gbar)
    for b in range(B):
        H = np.zeros((T * n, T * n))
        for t in range(T):
            H[t * n:(t + 1) * n, t * n:(t + 1) * n] = Hd[b, t]
        for t in range(T - 1):
            H[(t + 1) * n:(t + 2) * n, t * n:(t + 1) * n] = Hs[b, t]
            H[t * n:(t + 1) * n, (t + 1) * n:(t + 2) * n] = Hs[b, t].T
        w = -np.linalg.solve(H, gbar[b].reshape(-1))
        qg[b] = w.reshape(T, n)
        Qg[b] = qg[b] * z[b]
    return qg, Qg


@pytest.mark.parametrize("nx,nu", [(13, 4), (2, 1), (6, 1)])
def test_oracle_backward_on_newton_factor_equals_dense_solve(nx, nu):
    """CPU: the reference chain the GPU tests below rely on - orc.backward on newton_dir's factor is -H^-1 gbar with
    H from grad_hess (dense numpy float64 solve), at points with active bounds."""
    B, T = 5, 7
    from deq_mpc_corl_amd import synthetic_problem
    p = synthetic_problem(B, T, nx, nu, seed=3, dtype=torch.float64, active=True)
    rng = np.random.default_rng(4)
    M = T * nx + 2 * T * nu
    c = lambda a: a.numpy()
    z = c(p.z0) + 0.2 * rng.standard_normal(c(p.z0).shape)
    xn = np.einsum("btij,btj->bti", c(p.F), z[:, :-1]) + c(p.c) + 0.05 * rng.standard_normal((B, T - 1, nx))
    lam = 0.3 * rng.standard_normal((B, M))
    lam[:, T * nx:] = np.maximum(lam[:, T * nx:], 0)
    rho = 1.0 + 9.0 * rng.random(B)
    go, Hd, Hs = orc.grad_hess("f64", z, xn, c(p.F), c(p.x0), lam, rho, c(p.Qd), c(p.q), c(p.u_lo), c(p.u_hi))
    _, info, L, _ = orc.newton_dir("f64", go, Hd, Hs, nx, want_factor=True)
    assert (info == 0).all()
    gbar = rng.standard_normal(z.shape)
    qg, Qg = orc.backward("f64", L, c(p.F), rho, z, gbar)
    dq, dQ = _dense_backward(go, Hd, Hs, gbar, z)
    assert np.abs(qg - dq).max() < 1e-10 * np.abs(dq).max()
    assert np.abs(Qg - dQ).max() < 1e-10 * np.abs(dQ).max()


@pytest.mark.gpu
@pytest.mark.parametrize("B", [17, 19])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("nx,nu", DIMS)
def test_backward_ws_after_newton_step_vs_float64_oracle(nx, nu, dtype, B):
    from deq_mpc_corl_amd.backend import default_backend
    be = default_backend()
    T = 7
    dims = (B, T, nx, nu)
    dt = TD[dtype]
    p, z, xn, lam, rho = _problem(B, T, nx, nu, dt, seed=nx * 10 + nu, active=True)
    ws = be.new_workspace(dims, z)
    d = torch.empty_like(z)
    info = torch.zeros(B, dtype=torch.int32, device=DEV)
    be.newton_step(dims, z, xn, p.F, p.x0, lam, rho, p.Qd, p.q, p.u_lo, p.u_hi, 0, 0, d, info=info, workspace=ws)
    gen = torch.Generator(device="cpu").manual_seed(B)
    gbar = torch.randn(B, T, nx + nu, generator=gen, dtype=torch.float64).to(dt).to(DEV)
    qg, Qg = torch.full_like(z, float("nan")), torch.full_like(z, float("nan"))
    be.backward_ws(dims, ws, p.F, rho, z, gbar, qg, Qg)
    torch.cuda.synchronize()
    assert int(info.abs().max()) == 0
    c = lambda a: a.cpu().numpy().astype(np.float64)
    go, Hd, Hs = orc.grad_hess("f64", c(z), c(xn), c(p.F), c(p.x0), c(lam), c(rho), c(p.Qd), c(p.q), c(p.u_lo),
                               c(p.u_hi))
    _, oinfo, L, _ = orc.newton_dir("f64", go, Hd, Hs, nx, want_factor=True)
    assert (oinfo == 0).all()
    rq, rQ = orc.backward("f64", L, c(p.F), c(rho), c(z), c(gbar))
    eq = np.abs(c(qg) - rq).max() / np.abs(rq).max()
    eQ = np.abs(c(Qg) - rQ).max() / np.abs(rQ).max()
    # per instance too: the last (half-used) pair / the last wavefront's single instance must not hide in a batch max
    per = (np.abs(c(qg) - rq).reshape(B, -1).max(1) / np.abs(rq).max())
    print(f"backward_ws step route {dtype} ({nx},{nu}) B={B}: q_grad {eq:.2e}, Qd_grad {eQ:.2e}, "
          f"last instance {per[-1]:.2e} (relative to max |grad|)")
    assert np.isfinite(c(qg)).all() and np.isfinite(c(Qg)).all()
    assert eq < STEP_TOL[dtype] and eQ < STEP_TOL[dtype], (eq, eQ)


# solve route: near-tie instances counted on the CPU from the oracle's fp32 trace of each configuration (+1 = budget)
# (T = 10, seed 29; at B = 4099 a sizeable share of instances end in a converged line search whose candidates tie)
SOLVE_NEAR_TIES_F32 = {((13, 4), 19): 4, ((13, 4), 4099): 563, ((8, 2), 19): 5, ((8, 2), 4099): 518, ((2, 1), 19): 1,
                       ((2, 1), 4099): 168, ((13, 4), 16384): 2}
SOLVE_SEED = 29
# largest measured (instances compared): fp64 3.3e-15, fp32 2.1e-6 (Qd_grad; q_grad 1.5e-7)
SOLVE_TOL = {"f64": 1e-12, "f32": 1e-5}


def _solve_route(nx, nu, dtype, B, T=10, sample=None):
    from deq_mpc_corl_amd import synthetic_problem
    from deq_mpc_corl_amd.backend import default_backend
    be = default_backend()
    dims = (B, T, nx, nu)
    dt = TD[dtype]
    al = 2
    p = synthetic_problem(B, T, nx, nu, seed=SOLVE_SEED, dtype=dt, device=DEV)
    M = T * nx + 2 * T * nu
    z = p.z0.clone()
    lam = torch.zeros(B, M, dtype=dt, device=DEV)
    rho = torch.ones(B, dtype=dt, device=DEV)
    phi = torch.zeros(B, dtype=dt, device=DEV)
    rn2 = torch.zeros(B, dtype=dt, device=DEV)
    info = torch.zeros(B, dtype=torch.int32, device=DEV)
    st = torch.zeros(B, dtype=torch.uint8, device=DEV)
    ws = be.new_workspace(dims, z)
    be.solve_lin(dims, p.Qd, p.q, p.F, p.c, p.x0, p.u_lo, p.u_hi, 0, 0, z, lam, rho, phi, rn2, info, st,
                 al_iter=al, max_newton=4, n_ls=20, flags=3, rho_scale=RHO_SCALE, variant="quad", workspace=ws)
    assert be.last_variant == "quad"
    gen = torch.Generator(device="cpu").manual_seed(B + 1)
    gbar = torch.randn(B, T, nx + nu, generator=gen, dtype=torch.float64).to(dt).to(DEV)
    rho_f = rho / RHO_SCALE
    qg, Qg = torch.full_like(z, float("nan")), torch.full_like(z, float("nan"))
    be.backward_ws(dims, ws, p.F, rho_f, z, gbar, qg, Qg)
    torch.cuda.synchronize()
    assert int(info.abs().sum()) == 0 and bool(st.all())
    idx = np.arange(B) if sample is None else sample
    c = lambda a: a.cpu().numpy()[idx]
    prob = dict(Qd=c(p.Qd), q=c(p.q), F=c(p.F), c=c(p.c), x0=c(p.x0), u_lo=p.u_lo.cpu().numpy(),
                u_hi=p.u_hi.cpu().numpy())
    o = orc.solve_lin(dtype, prob["Qd"], prob["q"], prob["F"], prob["c"], prob["x0"], prob["u_lo"], prob["u_hi"],
                      c(p.z0), al_iter=al, exit_mode="fixed", trace_steps=al * 4 if dtype == "f32" else 0,
                      save_factor=True)
    # z_final: the GPU's (the oracle saves z at its last factorisation, one step before the end; q_grad does not depend on
    # it, Qd_grad = q_grad * z_final)
    rq, rQ = orc.backward(dtype, o["L"], prob["F"], o["rho"] / RHO_SCALE, c(z), c(gbar))
    return dict(qg=c(qg), Qg=c(Qg), z=c(z), lam=c(lam), rho=c(rho), rq=rq, rQ=rQ, o=o, prob=prob)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [19, 4099])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("nx,nu", [(13, 4), (8, 2), (2, 1)])
def test_backward_ws_after_quad_solve_vs_oracle(nx, nu, dtype, B):
    _check_solve_route(nx, nu, dtype, B)


def _sample32(B):
    """both halves of the first pairs, the last (half-filled) wavefront's instances, a spread in between"""
    if B <= 32:
        return np.arange(B)
    idx = np.unique(np.concatenate([np.arange(4), np.arange(B - 18, B), np.linspace(4, B - 19, 10).astype(int)]))
    assert len(idx) == 32
    return idx


@pytest.mark.gpu
def test_backward_ws_after_quad_solve_headline_batch_f32():
    """fp32 (13,4) at the benchmark's batch, on a 32-instance sample."""
    _check_solve_route(13, 4, "f32", 16384, sample=_sample32(16384))


def _check_solve_route(nx, nu, dtype, B, sample=None):
    r = _solve_route(nx, nu, dtype, B, sample=sample)
    n_inst = len(r["qg"])
    scale_q, scale_Q = np.abs(r["rq"]).max(), np.abs(r["rQ"]).max()
    eq = np.abs(r["qg"] - r["rq"]).reshape(n_inst, -1).max(1) / scale_q
    eQ = np.abs(r["Qg"] - r["rQ"]).reshape(n_inst, -1).max(1) / scale_Q
    assert np.isfinite(r["qg"]).all() and np.isfinite(r["Qg"]).all()
    ok = np.ones(n_inst, bool)
    if dtype == "f32":
        label = f"backward_ws solve route ({nx},{nu}) B={B}"
        excluded = near_tie_instances(r["o"], dtype)
        budget = SOLVE_NEAR_TIES_F32[((nx, nu), B)] + 1
        assert int(excluded.sum()) <= budget, (label, int(excluded.sum()), budget)
        # check_excluded's accounting (finite, no worse merit than the oracle's) on the 32-instance sample: over a whole
        # batch of 4099 with ~500 near-ties, one or two instances end 0.2-1.6 % above the oracle's merit after the 8 fixed
        # Newton steps - on the team kernel exactly as on the quad kernel, and the same wherever the instance sits in the
        # batch (measured on the MI355X): a property of the fixed-step fp32 solve, not of the workspace records
        s = _sample32(n_inst)
        o = {k: r["o"][k][s] for k in ("z", "lam", "rho")}
        prob = {k: (v if k in ("u_lo", "u_hi") else v[s]) for k, v in r["prob"].items()}
        check_excluded(dtype, excluded[s], r["z"][s], r["lam"][s], r["rho"][s], o, prob, max_count=budget, label=label)
        ok = ~excluded
    print(f"backward_ws solve route {dtype} ({nx},{nu}) B={B}: q_grad {eq[ok].max():.2e}, Qd_grad {eQ[ok].max():.2e} "
          f"(relative to max |grad|, {int(ok.sum())} instances)")
    assert eq[ok].max() < SOLVE_TOL[dtype] and eQ[ok].max() < SOLVE_TOL[dtype], (eq[ok].max(), eQ[ok].max())
