"""The quad sweeps after loads and stores they do not need were taken out (csrc/alqp_quad.hpp): the forward sweep
hands the own x-slots of z_{t+1} to the next stage in registers, and the backward sweep stores s_t only when iter_end()
or a merit pass will read it. (The F load of the horizon's last stage, whose result is discarded, stays: skipping it was
slower. The cases that watch that stage stay too.) Every case is compared with the CPU oracle, at the shapes where that
bookkeeping can go wrong:

* T = 2 (the last stage is the second stage, the carry crosses one boundary), 3 and 5;
* (13,4): SW = 4, SY = 5, the carried slots are the whole head chunk and only the tail word is read; (2,1): SY = SW = 1,
  nothing of z is left to read; (8,2): SW = 2, SY = 3, tail words only (SY / 4 == 0); (10,3): SW = 3, SY = 4, the one
  head chunk holds carried slots and a slot that is read (SW % 4 != 0). No compiled size has SY > SW + 1;
* B = 1 (a lone instance), 17 (an odd pair count) and 33 (padding quads that alias instance B - 1);
* the fused solve with al_iter = 2, max_newton = 4 (forward sweeps with and without a pending step; s stored on the last of
  the four steps only), one Newton step per launch on a primed workspace (s stored by every step) and the reference's
  exit test inside the launch (iter_end() after every step);
* after the fused solve, the backward pass on the workspace it left behind (k_backward_quad: the factor in the records
  is whole and the pass does not need the record's s group), and the Newton step kernel (EXT route) against the team kernel.

Tolerances. fp64: 1e-9 (z, lam relative to max(1, |lam|)), 1e-12 for the backward pass as in test_gpu_quad_backward_ws.py.
fp32, z: the rule of test_gpu_quad_own_solves.py (median of the per-instance error below 1e-5, at most B // 17 instances
at or above 2e-3: line-search near-ties). The other outputs are compared on the instances whose z agrees (below 2e-3):
rho, info, status exactly; lam = lam + rho r with r = z_{t+1}[x] - F z_t - c, so an error e in z becomes at most
g e with g = rho_max (1 + max row sum |F|): median below g 1e-5 and every compared instance below g 2e-3; phi and rnorm2
within 1e-3 (|value| + 1), the merit tolerance of check_excluded (test_gpu_parity.py). fp64 phi, rnorm2: 1e-9 (|value| + 1)."""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle_py as orc
from tests.oracle_backend import OracleBackend
from tests.test_gpu_parity import near_tie_instances
from tests.test_gpu_quad_own_solves import STEP_TOL, _row_sets, _step, _step_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TD = {"f32": torch.float32, "f64": torch.float64}
DIMS = [(13, 4), (2, 1), (8, 2), (10, 3)]
HORIZONS = [2, 3, 5]
BATCHES = [1, 17, 33]
SEED = 11
RHO_SCALE = 10.0
BWD_TOL = {"f64": 1e-12, "f32": 1e-5}   # test_gpu_quad_backward_ws.py, solve route
WS_PRIMED = 8

grid = pytest.mark.parametrize("nx,nu,T,B,dtype", [(nx, nu, T, B, dt) for (nx, nu) in DIMS for T in HORIZONS
                                                   for B in BATCHES for dt in ("f32", "f64")])
grid17 = pytest.mark.parametrize("nx,nu,T,dtype", [(nx, nu, T, dt) for (nx, nu) in DIMS for T in HORIZONS
                                                   for dt in ("f32", "f64")])


# (nx, nu, T, B) -> seed of the cases that are not drawn with SEED. Empty for every case of this file and of
# test_gpu_quad_factor_lds.py; test_gpu_quad_all_dims.py enters its two (chosen from the oracle's trace on the CPU,
# test_quad_all_dims_cases_cpu.py), so that _reference here and _run / _oracle there draw the same problem for them.
CASE_SEEDS = {}


@functools.lru_cache(maxsize=None)
def _problem_cpu(nx, nu, T, B, dtype, seed=None):
    """seed = None: the case's seed, SEED unless CASE_SEEDS names another"""
    from deq_mpc_corl_amd import synthetic_problem
    if seed is None:
        seed = CASE_SEEDS.get((nx, nu, T, B), SEED)
    return synthetic_problem(B, T, nx, nu, seed=seed, dtype=TD[dtype])


def _state(p, B, T, nx, nu, dt, dev):
    return dict(z=p.z0.clone().to(dev), lam=torch.zeros(B, T * nx + 2 * T * nu, dtype=dt, device=dev),
                rho=torch.ones(B, dtype=dt, device=dev), phi=torch.zeros(B, dtype=dt, device=dev),
                rn2=torch.zeros(B, dtype=dt, device=dev), info=torch.zeros(B, dtype=torch.int32, device=dev),
                st=torch.zeros(B, dtype=torch.uint8, device=dev))


def _launches(be, p, dims, s, calls, **kw):
    """calls: (al_iter, max_newton, flags) per launch, the state carried in s"""
    for al_iter, max_newton, flags in calls:
        be.solve_lin(dims, p.Qd, p.q, p.F, p.c, p.x0, p.u_lo, p.u_hi, 0, 0, s["z"], s["lam"], s["rho"], s["phi"], s["rn2"],
                     s["info"], s["st"], al_iter=al_iter, max_newton=max_newton, n_ls=20, flags=flags, rho_scale=RHO_SCALE,
                     **kw)


FUSED = ((2, 4, 3),)
# merit at the start, three launches of one Newton step each on the records the first launch filled, the dual update
STEPWISE = ((1, 0, 1), (1, 1, WS_PRIMED), (1, 1, WS_PRIMED), (1, 1, WS_PRIMED), (1, 0, 2))


@functools.lru_cache(maxsize=None)
def _reference(nx, nu, T, B, dtype, calls):
    """The same launches through the oracle backend on the CPU: computed once per case, shared, never written to."""
    p = _problem_cpu(nx, nu, T, B, dtype)
    s = _state(p, B, T, nx, nu, TD[dtype], "cpu")
    # the oracle backend has no workspace: ALQP_WS_PRIMED means nothing to it
    _launches(OracleBackend(), p, (B, T, nx, nu), s, tuple((a, m, f & ~WS_PRIMED) for a, m, f in calls))
    return {k: v.numpy().copy() for k, v in s.items()}


def _to_dev(p):
    return p._replace(**{k: v.to(DEV) for k, v in p._asdict().items() if torch.is_tensor(v)})


def _compare(label, dtype, B, g, o, F):
    """g: the GPU's state (numpy), o: the oracle's; F: the problem's dynamics (numpy)"""
    err = np.abs(g["z"] - o["z"]).reshape(B, -1).max(1)
    lam_scale = max(1.0, float(np.abs(o["lam"]).max()))
    el = np.abs(g["lam"] - o["lam"]).reshape(B, -1).max(1) / lam_scale
    ep = np.abs(g["phi"] - o["phi"]) / (np.abs(o["phi"]) + 1)
    er = np.abs(g["rn2"] - o["rn2"]) / (np.abs(o["rn2"]) + 1)
    print(f"{label}: z median {np.median(err):.3e} max {err.max():.3e} ({int((err >= 2e-3).sum())} at or above 2e-3), "
          f"lam {el.max():.3e}, phi {ep.max():.3e}, rnorm2 {er.max():.3e}")
    assert np.isfinite(g["z"]).all() and np.isfinite(g["lam"]).all()
    if dtype == "f64":
        assert err.max() < 1e-9 and el.max() < 1e-9, (err.max(), el.max())
        assert ep.max() < 1e-9 and er.max() < 1e-9, (ep.max(), er.max())
        ok = np.ones(B, bool)
    else:
        assert np.median(err) < 1e-5 and (err >= 2e-3).sum() <= B // 17, np.sort(err)[-4:]
        ok = err < 2e-3
        gain = float(o["rho"].max()) * (1.0 + float(np.abs(F).sum(-1).max()))
        assert np.median(el) < gain * 1e-5 and el[ok].max() < gain * 2e-3, (gain, np.sort(el)[-4:])
        assert ep[ok].max() < 1e-3 and er[ok].max() < 1e-3, (ep[ok].max(), er[ok].max())
    assert np.array_equal(g["rho"][ok], o["rho"][ok])
    assert np.array_equal(g["info"][ok], o["info"][ok]) and np.array_equal(g["st"][ok], o["st"][ok])
    return ok


@grid
def test_fused_solve_then_backward_pass(nx, nu, T, B, dtype):
    """al_iter = 2, max_newton = 4 in one launch against the oracle, then k_backward_quad on the workspace the solve
    left behind against the oracle's backward on the oracle's factor."""
    from deq_mpc_corl_amd.backend import default_backend
    be = default_backend()
    dt, dims = TD[dtype], (B, T, nx, nu)
    pc = _problem_cpu(nx, nu, T, B, dtype)
    p = _to_dev(pc)
    s = _state(p, B, T, nx, nu, dt, DEV)
    ws = be.new_workspace(dims, s["z"])
    _launches(be, p, dims, s, FUSED, variant="quad", workspace=ws)
    assert be.last_variant == "quad"
    gen = torch.Generator(device="cpu").manual_seed(B + 1)
    gbar = torch.randn(B, T, nx + nu, generator=gen, dtype=torch.float64).to(dt)
    qg, Qg = torch.full_like(s["z"], float("nan")), torch.full_like(s["z"], float("nan"))
    be.backward_ws(dims, ws, p.F, s["rho"] / RHO_SCALE, s["z"], gbar.to(DEV), qg, Qg)
    torch.cuda.synchronize()
    g = {k: v.cpu().numpy() for k, v in s.items()}
    label = f"fused ({nx},{nu}) T={T} B={B} {dtype}"
    ok = _compare(label, dtype, B, g, _reference(nx, nu, T, B, dtype, FUSED), pc.F.numpy())
    # backward pass: the oracle's solve with its factor saved, its backward at the GPU's final z (Qd_grad = q_grad z)
    c = lambda a: a.numpy()
    o = orc.solve_lin(dtype, c(pc.Qd), c(pc.q), c(pc.F), c(pc.c), c(pc.x0), c(pc.u_lo), c(pc.u_hi), c(pc.z0), al_iter=2,
                      exit_mode="fixed", trace_steps=8 if dtype == "f32" else 0, save_factor=True)
    rq, rQ = orc.backward(dtype, o["L"], c(pc.F), o["rho"] / RHO_SCALE, g["z"], c(gbar))
    if dtype == "f32":
        ok &= ~near_tie_instances(o, dtype)   # another step there: another factor
    qg, Qg = qg.cpu().numpy(), Qg.cpu().numpy()
    assert np.isfinite(qg).all() and np.isfinite(Qg).all()
    if ok.any():
        eq = np.abs(qg - rq).reshape(B, -1).max(1)[ok].max() / np.abs(rq).max()
        eQ = np.abs(Qg - rQ).reshape(B, -1).max(1)[ok].max() / np.abs(rQ).max()
        print(f"{label} backward pass: q_grad {eq:.2e}, Qd_grad {eQ:.2e} ({int(ok.sum())} instances)")
        assert eq < BWD_TOL[dtype] and eQ < BWD_TOL[dtype], (eq, eQ)


@grid
def test_one_newton_step_per_launch_on_primed_workspace(nx, nu, T, B, dtype):
    """max_newton = 1 per launch: every step is the launch's last, iter_end() applies it with r += alpha s from the
    record, so every backward sweep has to store s."""
    from deq_mpc_corl_amd.backend import default_backend
    be = default_backend()
    dt, dims = TD[dtype], (B, T, nx, nu)
    pc = _problem_cpu(nx, nu, T, B, dtype)
    p = _to_dev(pc)
    s = _state(p, B, T, nx, nu, dt, DEV)
    _launches(be, p, dims, s, STEPWISE, variant="quad", workspace=be.new_workspace(dims, s["z"]))
    torch.cuda.synchronize()
    g = {k: v.cpu().numpy() for k, v in s.items()}
    assert float(np.abs(g["z"] - pc.z0.numpy()).max()) > 1e-3   # the steps moved z
    _compare(f"stepwise ({nx},{nu}) T={T} B={B} {dtype}", dtype, B, g, _reference(nx, nu, T, B, dtype, STEPWISE), pc.F.numpy())


@grid17
def test_reference_exit_inside_the_launch(nx, nu, T, dtype):
    """ALQP_EXIT_IN_KERNEL at B = 17: iter_end() runs after every Newton step and reads s; z, lam, rho and the Newton
    counts against the oracle in its reference exit mode."""
    from deq_mpc_corl_amd.backend import default_backend
    be = default_backend()
    B = 17
    dt, dims = TD[dtype], (B, T, nx, nu)
    pc = _problem_cpu(nx, nu, T, B, dtype)
    p = _to_dev(pc)
    s = _state(p, B, T, nx, nu, dt, DEV)
    counts = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    _launches(be, p, dims, s, FUSED, variant="quad", workspace=be.new_workspace(dims, s["z"]), newton_counts=counts)
    torch.cuda.synchronize()
    c = lambda a: a.numpy()
    o = orc.solve_lin(dtype, c(pc.Qd), c(pc.q), c(pc.F), c(pc.c), c(pc.x0), c(pc.u_lo), c(pc.u_hi), c(pc.z0), al_iter=2,
                      exit_mode="reference")
    g = {k: v.cpu().numpy() for k, v in s.items()}
    err = np.abs(g["z"] - o["z"]).reshape(B, -1).max(1)
    lam_scale = max(1.0, float(np.abs(o["lam"]).max()))
    el = np.abs(g["lam"] - o["lam"]).reshape(B, -1).max(1) / lam_scale
    print(f"in-kernel exit ({nx},{nu}) T={T} {dtype}: Newton counts {counts.tolist()} / {o['newton_per_al'].tolist()}, "
          f"z median {np.median(err):.3e} max {err.max():.3e}, lam {el.max():.3e}")
    assert counts.tolist() == o["newton_per_al"].tolist()
    assert int(np.abs(g["info"]).sum()) == 0 and g["st"].all()
    if dtype == "f64":
        assert err.max() < 1e-9 and el.max() < 1e-9, (err.max(), el.max())
    else:
        assert np.median(err) < 1e-5 and (err >= 2e-3).sum() <= B // 17, np.sort(err)[-4:]
        ok = err < 2e-3
        gain = float(o["rho"].max()) * (1.0 + float(np.abs(c(pc.F)).sum(-1).max()))
        assert np.median(el) < gain * 1e-5 and el[ok].max() < gain * 2e-3, (gain, np.sort(el)[-4:])
    assert np.array_equal(g["rho"], o["rho"])


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("T", [2, 5])
@pytest.mark.parametrize("nx,nu", DIMS)
def test_newton_step_kernel_equals_team_step(nx, nu, T, dtype):
    """k_newton_step_quad (the forward sweep's EXT route: the caller's arrays are read element-wise, nothing is carried
    from stage to stage; the last stage's F rows are discarded) against the team kernel's direction, B = 17, without
    and with obstacle rows, on a workspace full of NaN."""
    from deq_mpc_corl_amd.backend import default_backend
    be = default_backend()
    dims = (17, T, nx, nu)
    for with_obs in _row_sets(nx):
        inp = _step_inputs(dims, TD[dtype], with_obs)
        d_team = _step(be, dims, inp, None).cpu().numpy()
        d_quad = _step(be, dims, inp, be.new_workspace(dims, inp[1]).fill_(float("nan"))).cpu().numpy()
        err = np.abs(d_quad - d_team).max() / max(1.0, float(np.abs(d_team).max()))
        print(f"quad vs team step ({nx},{nu}) T={T} {dtype} obs={with_obs}: {err:.3e}")
        assert np.isfinite(d_quad).all()
        assert err < STEP_TOL[dtype], (with_obs, err)
