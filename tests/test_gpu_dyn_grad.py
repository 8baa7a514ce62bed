"""Gradients w.r.t. the affine dynamics (dF, dc) and the initial state (dx0) out of the two backward kernels
(alqp_backward_* with an AlqpBwdDyn: k_backward<DYN> on a packed factor, k_backward_quad<DYN> on a workspace) against
the float64 oracle: w from orc.backward, then the three formulas of tests/test_dyn_grad_cpu.dyn_grads (pinned there by
finite differences).

Step route, as test_gpu_quad_backward_ws.py: one Newton step leaves the factor of H at (z, lam, rho) - in the workspace
records (quad) or packed (team) - so the comparison sees only the backward pass and its epilogue. End to end: MPC with
LinDx(F, f) and x0 requiring grad, both launch routes and both exit modes."""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle_py as orc
from tests.test_dyn_grad_cpu import dyn_grads
from tests.test_gpu_nonlin_scale import _problem
from tests.test_gpu_parity import check_excluded, near_tie_instances
from tests.test_gpu_quad_backward_ws import (RHO_SCALE, SOLVE_NEAR_TIES_F32, SOLVE_SEED, SOLVE_TOL, _sample32)
from tests.test_quad_record_layout_cpu import _dims

DEV = "cuda:0"
TD = {"f32": torch.float32, "f64": torch.float64}
DIMS = _dims()   # every (nx, nu) compiled into the library
NAMES = ("dF", "dc", "dx0")

# step route, per instance, relative to max |grad| of the batch. fp64: the bound the project uses for this chain
# (test_gpu_quad_backward_ws.STEP_TOL). fp32: 10x the largest value measured on the MI355X over all sizes, both routes,
# B in {17, 19} and T in {7, 2}. Largest measured: fp64 9.5e-15 (dx0, quad, (4,2) B=19); fp32 2.48e-6 (dx0, quad, (4,2)
# B=19; dc 1.7e-6, dF 8.6e-7 - s_t = w_{t+1}[x] - F_t w_t is a difference of near-equal terms, and dx0 is measured
# against max |w_0[x]| alone, hence above q_grad's 7.4e-8)
DYN_STEP_TOL = {"f64": 1e-12, "f32": 2.5e-5}


def _c(a):
    return a.cpu().numpy().astype(np.float64)


@functools.lru_cache(maxsize=None)
def _step_case(nx, nu, dtype, B, T, route):
    """One Newton step (route "quad": factor in a workspace, "team": packed factor), then everything the tests below
    compare: a callable that runs the new backward with any subset of outputs, and the float64 reference."""
    from deq_mpc_corl_amd.backend import DynGrads, default_backend
    be = default_backend()
    dims = (B, T, nx, nu)
    dt = TD[dtype]
    n = nx + nu
    p, z, xn, lam, rho = _problem(B, T, nx, nu, dt, seed=nx * 10 + nu, active=True)
    d = torch.empty_like(z)
    info = torch.zeros(B, dtype=torch.int32, device=DEV)
    if route == "quad":
        fac = be.new_workspace(dims, z)
        be.newton_step(dims, z, xn, p.F, p.x0, lam, rho, p.Qd, p.q, p.u_lo, p.u_hi, 0, 0, d, info=info, workspace=fac)
        plain = be.backward_ws
    else:
        fac = torch.empty(B, T, n * (n + 1) // 2, dtype=dt, device=DEV)
        be.newton_step(dims, z, xn, p.F, p.x0, lam, rho, p.Qd, p.q, p.u_lo, p.u_hi, 0, 0, d, info=info, factor=fac)
        plain = be.backward
    gen = torch.Generator(device="cpu").manual_seed(B)
    gbar = torch.randn(B, T, n, generator=gen, dtype=torch.float64).to(dt).to(DEV)
    M = T * nx + 2 * T * nu
    lam_ret = torch.randn(B, M, generator=gen, dtype=torch.float64).to(dt).to(DEV)   # batch stride M > (T-1) nx

    def run(which=NAMES, with_dyn=True):
        """-> q_grad, Qd_grad, {name: [B+1, ...] output, NaN-prefilled, the last instance a guard}"""
        nan = lambda *s: torch.full(s, float("nan"), dtype=dt, device=DEV)
        qg, Qg = nan(B, T, n), nan(B, T, n)
        full = dict(dF=nan(B + 1, T - 1, nx, n), dc=nan(B + 1, T - 1, nx), dx0=nan(B + 1, nx))
        kw = {}
        if with_dyn:
            kw["dyn"] = DynGrads(lam_ret if "dF" in which else None, *(full[k][:B] if k in which else None for k in NAMES))
        plain(dims, fac, p.F, rho, z, gbar, qg, Qg, **kw)
        torch.cuda.synchronize()
        return qg, Qg, full

    go, Hd, Hs = orc.grad_hess("f64", _c(z), _c(xn), _c(p.F), _c(p.x0), _c(lam), _c(rho), _c(p.Qd), _c(p.q),
                               _c(p.u_lo), _c(p.u_hi))
    _, oinfo, L, _ = orc.newton_dir("f64", go, Hd, Hs, nx, want_factor=True)
    assert (oinfo == 0).all()
    w, _ = orc.backward("f64", L, _c(p.F), _c(rho), _c(z), _c(gbar))
    ref = dict(zip(NAMES, dyn_grads(w, _c(p.F), _c(z), _c(lam_ret), _c(rho))))
    return dict(run=run, ref=ref, info=info, B=B)


def _check_step(nx, nu, dtype, B, T, route):
    r = _step_case(nx, nu, dtype, B, T, route)
    _, _, out = r["run"]()
    assert int(r["info"].abs().max()) == 0
    worst = 0.0
    for k in NAMES:
        got, want = _c(out[k][:B]), r["ref"][k]
        assert np.isfinite(got).all(), k
        assert bool(torch.isnan(out[k][B]).all()), f"{k}: written past instance B"
        per = np.abs(got - want).reshape(B, -1).max(1) / np.abs(want).max()   # per instance, not only the batch max
        print(f"dyn grads step route {route} {dtype} ({nx},{nu}) B={B} T={T}: {k} {per.max():.2e}, last instance "
              f"{per[-1]:.2e} (relative to max |grad|)")
        worst = max(worst, per.max())
        assert (per < DYN_STEP_TOL[dtype]).all(), (k, per)
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["quad", "team"])
@pytest.mark.parametrize("B", [17, 19])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("nx,nu", DIMS)
def test_dyn_grads_after_newton_step_vs_float64_oracle(nx, nu, dtype, B, route):
    _check_step(nx, nu, dtype, B, 7, route)


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["quad", "team"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("nx,nu", [(13, 4), (2, 1)])
def test_dyn_grads_single_dynamics_stage(nx, nu, dtype, route):
    """T = 2: one dynamics stage, the epilogue's loop runs once."""
    _check_step(nx, nu, dtype, 19, 2, route)


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["quad", "team"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("nx,nu", [(13, 4), (2, 1)])
def test_dyn_outputs_are_nullable_and_leave_plain_gradients_alone(nx, nu, dtype, route):
    B = 19
    r = _step_case(nx, nu, dtype, B, 7, route)
    qg0, Qg0, _ = r["run"](with_dyn=False)            # the plain entry point
    qg, Qg, out = r["run"]()
    assert torch.equal(qg, qg0) and torch.equal(Qg, Qg0)
    for k in NAMES:
        qg1, Qg1, one = r["run"](which=(k,))
        assert torch.equal(qg1, qg0) and torch.equal(Qg1, Qg0)
        assert torch.equal(one[k][:B], out[k][:B]), k
        for other in NAMES:   # a null output is not written: its buffer never reached the call
            if other != k:
                assert bool(torch.isnan(one[other]).all())
    _, _, none = r["run"](which=())
    assert all(bool(torch.isnan(none[k]).all()) for k in NAMES)


def test_dF_without_lam_is_refused():
    """alqp_backward_* with an AlqpBwdDyn: ALQP_E_BADARG when lam is null while dF is not - checked on the host before any
    launch, so no device is needed for the refusal itself. Once on the factor route, once on the workspace route."""
    from deq_mpc_corl_amd import _lib
    import ctypes as C
    lib = _lib.load()
    d = _lib.AlqpDims(4, 5, 4, 2)
    one = C.c_void_p(64)   # never dereferenced: the call is refused first
    dyn = _lib.AlqpBwdDyn(None, 0, 64, None, None)   # dF without lam
    for sfx in ("f32", "f64"):
        fn = getattr(lib, "alqp_backward_" + sfx)
        rc = fn(C.byref(d), one, None, 0, one, one, one, one, one, one, C.byref(dyn), None)
        assert rc == -1   # ALQP_E_BADARG
        rc = fn(C.byref(d), None, one, 1 << 40, one, one, one, one, one, one, C.byref(dyn), None)
        assert rc == -1


# ---- end to end -------------------------------------------------------------------------------------------------
class _Spy:
    """The product backend, plus a copy of the z_final the backward pass was handed (MPC returns x, u as float32)."""

    def __init__(self, be):
        self._be = be
        self.z_final = None
        self.dyn_seen = []

    def __getattr__(self, name):
        return getattr(self._be, name)

    def backward(self, dims, factor, F, rho, z_final, *a, **kw):
        self.z_final, self.kind = z_final.clone(), "packed"
        self.dyn_seen.append("dyn" in kw)
        return self._be.backward(dims, factor, F, rho, z_final, *a, **kw)

    def backward_ws(self, dims, ws, F, rho, z_final, *a, **kw):
        self.z_final, self.kind = z_final.clone(), "workspace"
        self.dyn_seen.append("dyn" in kw)
        return self._be.backward_ws(dims, ws, F, rho, z_final, *a, **kw)


def _mpc_dyn_grads(nx, nu, dtype, B, exit_mode, T=10):
    from deq_mpc_corl_amd import MPC, QuadCost, synthetic_problem
    from deq_mpc_corl_amd.backend import default_backend
    from deq_mpc_corl_amd.qpth.al_utils import LinDx
    dt = TD[dtype]
    p = synthetic_problem(B, T, nx, nu, seed=SOLVE_SEED, dtype=dt, device=DEV)
    be = _Spy(default_backend())
    mpc = MPC(nx, nu, T, u_lower=p.u_lo, u_upper=p.u_hi, n_batch=B, dtype=dt, exit_mode=exit_mode, al_iter=2, backend=be)
    mpc.reinitialize(p.x0, None)
    F, f, x0 = (t.clone().requires_grad_(True) for t in (p.F, p.c, p.x0))
    x, u, _ = mpc(x0, QuadCost(torch.diag_embed(p.Qd), p.q), LinDx(F, f), None, x_init=p.z0[..., :nx].clone(),
                  u_init=p.z0[..., nx:].clone())
    gen = torch.Generator(device="cpu").manual_seed(B + 1)
    gbar = torch.randn(B, T, nx + nu, generator=gen, dtype=torch.float32).to(DEV)
    (torch.cat((x, u), -1) * gbar).sum().backward()
    torch.cuda.synchronize()
    assert be.dyn_seen == [True]
    assert be.kind == ("workspace" if B >= 4096 else "packed")
    for t in (F, f, x0):
        assert t.grad is not None and t.grad.dtype == dt and t.grad.shape == t.shape
    # the oracle's solve of the whole batch (the reference exit is batch-global), its saved factor -> w
    c = lambda a: a.detach().cpu().numpy()
    prob = dict(Qd=c(p.Qd), q=c(p.q), F=c(p.F), c=c(p.c), x0=c(p.x0), u_lo=c(p.u_lo), u_hi=c(p.u_hi))
    o = orc.solve_lin(dtype, prob["Qd"], prob["q"], prob["F"], prob["c"], prob["x0"], prob["u_lo"], prob["u_hi"], c(p.z0),
                      al_iter=2, exit_mode=exit_mode, trace_steps=8 if dtype == "f32" else 0, save_factor=True)
    assert list(o["newton_per_al"]) == list(mpc.last_newton_per_al)
    zf, lam, rho = c(be.z_final), c(mpc.lamda_prev), c(mpc.rho_prev).reshape(-1)
    w, _ = orc.backward(dtype, o["L"], prob["F"], o["rho"] / RHO_SCALE, zf, c(gbar).astype(zf.dtype))
    ref = dyn_grads(w, prob["F"], zf, lam, rho / RHO_SCALE)
    got = (c(F.grad), c(f.grad), c(x0.grad))
    return dict(got=got, ref=ref, o=o, prob=prob, z=zf, lam=lam, rho=rho)


def _check_mpc(nx, nu, dtype, B, exit_mode, ok=None):
    r = _mpc_dyn_grads(nx, nu, dtype, B, exit_mode)
    s = _sample32(B)
    ok = np.ones(B, bool) if ok is None else ok(r)
    for k, got, want in zip(NAMES, r["got"], r["ref"]):
        assert np.isfinite(got).all(), k
        per = np.abs(got - want).reshape(B, -1).max(1) / np.abs(want[ok]).max()
        print(f"dyn grads through MPC {dtype} ({nx},{nu}) B={B} {exit_mode}: {k} {per[s][ok[s]].max():.2e} on the sample, "
              f"{per[ok].max():.2e} over {int(ok.sum())} instances (relative to max |grad|)")
        assert per[s][ok[s]].max() < SOLVE_TOL[dtype], (k, per[s])
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("exit_mode", ["fixed", "reference"])
@pytest.mark.parametrize("B", [19, 4099])
@pytest.mark.parametrize("nx,nu", [(13, 4), (2, 1)])
def test_mpc_dynamics_gradients_f64(nx, nu, B, exit_mode):
    """B = 19: team kernels, packed factor; B = 4099: quad kernels, the factor in the solve's private workspace."""
    _check_mpc(nx, nu, "f64", B, exit_mode)


@pytest.mark.gpu
def test_mpc_dynamics_gradients_f32():
    """fp32, (13,4), B = 19: instances whose line search met a near-tie are accounted for as in test_gpu_parity.py."""
    nx, nu, B = 13, 4, 19
    label = f"dyn grads through MPC f32 ({nx},{nu}) B={B}"
    budget = SOLVE_NEAR_TIES_F32[((nx, nu), B)] + 1
    excl = {}

    def ok(r):
        excl["e"] = near_tie_instances(r["o"], "f32")
        return ~excl["e"]

    r = _check_mpc(nx, nu, "f32", B, "fixed", ok=ok)
    o = {k: r["o"][k] for k in ("z", "lam", "rho")}
    check_excluded("f32", excl["e"], r["z"], r["lam"], r["rho"], o, r["prob"], max_count=budget, label=label)
