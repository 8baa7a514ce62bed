"""GPU tests of the state-bound launch-per-step kernels (k_newton_step_xbox, k_merit_xbox, k_merit_pick_xbox, k_dual_xbox
behind alqp_*_xbox_*; MPC(x_lower=, x_upper=) with a callable dx). The reference is
tests/state_bounds_step_reference.py's backend (pinned on the CPU by tests/test_state_bounds_step_cpu.py), fed the kernel's
own inputs: lam, rho and the iterate after one reference AL iteration, where every instance has an upper and a lower
state row active and nonzero state-row multipliers. Tolerances: the Newton step's are tests/test_gpu_state_bounds.py's
(g within 10 RT, d and w within 100 RT of the largest); merit, pick and dual update get tests/aux_cases.py's
magnitude-derived bounds with the state rows' terms in the magnitudes."""
import functools

import numpy as np
import pytest
import torch

from tests import aux_cases as ax
from tests import state_bounds_reference as sbr
from tests import state_bounds_step_reference as ssr
from tests.aux_cases import Guarded
from tests.dense_cost_reference import dense_w
from tests.test_gpu_dense_cost import G_FLOOR, RT, scale_err

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TD = {"f64": torch.float64, "f32": torch.float32}
F64 = torch.float64
INERT = 1e20
CASE_IDS = [f"{nx}x{nu}-T{T}-B{B}-{'full' if ps else 'shared'}" for nx, nu, T, B, ps in ssr.GPU_CASES]


def _be():
    from deq_mpc_corl_amd.backend import default_backend
    return default_backend()


@functools.lru_cache(maxsize=None)
def _case(nx, nu, T, B, ps, dtype):
    """The case's problem, plant and reference inputs (CPU, computed once per session and never modified)."""
    pr, plant, inp = ssr.gpu_case(nx, nu, T, B, ps, TD[dtype])
    up, lo, nz = ssr.state_rows_active(pr, inp["z"], inp["lam"])
    assert up.all() and lo.all() and nz.all()   # on the reference alone
    return pr, plant, inp


def _dev(pr, inp):
    d = {k: v.to(DEV).contiguous() for k, v in pr.items() if torch.is_tensor(v)}
    d.update({k: v.to(DEV).contiguous() for k, v in inp.items() if torch.is_tensor(v)})
    return d


def _args(pr, t, lam=None, rho=None, xb=None):
    sb_u, st_u, sb_x, st_x = ssr.strides(pr)
    prob = (t["x0"], t["lam"] if lam is None else lam, t["rho"] if rho is None else rho, t["Qd"], t["q"], t["lo"], t["hi"],
            sb_u, st_u)
    return prob, ((t["xlo"], t["xhi"], sb_x, st_x) if xb is None else xb)


def _candidates(plant, z, d, n_ls, nx):
    al = (2.0 ** -torch.arange(n_ls, dtype=z.dtype, device=z.device)).view(n_ls, 1, 1, 1)
    zc = (z.unsqueeze(0) + al * d.unsqueeze(0)).contiguous()
    return zc, ssr.true_next(plant, zc, nx)


def _up(pr, inp):
    """The case upcast to float64 (what the fp64 reference of merit, pick and dual update is fed)."""
    f = lambda v: v.double() if torch.is_tensor(v) else v
    return {k: f(v) for k, v in pr.items()}, {k: f(v) for k, v in inp.items() if torch.is_tensor(v)}


# ---- the Newton step, its packed factor into alqp_backward -------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("nx,nu,T,B,ps", ssr.GPU_CASES, ids=CASE_IDS)
def test_newton_step_and_saved_factor(nx, nu, T, B, ps, dtype):
    pr, plant, inp = _case(nx, nu, T, B, ps, dtype)
    t = _dev(pr, inp)
    dt, n = TD[dtype], nx + nu
    prob, xb = _args(pr, t)
    d, g = Guarded((B, T, n), dt, DEV), Guarded((B, T, n), dt, DEV)
    fac = Guarded((B, T, n * (n + 1) // 2), dt, DEV)
    info = Guarded((B,), torch.int32, DEV, init=torch.zeros(B, dtype=torch.int32))
    be = _be()
    be.newton_step_xbox(pr["dims"], t["z"], t["xn"], t["F"], *prob, xb, d.t, g_out=g.t, factor=fac.t, info=info.t)
    d2 = Guarded((B, T, n), dt, DEV)
    be.newton_step_xbox(pr["dims"], t["z"], t["xn"], t["F"], *prob, xb, d2.t)   # without the optional outputs
    torch.cuda.synchronize()
    assert be.last_step_kernel == "k_newton_step_xbox"
    assert d.intact() and g.intact() and fac.intact() and info.intact() and d2.intact()
    assert (info.t == 0).all() and torch.equal(d.t, d2.t)
    assert torch.equal(t["lam"].cpu(), inp["lam"]) and torch.equal(t["z"].cpu(), inp["z"])   # read-only
    g_ref, d_ref = inp["g"].numpy(), inp["d"].numpy()
    zs = float(pr["z0"].abs().max())
    eg = scale_err(g.t.cpu().numpy(), g_ref, G_FLOOR[dtype] * float(np.abs(g_ref).max()))
    ed = scale_err(d.t.cpu().numpy(), d_ref, 1e-5 * zs)
    # the saved factor in alqp_backward: w = -H^{-1} gbar against the dense solve with the reference's Hessian of this step
    Hd, Hs = inp["hessian"]
    i = np.arange(nx)
    # active state rows are on its diagonal: the last stage has rho (its equality row) and rho per active state row, no F'F
    assert (Hd[:, T - 1][..., i, i] > pr["Qd"].numpy()[:, T - 1, :nx] + 1.5 * 10).any()   # (rho = 10)
    gbar = torch.randn(B, T, n, generator=torch.Generator().manual_seed(1), dtype=F64).to(dt)
    qg, Qg = Guarded((B, T, n), dt, DEV), Guarded((B, T, n), dt, DEV)
    be.backward(pr["dims"], fac.t, t["F"], t["rho"], t["z"], gbar.to(DEV), qg.t, Qg.t)
    torch.cuda.synchronize()
    assert qg.intact() and Qg.intact()
    w_ref = dense_w(Hd.astype(np.float64), Hs.astype(np.float64), gbar.double().numpy())
    ew = scale_err(qg.t.cpu().double().numpy(), w_ref, 1e-30)
    print(f"XSTEP step ({nx},{nu}) T={T} B={B} {dtype}: g {eg:.2e} d {ed:.2e} w {ew:.2e} (of the largest; bounds "
          f"{10 * RT[dtype]:.0e} {100 * RT[dtype]:.0e} {100 * RT[dtype]:.0e})")
    assert eg < 10 * RT[dtype], ("g", eg)
    assert ed < 100 * RT[dtype], ("d", ed)
    assert ew < 100 * RT[dtype], ("w", ew)


# ---- merit, line search, dual update ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("nx,nu,T,B,ps", ssr.GPU_CASES, ids=CASE_IDS)
def test_merit_pick_and_dual_update(nx, nu, T, B, ps, dtype):
    pr, plant, inp = _case(nx, nu, T, B, ps, dtype)
    t = _dev(pr, inp)
    dt, n, eps = TD[dtype], nx + nu, ax.EPS[TD[dtype]]
    prob, xb = _args(pr, t)
    be, ref = _be(), ssr.XboxStepOracleBackend()
    pr64, in64 = _up(pr, inp)
    prob64, xb64 = _args(pr64, {**pr64, **in64})
    # -- merit of two stacked points: the iterate and the full step
    zc, xn_all = _candidates(plant, t["z"], t["d"], 2, nx)
    phi, rn2 = Guarded((2, B), dt, DEV), Guarded((2, B), dt, DEV)
    be.merit_xbox(pr["dims"], 2, zc, xn_all, *prob, xb, phi.t, rn2.t)
    torch.cuda.synchronize()
    assert phi.intact() and rn2.intact()
    zc64, xn64 = zc.cpu().double(), xn_all.cpu().double()
    p_ref, r_ref = torch.empty(2, B, dtype=F64), torch.empty(2, B, dtype=F64)
    ref.merit_xbox(pr["dims"], 2, zc64, xn64, *prob64, xb64, p_ref, r_ref)
    gam, gam2 = ax.gamma_merit(T, nx, nu, 0), ax.gamma_rnorm2(T, nx, nu, 0)
    worst = {}
    for k in range(2):
        _, A, _, A2 = ssr.merit_magnitude_xbox(pr64, zc64[k], xn64[k], in64["lam"], in64["rho"])
        e1 = np.abs(phi.t[k].cpu().double().numpy() - p_ref[k].numpy()) / (eps * A)
        e2 = np.abs(rn2.t[k].cpu().double().numpy() - r_ref[k].numpy()) / (eps * A2)
        worst["merit"] = max(worst.get("merit", 0), e1.max() / gam)
        worst["rn2"] = max(worst.get("rn2", 0), e2.max() / gam2)
        assert (e1 <= gam).all() and (e2 <= gam2).all(), (k, e1.max(), gam, e2.max(), gam2)
    # -- the line search in one launch, all 20 candidates and fewer
    gamc = ax.gamma_merit(T, nx, nu, 0, cand=True)
    excused = 0
    for n_ls in (20, 7):
        zc, xn_all = _candidates(plant, t["z"], t["d"], n_ls, nx)
        z = Guarded((B, T, n), dt, DEV, init=inp["z"])
        pa = Guarded((n_ls, B), dt, DEV)
        pp = Guarded((B,), dt, DEV, init=phi.t[0])
        r2 = Guarded((B,), dt, DEV, init=torch.full((B,), -1.0, dtype=dt))
        kk = Guarded((B,), torch.int32, DEV)
        acc = Guarded((B,), torch.int32, DEV)
        be.merit_pick_xbox(pr["dims"], n_ls, t["d"], xn_all, *prob, xb, z.t, pp.t, rnorm2=r2.t, phi_all=pa.t, k_out=kk.t,
                           accept_out=acc.t)
        torch.cuda.synchronize()
        assert all(v.intact() for v in (z, pa, pp, r2, kk, acc))
        z64, pp64 = in64["z"].clone(), phi.t[0].cpu().double()
        pa64, k64, a64 = torch.empty(n_ls, B, dtype=F64), torch.zeros(B, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)
        ref.merit_pick_xbox(pr["dims"], n_ls, in64["d"], xn_all.cpu().double(), *prob64, xb64, z64, pp64, phi_all=pa64,
                            k_out=k64, accept_out=a64)
        al = (2.0 ** -np.arange(n_ls)).reshape(n_ls, 1, 1, 1)
        zmag = np.abs(in64["z"].numpy())[None] + al * np.abs(in64["d"].numpy())[None]
        A = np.stack([ssr.merit_magnitude_xbox(pr64, zc[k].cpu().double(), xn_all[k].cpu().double(), in64["lam"], in64["rho"],
                                               zmag=zmag[k])[1] for k in range(n_ls)])
        tol = gamc * eps * A
        e = np.abs(pa.t.cpu().double().numpy() - pa64.numpy())
        worst["pick"] = max(worst.get("pick", 0), (e / tol).max())
        assert (e <= tol).all(), (n_ls, (e / tol).max())
        # k equals the reference's wherever its two best merits are further apart than the merit tolerance
        srt = np.sort(pa64.numpy(), 0)
        decided = srt[1] - srt[0] > 2 * tol.max(0)
        kg, ag = kk.t.cpu().numpy(), acc.t.cpu().numpy()
        assert np.array_equal(kg[decided], k64.numpy()[decided]), (kg, k64)
        if n_ls == 20:
            excused = int((~decided).sum())
        sure = np.abs(pa64.numpy().min(0) - phi.t[0].cpu().double().numpy()) > 2 * tol.max(0)   # accept: strictly below phi_prev
        assert np.array_equal(ag[sure & decided], a64.numpy()[sure & decided])
        assert torch.equal(pp.t.cpu(), pa.t.cpu()[torch.from_numpy(kg).long(), torch.arange(B)])   # phi_prev <- the minimum
        step = torch.from_numpy(np.where(ag > 0, 2.0 ** -kg.astype(np.float64), 0.0)).to(dt)[:, None, None]
        ulp = torch.finfo(dt).eps * float(inp["z"].abs().max() + inp["d"].abs().max())   # (the kernel may fuse the multiply-add)
        assert (z.t.cpu() - (inp["z"] + step * inp["d"])).abs().max() <= 2 * ulp
        assert ((r2.t.cpu() == -1.0) == torch.from_numpy(ag == 0)).all()
    assert excused <= B // 4, excused
    # -- dual update
    lam = Guarded(tuple(inp["lam"].shape), dt, DEV, init=inp["lam"])
    rho = Guarded((B,), dt, DEV, init=inp["rho"])
    xn = ssr.true_next(plant, t["z"], nx)
    sb_u, st_u, _, _ = ssr.strides(pr)
    be.dual_update_xbox(pr["dims"], t["z"], xn, t["x0"], t["lo"], t["hi"], sb_u, st_u, xb, lam.t, rho.t)
    torch.cuda.synchronize()
    assert lam.intact() and rho.intact()
    l64, r64 = in64["lam"].clone(), in64["rho"].clone()
    ref.dual_update_xbox(pr["dims"], in64["z"], xn.cpu().double(), pr64["x0"], pr64["lo"], pr64["hi"], sb_u, st_u, xb64, l64, r64)
    assert torch.equal(rho.t.cpu(), inp["rho"] * 10)
    # |lam| + rho (|a| + |b|) per row, three roundings (aux_cases.gamma_dual_rows): equality and control rows from
    # aux_cases.dual_magnitude on the plain part, the state rows stated here
    f = lambda v: v.double().numpy()
    plain, lxu, lxl = sbr.split_lam(f(inp["lam"]), T, nx, nu)
    bc = lambda v, m: np.broadcast_to(f(v), (B, T, m))
    dm = ax.dual_magnitude(f(inp["z"]), f(xn.cpu()), f(pr["x0"]), plain, f(inp["rho"]), bc(pr["lo"], nu), bc(pr["hi"], nu))
    rr = f(inp["rho"]).reshape(B, 1, 1)
    xm = np.abs(f(inp["z"])[..., :nx])
    mag = sbr.join_lam(dm.mag, np.abs(lxu) + rr * (xm + np.abs(bc(pr["xhi"], nx))), np.abs(lxl) + rr * (xm + np.abs(bc(pr["xlo"], nx))),
                       T, nx, nu)
    e = np.abs(f(lam.t.cpu()) - l64.numpy())
    worst["dual"] = (e / (3 * eps * mag)).max()
    assert (e <= 3 * eps * mag).all(), worst["dual"]
    _, nxu, nxl = sbr.split_lam(f(lam.t.cpu()), T, nx, nu)
    assert (nxu > 0).any() and (nxl > 0).any() and (nxu == 0).any() and (nxu >= 0).all() and (nxl >= 0).all()
    print(f"XSTEP aux ({nx},{nu}) T={T} B={B} {dtype}: worst share of its bound: merit {worst['merit']:.2f} rn2 {worst['rn2']:.2f} "
          f"pick {worst['pick']:.2f} dual {worst['dual']:.2f}; k excused for {excused} of {B} instances")


# ---- inert bounds against the plain kernels ----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("nx,nu,T,B,ps", ssr.GPU_CASES, ids=CASE_IDS)
def test_inert_bounds_equal_the_plain_kernels_bitwise(nx, nu, T, B, ps, dtype):
    pr, plant, inp = _case(nx, nu, T, B, ps, dtype)
    t = _dev(pr, inp)
    dt, n = TD[dtype], nx + nu
    be = _be()
    plain_np, _, _ = sbr.split_lam(inp["lam"].numpy(), T, nx, nu)
    lam_p = torch.from_numpy(plain_np).to(DEV)
    zero = np.zeros((B, T, nx), plain_np.dtype)
    lam_x = torch.from_numpy(sbr.join_lam(plain_np, zero, zero, T, nx, nu)).to(DEV)
    if ps:
        xlo, xhi = torch.full((B, T, nx), -INERT, dtype=dt, device=DEV), torch.full((B, T, nx), INERT, dtype=dt, device=DEV)
        xbi = (xlo, xhi, T * nx, nx)
    else:
        xbi = (torch.full((nx,), -INERT, dtype=dt, device=DEV), torch.full((nx,), INERT, dtype=dt, device=DEV), 0, 0)
    pp, _ = _args(pr, t, lam=lam_p)
    px, _ = _args(pr, t, lam=lam_x)
    new = lambda *s: torch.empty(*s, dtype=dt, device=DEV)
    out = {}
    for name in ("plain", "xbox"):
        o = dict(d=new(B, T, n), g=new(B, T, n), fac=new(B, T, n * (n + 1) // 2), phi=new(1, B), rn2=new(1, B), pa=new(20, B),
                 z=t["z"].clone(), k=torch.zeros(B, dtype=torch.int32, device=DEV), acc=torch.zeros(B, dtype=torch.int32, device=DEV),
                 lam=(lam_p if name == "plain" else lam_x).clone(), rho=t["rho"].clone())
        out[name] = o
        if name == "plain":
            be.newton_step(pr["dims"], t["z"], t["xn"], t["F"], *pp, o["d"], g_out=o["g"], factor=o["fac"])
            be.merit(pr["dims"], 1, t["z"], ssr.true_next(plant, t["z"], nx), *pp, o["phi"], o["rn2"])
        else:
            be.newton_step_xbox(pr["dims"], t["z"], t["xn"], t["F"], *px, xbi, o["d"], g_out=o["g"], factor=o["fac"])
            be.merit_xbox(pr["dims"], 1, t["z"], ssr.true_next(plant, t["z"], nx), *px, xbi, o["phi"], o["rn2"])
        _, xn_all = _candidates(plant, t["z"], o["d"], 20, nx)
        o["pp"] = o["phi"][0].clone()
        sb_u, st_u, _, _ = ssr.strides(pr)
        if name == "plain":
            be.merit_pick(pr["dims"], 20, o["d"], xn_all, *pp, o["z"], o["pp"], rnorm2=o["rn2"][0], phi_all=o["pa"], k_out=o["k"],
                          accept_out=o["acc"])
            be.dual_update(pr["dims"], o["z"], ssr.true_next(plant, o["z"], nx), t["x0"], t["lo"], t["hi"], sb_u, st_u, o["lam"], o["rho"])
        else:
            be.merit_pick_xbox(pr["dims"], 20, o["d"], xn_all, *px, xbi, o["z"], o["pp"], rnorm2=o["rn2"][0], phi_all=o["pa"],
                               k_out=o["k"], accept_out=o["acc"])
            be.dual_update_xbox(pr["dims"], o["z"], ssr.true_next(plant, o["z"], nx), t["x0"], t["lo"], t["hi"], sb_u, st_u, xbi,
                                o["lam"], o["rho"])
    torch.cuda.synchronize()
    a, b = out["plain"], out["xbox"]
    bits = lambda v: v.contiguous().view(torch.int64 if v.dtype == F64 else torch.int32)
    for key in ("d", "g", "fac", "phi", "pa", "pp", "rn2", "z", "rho"):
        assert torch.equal(bits(a[key]), bits(b[key])), key
    assert torch.equal(a["k"], b["k"]) and torch.equal(a["acc"], b["acc"])
    lp, lxu, lxl = sbr.split_lam(b["lam"].cpu().numpy(), T, nx, nu)
    assert np.array_equal(lp.view(np.int64 if dt == F64 else np.int32), a["lam"].cpu().numpy().view(np.int64 if dt == F64 else np.int32))
    assert not lxu.any() and not lxl.any()   # every inert multiplier exactly 0


# ---- whole solves through MPC -------------------------------------------------------------------------------------------
def _mpc_solve(pr, plant, be, dev, mode, requires_grad=True, al_iter=3):
    from deq_mpc_corl_amd import MPC, QuadCost
    B, T, nx, nu = pr["dims"]
    d = lambda a: a.to(dev)
    mpc = MPC(nx, nu, T, u_lower=d(pr["lo"]), u_upper=d(pr["hi"]), n_batch=B, dtype=F64, backend=be, exit_mode=mode,
              al_iter=al_iter, x_lower=d(pr["xlo"]), x_upper=d(pr["xhi"]))
    mpc.reinitialize(d(pr["x0"]), None)
    leaf = {k: d(pr[k]).clone().requires_grad_(requires_grad) for k in ("Qd", "q")}
    x, u, _ = mpc(d(pr["x0"]), QuadCost(torch.diag_embed(leaf["Qd"]), leaf["q"]), plant, plant.jac,
                  x_init=d(pr["z0"][..., :nx]).clone(), u_init=d(pr["z0"][..., nx:]).clone())
    return mpc, x, u, leaf


class _NoQuad:
    """HipBackend with its calls watched: no quad workspace may be asked for, and the step must be the team kernel's."""

    def __init__(self, be):
        self._be, self.steps = be, 0

    def __getattr__(self, name):
        if name in ("_workspace", "new_workspace", "backward_ws"):
            be = self._be

            def wrapped(*a, **kw):
                raise AssertionError(f"{name} was reached with state bounds")
            return wrapped if hasattr(be, name) else getattr(be, name)
        return getattr(self._be, name)

    def newton_step_xbox(self, *a, **kw):
        self.steps += 1
        return self._be.newton_step_xbox(*a, **kw)

    def newton_step(self, *a, **kw):
        raise AssertionError("the plain step kernel was reached with state bounds")


@pytest.mark.parametrize("mode", ["reference", "fixed"])
@pytest.mark.parametrize("nx,nu,T,B", [(2, 1, 5, 5), (13, 4, 5, 3)])
def test_whole_solves_through_mpc(nx, nu, T, B, mode):
    """HipBackend against the reference backend on the nonlinear plant: Newton counts, x, u, lam and the cost gradients,
    with the bounds tests/test_gpu_state_bounds.py has for its whole solves through MPC (1e-6 on the float32 x, u; 2e-9 on
    lam; 100 RT on a gradient)."""
    pr, plant = ssr.bounded_plant_problem(B, T, nx, nu, F64)
    m0, x0, u0, leaf0 = _mpc_solve(pr, plant, ssr.XboxStepOracleBackend(), "cpu", mode)
    be = _NoQuad(_be())
    m1, x1, u1, leaf1 = _mpc_solve(pr, plant, be, DEV, mode)
    gen = torch.Generator().manual_seed(5)
    gx, gu = torch.randn(x0.shape, generator=gen), torch.randn(u0.shape, generator=gen)
    ((x1 * gx.to(DEV)).sum() + (u1 * gu.to(DEV)).sum()).backward()
    ((x0 * gx).sum() + (u0 * gu).sum()).backward()
    torch.cuda.synchronize()
    assert list(m1.last_newton_per_al) == list(m0.last_newton_per_al) and be.steps == sum(m0.last_newton_per_al)
    dev_xu = max(float((x1.detach().cpu() - x0.detach()).abs().max()), float((u1.detach().cpu() - u0.detach()).abs().max()))
    el = float((m1.lamda_prev.cpu() - m0.lamda_prev).abs().max())
    _, lxu, lxl = sbr.split_lam(m0.lamda_prev.numpy(), T, nx, nu)
    assert m1.lamda_prev.shape == (B, sbr.lam_width(T, nx, nu)) and (lxu.max() > 0 or lxl.max() > 0)
    eg = {k: scale_err(leaf1[k].grad.cpu().numpy(), leaf0[k].grad.numpy(), 1e-30) for k in ("Qd", "q")}
    print(f"XSTEP mpc ({nx},{nu}) {mode}: Newton counts {list(m1.last_newton_per_al)}, |x,u - ref| {dev_xu:.2e}, |lam - ref| {el:.2e}, "
          f"dQd {eg['Qd']:.2e} dq {eg['q']:.2e} (of the largest)")
    assert dev_xu < 1e-6 and el < 2e-9
    assert torch.equal(m1.rho_prev.cpu(), m0.rho_prev)
    assert all(float(leaf1[k].grad.abs().max()) > 0 and eg[k] < 100 * RT["f64"] for k in eg), eg


def test_large_batch_takes_the_team_step():
    """B = 4096, (2,1), T = 3: the batch from which the plain callable route takes the quad step. With state bounds the
    team step runs (no workspace), and the results are the reference backend's. Reference exit mode: the Newton loop ends
    when the batch has converged. (With a fixed 4 steps the later ones are taken past convergence, where d ~ 1e-7 moves
    the merit by less than its rounding error, all 20 candidates tie and the pick is decided by the last bit; over 4096
    instances one such step shows: measured |lam - ref| 2.1e-6 in fixed mode.)"""
    nx, nu, T, B = 2, 1, 3, 4096
    pr, plant = ssr.bounded_plant_problem(B, T, nx, nu, F64)
    hip = _be()
    assert B >= hip.QUAD_MIN_BATCH
    be = _NoQuad(hip)
    m1, x1, u1, leaf1 = _mpc_solve(pr, plant, be, DEV, "reference", al_iter=2)
    (x1.sum() + u1.sum()).backward()
    torch.cuda.synchronize()
    m0, x0, u0, leaf0 = _mpc_solve(pr, plant, ssr.XboxStepOracleBackend(), "cpu", "reference", al_iter=2)
    (x0.sum() + u0.sum()).backward()
    assert list(m1.last_newton_per_al) == list(m0.last_newton_per_al)
    assert be.steps == sum(m0.last_newton_per_al) and hip.last_step_kernel == "k_newton_step_xbox"
    dev_xu = max(float((x1.detach().cpu() - x0.detach()).abs().max()), float((u1.detach().cpu() - u0.detach()).abs().max()))
    el = float((m1.lamda_prev.cpu() - m0.lamda_prev).abs().max())
    eq = scale_err(leaf1["q"].grad.cpu().numpy(), leaf0["q"].grad.numpy(), 1e-30)
    print(f"XSTEP mpc B=4096: Newton counts {list(m1.last_newton_per_al)}, |x,u - ref| {dev_xu:.2e}, |lam - ref| {el:.2e}, dq {eq:.2e}")
    assert dev_xu < 1e-6 and el < 2e-9 and eq < 100 * RT["f64"]
