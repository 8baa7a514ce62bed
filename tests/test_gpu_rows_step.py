"""GPU tests of the launch-per-step kernels with general rows (k_newton_step_rows, k_merit_rows, k_merit_pick_rows,
k_dual_rows behind alqp_*_rows_*; MPC(ineqG=, ineqh=) with a callable dx, with or without state bounds; DESIGN section
25). The reference is tests/rows_step_reference.py's backend (pinned on the CPU by tests/test_rows_step_cpu.py), fed the
kernel's own inputs: lam, rho and the iterate after one reference AL iteration, where every instance has a general row
active with a nonzero multiplier (and, with state bounds, a state row active). Tolerances: the Newton step's are
tests/test_gpu_dense_cost.py's (g within 10 RT, d and w within 100 RT of the largest); merit, pick and dual update get
tests/aux_cases.py's magnitude-derived bounds with the rows' terms |lam_k| |r_k| and |G_k| . |z_t| in the magnitudes and
the rows' roundings in the counts (rows_step_reference.gamma_rows)."""
import functools

import numpy as np
import pytest
import torch

from tests import aux_cases as ax
from tests import gen_rows_reference as grr
from tests import rows_step_reference as rsr
from tests import state_bounds_reference as sbr
from tests import state_bounds_step_reference as ssr
from tests.aux_cases import Guarded
from tests.dense_cost_reference import dense_w
from tests.poly_rows_reference import poly_rows
from tests.test_gpu_dense_cost import G_FLOOR, RT, scale_err

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TD = {"f64": torch.float64, "f32": torch.float32}
F64 = torch.float64
INERT = 1e20
CASE_IDS = [f"{nx}x{nu}-T{T}-B{B}-m{m}-{lay}" for nx, nu, T, B, m, lay in rsr.GPU_CASES]
XB_IDS = ["rows", "rows+xbox"]


def _be():
    from deq_mpc_corl_amd.backend import default_backend
    return default_backend()


@functools.lru_cache(maxsize=None)
def _case(nx, nu, T, B, m, layout, xbox, dtype):
    """The case's problem, plant and reference inputs (CPU, computed once per session and never modified)."""
    return rsr.gpu_case(nx, nu, T, B, m, layout, xbox, TD[dtype])


def _dev(pr, inp):
    d = {k: v.to(DEV).contiguous() for k, v in pr.items() if torch.is_tensor(v)}
    d.update({k: v.to(DEV).contiguous() for k, v in inp.items() if torch.is_tensor(v)})
    return d


def _args(pr, t, xbox, lam=None, h=None):
    """prob, xbnd (None without state bounds), poly of the four methods on the tensors of `t`."""
    sb_u, st_u, xb, poly = rsr.args({**pr, **{k: t[k] for k in ("xlo", "xhi", "G", "h")}, **({"h": h} if h is not None else {})}, xbox)
    prob = (t["x0"], t["lam"] if lam is None else lam, t["rho"], t["Qd"], t["q"], t["lo"], t["hi"], sb_u, st_u)
    return prob, xb, poly


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
@pytest.mark.parametrize("xbox", [False, True], ids=XB_IDS)
@pytest.mark.parametrize("nx,nu,T,B,m,layout", rsr.GPU_CASES, ids=CASE_IDS)
def test_newton_step_and_saved_factor(nx, nu, T, B, m, layout, xbox, dtype):
    pr, plant, inp = _case(nx, nu, T, B, m, layout, xbox, dtype)
    t = _dev(pr, inp)
    dt, n = TD[dtype], nx + nu
    prob, xb, poly = _args(pr, t, xbox)
    d, g = Guarded((B, T, n), dt, DEV), Guarded((B, T, n), dt, DEV)
    fac = Guarded((B, T, n * (n + 1) // 2), dt, DEV)
    info = Guarded((B,), torch.int32, DEV, init=torch.zeros(B, dtype=torch.int32))
    be = _be()
    be.newton_step_rows(pr["dims"], t["z"], t["xn"], t["F"], *prob, xb, poly, d.t, g_out=g.t, factor=fac.t, info=info.t)
    d2 = Guarded((B, T, n), dt, DEV)
    be.newton_step_rows(pr["dims"], t["z"], t["xn"], t["F"], *prob, xb, poly, d2.t)   # without the optional outputs
    torch.cuda.synchronize()
    assert be.last_step_kernel == "k_newton_step_rows"
    assert d.intact() and g.intact() and fac.intact() and info.intact() and d2.intact()
    assert (info.t == 0).all() and torch.equal(d.t, d2.t)
    assert torch.equal(t["lam"].cpu(), inp["lam"]) and torch.equal(t["z"].cpu(), inp["z"])   # read-only
    g_ref, d_ref = inp["g"].numpy(), inp["d"].numpy()
    zs = float(pr["z0"].abs().max())
    eg = scale_err(g.t.cpu().numpy(), g_ref, G_FLOOR[dtype] * float(np.abs(g_ref).max()))
    ed = scale_err(d.t.cpu().numpy(), d_ref, 1e-5 * zs)
    # the saved factor in alqp_backward: w = -H^{-1} gbar against the dense solve with the reference's Hessian of this step,
    # which holds the active rows' rho G_k' G_k: the last stage's block has no F'F, so its state-control corner is theirs alone
    Hd, Hs = inp["hessian"]
    G_, h_ = (np.broadcast_to(a.numpy(), s) for a, s in ((pr["G"], (B, T, m, n)), (pr["h"], (B, T, m))))
    _, _, _, lp = grr.split_lam(inp["lam"].numpy(), T, nx, nu, xbox, m)
    _, Hp, _, _, _ = poly_rows(inp["z"].numpy(), G_, h_, lp, inp["rho"].numpy())
    corner, want = Hd[:, T - 1, :nx, nx:], Hp[:, T - 1, :nx, nx:]
    assert np.abs(Hp).max() > 0.05 and np.abs(corner - want).max() <= 1e-5 * np.abs(Hp).max()
    assert T * m < 4 or np.abs(want).max() > 0.05   # (the one shared row of the smallest case is slack at its last stage)
    gbar = torch.randn(B, T, n, generator=torch.Generator().manual_seed(1), dtype=F64).to(dt)
    qg, Qg = Guarded((B, T, n), dt, DEV), Guarded((B, T, n), dt, DEV)
    be.backward(pr["dims"], fac.t, t["F"], t["rho"], t["z"], gbar.to(DEV), qg.t, Qg.t)
    torch.cuda.synchronize()
    assert qg.intact() and Qg.intact()
    w_ref = dense_w(Hd.astype(np.float64), Hs.astype(np.float64), gbar.double().numpy())
    ew = scale_err(qg.t.cpu().double().numpy(), w_ref, 1e-30)
    print(f"ROWSTEP step ({nx},{nu}) T={T} B={B} m={m} {layout} xbox={xbox} {dtype}: g {eg:.2e} d {ed:.2e} w {ew:.2e} (of the "
          f"largest; bounds {10 * RT[dtype]:.0e} {100 * RT[dtype]:.0e} {100 * RT[dtype]:.0e})")
    assert eg < 10 * RT[dtype], ("g", eg)
    assert ed < 100 * RT[dtype], ("d", ed)
    assert ew < 100 * RT[dtype], ("w", ew)


# ---- merit, line search, dual update ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("xbox", [False, True], ids=XB_IDS)
@pytest.mark.parametrize("nx,nu,T,B,m,layout", rsr.GPU_CASES, ids=CASE_IDS)
def test_merit_pick_and_dual_update(nx, nu, T, B, m, layout, xbox, dtype):
    pr, plant, inp = _case(nx, nu, T, B, m, layout, xbox, dtype)
    t = _dev(pr, inp)
    dt, n, eps = TD[dtype], nx + nu, ax.EPS[TD[dtype]]
    prob, xb, poly = _args(pr, t, xbox)
    be, ref = _be(), rsr.RowsStepOracleBackend()
    pr64, in64 = _up(pr, inp)
    prob64, xb64, poly64 = _args(pr64, {**pr64, **in64}, xbox)
    # -- merit of two stacked points: the iterate and the full step
    zc, xn_all = _candidates(plant, t["z"], t["d"], 2, nx)
    phi, rn2 = Guarded((2, B), dt, DEV), Guarded((2, B), dt, DEV)
    be.merit_rows(pr["dims"], 2, zc, xn_all, *prob, xb, poly, phi.t, rn2.t)
    torch.cuda.synchronize()
    assert phi.intact() and rn2.intact()
    zc64, xn64 = zc.cpu().double(), xn_all.cpu().double()
    p_ref, r_ref = torch.empty(2, B, dtype=F64), torch.empty(2, B, dtype=F64)
    ref.merit_rows(pr["dims"], 2, zc64, xn64, *prob64, xb64, poly64, p_ref, r_ref)
    gam, gam2 = rsr.gamma_merit_rows(T, nx, nu, m), rsr.gamma_rnorm2_rows(T, nx, nu, m)
    worst = {}
    for k in range(2):
        _, A, _, A2 = rsr.merit_magnitude_rows(pr64, zc64[k], xn64[k], in64["lam"], in64["rho"], xbox)
        e1 = np.abs(phi.t[k].cpu().double().numpy() - p_ref[k].numpy()) / (eps * A)
        e2 = np.abs(rn2.t[k].cpu().double().numpy() - r_ref[k].numpy()) / (eps * A2)
        worst["merit"] = max(worst.get("merit", 0), e1.max() / gam)
        worst["rn2"] = max(worst.get("rn2", 0), e2.max() / gam2)
        assert (e1 <= gam).all() and (e2 <= gam2).all(), (k, e1.max(), gam, e2.max(), gam2)
    # -- the line search in one launch, all 20 candidates and fewer
    gamc = rsr.gamma_merit_rows(T, nx, nu, m, cand=True)
    excused = 0
    for n_ls in (20, 7):
        zc, xn_all = _candidates(plant, t["z"], t["d"], n_ls, nx)
        z = Guarded((B, T, n), dt, DEV, init=inp["z"])
        pa = Guarded((n_ls, B), dt, DEV)
        pp = Guarded((B,), dt, DEV, init=phi.t[0])
        r2 = Guarded((B,), dt, DEV, init=torch.full((B,), -1.0, dtype=dt))
        kk = Guarded((B,), torch.int32, DEV)
        acc = Guarded((B,), torch.int32, DEV)
        be.merit_pick_rows(pr["dims"], n_ls, t["d"], xn_all, *prob, xb, poly, z.t, pp.t, rnorm2=r2.t, phi_all=pa.t, k_out=kk.t,
                           accept_out=acc.t)
        torch.cuda.synchronize()
        assert all(v.intact() for v in (z, pa, pp, r2, kk, acc))
        z64, pp64 = in64["z"].clone(), phi.t[0].cpu().double()
        pa64, k64, a64 = torch.empty(n_ls, B, dtype=F64), torch.zeros(B, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)
        ref.merit_pick_rows(pr["dims"], n_ls, in64["d"], xn_all.cpu().double(), *prob64, xb64, poly64, z64, pp64, phi_all=pa64,
                            k_out=k64, accept_out=a64)
        al = (2.0 ** -np.arange(n_ls)).reshape(n_ls, 1, 1, 1)
        zmag = np.abs(in64["z"].numpy())[None] + al * np.abs(in64["d"].numpy())[None]
        A = np.stack([rsr.merit_magnitude_rows(pr64, zc[k].cpu().double(), xn_all[k].cpu().double(), in64["lam"], in64["rho"],
                                               xbox, zmag=zmag[k])[1] for k in range(n_ls)])
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
    sb_u, st_u = prob[-2:]
    be.dual_update_rows(pr["dims"], t["z"], xn, t["x0"], t["lo"], t["hi"], sb_u, st_u, xb, poly, lam.t, rho.t)
    torch.cuda.synchronize()
    assert lam.intact() and rho.intact()
    l64, r64 = in64["lam"].clone(), in64["rho"].clone()
    ref.dual_update_rows(pr["dims"], in64["z"], xn.cpu().double(), pr64["x0"], pr64["lo"], pr64["hi"], sb_u, st_u, xb64, poly64,
                         l64, r64)
    assert torch.equal(rho.t.cpu(), inp["rho"] * 10)
    # per row |lam| + rho x the magnitude of r with its roundings: equality and control rows 3 (aux_cases.dual_magnitude and
    # gamma_dual_rows), state rows 3, a general row n + 3 on |lam_k| + rho (|G_k| . |z_t| + |h_k|) (the dot product's n,
    # the difference, the product, the sum)
    f = lambda v: v.double().numpy()
    plain, lxu, lxl, lp = grr.split_lam(f(inp["lam"]), T, nx, nu, xbox, m)
    bc = lambda v, w: np.broadcast_to(f(v), (B, T, w))
    dm = ax.dual_magnitude(f(inp["z"]), f(xn.cpu()), f(pr["x0"]), plain, f(inp["rho"]), bc(pr["lo"], nu), bc(pr["hi"], nu))
    rr = f(inp["rho"]).reshape(B, 1, 1)
    zm = np.abs(f(inp["z"]))
    xu = xl = None
    if xbox:
        xu = 3 * (np.abs(lxu) + rr * (zm[..., :nx] + np.abs(bc(pr["xhi"], nx))))
        xl = 3 * (np.abs(lxl) + rr * (zm[..., :nx] + np.abs(bc(pr["xlo"], nx))))
    Gm = np.abs(np.broadcast_to(f(pr["G"]), (B, T, m, n)))
    pm = (n + 3) * (np.abs(lp) + rr * (np.einsum("btkj,btj->btk", Gm, zm) + np.abs(bc(pr["h"], m))))
    bound = eps * grr.join_lam(3 * dm.mag, xu, xl, pm, T, nx, nu)
    e = np.abs(f(lam.t.cpu()) - l64.numpy())
    worst["dual"] = (e / bound).max()
    assert (e <= bound).all(), worst["dual"]
    _, _, _, new = grr.split_lam(f(lam.t.cpu()), T, nx, nu, xbox, m)
    assert (new.reshape(B, -1) > 0).any(1).all() and (new >= 0).all() and (m == 1 or (new == 0).any())
    print(f"ROWSTEP aux ({nx},{nu}) T={T} B={B} m={m} {layout} xbox={xbox} {dtype}: worst share of its bound: merit "
          f"{worst['merit']:.2f} rn2 {worst['rn2']:.2f} pick {worst['pick']:.2f} dual {worst['dual']:.2f}; k excused for "
          f"{excused} of {B} instances")


# ---- inert rows against the plain / the state-bound kernels ------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("xbox", [False, True], ids=XB_IDS)
@pytest.mark.parametrize("nx,nu,T,B,m,layout", rsr.GPU_CASES, ids=CASE_IDS)
def test_inert_rows_equal_the_kernels_without_rows_bitwise(nx, nu, T, B, m, layout, xbox, dtype):
    """h = 1e20 on every row and zero row multipliers: the _rows kernels against the plain ones (no state bounds) or the
    _xbox ones (state bounds), on the plain / state-bound part of the case's lam."""
    pr, plant, inp = _case(nx, nu, T, B, m, layout, xbox, dtype)
    t = _dev(pr, inp)
    dt, n = TD[dtype], nx + nu
    be = _be()
    plain, lxu, lxl, _ = grr.split_lam(inp["lam"].numpy(), T, nx, nu, xbox, m)
    base = sbr.join_lam(plain, lxu, lxl, T, nx, nu) if xbox else plain
    lam_b = torch.from_numpy(base).to(DEV)
    lam_r = torch.from_numpy(grr.join_lam(plain, lxu, lxl, np.zeros((B, T, m), plain.dtype), T, nx, nu)).to(DEV)
    h_inert = torch.full_like(t["h"], INERT)
    pb, xb, _ = _args(pr, t, xbox, lam=lam_b)
    px, _, poly = _args(pr, t, xbox, lam=lam_r, h=h_inert)
    sb_u, st_u = pb[-2:]
    sfx = "_xbox" if xbox else ""
    ex = (xb,) if xbox else ()
    new = lambda *s: torch.empty(*s, dtype=dt, device=DEV)
    out = {}
    for name in ("base", "rows"):
        o = dict(d=new(B, T, n), g=new(B, T, n), fac=new(B, T, n * (n + 1) // 2), phi=new(1, B), rn2=new(1, B), pa=new(20, B),
                 z=t["z"].clone(), k=torch.zeros(B, dtype=torch.int32, device=DEV), acc=torch.zeros(B, dtype=torch.int32, device=DEV),
                 lam=(lam_b if name == "base" else lam_r).clone(), rho=t["rho"].clone())
        out[name] = o
        xn0 = ssr.true_next(plant, t["z"], nx)
        if name == "base":
            getattr(be, "newton_step" + sfx)(pr["dims"], t["z"], t["xn"], t["F"], *pb, *ex, o["d"], g_out=o["g"], factor=o["fac"])
            getattr(be, "merit" + sfx)(pr["dims"], 1, t["z"], xn0, *pb, *ex, o["phi"], o["rn2"])
        else:
            be.newton_step_rows(pr["dims"], t["z"], t["xn"], t["F"], *px, xb, poly, o["d"], g_out=o["g"], factor=o["fac"])
            be.merit_rows(pr["dims"], 1, t["z"], xn0, *px, xb, poly, o["phi"], o["rn2"])
        _, xn_all = _candidates(plant, t["z"], o["d"], 20, nx)
        o["pp"] = o["phi"][0].clone()
        if name == "base":
            getattr(be, "merit_pick" + sfx)(pr["dims"], 20, o["d"], xn_all, *pb, *ex, o["z"], o["pp"], rnorm2=o["rn2"][0],
                                            phi_all=o["pa"], k_out=o["k"], accept_out=o["acc"])
            getattr(be, "dual_update" + sfx)(pr["dims"], o["z"], ssr.true_next(plant, o["z"], nx), t["x0"], t["lo"], t["hi"], sb_u,
                                             st_u, *ex, o["lam"], o["rho"])
        else:
            be.merit_pick_rows(pr["dims"], 20, o["d"], xn_all, *px, xb, poly, o["z"], o["pp"], rnorm2=o["rn2"][0], phi_all=o["pa"],
                               k_out=o["k"], accept_out=o["acc"])
            be.dual_update_rows(pr["dims"], o["z"], ssr.true_next(plant, o["z"], nx), t["x0"], t["lo"], t["hi"], sb_u, st_u, xb,
                                poly, o["lam"], o["rho"])
    torch.cuda.synchronize()
    a, b = out["base"], out["rows"]
    bits = lambda v: v.contiguous().view(torch.int64 if v.dtype == F64 else torch.int32)
    for key in ("d", "g", "fac", "phi", "pa", "pp", "rn2", "z", "rho"):
        assert torch.equal(bits(a[key]), bits(b[key])), key
    assert torch.equal(a["k"], b["k"]) and torch.equal(a["acc"], b["acc"])
    pl, xu, xl, lp = grr.split_lam(b["lam"].cpu().numpy(), T, nx, nu, xbox, m)
    got = sbr.join_lam(pl, xu, xl, T, nx, nu) if xbox else pl
    iv = np.int64 if dt == F64 else np.int32
    assert np.array_equal(got.view(iv), a["lam"].cpu().numpy().view(iv))
    assert not lp.any()   # every inert multiplier exactly 0


# ---- whole solves through MPC -------------------------------------------------------------------------------------------
def _mpc_solve(pr, plant, be, dev, mode, xbox, al_iter=3):
    from deq_mpc_corl_amd import MPC, QuadCost
    B, T, nx, nu = pr["dims"]
    d = lambda a: a.to(dev)
    kwx = dict(x_lower=d(pr["xlo"]), x_upper=d(pr["xhi"])) if xbox else {}
    hleaf = d(pr["h"]).clone().requires_grad_(True)
    mpc = MPC(nx, nu, T, u_lower=d(pr["lo"]), u_upper=d(pr["hi"]), n_batch=B, dtype=F64, backend=be, exit_mode=mode,
              al_iter=al_iter, ineqG=d(pr["G"]), ineqh=hleaf, **kwx)
    mpc.reinitialize(d(pr["x0"]), None)
    leaf = {k: d(pr[k]).clone().requires_grad_(True) for k in ("Qd", "q")}
    leaf["h"] = hleaf
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
                raise AssertionError(f"{name} was reached with general rows")
            return wrapped if hasattr(be, name) else getattr(be, name)
        return getattr(self._be, name)

    def newton_step_rows(self, *a, **kw):
        self.steps += 1
        return self._be.newton_step_rows(*a, **kw)

    def newton_step(self, *a, **kw):
        raise AssertionError("the plain step kernel was reached with general rows")

    def newton_step_xbox(self, *a, **kw):
        raise AssertionError("the state-bound step kernel was reached with general rows")


def _compare(tag, m0, x0, u0, leaf0, m1, x1, u1, leaf1, lam_bound, keep=None):
    """The issue's bounds on the instances of `keep` (all of them when None): x, u equal as float32, lam within lam_bound,
    the three gradients within 100 RT of the largest; Newton counts and rho for the whole batch."""
    B = x0.shape[0]
    keep = torch.ones(B, dtype=torch.bool) if keep is None else torch.as_tensor(keep)
    kn = keep.numpy()
    dev_xu = max(float((x1.detach().cpu() - x0.detach())[keep].abs().max()), float((u1.detach().cpu() - u0.detach())[keep].abs().max()))
    el = float((m1.lamda_prev.cpu() - m0.lamda_prev)[keep].abs().max())
    eg = {k: scale_err(leaf1[k].grad.cpu().numpy()[kn], leaf0[k].grad.numpy()[kn], 1e-30) for k in ("Qd", "q", "h")}
    print(f"ROWSTEP mpc {tag}: Newton counts {list(m1.last_newton_per_al)}, compared {int(keep.sum())} of {B} instances, "
          f"|x,u - ref| {dev_xu:.2e}, |lam - ref| {el:.2e} (bound {lam_bound:.1e}), dQd {eg['Qd']:.2e} dq {eg['q']:.2e} dineqh "
          f"{eg['h']:.2e} (of the largest)")
    assert list(m1.last_newton_per_al) == list(m0.last_newton_per_al)
    assert dev_xu == 0.0   # x, u come back as float32: equal as such
    assert el <= lam_bound
    assert torch.equal(m1.rho_prev.cpu(), m0.rho_prev)
    assert all(float(leaf1[k].grad.abs().max()) > 0 and eg[k] < 100 * RT["f64"] for k in eg), eg


def _twin_bound(nx, nu, xbox, m0):
    return max(8 * rsr.INERT_TWIN[(nx, nu, xbox)], 64 * 2.0 ** -53 * float(m0.lamda_prev.abs().max()))


@pytest.mark.parametrize("xbox", [False, True], ids=XB_IDS)
@pytest.mark.parametrize("mode", ["reference", "fixed"])
@pytest.mark.parametrize("nx,nu,T,B", [(2, 1, 5, 5), (13, 4, 5, 3)])
def test_whole_solves_through_mpc(nx, nu, T, B, mode, xbox):
    """HipBackend against the reference backend on the nonlinear plant with a coupled row x_0 + x_1 <= h: Newton counts,
    x, u (equal as float32), lam and the gradients w.r.t. q, diag(Q) and ineqh (100 RT of the largest). lam: 2e-9 with a
    fixed 4 steps (steps past convergence, section 24), the twin bound with the reference exit - the larger of 8 times the
    route twin's inert |dlam| (rows_step_reference.INERT_TWIN) and 64 eps of the largest multiplier.

    The (2,1) problem is rows_step_reference.WHOLE_SOLVE_KW's (a heavier sine): with SinPlant's own, every solve at this
    size has a line search whose two best candidates are exactly equal in the reference (a step taken past convergence),
    the pick hangs on the last bit, and the solvers end one float32 ulp apart (measured: x, u 1.5e-8 to 4.5e-8, lam 9.6e-8
    to 5.1e-7). The chosen problem has no such step; that is asserted on the reference alone in tests/test_rows_step_cpu.py.

    Measured on an MI355X: x, u equal as float32 in all eight cases, Newton counts equal, gradients within 2.6e-14; lam at
    (2,1) within 1.1e-13 / 6.1e-14 (reference exit, twin bounds 5.8e-13 / 1.9e-13) and 1.1e-13 / 4.6e-14 (fixed), at (13,4)
    within 2.9e-14 (bounds 3.4e-13 / 6.8e-13) and 2.5e-14. A heavier sine still (gain 10, seed 4) is as free of ties but
    more sensitive to rounding - a one-ulp change of q moves the reference's lam by 11.6 times the twin bound - and the
    kernels ended 9 and 17 times the bound from the reference there (1.4e-11, 3.9e-11)."""
    pr, plant, _ = rsr.coupled_row_problem(B, T, nx, nu, xbox, mode, **rsr.WHOLE_SOLVE_KW[(nx, nu)])
    m0, x0, u0, leaf0 = _mpc_solve(pr, plant, rsr.RowsStepOracleBackend(), "cpu", mode, xbox)
    be = _NoQuad(_be())
    m1, x1, u1, leaf1 = _mpc_solve(pr, plant, be, DEV, mode, xbox)
    gen = torch.Generator().manual_seed(5)
    gx, gu = torch.randn(x0.shape, generator=gen), torch.randn(u0.shape, generator=gen)
    ((x1 * gx.to(DEV)).sum() + (u1 * gu.to(DEV)).sum()).backward()
    ((x0 * gx).sum() + (u0 * gu).sum()).backward()
    torch.cuda.synchronize()
    assert be.steps == sum(m0.last_newton_per_al)
    _, _, _, lp = grr.split_lam(m0.lamda_prev.numpy(), T, nx, nu, xbox, 1)
    assert m1.lamda_prev.shape == (B, grr.lam_width(T, nx, nu, xbox, 1)) and lp.max() > 0
    bound = 2e-9 if mode == "fixed" else _twin_bound(nx, nu, xbox, m0)
    _compare(f"({nx},{nu}) {mode} xbox={xbox}", m0, x0, u0, leaf0, m1, x1, u1, leaf1, bound)


@pytest.mark.parametrize("xbox", [False, True], ids=XB_IDS)
@pytest.mark.parametrize("mode", ["reference"])
def test_whole_solves_on_the_plain_sin_plant_at_2_1(mode, xbox):
    """The (2,1) whole solve on SinPlant itself (the case above runs a heavier sine, for the reason its docstring gives),
    with the near-tie rule applied per instance: an instance in which some line search of the REFERENCE solve is not
    decided by float64 arithmetic (rows_step_reference.TieBackend: the two best merits, or the best and phi_prev, within
    twice the merit's rounding bound) is excused from the comparison of the iterates - two correct solvers may part ways
    there by that step's |d| - and every other instance is held to the bounds of the case above. No cap on the share at
    this size: with the reference exit 3 of the 5 instances have such a step, and with a fixed 4 steps all 5 have one,
    which leaves nothing to compare - hence the reference exit alone here (both counts asserted on the CPU,
    tests/test_rows_step_cpu.py). Newton counts and rho are compared for the whole batch, and an excused instance must
    stay within 10 of its tied steps."""
    nx, nu, T, B = 2, 1, 5, 5
    pr, plant, _ = rsr.coupled_row_problem(B, T, nx, nu, xbox, mode)
    ref = rsr.TieBackend()
    m0, x0, u0, leaf0 = _mpc_solve(pr, plant, ref, "cpu", mode, xbox)
    be = _NoQuad(_be())
    m1, x1, u1, leaf1 = _mpc_solve(pr, plant, be, DEV, mode, xbox)
    (x1.sum() + u1.sum()).backward()
    (x0.sum() + u0.sum()).backward()
    torch.cuda.synchronize()
    keep = ~ref.undecided
    assert keep.any()
    bound = 2e-9 if mode == "fixed" else _twin_bound(nx, nu, xbox, m0)
    _compare(f"(2,1) SinPlant {mode} xbox={xbox}", m0, x0, u0, leaf0, m1, x1, u1, leaf1, bound, keep)
    dz = torch.maximum((x1.detach().cpu() - x0.detach()).abs().reshape(B, -1).max(1).values,
                       (u1.detach().cpu() - u0.detach()).abs().reshape(B, -1).max(1).values).numpy()
    print(f"ROWSTEP mpc (2,1) SinPlant {mode} xbox={xbox}: excused {int(ref.undecided.sum())} of {B}; their |x,u - ref| "
          f"{dz[ref.undecided].max() if ref.undecided.any() else 0:.2e}, largest tied step {ref.tied_step.max():.2e}")
    assert (dz[ref.undecided] <= 10 * ref.tied_step[ref.undecided] + 1e-7).all()   # (+ a float32 ulp of the returned x, u)


def test_large_batch_takes_the_team_step():
    """B = 4096, (2,1), T = 3, SinPlant: the batch from which the plain callable route takes the quad step. With rows the
    team step runs (no workspace), with the reference backend's Newton counts. Reference exit mode. The iterates, lam and
    the gradients are held to the bounds of the whole solves above (x, u equal as float32, lam within the twin bound, the
    gradients within 100 RT) in every instance whose reference solve has no undecided line search
    (rows_step_reference.TieBackend, the near-tie rule per instance); at most a quarter of the instances may be excused
    (666 of 4096 are: asserted on the CPU too). An excused instance must stay within 10 of its tied steps."""
    nx, nu, T, B = 2, 1, 3, 4096
    pr, plant, _ = rsr.coupled_row_problem(B, T, nx, nu, False, "reference", every_instance=False)
    hip = _be()
    assert B >= hip.QUAD_MIN_BATCH
    be = _NoQuad(hip)
    m1, x1, u1, leaf1 = _mpc_solve(pr, plant, be, DEV, "reference", False, al_iter=2)
    (x1.sum() + u1.sum()).backward()
    torch.cuda.synchronize()
    ref = rsr.TieBackend()
    m0, x0, u0, leaf0 = _mpc_solve(pr, plant, ref, "cpu", "reference", False, al_iter=2)
    (x0.sum() + u0.sum()).backward()
    assert be.steps == sum(m0.last_newton_per_al) and hip.last_step_kernel == "k_newton_step_rows"
    assert ref.undecided.sum() <= B // 4, int(ref.undecided.sum())
    _compare("B=4096 (2,1) reference", m0, x0, u0, leaf0, m1, x1, u1, leaf1, _twin_bound(nx, nu, False, m0), ~ref.undecided)
    dz = torch.maximum((x1.detach().cpu() - x0.detach()).abs().reshape(B, -1).max(1).values,
                       (u1.detach().cpu() - u0.detach()).abs().reshape(B, -1).max(1).values).numpy()
    print(f"ROWSTEP mpc B=4096: excused {int(ref.undecided.sum())} of {B}; their |x,u - ref| {dz[ref.undecided].max():.2e}, "
          f"largest tied step {ref.tied_step.max():.2e}")
    assert (dz[ref.undecided] <= 10 * ref.tied_step[ref.undecided] + 1e-7).all()   # (+ a float32 ulp of the returned x, u)
