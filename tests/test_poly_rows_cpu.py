"""Stage-wise linear rows G_t z_t <= h_t through MPC(ineqG=, ineqh=), without a GPU: the host wiring on the test backend of
tests/poly_rows_reference.py, and that backend itself pinned.

The reference carries ineqG / ineqh but never calls the code that reads them (AL_mpc.py:496-498), so there is no golden.
The pins are: the row function `poly_rows` with G selecting the controls equals what the reference-pinned oracle adds for
its control rows (1), rows that state a state box reproduce the pinned state-bound backend (2), inert rows reproduce the
reference-generated goldens (3), g is the gradient of the merit (4), the KKT residuals of a solve with mixed rows are those
of the state-bound twin (5), and central finite differences for the gradients, ineqh's included (6)."""
import numpy as np
import pytest
import torch

from oracle import oracle_py as orc
from tests import aux_cases as ax
from tests import golden_util as gu
from tests import poly_rows_reference as prr
from tests import state_bounds_reference as sbr
from tests.oracle_backend import OracleBackend
from tests.test_dyn_grad_cpu import FD_H, FD_TOL, dyn_grads

F64 = torch.float64
INERT = 1e20
SHAPES = [(2, 1), (4, 2), (13, 4)]


def t64(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(F64)


def _mpc(dims, lo, hi, be, exit_mode="reference", al_iter=2, **kw):
    from deq_mpc_corl_amd import MPC
    B, T, nx, nu = dims
    return MPC(nx, nu, T, u_lower=lo, u_upper=hi, n_batch=B, dtype=F64, exit_mode=exit_mode, al_iter=al_iter, backend=be, **kw)


def _solve(mpc, Qd, q, F, c, x0, z0, nx):
    from deq_mpc_corl_amd import QuadCost
    from deq_mpc_corl_amd.qpth.al_utils import LinDx
    mpc.reinitialize(x0, None)
    return mpc(x0, QuadCost(torch.diag_embed(Qd), q), LinDx(F, c), None, x_init=z0[..., :nx].clone(), u_init=z0[..., nx:].clone())


# ---- 1. the row function pinned to the oracle, with G selecting the controls -----------------------------------------
@pytest.mark.parametrize("dims,bounds", [((3, 2, 3, 1), "shared"), ((5, 4, 13, 3), "full"), ((37, 20, 13, 4), "per_stage")],
                         ids=ax.grid_id)
def test_row_function_equals_the_oracles_control_rows(dims, bounds):
    """(oracle with the real control bounds) - (oracle with inert control bounds +-1e20 and zero control multipliers) is
    what the control rows contribute; poly_rows with G = [0 I; 0 -I], h = [uhi; -ulo] must give exactly that, to the
    rounding of the subtraction (bounds: tests/test_state_bounds_cpu.py's, from tests/aux_cases.py's magnitudes). The
    case's iterate has controls inside and outside their bounds; one is put exactly on its upper bound."""
    c = ax.case(dims, F64, "plain", bounds)
    B, T, nx, nu = dims
    n = nx + nu
    f = lambda a: a.double().numpy().copy()
    z, xn, lam, rho, lo, hi = f(c.z), f(c.xnext), f(c.lam), f(c.rho), f(c.ulo_full), f(c.uhi_full)
    z[0, T - 1, nx] = hi[0, T - 1, 0]   # exactly on its bound: r = 0 counts in H (>= 0), not in g (> 0)
    u = z[..., nx:]
    ru, rl = u - hi, -u + lo
    assert (ru > 0).any() and (rl > 0).any() and ((ru < 0) & (rl < 0)).any() and (ru == 0).any()
    le, lu, ll, _ = ax._split_lam(lam, T, nx, nu, 0)
    G = np.zeros((2 * nu, n))
    G[:nu, nx:], G[nu:, nx:] = np.eye(nu), -np.eye(nu)
    gx, Hx, px, rx, lnew = prr.poly_rows(z, G, np.concatenate([hi, -lo], 2), np.concatenate([lu, ll], 2), rho)
    lam0 = lam.copy()
    lam0[:, T * nx:] = 0
    big = np.full((B, T, nu), INERT)
    args = (xn, f(c.p.x0))
    cost = (f(c.p.Qd), f(c.p.q))
    eps = ax.EPS[F64]
    p1, r1 = orc.merit("f64", z, *args, lam, rho, *cost, lo, hi)
    p0, r0 = orc.merit("f64", z, *args, lam0, rho, *cost, -big, big)
    mm = ax.merit_magnitude(z, xn, f(c.p.x0), lam, rho, *cost, lo, hi)
    gam = ax.gamma_merit(T, nx, nu, 0) + T * n   # + the oracle's sequential sums
    e_phi = np.abs((p1 - p0) - px)
    assert (e_phi <= 2 * gam * eps * mm.A).all(), (e_phi / (eps * mm.A)).max()
    assert (np.abs((r1 - r0) - rx) <= 2 * gam * eps * mm.A2).all()
    g1, H1, _ = orc.grad_hess("f64", z, *args[:1], f(c.p.F), args[1], lam, rho, *cost, lo, hi)
    g0, H0, _ = orc.grad_hess("f64", z, *args[:1], f(c.p.F), args[1], lam0, rho, *cost, -big, big)
    dm = ax.dual_magnitude(z, xn, f(c.p.x0), lam, rho, lo, hi)
    vm = dm.mag[:, :T * nx].reshape(B, T, nx)            # |lam| + rho |r| of the equality rows
    bm = dm.mag[:, T * nx:].reshape(B, T, 2 * nu)        # of the control rows
    Fm = np.abs(f(c.p.F))
    gm = np.abs(cost[0]) * np.abs(z) + np.abs(cost[1])
    gm[:, :T - 1] += np.einsum("btij,bti->btj", Fm, vm[:, :T - 1])
    gm[..., nx:] += bm[..., :nu] + bm[..., nu:]
    e_g = np.abs((g1 - g0) - gx)
    assert (e_g[..., nx:] <= 2 * (n + 6) * eps * gm[..., nx:]).all(), (e_g[..., nx:] / (eps * gm[..., nx:])).max()
    assert not gx[..., :nx].any() and not (g1 - g0)[..., :nx].any()
    i = np.arange(nx, n)
    hm = np.abs(cost[0])[..., nx:] + rho[:, None, None] * (2 + np.pad((Fm ** 2).sum(2), ((0, 0), (0, 1), (0, 0)))[..., nx:])
    e_h = np.abs((H1 - H0)[..., i, i] - Hx[..., i, i])
    assert (e_h <= 2 * (nx + 4) * eps * hm).all()
    off = Hx.copy()
    off[..., i, i] = 0
    assert not off.any()   # unit rows: nothing off the diagonal, nothing on the states
    l1, _ = orc.dual_update("f64", z, *args, lo, hi, lam, rho)
    tol = (ax.gamma_dual_rows(T, nx, nu, 0) * eps * dm.mag)[:, T * nx:]
    assert (np.abs(l1[:, T * nx:] - lnew.reshape(B, -1)) <= tol).all()
    print(f"{dims} {bounds}: phi {e_phi.max():.1e} g {e_g.max():.1e} H {e_h.max():.1e}; rows active {(ru > 0).sum() + (rl > 0).sum()}, "
          f"inactive {((ru < 0) & (rl < 0)).sum()}, on the bound {(ru == 0).sum()}")


# ---- 2. rows that state a state box: the pinned state-bound backend ---------------------------------------------------
# Both backends run the same arithmetic on these rows: residuals (one entry of z times +-1, minus h), g, the diagonal of H
# and the dual update are bit-equal; only the merit's sums run in another order (numpy's pairwise sum over [T, 2 nx]
# against two sums over [T, nx]), about T nx eps |phi|, which can move an iterate only through a line-search near-tie.
# So the bound is a rounding bound on values of magnitude <= ~10: 64 eps. Measured: 0.0 on every case (bit-equal).
TWIN_TOL = 64 * 2.0 ** -53


@pytest.mark.parametrize("T", [20, 2])
@pytest.mark.parametrize("nx,nu", SHAPES)
@pytest.mark.parametrize("exit_mode", ["fixed", "reference"])
def test_box_twin(nx, nu, T, exit_mode):
    B = 3
    pr = sbr.xbox_problem(B, T, nx, nu, F64, per_stage=True)
    G, h = prr.box_as_rows(pr["xlo"], pr["xhi"], nx, nu)
    out = {}
    for kind in ("xbox", "poly"):
        be = sbr.XboxOracleBackend() if kind == "xbox" else prr.PolyOracleBackend()
        kw = dict(x_lower=pr["xlo"], x_upper=pr["xhi"]) if kind == "xbox" else dict(ineqG=G, ineqh=h)
        mpc = _mpc(pr["dims"], pr["lo"], pr["hi"], be, exit_mode, **kw)
        x, u, _ = _solve(mpc, pr["Qd"], pr["q"], pr["F"], pr["c"], pr["x0"], pr["z0"], nx)
        assert set(be.calls) == {"solve_lin_" + kind}
        out[kind] = (torch.cat((x, u), -1).double(), mpc.lamda_prev.clone(), list(mpc.last_newton_per_al), mpc.rho_prev.clone())
    assert out["xbox"][2] == out["poly"][2], (out["xbox"][2], out["poly"][2])   # Newton counts
    assert torch.equal(out["xbox"][3], out["poly"][3])
    # same layout: [u - uhi | -u + ulo | x - xhi | -x + xlo] is [u - uhi | -u + ulo | rows] for G = [I 0; -I 0]
    assert out["xbox"][1].shape == out["poly"][1].shape == (B, prr.lam_width(T, nx, nu, 2 * nx))
    dz = float((out["xbox"][0] - out["poly"][0]).abs().max())
    scale = max(1.0, float(out["xbox"][1].abs().max()))
    dl = float((out["xbox"][1] - out["poly"][1]).abs().max())
    print(f"({nx},{nu}) T={T} {exit_mode}: Newton steps {out['poly'][2]}, |z_xbox - z_poly| {dz:.1e}, |lam_xbox - lam_poly| {dl:.1e} "
          f"(largest multiplier {scale:.3g})")
    assert (out["poly"][1][:, T * nx:].reshape(B, T, -1)[..., 2 * nu:] > 0).any()   # state rows bind
    assert dz <= TWIN_TOL * 10 and dl <= TWIN_TOL * scale
    # the fp64 iterates themselves (MPC returns float32): one fixed-exit solve through the backends directly
    if exit_mode == "fixed":
        a = sbr.run_solve(sbr.XboxOracleBackend(), pr["Qd"], pr["q"], pr["F"], pr["c"], pr["x0"], pr["lo"], pr["hi"], pr["xlo"],
                          pr["xhi"], pr["z0"])
        b = prr.run_solve(prr.PolyOracleBackend(), pr["Qd"], pr["q"], pr["F"], pr["c"], pr["x0"], pr["lo"], pr["hi"], G, h, pr["z0"])
        dz = float((a["z"] - b["z"]).abs().max())
        print(f"   fp64 iterates: |z_xbox - z_poly| {dz:.1e}")
        assert dz <= TWIN_TOL * max(1.0, float(a["z"].abs().max()))
        assert float((a["lam"] - b["lam"]).abs().max()) <= TWIN_TOL * scale


# ---- 3. inert rows change nothing -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pend_f64_al2", "cart_f64_al2", "pend_active_f64_al6"])
def test_inert_rows_reproduce_goldens(name):
    g = gu.load(name)
    B, T, nx, nu = g["B"], g["T"], g["nx"], g["nu"]
    m = 3
    Gm = torch.randn(m, nx + nu, generator=torch.Generator().manual_seed(3), dtype=F64)
    out = {}
    for rows in (False, True):
        be = prr.PolyOracleBackend()
        kw = dict(ineqG=Gm, ineqh=torch.full((m,), float("inf"))) if rows else {}
        mpc = _mpc((B, T, nx, nu), t64(g["u_lo"]), t64(g["u_hi"]), be, al_iter=g["al_iter"], **kw)
        x, u, _ = _solve(mpc, t64(g["Qd"]), t64(g["q"]), t64(g["F"]), t64(g["c"]), t64(g["x0"]), t64(g["z0"]), nx)
        assert set(be.calls) == {"solve_lin_poly" if rows else "solve_lin"}
        out[rows] = (x, u, mpc.lamda_prev.numpy(), mpc.rho_prev, list(mpc.last_newton_per_al))
    assert out[True][4] == out[False][4] == list(g["newton_per_al"])
    for x, u, *_ in out.values():   # tests/test_host_logic.py's tolerance for the fp64 goldens
        assert np.abs(x.numpy() - g["x"]).max() < 2e-5 and np.abs(u.numpy() - g["u"]).max() < 2e-5
    assert torch.equal(out[True][0], out[False][0]) and torch.equal(out[True][1], out[False][1])
    assert torch.equal(out[True][3], out[False][3])
    plain, lp = prr.split_lam(out[True][2], T, nx, nu, m)
    assert out[True][2].shape == (B, prr.lam_width(T, nx, nu, m))
    assert np.array_equal(plain, out[False][2])
    assert not lp.any()   # exactly 0


# ---- 4. g is the gradient of the merit ---------------------------------------------------------------------------------
FD_TOL_MERIT = 1.6e-7   # tests/test_dense_cost_cpu.py's bound for its difference checks, same step 1e-5


@pytest.mark.parametrize("nx,nu,T,B,layout", [(2, 1, 5, 3, "per_stage"), (4, 2, 6, 3, "shared"), (13, 4, 4, 2, "per_instance")])
def test_g_is_the_gradient_of_the_merit(nx, nu, T, B, layout):
    m = 3
    pr = prr.poly_problem(B, T, nx, nu, m, F64, layout)
    gen = np.random.default_rng(4)
    f = lambda a: a.numpy().copy()
    z = f(pr["z0"]) + 0.3 * gen.standard_normal((B, T, nx + nu))
    lo, hi = f(pr["lo"]), f(pr["hi"])
    G = np.broadcast_to(f(pr["G"]), (B, T, m, nx + nu))
    h = np.broadcast_to(f(pr["h"]), (B, T, m))
    rho = np.full(B, 10.0)
    lam = 0.3 * gen.standard_normal((B, prr.lam_width(T, nx, nu, m)))
    lam[:, T * nx:] = np.maximum(lam[:, T * nx:], 0)
    ll, lp = prr.split_lam(lam, T, nx, nu, m)
    # no row within 1e-3 of its kink (probes of +-1e-5 then stay on one quadratic piece): move the offenders
    for _ in range(4):
        u = z[..., nx:]
        z[..., nx:] += 5e-3 * ((np.abs(u - hi) < 2e-3) | (np.abs(u - lo) < 2e-3))
        r = np.einsum("btkj,btj->btk", G, z) - h
        near = np.abs(r) < 2e-3   # move z_t along the row, off the kink, by 5e-3 in the residual
        z += np.einsum("btk,btkj->btj", 5e-3 * near / (G ** 2).sum(-1), G)
    u = z[..., nx:]
    r = np.einsum("btkj,btj->btk", G, z) - h
    assert min(np.abs(r).min(), np.abs(u - hi).min(), np.abs(lo - u).min()) > 1e-3
    assert (r > 0).any() and (r < 0).any()
    Fn, cn, x0 = f(pr["F"]), f(pr["c"]), f(pr["x0"])
    xnext = lambda v: np.einsum("btij,btj->bti", Fn, v[:, :-1]) + cn
    merit = lambda v: prr.merit_poly("f64", v, xnext(v), x0, ll, lp, rho, f(pr["Qd"]), f(pr["q"]), lo, hi, G, h)[0]
    g, _, _ = prr.grad_hess_poly("f64", z, xnext(z), Fn, x0, ll, lp, rho, f(pr["Qd"]), f(pr["q"]), lo, hi, G, h)
    probes = []
    for _ in range(12):
        b, t, i = (int(gen.integers(0, s)) for s in z.shape)
        zp, zm = z.copy(), z.copy()
        zp[b, t, i] += FD_H
        zm[b, t, i] -= FD_H
        probes.append((g[b, t, i], (merit(zp)[b] - merit(zm)[b]) / (2 * FD_H)))
    scale = max(abs(a) for a, _ in probes)
    err = max(abs(a - fd) for a, fd in probes) / scale
    print(f"({nx},{nu}) {layout}: g vs central differences of the merit: {err:.2e} (relative to the largest probed {scale:.3g}); "
          f"rows violated {(r > 0).sum()} of {r.size}")
    assert err < FD_TOL_MERIT, (err, probes)


# ---- 5. independent minimiser: KKT residuals of a solve with mixed rows -----------------------------------------------
def _lagrangian_grad(pr, z, plain, extra):
    """C z + q + J' lam: the oracle's gradient at rho = 0 is the Lagrangian's for the plain rows; `extra` adds the rest."""
    f = lambda a: a.numpy()
    zn = f(z)
    xn = np.einsum("btij,btj->bti", f(pr["F"]), zn[:, :-1]) + f(pr["c"])
    zero = np.zeros(zn.shape[0])
    g, _, _ = orc.grad_hess("f64", zn, xn, f(pr["F"]), f(pr["x0"]), plain, zero, f(pr["Qd"]), f(pr["q"]), f(pr["lo"]), f(pr["hi"]))
    return g + extra(zn, zero)


def _kkt_poly(pr, o):
    B, T, nx, nu = pr["dims"]
    m = pr["m"]
    plain, lp = prr.split_lam(o["lam"].numpy(), T, nx, nu, m)
    G = np.broadcast_to(pr["G"].numpy(), (B, T, m, nx + nu))
    h = np.broadcast_to(pr["h"].numpy(), (B, T, m))
    g = _lagrangian_grad(pr, o["z"], plain, lambda zn, zero: prr.poly_rows(zn, G, h, lp, zero)[0])
    r = prr.poly_residuals(pr, o["z"])
    active = float(((r > -1e-6) | (lp > 0)).mean())
    return np.array([np.abs(g).max(), np.maximum(r, 0).max(), max(0.0, -lp.min()), np.abs(lp * r).max()]), active


def _kkt_xbox(pr, o):
    B, T, nx, nu = pr["dims"]
    plain, lxu, lxl = sbr.split_lam(o["lam"].numpy(), T, nx, nu)
    xl, xh = pr["xlo"].numpy(), pr["xhi"].numpy()

    def extra(zn, zero):
        e = np.zeros_like(zn)
        e[..., :nx] = sbr.box_rows(zn[..., :nx], xl, xh, lxu, lxl, zero)[0]
        return e
    g = _lagrangian_grad(pr, o["z"], plain, extra)
    ru, rl = sbr.xbox_residuals(pr, o["z"])
    r, lam = np.concatenate([ru, rl], 2), np.concatenate([lxu, lxl], 2)
    return np.array([np.abs(g).max(), np.maximum(r, 0).max(), max(0.0, -lam.min()), np.abs(lam * r).max()])


# The yardstick is the pinned state-bound backend's own KKT residuals on the box twin of item 2 after the same 9 AL
# iterations of 8 Newton steps (rho 1 .. 1e8). The multiple: a mixed row has norm up to about 3 where a box row has 1,
# and three such rows meet in one variable: 10. A floor of 64 eps times the largest multiplier stands in where the twin's
# figure is exactly 0 (feasible to the last bit, or no negative multiplier - the projection makes that exact for both).
# What the figures are made of: feasibility, the sign of lam and complementarity come out orders of magnitude below the
# twin's (the twin's state box is infeasible for its dynamics, ||r+|| stays 0.4 - 0.6 and its multipliers grow with rho).
# Stationarity is taken at the RETURNED lam, after the last dual update, and is dominated in both solves by rows that
# end with r < 0 and an old multiplier > 0: the iterate balanced the old multiplier, the update projected it to
# max(0, lam + rho r), up to 0 at rho = 1e8. An infeasible row (r > 0) has no such lag, which is why the twin's figure is
# the smaller one. The generator: rows signed towards the rowless minimiser (`toward`), slacks 0.01 .. 0.05, so that they
# bind; of seeds 5..44 at (4,2) those where at least a quarter of the rows end active AND the reference meets the bound
# are 27 and 37 (stationarity 4.0 and 6.2 times the twin's; the other seeds range from 3 to 250 times, mostly with fewer
# rows active), and at (2,1) there is none (29 times and up): the check holds for the chosen problems, not for the method.
KKT_MULTIPLE = 10.0
AL_ITERS = 9


@pytest.mark.parametrize("nx,nu,seed", [(4, 2, 27), (4, 2, 37)])
def test_kkt_residuals_of_mixed_rows_against_the_box_twin(nx, nu, seed):
    T, B, m = 6, 4, 3
    px = sbr.xbox_problem(B, T, nx, nu, F64, per_stage=True)
    ox = sbr.run_solve(sbr.XboxOracleBackend(), px["Qd"], px["q"], px["F"], px["c"], px["x0"], px["lo"], px["hi"], px["xlo"], px["xhi"],
                       px["z0"], al_iter=AL_ITERS, max_newton=8)
    kx = _kkt_xbox(px, ox)
    # the rowless minimiser the rows are signed towards: the plain problem through the pinned oracle backend
    p0 = prr.poly_problem(B, T, nx, nu, m, F64, "per_instance", seed=seed)
    zt, lt = p0["z0"].clone(), torch.zeros(B, T * nx + 2 * T * nu, dtype=F64)
    OracleBackend().solve_lin(p0["dims"], p0["Qd"], p0["q"], p0["F"], p0["c"], p0["x0"], p0["lo"], p0["hi"], 0, 0, zt, lt,
                              torch.ones(B, dtype=F64), torch.zeros(B, dtype=F64), al_iter=6, max_newton=8)
    pp = prr.poly_problem(B, T, nx, nu, m, F64, "per_instance", seed=seed, toward=zt, slack=(0.01, 0.05))
    op = prr.run_solve(prr.PolyOracleBackend(), pp["Qd"], pp["q"], pp["F"], pp["c"], pp["x0"], pp["lo"], pp["hi"], pp["G"], pp["h"],
                       pp["z0"], al_iter=AL_ITERS, max_newton=8)
    kp, active = _kkt_poly(pp, op)
    names = ("stationarity |C z + q + J' lam|_inf", "max (G z - h)+", "-min lam", "max |lam_k r_k|")
    floor = 64 * 2.0 ** -53 * max(1.0, float(op["lam"].abs().max()), float(ox["lam"].abs().max()))
    for nm, a, b in zip(names, kp, kx):
        print(f"({nx},{nu}): {nm}: mixed rows {a:.2e}, box twin {b:.2e}")
    print(f"({nx},{nu}): rows active at the end {active:.2f}; rho {float(op['rho'].max()):.1e}")
    assert active >= 0.25, active
    assert op["info"].eq(0).all() and ox["info"].eq(0).all()
    assert (kp <= KKT_MULTIPLE * np.maximum(kx, floor)).all(), (kp, kx, floor)


# ---- 6. gradients through MPC against central differences -------------------------------------------------------------
class _WiringBackend(prr.PolyOracleBackend):
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


def _stationary(nx, nu, seed, layout, B=4, T=5, m=3):
    """The poly problem, a warm stage (2 AL iterations) and `stage`: one AL iteration of 4 Newton steps - what
    MPC(al_iter=1, exit_mode='fixed') runs - from the warm stage's (z, lam, rho)."""
    pr = prr.poly_problem(B, T, nx, nu, m, F64, layout, seed=seed, **(SHARED_KW if layout == "shared" else {}))
    be = prr.PolyOracleBackend()
    args = lambda d: (d["Qd"], d["q"], d["F"], d["c"], d["x0"], pr["lo"], pr["hi"], d["G"], d["h"])
    warm = prr.run_solve(be, *args(pr), pr["z0"], al_iter=2, max_newton=4)
    assert torch.allclose(warm["rho"], torch.full_like(warm["rho"], 100.0))

    def stage(**over):
        return prr.run_solve(be, *args({**pr, **over}), warm["z"], warm["lam"], warm["rho"], al_iter=1, max_newton=4)
    return pr, warm, stage


def _stage_conditions(pr, warm, stage):
    """(max |g(z_final)|, rows active at z_final, distance of the nearest row - general or control - to switching)."""
    B, T, nx, nu = pr["dims"]
    m = pr["m"]
    zf = stage()["z"]
    f = lambda t: t.numpy()
    ll, lp = prr.split_lam(f(warm["lam"]), T, nx, nu, m)
    xn = np.einsum("btij,btj->bti", f(pr["F"]), f(zf)[:, :-1]) + f(pr["c"])
    G = np.broadcast_to(f(pr["G"]), (B, T, m, nx + nu))
    h = np.broadcast_to(f(pr["h"]), (B, T, m))
    g, _, _ = prr.grad_hess_poly("f64", f(zf), xn, f(pr["F"]), f(pr["x0"]), ll, lp, f(warm["rho"]), f(pr["Qd"]), f(pr["q"]),
                                 f(pr["lo"]), f(pr["hi"]), G, h)
    r = prr.poly_residuals(pr, zf)
    u = f(zf)[..., nx:]
    margin = min(np.abs(r).min(), np.abs(u - f(pr["hi"])).min(), np.abs(f(pr["lo"]) - u).min())
    return zf, np.abs(g).reshape(B, -1).max(1), int((r >= 0).sum()), r.size, margin


# An h shared by every (b, t) binds only near the (b, t) where G_k z_feas is largest: small slacks, state columns scaled down
# (tests/poly_rows_reference.py:poly_problem says why)
SHARED_KW = dict(slack=(0.005, 0.02), state_scale=0.1)
# seed per (size, form of ineqh): of seeds 3..90 one at which the stage is stationary after its 4 Newton steps AND has a row
# active, none (general or control) within 1e-3 of switching - all asserted in the test
GRAD_SEEDS = {(2, 1, "shared"): 74, (2, 1, "per_instance"): 29, (4, 2, "shared"): 47, (4, 2, "per_instance"): 25,
              (13, 4, "shared"): 87, (13, 4, "per_instance"): 10}


@pytest.mark.parametrize("nx,nu,layout", list(GRAD_SEEDS), ids=lambda v: str(v))
def test_gradients_through_mpc_vs_finite_differences(nx, nu, layout):
    """`layout` "shared": ineqG [m,n], ineqh [m]; "per_instance": [B,T,m,n] and [B,T,m]."""
    from deq_mpc_corl_amd import QuadCost
    from deq_mpc_corl_amd.qpth.al_utils import LinDx
    seed = GRAD_SEEDS[(nx, nu, layout)]
    pr, warm, stage = _stationary(nx, nu, seed, layout)
    B, T = pr["dims"][:2]
    zf, gmax, n_act, n_rows, margin = _stage_conditions(pr, warm, stage)
    print(f"({nx},{nu}) {layout} seed {seed}: max |g(z_final)| per instance {gmax}")
    print(f"({nx},{nu}) {layout}: rows active at z_final: {n_act} of {n_rows}; nearest to switching {margin:.2e}")
    assert (gmax < 1e-10).all(), gmax
    assert n_act >= 1 and margin > 1e-3
    be = _WiringBackend()
    hleaf = pr["h"].clone().requires_grad_(True)
    mpc = _mpc(pr["dims"], pr["lo"], pr["hi"], be, "fixed", al_iter=1, ineqG=pr["G"], ineqh=hleaf)
    mpc.reinitialize(pr["x0"], None)
    leaf = {k: pr[k].clone().requires_grad_(True) for k in ("Qd", "q", "F", "c", "x0")}
    leaf["h"] = hleaf
    x, u, _ = mpc.al_solve(warm["z"][..., :nx].clone(), warm["z"][..., nx:].clone(), LinDx(leaf["F"], leaf["c"]), None, leaf["x0"],
                           QuadCost(leaf["Qd"], leaf["q"]), lamda_init=warm["lam"].clone(), rho_init=warm["rho"].clone())
    assert set(be.calls) == {"solve_lin_poly"}
    gbar = torch.randn(B, T, nx + nu, generator=torch.Generator().manual_seed(1), dtype=F64).float().double()
    ((x.double() * gbar[..., :nx]).sum() + (u.double() * gbar[..., nx:]).sum()).backward()
    assert torch.equal(be.z_final, zf)   # the MPC ran the stage the differences go through
    assert hleaf.grad.shape == pr["h"].shape
    loss = lambda o: float((gbar * o["z"]).sum())
    rng = np.random.default_rng(2)
    # ineqh: every entry whose row is active in some (b, t) it applies to, else random ones (their gradient is 0)
    r = prr.poly_residuals(pr, zf)
    act = (r >= 0)
    if layout == "shared":
        h_idx = [(int(k),) for k in np.nonzero(act.any((0, 1)))[0]][:4]
    else:
        h_idx = [tuple(int(v) for v in i) for i in np.argwhere(act)][:4]
    h_idx += [tuple(int(rng.integers(0, s)) for s in pr["h"].shape) for _ in range(4 - len(h_idx))]
    probes = []
    for name in ("Qd", "q", "F", "c", "x0", "h"):
        for j in range(4):
            idx = h_idx[j] if name == "h" else tuple(int(rng.integers(0, s)) for s in pr[name].shape)
            vals = []
            for sgn in (1.0, -1.0):
                a = pr[name].clone()
                a[idx] += sgn * FD_H
                vals.append(loss(stage(**{name: a})))
            probes.append((name, float(leaf[name].grad[idx]), (vals[0] - vals[1]) / (2 * FD_H)))
    scale = max(abs(a) for _, a, _ in probes)
    for name in ("Qd", "q", "F", "c", "x0", "h"):
        e = max(abs(a - fd) for nm, a, fd in probes if nm == name) / scale
        print(f"({nx},{nu}) {layout}: d{name} vs central differences: {e:.2e} (relative to the largest probed gradient {scale:.3g})")
    assert max(abs(a) for nm, a, _ in probes if nm == "h") > 0   # an active row was probed
    err = max(abs(a - fd) for _, a, fd in probes) / scale
    assert err < FD_TOL, (err, probes)


# ---- 7. guards, layout, generator ------------------------------------------------------------------------------------
def test_guarded_combinations_raise():
    from deq_mpc_corl_amd import MPC, PendulumDynamics, QuadCost
    from deq_mpc_corl_amd.qpth.al_utils import LinDx
    from deq_mpc_corl_amd.qpth.AL_mpc_custom import Obstacle_MPC
    nx, nu, B, T, m = 2, 1, 3, 4, 2
    pr = prr.poly_problem(B, T, nx, nu, m, F64, "shared")
    kw = dict(u_lower=pr["lo"], u_upper=pr["hi"], n_batch=B, dtype=F64, backend=prr.PolyOracleBackend(), ineqG=pr["G"], ineqh=pr["h"])
    with pytest.raises(NotImplementedError, match="state_estimator"):
        MPC(nx, nu, T, state_estimator=True, **kw)
    with pytest.raises(NotImplementedError, match="diag_cost"):
        MPC(nx, nu, T, diag_cost=False, **kw)
    # the diag_cost guard comes before anything is asked of ineqG's shape, and before ineqh is asked for
    with pytest.raises(NotImplementedError, match="diag_cost"):
        MPC(nx, nu, T, diag_cost=False, **{**kw, "ineqG": torch.zeros(1), "ineqh": None})
    with pytest.raises(NotImplementedError, match="Obstacle_MPC"):
        Obstacle_MPC(3, nu, T, **{**kw, "ineqG": torch.zeros(m, 3 + nu, dtype=F64)})
    with pytest.raises(NotImplementedError, match="rows of ineqG"):   # says how to write the state box as rows
        MPC(nx, nu, T, x_lower=-1.0, x_upper=1.0, **kw)
    with pytest.raises(NotImplementedError, match="ineqG"):   # no gradient w.r.t. G
        MPC(nx, nu, T, **{**kw, "ineqG": pr["G"].clone().requires_grad_(True)})
    with pytest.raises(NotImplementedError):   # goal constraints stay unbuilt
        MPC(nx, nu, T, add_goal_constraint=True, **kw)
    for one in (dict(ineqG=None), dict(ineqh=None)):
        with pytest.raises(ValueError, match="ineqG and ineqh"):
            MPC(nx, nu, T, **{**kw, **one})
    for bad in (dict(ineqG=torch.zeros(m, nx + nu + 1)), dict(ineqG=torch.zeros(T + 1, m, nx + nu)), dict(ineqh=torch.zeros(m + 1)),
                dict(ineqh=torch.zeros(T + 1, m)), dict(ineqG=torch.zeros(65, nx + nu), ineqh=torch.zeros(65))):
        with pytest.raises(ValueError, match="ineq"):
            MPC(nx, nu, T, **{**kw, **bad})
    dyn = PendulumDynamics()
    cost = QuadCost(torch.diag_embed(pr["Qd"]), pr["q"])
    xi, ui = pr["z0"][..., :nx].clone(), pr["z0"][..., nx:].clone()
    mpc = MPC(nx, nu, T, **kw)
    mpc.reinitialize(pr["x0"], None)
    with pytest.raises(NotImplementedError, match="LinDx"):   # a callable dx
        mpc(pr["x0"], cost, dyn, dyn.jac, x_init=xi, u_init=ui)
    mpc = MPC(nx, nu, T, **kw)
    mpc.reinitialize(pr["x0"], None)
    mpc.linearize_once = True
    with pytest.raises(NotImplementedError, match="linearize_once"):
        mpc.al_solve_stream(xi, ui, LinDx(pr["F"], pr["c"]), dyn.jac, pr["x0"], QuadCost(pr["Qd"], pr["q"]))
    mpc = MPC(nx, nu, T, **kw)   # a lamda of the plain width handed to a solve with rows
    mpc.reinitialize(pr["x0"], None)
    with pytest.raises(ValueError, match="lamda"):
        mpc.al_solve(xi, ui, LinDx(pr["F"], pr["c"]), None, pr["x0"], QuadCost(pr["Qd"], pr["q"]),
                     lamda_init=torch.zeros(B, T * nx + 2 * T * nu, dtype=F64))
    mpc = MPC(nx, nu, T, **{**kw, "ineqG": torch.zeros(B + 1, T, m, nx + nu, dtype=F64)})   # rows for another batch size
    mpc.reinitialize(pr["x0"], None)
    with pytest.raises(ValueError, match="per instance"):
        mpc.al_solve(xi, ui, LinDx(pr["F"], pr["c"]), None, pr["x0"], QuadCost(pr["Qd"], pr["q"]))


def test_multiplier_width_and_row_forms():
    nx, nu, B, T, m = 2, 1, 3, 4, 3
    pr = prr.poly_problem(B, T, nx, nu, m, F64, "shared", seed=6, **SHARED_KW)
    M = T * nx + T * (2 * nu + m)

    def run(G, h, stream=False):
        from deq_mpc_corl_amd import QuadCost
        from deq_mpc_corl_amd.qpth.al_utils import LinDx
        be = prr.PolyOracleBackend()
        mpc = _mpc(pr["dims"], pr["lo"], pr["hi"], be, "fixed", ineqG=G, ineqh=h)
        assert mpc.nineq == 2 * nu * T + m * T and mpc.lamda_prev.shape == (B, M)
        if stream:
            mpc.reinitialize(pr["x0"], None)
            x, u, _ = mpc.al_solve_stream(pr["z0"][..., :nx].clone(), pr["z0"][..., nx:].clone(), LinDx(pr["F"], pr["c"]), None,
                                          pr["x0"], QuadCost(pr["Qd"], pr["q"]))
        else:
            x, u, _ = _solve(mpc, pr["Qd"], pr["q"], pr["F"], pr["c"], pr["x0"], pr["z0"], nx)
        assert set(be.calls) == {"solve_lin_poly"} and mpc.lamda_prev.shape == (B, M)
        return mpc, x, u
    # the three forms of one set of rows, G and h independently; the stream route takes them too
    G, h = pr["G"], pr["h"]
    m0, x0_, u0_ = run(G, h)
    forms = [(G.expand(T, m, nx + nu), h), (G, h.expand(T, m)), (G.expand(B, T, m, nx + nu).contiguous(), h.expand(B, T, m)),
             (G.expand(T, m, nx + nu), h.expand(B, T, m).contiguous())]
    for Gf, hf in forms:
        mf, x, u = run(Gf, hf)
        assert torch.equal(x, x0_) and torch.equal(u, u0_) and torch.equal(mf.lamda_prev, m0.lamda_prev)
    ms, xs, us = run(G, h, stream=True)
    assert torch.equal(xs, x0_) and torch.equal(us, u0_)
    rows = m0.lamda_prev[:, T * nx:].reshape(B, T, 2 * nu + m)[..., 2 * nu:]
    assert (rows >= 0).all() and (rows > 0).any()
    # a non-finite h entry is "no row": its multiplier stays exactly 0, the others are those of the m - 1 row problem
    h2 = h.clone()
    h2[1] = float("inf")
    m2, x2, u2 = run(G, h2)
    r2 = m2.lamda_prev[:, T * nx:].reshape(B, T, 2 * nu + m)[..., 2 * nu:]
    assert not r2[..., 1].any()
    # reinitialize / warm_start_initialize size lamda_prev by neq + nineq
    m0.reinitialize(pr["x0"], None)
    assert m0.lamda_prev.shape == (B, M)

    class A:
        rho_init_max = 10.0
    m0.warm_start_initialize(x0_, u0_, A())
    assert m0.lamda_prev.shape == (B, M)


@pytest.mark.parametrize("layout", prr.LAYOUTS)
@pytest.mark.parametrize("nx,nu,T,B,m", [(2, 1, 5, 3, 9), (8, 2, 4, 3, 5), (13, 4, 3, 2, 3)])
def test_generator_conditions(nx, nu, T, B, m, layout):
    ob = layout != "shared"
    pr = prr.poly_problem(B, T, nx, nu, m, F64, layout, on_boundary=ob)
    n = nx + nu
    G = pr["G"].expand(B, T, m, n)
    h = pr["h"].expand(B, T, m)
    # feasible by construction: the rollout under u = 0 satisfies every row and the control bounds
    zf = pr["zfeas"]
    assert not zf[..., nx:].any()
    assert torch.allclose(zf[:, 1:, :nx], torch.einsum("btij,btj->bti", pr["F"], zf[:, :-1]) + pr["c"]) and torch.equal(zf[:, 0, :nx], pr["x0"])
    assert (torch.einsum("btkj,btj->btk", G, zf) <= h).all()
    # rows couple states and controls
    assert (G[..., :nx].abs().sum(-1) > 0).sum() >= G[..., 0].numel() - B * T and (G[..., nx:].abs().sum(-1) > 0).all()
    # at the starting iterate every instance has a violated and a slack row
    r = prr.poly_residuals(pr, pr["z0"])
    assert ((r > 1e-3).reshape(B, -1).any(1) & (r < -1e-3).reshape(B, -1).any(1)).all()
    if ob:
        assert (r[:, 1, m - 1] == 0).all()   # the unit row sits exactly on its boundary
        assert torch.equal(G[:, 1, m - 1], torch.eye(n, dtype=F64)[nx].expand(B, n))
    assert prr.strides(pr["G"], pr["h"], T, m, n) == {"shared": (0, 0, 0, 0), "per_stage": (0, m * n, 0, m),
                                                       "per_instance": (T * m * n, m * n, T * m, m)}[layout]
