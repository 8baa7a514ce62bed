"""State bounds on the callable-dynamics route (MPC(x_lower=, x_upper=) with a callable dx), without a
GPU: the host wiring on the composed reference backend of tests/state_bounds_step_reference.py, and that backend pinned:
inert bounds reproduce the plain callable route bit for bit (1), an affine model given as a callable is the LinDx route's
twin (2), g is the gradient of the merit on a nonlinear plant (3), the dual update and the line search equal a direct
statement of the five row terms (4), gradients through MPC against central differences (5), the host routing (6), and
the GPU tests' inputs (7)."""
import numpy as np
import pytest
import torch

from tests import aux_cases as ax
from tests import golden_util as gu
from tests import state_bounds_reference as sbr
from tests import state_bounds_step_reference as ssr
from tests.oracle_backend import OracleBackend
from tests.recording_backend import RecordingBackend
from tests.test_dyn_grad_cpu import FD_H, FD_TOL

F64 = torch.float64
EPS64 = 2.0 ** -53


def t64(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(F64)


def _mpc(dims, lo, hi, be, exit_mode="reference", al_iter=2, **kw):
    from deq_mpc_corl_amd import MPC
    B, T, nx, nu = dims
    return MPC(nx, nu, T, u_lower=lo, u_upper=hi, n_batch=B, dtype=F64, exit_mode=exit_mode, al_iter=al_iter, backend=be, **kw)


def _call(mpc, pr, dx, dx_jac, Qd=None, q=None):
    from deq_mpc_corl_amd import QuadCost
    nx = pr["dims"][2]
    mpc.reinitialize(pr["x0"], None)
    cost = QuadCost(torch.diag_embed(pr["Qd"] if Qd is None else Qd), pr["q"] if q is None else q)
    return mpc(pr["x0"], cost, dx, dx_jac, x_init=pr["z0"][..., :nx].clone(), u_init=pr["z0"][..., nx:].clone())


# ---- 1. inert bounds change nothing ----------------------------------------------------------------------------------
def test_inert_bounds_reproduce_the_plain_callable_route():
    """pend_nonlin_f64_al4, the golden the callable route replays (tests/test_host_logic.py), with its gradients."""
    from deq_mpc_corl_amd import PendulumDynamics, QuadCost
    g = gu.load("pend_nonlin_f64_al4")
    B, T, nx, nu = g["B"], g["T"], g["nx"], g["nu"]
    out = {}
    for xb in (False, True):
        be = ssr.XboxStepOracleBackend() if xb else OracleBackend()
        kw = dict(x_lower=-float("inf"), x_upper=float("inf")) if xb else {}
        mpc = _mpc((B, T, nx, nu), t64(g["u_lo"]), t64(g["u_hi"]), be, al_iter=g["al_iter"], **kw)
        x0, z0 = t64(g["x0"]), t64(g["z0"])
        mpc.reinitialize(x0, None)
        Qd, q = t64(g["Qd"]).requires_grad_(True), t64(g["q"]).requires_grad_(True)
        dyn = PendulumDynamics()
        x, u, _ = mpc(x0, QuadCost(torch.diag_embed(Qd), q), dyn, dyn.jac, x_init=z0[..., :nx].clone(), u_init=z0[..., nx:].clone())
        ((x * torch.as_tensor(g["bwd_wx"]).float()).sum() + (u * torch.as_tensor(g["bwd_wu"]).float()).sum()).backward()
        if xb:
            assert set(be.calls) == {"newton_step_xbox", "merit_xbox", "merit_pick_xbox", "dual_update_xbox"}
        out[xb] = (x.detach(), u.detach(), mpc.lamda_prev.numpy(), mpc.rho_prev, list(mpc.last_newton_per_al), q.grad, Qd.grad)
    assert out[True][4] == out[False][4] == list(g["newton_per_al"])
    assert np.abs(out[True][0].numpy() - g["x"]).max() < 2e-5 and np.abs(out[True][1].numpy() - g["u"]).max() < 2e-5
    for i in (0, 1, 3, 5, 6):
        assert torch.equal(out[True][i], out[False][i]), i
    plain, lxu, lxl = sbr.split_lam(out[True][2], T, nx, nu)
    assert out[True][2].shape == (B, sbr.lam_width(T, nx, nu))
    assert np.array_equal(plain, out[False][2])
    assert not lxu.any() and not lxl.any()   # exactly 0


# ---- 2. route twin: an affine model as a callable against LinDx through solve_lin_xbox ---------------------------------
def _twin(nx, nu, mode, inert, B=3, T=5):
    from deq_mpc_corl_amd.qpth.al_utils import LinDx
    pr = sbr.xbox_problem(B, T, nx, nu, F64, per_stage=True, push=True)
    kw = dict(x_lower=-float("inf"), x_upper=float("inf")) if inert else dict(x_lower=pr["xlo"], x_upper=pr["xhi"])
    res = []
    for route in ("lin", "callable"):
        be = ssr.XboxStepOracleBackend()
        mpc = _mpc(pr["dims"], pr["lo"], pr["hi"], be, mode, al_iter=3, **kw)
        if route == "lin":
            x, u, _ = _call(mpc, pr, LinDx(pr["F"], pr["c"]), None)
            assert set(be.calls) == {"solve_lin_xbox"}
        else:
            dyn = ssr.AffineCallable(pr["F"], pr["c"])
            x, u, _ = _call(mpc, pr, dyn, dyn.jac)
            assert "solve_lin_xbox" not in be.calls and "newton_step_xbox" in be.calls
        res.append((mpc.x_init.double(), mpc.u_init.double(), mpc.lamda_prev.clone(), list(mpc.last_newton_per_al)))
    return pr, res


@pytest.mark.parametrize("mode", ["reference", "fixed"])
@pytest.mark.parametrize("nx,nu", [(2, 1), (4, 2), (13, 4)])
def test_route_twin(nx, nu, mode):
    """Both routes take the same steps on the same numbers; they order their sums differently (x_next is formed by the
    caller here, inside the reference's solve there). The same twin with inert bounds measures that difference; the bound
    with the bounds active is the larger of 8 times it and 64 eps of the largest entry."""
    figs = {}
    for inert in (True, False):
        pr, (a, b) = _twin(nx, nu, mode, inert)
        assert a[3] == b[3], (a[3], b[3])
        # x, u come back as float32: compare the carried multipliers in full precision, the iterate as returned
        figs[inert] = (max(float((a[0] - b[0]).abs().max()), float((a[1] - b[1]).abs().max())),
                       float((a[2] - b[2]).abs().max()),
                       max(float(a[0].abs().max()), float(a[1].abs().max())), float(a[2].abs().max()))
        if not inert:
            _, lxu, lxl = sbr.split_lam(a[2].numpy(), pr["dims"][1], nx, nu)
            assert (lxu > 0).any() and (lxl > 0).any()   # the bounds are active at the solution
    dz0, dl0, _, _ = figs[True]
    dz, dl, zmax, lmax = figs[False]
    print(f"({nx},{nu}) {mode}: inert twin |dz| {dz0:.2e} |dlam| {dl0:.2e}; active twin |dz| {dz:.2e} |dlam| {dl:.2e} "
          f"(largest z {zmax:.3g}, lam {lmax:.3g})")
    assert dz <= max(8 * dz0, 64 * EPS64 * zmax), (dz, dz0)
    assert dl <= max(8 * dl0, 64 * EPS64 * lmax), (dl, dl0)


# ---- 3. g against central differences of the merit on the nonlinear plant ----------------------------------------------
@pytest.mark.parametrize("nx,nu,T,B,ps", [(2, 1, 5, 3, True), (4, 2, 6, 3, False), (13, 4, 4, 2, True)])
def test_g_is_the_gradient_of_the_merit(nx, nu, T, B, ps):
    pr, plant = ssr.step_problem(B, T, nx, nu, F64, per_stage=ps)
    gen = torch.Generator().manual_seed(4)
    z = pr["z0"] + 0.3 * torch.randn(B, T, nx + nu, generator=gen, dtype=F64)
    lam = 0.3 * torch.randn(B, sbr.lam_width(T, nx, nu), generator=gen, dtype=F64)
    lam[:, T * nx:].clamp_(min=0)
    rho = torch.full((B,), 10.0, dtype=F64)
    xl, xh = (a if a.dim() == 3 else a.reshape(1, 1, nx) for a in (pr["xlo"], pr["xhi"]))
    lo, hi = (a if a.dim() == 3 else a.reshape(1, 1, nu) for a in (pr["lo"], pr["hi"]))
    for _ in range(3):   # no row within 1e-3 of its kink (probes of +-1e-5 stay on one quadratic piece): move the offenders
        x, u = z[..., :nx], z[..., nx:]
        z[..., :nx] += 5e-3 * (((x - xh).abs() < 2e-3) | ((x - xl).abs() < 2e-3))
        z[..., nx:] += 5e-3 * (((u - hi).abs() < 2e-3) | ((u - lo).abs() < 2e-3))
    x, u = z[..., :nx], z[..., nx:]
    rows = torch.cat([(x - xh).ravel(), (xl - x).ravel(), (u - hi).ravel(), (lo - u).ravel()])
    assert rows.abs().min() > 1e-3
    assert (x - xh > 0).any() and (xl - x > 0).any() and (x - xh < 0).any() and (xl - x < 0).any()
    be = ssr.XboxStepOracleBackend()
    sb_u, st_u, sb_x, st_x = ssr.strides(pr)
    xb = (pr["xlo"], pr["xhi"], sb_x, st_x)
    prob = (pr["x0"], lam, rho, pr["Qd"], pr["q"], pr["lo"], pr["hi"], sb_u, st_u)
    xn, F = ssr.linearize(plant, z, nx)
    d, g = torch.empty_like(z), torch.empty_like(z)
    be.newton_step_xbox(pr["dims"], z, xn, F, *prob, xb, d, g_out=g)

    def merit(v):
        phi = torch.zeros(B, dtype=F64)
        be.merit_xbox(pr["dims"], 1, v, ssr.true_next(plant, v, nx), *prob, xb, phi)
        return phi
    rng = np.random.default_rng(4)
    probes = []
    for _ in range(12):
        b, t, i = (int(rng.integers(0, s)) for s in z.shape)
        zp, zm = z.clone(), z.clone()
        zp[b, t, i] += FD_H
        zm[b, t, i] -= FD_H
        probes.append((float(g[b, t, i]), float(merit(zp)[b] - merit(zm)[b]) / (2 * FD_H)))
    scale = max(abs(a) for a, _ in probes)
    err = max(abs(a - fd) for a, fd in probes) / scale
    print(f"({nx},{nu}): g_out vs central differences of merit_xbox: {err:.2e} (relative to the largest probed {scale:.3g})")
    assert err < FD_TOL, (err, probes)


# ---- 4. single kernels against a direct statement of the row terms -----------------------------------------------------
@pytest.mark.parametrize("nx,nu,T,B,ps", [(2, 1, 4, 3, False), (13, 4, 3, 2, True)])
def test_dual_update_and_pick_equal_the_row_terms(nx, nu, T, B, ps):
    pr, plant = ssr.step_problem(B, T, nx, nu, F64, per_stage=ps)
    inp = ssr.kernel_inputs(pr, plant)
    z, lam, rho = inp["z"].clone(), inp["lam"], inp["rho"]
    xhi = pr["xhi"] if ps else pr["xhi"].reshape(1, 1, nx).expand(B, T, nx)
    z[0, T - 1, 0] = xhi[0, T - 1, 0]   # one state exactly on its bound
    ru, rl = sbr.xbox_residuals(pr, z)
    assert (ru > 0).any() and (rl > 0).any() and (ru < 0).any() and (rl < 0).any() and (ru == 0).any()
    be = ssr.XboxStepOracleBackend()
    sb_u, st_u, sb_x, st_x = ssr.strides(pr)
    xb = (pr["xlo"], pr["xhi"], sb_x, st_x)
    xn = ssr.true_next(plant, z, nx)
    want = ssr.row_terms_numpy(pr, z, xn, lam, rho)
    phi0, A, _, A2 = ssr.merit_magnitude_xbox(pr, z, xn, lam, rho)
    # dual update: three roundings per row (aux_cases.gamma_dual_rows), the oracle's and the statement's each
    l2, r2 = lam.clone(), rho.clone()
    be.dual_update_xbox(pr["dims"], z, xn, pr["x0"], pr["lo"], pr["hi"], sb_u, st_u, xb, l2, r2)
    mag = np.abs(lam.numpy()) + rho.numpy()[:, None] * (np.abs(z.numpy()).max() + 2.0)
    e = np.abs(l2.numpy() - want["lam_new"])
    assert (e <= 2 * 3 * EPS64 * mag).all(), (e / (EPS64 * mag)).max()
    assert torch.equal(r2, rho * 10.0)
    _, lxu, lxl = sbr.split_lam(l2.numpy(), T, nx, nu)
    assert lxu[0, T - 1, 0] == lam.numpy()[0, T * nx + (T - 1) * (2 * nu + 2 * nx) + 2 * nu]   # on the bound: r = 0, lam stays
    assert (lxu > 0).any() and (lxl > 0).any() and (lxu == 0).any()
    # line search, all 20 candidates and fewer
    gam = ax.gamma_merit(T, nx, nu, 0, cand=True) + T * (nx + nu)   # + the oracle's sequential sums
    for n_ls in (20, 7):
        zz, ph = z.clone(), torch.tensor(phi0).clone()
        phis, kk, acc = torch.empty(n_ls, B, dtype=F64), torch.zeros(B, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)
        rn2 = torch.full((B,), -1.0, dtype=F64)
        al = (2.0 ** -torch.arange(n_ls, dtype=F64)).view(n_ls, 1, 1, 1)
        zc = (z.unsqueeze(0) + al * inp["d"].unsqueeze(0)).contiguous()
        xn_all = ssr.true_next(plant, zc, nx)
        be.merit_pick_xbox(pr["dims"], n_ls, inp["d"], xn_all, pr["x0"], lam, rho, pr["Qd"], pr["q"], pr["lo"], pr["hi"],
                           sb_u, st_u, xb, zz, ph, rnorm2=rn2, phi_all=phis, k_out=kk, accept_out=acc)
        ref = np.stack([ssr.row_terms_numpy(pr, zc[k], xn_all[k], lam, rho)["phi"] for k in range(n_ls)])
        rp2 = np.stack([ssr.row_terms_numpy(pr, zc[k], xn_all[k], lam, rho)["rp2"] for k in range(n_ls)])
        Ak = np.stack([ssr.merit_magnitude_xbox(pr, zc[k], xn_all[k], lam, rho)[1] for k in range(n_ls)])
        assert (np.abs(phis.numpy() - ref) <= 2 * gam * EPS64 * Ak).all()
        for b in range(B):
            k = int(np.argmin(ref[:, b]))
            srt = np.sort(ref[:, b])
            if srt[1] - srt[0] > 4 * gam * EPS64 * Ak[:, b].max():
                assert int(kk[b]) == k
            ok = ref[int(kk[b]), b] < phi0[b]
            assert bool(acc[b]) == ok
            want_z = z[b] + (2.0 ** -int(kk[b])) * inp["d"][b] if ok else z[b]
            assert torch.equal(zz[b], want_z)
            assert abs(float(rn2[b]) - (rp2[int(kk[b]), b] if ok else -1.0)) <= 2 * gam * EPS64 * A2[b] + 1e-300
        assert acc.any()


# ---- 5. gradients through MPC against central differences --------------------------------------------------------------
# The plant here is an AFFINE model given as a callable (AffineCallable): the backward pass is the reference's, w = -H^{-1} gbar
# with the Gauss-Newton H of the last step, which leaves out the dynamics' second derivative, so on a curved plant it differs
# from the derivative of the stage by a term of the size of multiplier x curvature and no difference quotient can confirm it
# to 1e-8. On an affine model it is exact at a stationary point. The stage is then tests/test_state_bounds_cpu.py's, run
# through the four _xbox methods, and so are the seeds: (seed, width) per size, of seeds 3..9 at widths 0.6 and 0.4 the first
# at which the reference's stage alone is stationary after its 4 Newton steps (max |g| < 1e-10), has an upper and a lower
# state row active and no row within 1e-3 of switching - all three asserted below, on this reference.
GRAD_SEEDS = [(2, 1, 4, 0.4), (4, 2, 7, 0.6), (13, 4, 9, 0.6)]


def _stage(nx, nu, seed, width, B=4, T=5):
    pr = sbr.xbox_problem(B, T, nx, nu, F64, per_stage=True, seed=seed, width=width)
    plant = ssr.AffineCallable(pr["F"], pr["c"])
    be = ssr.XboxStepOracleBackend()
    z, lam, rho = pr["z0"].clone(), torch.zeros(B, sbr.lam_width(T, nx, nu), dtype=F64), torch.ones(B, dtype=F64)
    for _ in range(2):
        ssr.al_iteration(be, pr, plant, z, lam, rho)
    warm = dict(z=z, lam=lam, rho=rho)

    def stage(**over):
        zf = warm["z"].clone()
        ssr.al_iteration(be, {**pr, **over}, plant, zf, warm["lam"].clone(), warm["rho"].clone(), dual=False)
        return zf
    return pr, plant, warm, stage


def _grad_case(nx, nu, seed, width):
    pr, plant, warm, stage = _stage(nx, nu, seed, width)
    B, T = pr["dims"][:2]
    zf = stage()
    be = ssr.XboxStepOracleBackend()
    sb_u, st_u, sb_x, st_x = ssr.strides(pr)
    xn, F = ssr.linearize(plant, zf, nx)
    d, g = torch.empty_like(zf), torch.empty_like(zf)
    be.newton_step_xbox(pr["dims"], zf, xn, F, pr["x0"], warm["lam"], warm["rho"], pr["Qd"], pr["q"], pr["lo"], pr["hi"],
                        sb_u, st_u, (pr["xlo"], pr["xhi"], sb_x, st_x), d, g_out=g)
    gmax = g.abs().reshape(B, -1).max(1).values
    ru, rl = sbr.xbox_residuals(pr, zf)
    margin = min(np.abs(ru).min(), np.abs(rl).min())
    return pr, plant, warm, stage, zf, gmax, int((ru >= 0).sum()), int((rl >= 0).sum()), margin


@pytest.mark.parametrize("nx,nu,seed,width", GRAD_SEEDS)
def test_gradients_through_mpc_vs_finite_differences(nx, nu, seed, width):
    from deq_mpc_corl_amd import QuadCost
    pr, plant, warm, stage, zf, gmax, n_up, n_lo, margin = _grad_case(nx, nu, seed, width)
    B, T = pr["dims"][:2]
    print(f"({nx},{nu}): max |g(z_final)| per instance {gmax.numpy()}; state rows active {n_up} upper, {n_lo} lower; "
          f"nearest row to switching {margin:.2e}")
    assert (gmax < 1e-10).all() and n_up >= 1 and n_lo >= 1 and margin > 1e-3
    be = ssr.XboxStepOracleBackend()
    mpc = _mpc(pr["dims"], pr["lo"], pr["hi"], be, "fixed", al_iter=1, x_lower=pr["xlo"], x_upper=pr["xhi"])
    mpc.reinitialize(pr["x0"], None)
    leaf = {k: pr[k].clone().requires_grad_(True) for k in ("Qd", "q")}
    x, u, _ = mpc.al_solve(warm["z"][..., :nx].clone(), warm["z"][..., nx:].clone(), plant, plant.jac, pr["x0"],
                           QuadCost(leaf["Qd"], leaf["q"]), lamda_init=warm["lam"].clone(), rho_init=warm["rho"].clone())
    assert "newton_step_xbox" in be.calls and "solve_lin_xbox" not in be.calls
    gbar = torch.randn(B, T, nx + nu, generator=torch.Generator().manual_seed(1), dtype=F64).float().double()
    ((x.double() * gbar[..., :nx]).sum() + (u.double() * gbar[..., nx:]).sum()).backward()
    assert torch.equal(torch.cat((x, u), -1).detach(), zf.float())   # the MPC ran the stage the differences go through
    rng = np.random.default_rng(2)
    probes = []
    for name in ("Qd", "q"):
        for _ in range(4):
            idx = tuple(int(rng.integers(0, s)) for s in pr[name].shape)
            vals = []
            for sgn in (1.0, -1.0):
                a = pr[name].clone()
                a[idx] += sgn * FD_H
                vals.append(float((gbar * stage(**{name: a})).sum()))
            probes.append((name, float(leaf[name].grad[idx]), (vals[0] - vals[1]) / (2 * FD_H)))
    scale = max(abs(a) for _, a, _ in probes)
    for name in ("Qd", "q"):
        e = max(abs(a - fd) for nm, a, fd in probes if nm == name) / scale
        print(f"({nx},{nu}): d{name} vs central differences: {e:.2e} (relative to the largest probed gradient {scale:.3g})")
    err = max(abs(a - fd) for _, a, fd in probes) / scale
    assert err < FD_TOL, (err, probes)


# ---- 6. host ------------------------------------------------------------------------------------------------------------
class _XboxRecordingBackend(RecordingBackend):
    """RecordingBackend with the four _xbox methods (records as its plain ones, the name aside)."""

    def newton_step_xbox(self, dims, z, xnext, F, x0, lam, rho, Qd, q, ulo, uhi, sb_u, st_u, xbnd, d_out, g_out=None,
                         factor=None, info=None, **kw):
        assert not kw, kw   # no workspace, no obs
        self._note_factor(factor)
        self._lins.append(F)
        self.calls.append(["newton_step_xbox", factor is not None, info is not None, tuple(xbnd[2:])])
        d_out.zero_()

    def merit_xbox(self, dims, K, zc, xnext, x0, lam, rho, Qd, q, ulo, uhi, sb_u, st_u, xbnd, phi, rnorm2=None):
        self.calls.append(["merit_xbox", K])
        self._residual(rnorm2)

    def merit_pick_xbox(self, dims, n_ls, d, xnext_all, x0, lam, rho, Qd, q, ulo, uhi, sb_u, st_u, xbnd, z, phi_prev,
                        rnorm2=None, phi_all=None, k_out=None, accept_out=None):
        self.calls.append(["merit_pick_xbox", n_ls])

    def dual_update_xbox(self, dims, z, xnext, x0, ulo, uhi, sb_u, st_u, xbnd, lam, rho, rho_scale=10.0):
        self.calls.append(["dual_update_xbox"])
        rho.mul_(rho_scale)

    def _workspace(self, dims, like):
        self.calls.append(["_workspace"])
        return super()._workspace(dims, like)

    def new_workspace(self, dims, like):
        self.calls.append(["new_workspace"])
        return super().new_workspace(dims, like)


def _tiny(B=5):
    nx, nu, T = 2, 1, 2
    pr = sbr.xbox_problem(B, T, nx, nu, F64)
    return pr, ssr.SinPlant(nx, nu)


@pytest.mark.parametrize("grad", [False, True])
def test_no_quad_workspace_and_no_fused_model_with_bounds(grad):
    """B = 5 >= QUAD_MIN_BATCH = 4 of the recording backend: the plain callable route takes the quad step there; with
    state bounds the team step runs, with the packed factor when a backward pass follows."""
    from deq_mpc_corl_amd.dynamics import Pendulum1lDynamics
    from deq_mpc_corl_amd.qpth.AL_mpc import _SolveState
    pr, plant = _tiny()
    traces = {}
    for xb in (False, True):
        be = _XboxRecordingBackend()
        kw = dict(x_lower=-0.5, x_upper=0.5) if xb else {}
        mpc = _mpc(pr["dims"], pr["lo"], pr["hi"], be, "fixed", al_iter=1, **kw)
        Qd = pr["Qd"].clone().requires_grad_(grad)
        x, u, _ = _call(mpc, pr, plant, plant.jac, Qd=Qd)
        if grad:
            (x.sum() + u.sum()).backward()
        traces[xb] = be.calls
        st = _SolveState()
        st.lin, st.stream_mode, st.dx = None, False, Pendulum1lDynamics()   # a provider with a compiled-in model
        assert mpc._fused_model(st) is (not xb)
    names = [c[0] for c in traces[True]]
    assert "_workspace" not in names and "new_workspace" not in names and "backward_ws" not in names
    assert names[:-1 if grad else None] == ["merit_xbox"] + ["newton_step_xbox", "merit_pick_xbox"] * 4 + ["merit_xbox", "dual_update_xbox"]
    assert all(c == ["newton_step_xbox", grad, True, (0, 0)] for c in traces[True] if c[0] == "newton_step_xbox")
    if grad:
        assert traces[True][-1] == ["backward", "factor0", "last_linearisation"]
    # the plain route's trace is what it is without this feature: quad steps on a workspace
    plain = [c for c in traces[False] if c[0] == "newton_step"]
    assert len(plain) == 4 and all(c[1] == ("private0" if grad else "cached") for c in plain)
    assert not any(c[0].endswith("_xbox") for c in traces[False])


def test_plain_launch_trace_is_unchanged_without_bounds():
    """The recording backend WITH the _xbox methods against the one without: identical records on the callable route."""
    pr, plant = _tiny()
    got = []
    for cls in (RecordingBackend, _XboxRecordingBackend):
        be = cls()
        mpc = _mpc(pr["dims"], pr["lo"], pr["hi"], be, "reference", al_iter=2)
        _call(mpc, pr, plant, plant.jac)
        got.append([c for c in be.calls if c[0] not in ("_workspace", "new_workspace")])
    assert got[0] == got[1] and got[0]


def test_guards_are_kept():
    from deq_mpc_corl_amd import MPC, PendulumDynamics, QuadCost
    from deq_mpc_corl_amd.qpth.AL_mpc_custom import Obstacle_MPC
    nx, nu, B, T = 2, 1, 3, 4
    pr = sbr.xbox_problem(B, T, nx, nu, F64)
    dyn = PendulumDynamics()
    # a backend without newton_step_xbox: today's error, today's message
    kw = dict(u_lower=pr["lo"], u_upper=pr["hi"], n_batch=B, dtype=F64, x_lower=-1.0, x_upper=1.0)
    mpc = MPC(nx, nu, T, backend=sbr.XboxOracleBackend(), **kw)
    with pytest.raises(NotImplementedError, match=r"need affine dynamics given as LinDx\(F, f\): the nonlinear-caller kernels "
                                                  "and the compiled-in models know no state-bound rows"):
        _call(mpc, pr, dyn, dyn.jac)
    kw["backend"] = ssr.XboxStepOracleBackend()
    with pytest.raises(NotImplementedError, match="state_estimator"):
        MPC(nx, nu, T, state_estimator=True, **kw)
    with pytest.raises(NotImplementedError, match="Obstacle_MPC"):
        Obstacle_MPC(3, nu, T, **kw)
    mpc = MPC(nx, nu, T, **kw)
    mpc.reinitialize(pr["x0"], None)
    mpc.linearize_once = True
    xi, ui = pr["z0"][..., :nx].clone(), pr["z0"][..., nx:].clone()
    with pytest.raises(NotImplementedError, match="linearize_once"):
        mpc.al_solve_stream(xi, ui, dyn, dyn.jac, pr["x0"], QuadCost(pr["Qd"], pr["q"]))
    # diag_cost=False and ineqG stay LinDx-only: refused in the constructor on a backend without solve_lin_gen, in the
    # solve's guard block on one that has it
    with pytest.raises(NotImplementedError, match="diag_cost"):
        MPC(nx, nu, T, diag_cost=False, **kw)
    rows = dict(ineqG=torch.ones(1, nx + nu, dtype=F64), ineqh=torch.ones(1, dtype=F64))
    with pytest.raises(NotImplementedError, match="ineqG"):
        MPC(nx, nu, T, **rows, **kw)

    class _WithGen(ssr.XboxStepOracleBackend):
        def solve_lin_gen(self, *a, **k):
            raise AssertionError("not reached: the guards come first")
    kw["backend"] = _WithGen()
    mpc = MPC(nx, nu, T, diag_cost=False, **kw)
    mpc.reinitialize(pr["x0"], None)
    with pytest.raises(NotImplementedError, match="diag_cost=False needs affine dynamics given as LinDx"):
        mpc(pr["x0"], QuadCost(torch.diag_embed(pr["Qd"]), pr["q"]), dyn, dyn.jac, x_init=xi, u_init=ui)
    mpc = MPC(nx, nu, T, **rows, **kw)
    with pytest.raises(NotImplementedError, match="ineqG / ineqh need affine dynamics given as LinDx"):
        _call(mpc, pr, dyn, dyn.jac)
    # a lamda of the plain width handed to a state-bounded solve
    mpc = MPC(nx, nu, T, **kw)
    mpc.reinitialize(pr["x0"], None)
    with pytest.raises(ValueError, match="lamda"):
        mpc.al_solve(xi, ui, dyn, dyn.jac, pr["x0"], QuadCost(pr["Qd"], pr["q"]),
                     lamda_init=torch.zeros(B, T * nx + 2 * T * nu, dtype=F64))


@pytest.mark.parametrize("mode", ["reference", "fixed"])
@pytest.mark.parametrize("nx,nu", [(2, 1), (13, 4)])
def test_callable_dx_with_state_bounds_runs_and_ends_inside_the_bounds(nx, nu, mode):
    """The case that raises NotImplementedError without the feature. The cost pulls state 0 above and state 1 below the
    box |x| <= 0.4 on every stage (without the bounds the solution leaves it by more than half its width), x0 lies inside,
    and the controls (|u| <= 2) can hold the plant there: every state ends inside its bounds to the residual reported."""
    B, T, w = 3, 5, 0.4
    pr, plant = ssr.bounded_plant_problem(B, T, nx, nu, F64, width=w)
    be = ssr.XboxStepOracleBackend()
    mpc = _mpc(pr["dims"], pr["lo"], pr["hi"], be, mode, al_iter=6, x_lower=pr["xlo"], x_upper=pr["xhi"])
    free = _mpc(pr["dims"], pr["lo"], pr["hi"], OracleBackend(), mode, al_iter=6)
    x, u, _ = _call(mpc, pr, plant, plant.jac)
    xf, _, _ = _call(free, pr, plant, plant.jac)
    assert set(be.calls) == {"newton_step_xbox", "merit_xbox", "merit_pick_xbox", "dual_update_xbox"}
    assert mpc.lamda_prev.shape == (B, sbr.lam_width(T, nx, nu))
    res = mpc.dyn_res_prev   # ||r+||_2 per instance, state rows included
    viol = (x.double().abs() - w).clamp(min=0).reshape(B, -1).max(1).values
    out_free = float((xf.abs() - w).max())
    print(f"({nx},{nu}) {mode}: ||r+|| {res.numpy()}, largest state violation {viol.numpy()}, without bounds {out_free:.3f} outside; "
          f"Newton steps {mpc.last_newton_per_al}")
    assert out_free > 0.5 * w                   # the bounds matter: the free solution leaves the box
    assert (viol <= res + 1e-6).all()           # (x comes back as float32)
    assert (res < 0.05).all() and (viol < 0.02).all()
    _, lxu, lxl = sbr.split_lam(mpc.lamda_prev.numpy(), T, nx, nu)
    assert (lxu > 0).any() or (lxl > 0).any()


def test_sharded_norm_counts_the_state_rows():
    """rn2 of the _xbox merit holds the state rows, so the batch-global exit of a sharded batch sees them: the norm the
    host reduces equals the direct statement's."""
    pr, plant = ssr.step_problem(3, 4, 2, 1, F64)
    be = ssr.XboxStepOracleBackend()
    B, T, nx, nu = pr["dims"]
    sb_u, st_u, sb_x, st_x = ssr.strides(pr)
    lam, rho = torch.zeros(B, sbr.lam_width(T, nx, nu), dtype=F64), torch.ones(B, dtype=F64)
    phi, rn2 = torch.zeros(B, dtype=F64), torch.zeros(B, dtype=F64)
    xn = ssr.true_next(plant, pr["z0"], nx)
    be.merit_xbox(pr["dims"], 1, pr["z0"], xn, pr["x0"], lam, rho, pr["Qd"], pr["q"], pr["lo"], pr["hi"], sb_u, st_u,
                  (pr["xlo"], pr["xhi"], sb_x, st_x), phi, rn2)
    want = ssr.row_terms_numpy(pr, pr["z0"], xn, lam, rho)["rp2"]
    plain = torch.zeros(B, dtype=F64)
    OracleBackend().merit(pr["dims"], 1, pr["z0"], xn, pr["x0"], lam[:, :T * nx + 2 * T * nu].contiguous(), rho, pr["Qd"],
                          pr["q"], pr["lo"], pr["hi"], sb_u, st_u, phi.clone(), plain)
    assert np.allclose(rn2.numpy(), want, rtol=1e-13) and (rn2 > plain + 0.1).all()


# ---- 7. the GPU tests' inputs, on the reference alone -------------------------------------------------------------------
@pytest.mark.parametrize("nx,nu,T,B,ps", ssr.GPU_CASES, ids=lambda v: str(v))
def test_gpu_case_inputs(nx, nu, T, B, ps):
    """After one reference AL iteration every instance has an upper and a lower state row active and nonzero state-row
    multipliers; and at most a quarter of the instances have their two best line-search merits closer than the fp32
    merit tolerance (the GPU test excuses the pick's k there)."""
    pr, plant, inp = ssr.gpu_case(nx, nu, T, B, ps, F64)
    up, lo, nz = ssr.state_rows_active(pr, inp["z"], inp["lam"])
    assert up.all() and lo.all() and nz.all()
    assert not np.isnan(inp["d"].numpy()).any() and (inp["rho"] == 10.0).all()
    be = ssr.XboxStepOracleBackend()
    sb_u, st_u, sb_x, st_x = ssr.strides(pr)
    al = (2.0 ** -torch.arange(20, dtype=F64)).view(20, 1, 1, 1)
    zc = (inp["z"].unsqueeze(0) + al * inp["d"].unsqueeze(0)).contiguous()
    xn_all = ssr.true_next(plant, zc, nx)
    phis = torch.empty(20, B, dtype=F64)
    be.merit_xbox(pr["dims"], 20, zc, xn_all, pr["x0"], inp["lam"], inp["rho"], pr["Qd"], pr["q"], pr["lo"], pr["hi"], sb_u,
                  st_u, (pr["xlo"], pr["xhi"], sb_x, st_x), phis)
    zmag = inp["z"].abs().numpy()[None] + al.numpy() * inp["d"].abs().numpy()[None]
    A = np.stack([ssr.merit_magnitude_xbox(pr, zc[k], xn_all[k], inp["lam"], inp["rho"], zmag=zmag[k])[1] for k in range(20)])
    tol32 = ax.gamma_merit(T, nx, nu, 0, cand=True) * ax.EPS[torch.float32] * A
    srt = np.sort(phis.numpy(), 0)
    close = (srt[1] - srt[0]) <= 2 * tol32.max(0)
    print(f"({nx},{nu},{T},{B}): instances with a near-tie of the two best merits at fp32 tolerance: {int(close.sum())} of {B}")
    assert close.sum() <= B // 4
