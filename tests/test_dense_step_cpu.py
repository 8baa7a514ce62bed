"""Dense stage cost on the callable-dynamics route (MPC(diag_cost=False) with a callable dx, alone or with x_lower /
x_upper and / or ineqG / ineqh), without a GPU: the host wiring on the composed reference backend of
tests/dense_step_reference.py, and that backend pinned: the case that does not run without the feature (1), a diagonal C
reproduces the diagonal routes bit for bit (2), an affine model given as a callable is the LinDx routes' twin (3), a
diagonal problem in rotated state coordinates on the rotated plant (4), g is the gradient of the merit and the line search
equals a direct statement (5), gradients through MPC against central differences (6), the host routing (7), and the GPU
tests' inputs (8)."""
import numpy as np
import pytest
import torch

from tests import aux_cases as ax
from tests import dense_step_reference as dsr
from tests import gen_rows_reference as grr
from tests import poly_rows_reference as prr
from tests import rows_step_reference as rsr
from tests import state_bounds_reference as sbr
from tests import state_bounds_step_reference as ssr
from tests.dense_cost_reference import DenseOracleBackend
from tests.oracle_backend import OracleBackend
from tests.recording_backend import RecordingBackend
from tests.test_dyn_grad_cpu import FD_H, FD_TOL

F64 = torch.float64
EPS64 = 2.0 ** -53
INF = float("inf")
COMBOS, COMBO_IDS = dsr.COMBOS, dsr.COMBO_IDS
OLD_MSG = (r"diag_cost=False needs affine dynamics given as LinDx\(F, f\): the nonlinear-caller kernels and the compiled-in "
           "models read diag")


def _mpc(dims, lo, hi, be, exit_mode="reference", al_iter=2, **kw):
    from deq_mpc_corl_amd import MPC
    B, T, nx, nu = dims
    return MPC(nx, nu, T, u_lower=lo, u_upper=hi, n_batch=B, dtype=F64, exit_mode=exit_mode, al_iter=al_iter, backend=be, **kw)


def _call(mpc, pr, dx, dx_jac, C=None, q=None):
    """One solve from the problem's start; C None: the problem's own dense C."""
    from deq_mpc_corl_amd import QuadCost
    nx = pr["dims"][2]
    mpc.reinitialize(pr["x0"], None)
    cost = QuadCost(pr["C"] if C is None else C, pr["q"] if q is None else q)
    return mpc(pr["x0"], cost, dx, dx_jac, x_init=pr["z0"][..., :nx].clone(), u_init=pr["z0"][..., nx:].clone())


# ---- 1. the case that raises NotImplementedError without the feature -----------------------------------------------------
@pytest.mark.parametrize("xbox,poly", COMBOS, ids=COMBO_IDS)
@pytest.mark.parametrize("mode", ["reference", "fixed"])
@pytest.mark.parametrize("nx,nu", [(2, 1), (13, 4)])
def test_callable_dx_with_a_dense_cost_runs_and_ends_inside_its_constraints(nx, nu, mode, xbox, poly):
    """MPC(diag_cost=False) on the sin plant: alone, with |x| <= 0.8, with the coupled row x_0 + x_1 <= h on every stage,
    and with both. The solve ends with every constraint satisfied to the residual it reports, and with the row (or,
    without it, the state box) active: a nonzero multiplier. (Next to the row the box may stay slack: the row is the
    tighter of the two on states 0 and 1.)"""
    B, T = 3, 5
    pr, plant = dsr.dense_whole_problem(B, T, nx, nu, xbox, poly, mode)
    off = pr["C"] - torch.diag_embed(pr["C"].diagonal(dim1=-2, dim2=-1))
    assert off.abs().max() > 0.1   # a dense problem indeed
    be = dsr.DenseStepOracleBackend()
    mpc = _mpc(pr["dims"], pr["lo"], pr["hi"], be, mode, al_iter=6, diag_cost=False, **dsr.mpc_kwargs(pr, xbox, poly))
    x, u, _ = _call(mpc, pr, plant, plant.jac)
    assert set(be.calls) == dsr.dense_methods(xbox, poly)
    assert mpc.lamda_prev.shape == (B, grr.lam_width(T, nx, nu, xbox, 1 if poly else 0))
    res = mpc.dyn_res_prev   # ||r+||_2 per instance, every row in use included
    viol = (u.double() - pr["hi"]).clamp(min=0).reshape(B, -1).max(1).values
    viol = torch.maximum(viol, (pr["lo"] - u.double()).clamp(min=0).reshape(B, -1).max(1).values)
    if poly:
        viol = torch.maximum(viol, ((x[..., 0] + x[..., 1]).double() - pr["h"][..., 0]).clamp(min=0).max(1).values)
    if xbox:
        viol = torch.maximum(viol, (x.double().abs() - 0.8).clamp(min=0).reshape(B, -1).max(1).values)
    print(f"DENSESTEP runs ({nx},{nu}) {mode} xbox={xbox} rows={poly}: ||r+|| {res.numpy()}, largest violation {viol.numpy()}; "
          f"Newton steps {mpc.last_newton_per_al}")
    assert (viol <= res + 1e-6).all()           # (x comes back as float32)
    assert (res < 0.05).all() and (viol < 0.02).all()
    _, lxu, lxl, lp = grr.split_lam(mpc.lamda_prev.numpy(), T, nx, nu, xbox, 1 if poly else 0)
    assert not poly or (lp > 0).any()
    assert poly or not xbox or (lxu > 0).any() or (lxl > 0).any()


# ---- 2. a diagonal C through the new route is the diagonal route ------------------------------------------------------------
def _recording(cls):
    class _Rec(cls):
        """Records the line-search index and the accept flag of every step (every pick goes through linesearch_pick)."""

        def __init__(self):
            super().__init__()
            self.picks = []

        def linesearch_pick(self, dims, n_ls, phi, phi_prev, d, z, k_out=None, accept_out=None):
            super().linesearch_pick(dims, n_ls, phi, phi_prev, d, z, k_out, accept_out)
            self.picks.append((k_out.clone(), accept_out.clone()))
    return _Rec()


@pytest.mark.parametrize("xbox,poly", COMBOS, ids=COMBO_IDS)
@pytest.mark.parametrize("mode", ["reference", "fixed"])
@pytest.mark.parametrize("nx,nu", [(2, 1), (13, 4)])
def test_diagonal_c_reproduces_the_diagonal_callable_route(nx, nu, mode, xbox, poly):
    """C = diag_embed(Qd) through the _dense methods against the plain / _xbox / _rows callable route with Qd: Newton
    counts, line-search indices, x, u and lam equal (the off-diagonal part adds exact zeros)."""
    B, T = 3, 5
    pr, plant, _ = rsr.coupled_row_problem(B, T, nx, nu, xbox, mode)
    out = {}
    for dense in (False, True):
        be = _recording(dsr.DenseStepOracleBackend)
        mpc = _mpc(pr["dims"], pr["lo"], pr["hi"], be, mode, al_iter=3, diag_cost=not dense, **dsr.mpc_kwargs(pr, xbox, poly))
        x, u, _ = _call(mpc, pr, plant, plant.jac, C=torch.diag_embed(pr["Qd"]))
        assert ("newton_step_dense" in be.calls) == dense
        out[dense] = (x, u, mpc.lamda_prev.clone(), list(mpc.last_newton_per_al), be.picks)
    a, b = out[False], out[True]
    assert a[3] == b[3]
    assert len(a[4]) == len(b[4]) == sum(a[3])
    assert all(torch.equal(p[0], r[0]) and torch.equal(p[1], r[1]) for p, r in zip(a[4], b[4]))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


# ---- 3. route twin: an affine model as a callable against LinDx through solve_lin_dense / solve_lin_gen -------------------
def _twin(nx, nu, mode, xbox, poly, inert, B=3, T=5, m=3):
    from deq_mpc_corl_amd.qpth.al_utils import LinDx
    pr = grr.gen_problem(B, T, nx, nu, m, F64, "per_instance", box="per_stage")
    C = pr["C"]
    kw = {}
    if inert:   # what is left is the two routes' orders of summation
        C = torch.diag_embed(C.diagonal(dim1=-2, dim2=-1))
    if xbox:
        kw.update(x_lower=torch.full_like(pr["xlo"], -INF) if inert else pr["xlo"],
                  x_upper=torch.full_like(pr["xhi"], INF) if inert else pr["xhi"])
    if poly:
        kw.update(ineqG=pr["G"], ineqh=torch.full_like(pr["h"], INF) if inert else pr["h"])
    lin_entry = "solve_lin_gen" if xbox or poly else "solve_lin_dense"
    res = []
    for route in ("lin", "callable"):
        be = dsr.DenseStepOracleBackend() if route == "callable" else grr.GenOracleBackend() if xbox or poly else DenseOracleBackend()
        mpc = _mpc(pr["dims"], pr["lo"], pr["hi"], be, mode, al_iter=3, diag_cost=False, **kw)
        if route == "lin":
            _call(mpc, pr, LinDx(pr["F"], pr["c"]), None, C=C, q=pr["qC"])
            assert set(be.calls) == {lin_entry}
        else:
            dyn = ssr.AffineCallable(pr["F"], pr["c"])
            _call(mpc, pr, dyn, dyn.jac, C=C, q=pr["qC"])
            assert set(be.calls) == dsr.dense_methods(xbox, poly)
        res.append((mpc.x_init.double(), mpc.u_init.double(), mpc.lamda_prev.clone(), list(mpc.last_newton_per_al)))
    return pr, res


@pytest.mark.parametrize("xbox,poly", COMBOS, ids=COMBO_IDS)
@pytest.mark.parametrize("mode", ["reference", "fixed"])
@pytest.mark.parametrize("nx,nu", [(2, 1), (4, 2), (13, 4)])
def test_route_twin(nx, nu, mode, xbox, poly):
    """Both routes take the same steps on the same numbers; they order their sums differently (x_next is formed by the
    caller here, inside the reference's solve there). The same twin on the inert problem (the off-diagonal part of C
    dropped, every state bound and row out of reach) measures that difference; the bound on the real problem is the
    larger of 8 times it and 64 eps of the largest entry."""
    figs = {}
    for inert in (True, False):
        pr, (a, b) = _twin(nx, nu, mode, xbox, poly, inert)
        assert a[3] == b[3], (a[3], b[3])
        figs[inert] = (max(float((a[0] - b[0]).abs().max()), float((a[1] - b[1]).abs().max())),
                       float((a[2] - b[2]).abs().max()),
                       max(float(a[0].abs().max()), float(a[1].abs().max())), float(a[2].abs().max()))
        _, lxu, lxl, lp = grr.split_lam(a[2].numpy(), pr["dims"][1], nx, nu, xbox, pr["m"] if poly else 0)
        if inert:
            assert (not poly or not lp.any()) and (not xbox or not (lxu.any() or lxl.any()))
        else:
            assert (not poly or (lp > 0).any()) and (not xbox or (lxu > 0).any() or (lxl > 0).any())   # active at the solution
    dz0, dl0, _, _ = figs[True]
    dz, dl, zmax, lmax = figs[False]
    print(f"DENSESTEP twin ({nx},{nu}) {mode} xbox={xbox} rows={poly}: inert twin |dz| {dz0:.2e} |dlam| {dl0:.2e}; real twin "
          f"|dz| {dz:.2e} |dlam| {dl:.2e} (largest z {zmax:.3g}, lam {lmax:.3g})")
    assert dz <= max(8 * dz0, 64 * EPS64 * zmax), (dz, dz0)
    assert dl <= max(8 * dl0, 64 * EPS64 * lmax), (dl, dl0)
    # the table the GPU whole solves take their twin bound from holds what is measured here (reference exit), to a factor 2
    if mode == "reference" and (nx, nu, xbox, poly) in dsr.INERT_TWIN:
        want = dsr.INERT_TWIN[(nx, nu, xbox, poly)]
        assert 0.5 * want <= dl0 <= 2 * want, (dl0, want)


def test_inert_twin_table_covers_the_gpu_whole_solves():
    assert set(dsr.INERT_TWIN) == {(nx, nu, xb, pl) for nx, nu in dsr.WHOLE_SOLVE_KW for xb, pl in COMBOS}


# ---- 4. rotated states on the rotated plant -------------------------------------------------------------------------------
class _RotatedPlant:
    """f_rot(x, u) = P f(P' x, u) for a plant f and one orthogonal P [nx,nx]: the same plant in rotated state coordinates."""

    def __init__(self, plant, P):
        self.plant, self.P = plant, P

    def __call__(self, x, u):
        P = self.P.to(x.dtype)
        return self.plant(x @ P, u) @ P.T

    def jac(self, x, u):
        P = self.P.to(x.dtype)
        xn, (A, Bm) = self.plant.jac(x @ P, u)
        return xn @ P.T, (P @ A @ P.T, P @ Bm)


@pytest.mark.parametrize("mode", ["reference", "fixed"])
@pytest.mark.parametrize("nx,nu", [(2, 1), (4, 2), (13, 4)])
def test_rotated_states_match_the_diagonal_callable_route(nx, nu, mode):
    """A diagonal problem on the sin plant through the plain callable route (the oracle, pinned to the reference) against
    the same problem in rotated state coordinates z = blockdiag(P, I) z~, a dense problem on the rotated plant, through
    the _dense methods: the AL iteration is equivariant under the rotation (tests/test_dense_cost_cpu.py's pin)."""
    B, T = 3, 5
    n = nx + nu
    pr, plant = ssr.bounded_plant_problem(B, T, nx, nu, F64)
    gen = torch.Generator().manual_seed(111)
    D = torch.cat((1.0 + 19.0 * torch.rand(B, T, nx, generator=gen, dtype=F64),   # distinct: else P D P' stays diagonal
                   torch.full((B, T, nu), 0.1, dtype=F64)), -1)
    xref = torch.where(pr["Qd"] > 1e-6, -pr["q"] / pr["Qd"].clamp(min=1e-6), torch.zeros_like(pr["q"]))
    qt = -D * xref
    P, _ = torch.linalg.qr(torch.randn(nx, nx, generator=gen, dtype=F64))
    Pn = torch.zeros(n, n, dtype=F64)
    Pn[:nx, :nx] = P
    Pn[nx:, nx:] = torch.eye(nu, dtype=F64)
    C = torch.einsum("ij,btj,kj->btik", Pn, D, Pn)
    C = 0.5 * (C + C.transpose(-1, -2))
    off = C - torch.diag_embed(C.diagonal(dim1=-2, dim2=-1))
    assert off.abs().max() > 1.0   # a dense problem indeed
    m0 = _mpc(pr["dims"], pr["lo"], pr["hi"], OracleBackend(), mode, al_iter=3)
    x0_, u0_, _ = _call(m0, pr, plant, plant.jac, C=torch.diag_embed(D), q=qt)
    rot = dict(pr, x0=pr["x0"] @ P.T, z0=pr["z0"] @ Pn.T)
    be = dsr.DenseStepOracleBackend()
    m1 = _mpc(pr["dims"], pr["lo"], pr["hi"], be, mode, al_iter=3, diag_cost=False)
    rp = _RotatedPlant(plant, P)
    x1, u1, _ = _call(m1, rot, rp, rp.jac, C=C, q=qt @ Pn.T)
    assert set(be.calls) == dsr.dense_methods(False, False)
    assert list(m1.last_newton_per_al) == list(m0.last_newton_per_al)
    dev = max(float((x1.double() @ P - x0_.double()).abs().max()), float((u1.double() - u0_.double()).abs().max()))
    print(f"DENSESTEP rotated ({nx},{nu}) {mode}: Newton counts {list(m1.last_newton_per_al)}, rotated-back deviation {dev:.2e}, "
          f"largest off-diagonal {float(off.abs().max()):.2f}")
    assert dev < 1e-6


# ---- 5. g against central differences of the merit; the line search against a direct statement ----------------------------
def _off_kinks(pr, z, xbox):
    """The iterate moved off the box rows' kinks (probes of +-1e-5 stay on one quadratic piece)."""
    nx, nu = pr["dims"][2:]
    xl, xh = (a if a.dim() == 3 else a.reshape(1, 1, nx) for a in (pr["xlo"], pr["xhi"]))
    lo, hi = (a if a.dim() == 3 else a.reshape(1, 1, nu) for a in (pr["lo"], pr["hi"]))
    for _ in range(3):
        x, u = z[..., :nx], z[..., nx:]
        if xbox:
            z[..., :nx] += 5e-3 * (((x - xh).abs() < 2e-3) | ((x - xl).abs() < 2e-3))
        z[..., nx:] += 5e-3 * (((u - hi).abs() < 2e-3) | ((u - lo).abs() < 2e-3))
    return z


@pytest.mark.parametrize("xbox,poly", COMBOS, ids=COMBO_IDS)
@pytest.mark.parametrize("nx,nu,T,B,m,layout", [(2, 1, 5, 3, 2, "shared"), (4, 2, 6, 3, 3, "per_stage"), (13, 4, 4, 2, 3, "per_instance")])
def test_g_is_the_gradient_of_the_merit(nx, nu, T, B, m, layout, xbox, poly):
    pr, plant = dsr.dense_problem(B, T, nx, nu, m, layout, F64)
    gen = torch.Generator().manual_seed(4)
    z = pr["z0"] + 0.3 * torch.randn(B, T, nx + nu, generator=gen, dtype=F64)
    lam = 0.3 * torch.randn(B, grr.lam_width(T, nx, nu, xbox, m if poly else 0), generator=gen, dtype=F64)
    lam[:, T * nx:].clamp_(min=0)
    rho = torch.full((B,), 10.0, dtype=F64)
    z = _off_kinks(pr, z, xbox)
    res = dsr.residuals(pr, z, xbox, poly)
    if poly and np.abs(res["p"]).min() <= 1e-3:
        pytest.fail(f"the seeded problem has a general row {np.abs(res['p']).min():.1e} from its kink: choose another seed")
    assert min(np.abs(v).min() for v in res.values() if v is not None) > 1e-3   # no row within 1e-3 of its kink
    assert not poly or ((res["p"] > 0).any() and (res["p"] < 0).any())
    be = dsr.DenseStepOracleBackend()
    sb_u, st_u, xb, pl = dsr.args(pr, xbox, poly)
    prob = (pr["x0"], lam, rho, pr["C"], pr["q"], pr["lo"], pr["hi"], sb_u, st_u)
    xn, F = ssr.linearize(plant, z, nx)
    d, g = torch.empty_like(z), torch.empty_like(z)
    be.newton_step_dense(pr["dims"], z, xn, F, *prob, xb, pl, d, g_out=g)

    def merit(v):
        phi = torch.zeros(B, dtype=F64)
        be.merit_dense(pr["dims"], 1, v, ssr.true_next(plant, v, nx), *prob, xb, pl, phi)
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
    print(f"DENSESTEP ({nx},{nu}) {layout} xbox={xbox} rows={poly}: g_out vs central differences of merit_dense: {err:.2e} (of the "
          f"largest probed {scale:.3g})")
    assert err < FD_TOL, (err, probes)


@pytest.mark.parametrize("xbox,poly", COMBOS, ids=COMBO_IDS)
@pytest.mark.parametrize("nx,nu,T,B,m,layout", [(2, 1, 4, 3, 2, "per_stage"), (13, 4, 3, 2, 3, "per_instance")])
def test_merit_and_pick_equal_a_direct_statement(nx, nu, T, B, m, layout, xbox, poly):
    pr, plant = dsr.dense_problem(B, T, nx, nu, m, layout, F64)
    inp = dsr.kernel_inputs(pr, plant, xbox, poly)
    z, lam, rho = inp["z"], inp["lam"], inp["rho"]
    be = dsr.DenseStepOracleBackend()
    sb_u, st_u, xb, pl = dsr.args(pr, xbox, poly)
    xn = ssr.true_next(plant, z, nx)
    phi0, _, _, A2 = dsr.merit_magnitude_dense(pr, z, xn, lam, rho, xbox, poly)
    want0 = dsr.terms_numpy(pr, z, xn, lam, rho, xbox, poly)
    n, mm = nx + nu, (m if poly else 0)
    # + the oracle's and the statement's sequential sums over the T n cost terms
    gam = dsr.gamma_merit_dense(T, nx, nu, mm, cand=True) + T * n
    A0 = dsr.merit_magnitude_dense(pr, z, xn, lam, rho, xbox, poly)[1]
    assert (np.abs(phi0 - want0["phi"]) <= 2 * gam * EPS64 * A0).all()
    for n_ls in (20, 7):
        zz, ph = z.clone(), torch.tensor(phi0).clone()
        phis, kk, acc = torch.empty(n_ls, B, dtype=F64), torch.zeros(B, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)
        rn2 = torch.full((B,), -1.0, dtype=F64)
        al = (2.0 ** -torch.arange(n_ls, dtype=F64)).view(n_ls, 1, 1, 1)
        zc = (z.unsqueeze(0) + al * inp["d"].unsqueeze(0)).contiguous()
        xn_all = ssr.true_next(plant, zc, nx)
        be.merit_pick_dense(pr["dims"], n_ls, inp["d"], xn_all, pr["x0"], lam, rho, pr["C"], pr["q"], pr["lo"], pr["hi"],
                            sb_u, st_u, xb, pl, zz, ph, rnorm2=rn2, phi_all=phis, k_out=kk, accept_out=acc)
        st = [dsr.terms_numpy(pr, zc[k], xn_all[k], lam, rho, xbox, poly) for k in range(n_ls)]
        ref, rp2 = np.stack([s["phi"] for s in st]), np.stack([s["rp2"] for s in st])
        Ak = np.stack([dsr.merit_magnitude_dense(pr, zc[k], xn_all[k], lam, rho, xbox, poly)[1] for k in range(n_ls)])
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
            assert float(ph[b]) == float(phis[int(kk[b]), b])   # phi_prev <- the minimum, accepted or not
        assert acc.any()


# ---- 6. gradients through MPC against central differences --------------------------------------------------------------
# An AFFINE model given as a callable, for the reason section 24 gives: the backward pass is Gauss-Newton, exact at a
# stationary point of an affine model only. The stage is tests/test_gen_rows_cpu.py's (section 23: gen_problem, B = 2,
# T = 4, m = 2, box [B,T,nx], its dense cost) run through the three _dense methods, with the rows of the combination alone.
# The seed of a case is the first of 3, 4, ... at which THIS reference meets the conditions sections 20 / 23 state: the
# stage is stationary after its 4 Newton steps (max |g| < 1e-10), a row of each kind in use is active, and no row of any
# kind is within 1e-3 of switching. All asserted below.


def _stage(nx, nu, xbox, poly, seed):
    pr = grr.gen_problem(2, 4, nx, nu, 2, F64, "per_instance", box="per_stage", seed=seed)
    pr = dict(pr, q=pr["qC"])
    B, T = pr["dims"][:2]
    plant = ssr.AffineCallable(pr["F"], pr["c"])
    be = dsr.DenseStepOracleBackend()
    z, rho = pr["z0"].clone(), torch.ones(B, dtype=F64)
    lam = torch.zeros(B, grr.lam_width(T, nx, nu, xbox, pr["m"] if poly else 0), dtype=F64)
    for _ in range(2):
        dsr.al_iteration(be, pr, plant, xbox, poly, z, lam, rho)
    warm = dict(z=z, lam=lam, rho=rho)

    def stage(**over):
        zf = warm["z"].clone()
        dsr.al_iteration(be, {**pr, **over}, plant, xbox, poly, zf, warm["lam"].clone(), warm["rho"].clone(), dual=False)
        return zf
    return pr, plant, warm, stage


def _conditions(pr, plant, warm, zf, xbox, poly):
    B, T, nx, nu = pr["dims"]
    be = dsr.DenseStepOracleBackend()
    sb_u, st_u, xb, pl = dsr.args(pr, xbox, poly)
    xn, F = ssr.linearize(plant, zf, nx)
    d, g = torch.empty_like(zf), torch.empty_like(zf)
    be.newton_step_dense(pr["dims"], zf, xn, F, pr["x0"], warm["lam"], warm["rho"], pr["C"], pr["q"], pr["lo"], pr["hi"], sb_u,
                         st_u, xb, pl, d, g_out=g)
    res = dsr.residuals(pr, zf, xbox, poly)
    margin = min(np.abs(v).min() for v in res.values() if v is not None)
    return (g.abs().reshape(B, -1).max(1).values, int((res["p"] >= 0).sum()) if poly else 0,
            int((res["x"] >= 0).sum()) if xbox else 0, margin)


def stage_ok(nx, nu, xbox, poly, seed):
    """The conditions a seed has to meet (used to choose GRAD_CASES, asserted in the test)."""
    pr, plant, warm, stage = _stage(nx, nu, xbox, poly, seed)
    gmax, n_act, n_box, margin = _conditions(pr, plant, warm, stage(), xbox, poly)
    return bool((gmax < 1e-10).all()) and (n_act >= 1 or not poly) and (n_box >= 1 or not xbox) and margin > 1e-3


# (nx, nu, xbox, poly, seed)
GRAD_CASES = [(2, 1, False, False, 20), (2, 1, True, False, 39), (2, 1, False, True, 6), (2, 1, True, True, 49),
              (4, 2, False, False, 7)]


@pytest.mark.parametrize("nx,nu,xbox,poly,seed", GRAD_CASES, ids=lambda v: str(v))
def test_gradients_through_mpc_vs_finite_differences(nx, nu, xbox, poly, seed):
    """dC (all n^2 entries of one stage's block, the symmetric part perturbed as the host hands it on), dq and dineqh."""
    from deq_mpc_corl_amd import QuadCost
    pr, plant, warm, stage = _stage(nx, nu, xbox, poly, seed)
    B, T = pr["dims"][:2]
    n = nx + nu
    zf = stage()
    gmax, n_act, n_box, margin = _conditions(pr, plant, warm, zf, xbox, poly)
    print(f"DENSESTEP grad ({nx},{nu}) xbox={xbox} rows={poly} seed {seed}: max |g(z_final)| per instance {gmax.numpy()}; general "
          f"rows active {n_act}, state rows {n_box}; nearest row to switching {margin:.2e}")
    assert (gmax < 1e-10).all() and (n_act >= 1 or not poly) and (n_box >= 1 or not xbox) and margin > 1e-3
    assert all(not stage_ok(nx, nu, xbox, poly, s) for s in range(3, seed))   # the first seed that does
    be = dsr.DenseStepOracleBackend()
    hleaf = pr["h"].clone().requires_grad_(True)
    mpc = _mpc(pr["dims"], pr["lo"], pr["hi"], be, "fixed", al_iter=1, diag_cost=False, **dsr.mpc_kwargs(pr, xbox, poly, h=hleaf))
    mpc.reinitialize(pr["x0"], None)
    leaf = {k: pr[k].clone().requires_grad_(True) for k in ("C", "q")}
    leaf["h"] = hleaf
    x, u, _ = mpc.al_solve(warm["z"][..., :nx].clone(), warm["z"][..., nx:].clone(), plant, plant.jac, pr["x0"],
                           QuadCost(leaf["C"], leaf["q"]), lamda_init=warm["lam"].clone(), rho_init=warm["rho"].clone())
    gbar = torch.randn(B, T, n, generator=torch.Generator().manual_seed(1), dtype=F64).float().double()
    ((x.double() * gbar[..., :nx]).sum() + (u.double() * gbar[..., nx:]).sum()).backward()
    assert set(be.calls) - {"backward"} == dsr.dense_methods(xbox, poly)
    assert torch.equal(torch.cat((x, u), -1).detach(), zf.float())   # the MPC ran the stage the differences go through
    assert leaf["C"].grad.shape == pr["C"].shape
    assert torch.equal(leaf["C"].grad, leaf["C"].grad.transpose(-1, -2))
    rng = np.random.default_rng(2)
    b0, t0 = int(rng.integers(0, B)), int(rng.integers(0, T))
    idxs = {"C": [(b0, t0, i, j) for i in range(n) for j in range(n)],
            "q": [tuple(int(rng.integers(0, s)) for s in pr["q"].shape) for _ in range(4)], "h": []}
    if poly:
        assert hleaf.grad.shape == pr["h"].shape
        act = dsr.residuals(pr, zf, xbox, poly)["p"] >= 0
        idxs["h"] = [tuple(int(v) for v in i) for i in np.argwhere(act)][:4]
        idxs["h"] += [tuple(int(rng.integers(0, s)) for s in pr["h"].shape) for _ in range(4 - len(idxs["h"]))]
    probes = []
    for name, ii in idxs.items():
        for idx in ii:
            vals = []
            for sgn in (1.0, -1.0):
                a = pr[name].clone()
                a[idx] += sgn * FD_H
                if name == "C":   # the solve takes the symmetric part: perturb it as the host would hand it on
                    a = 0.5 * (a + a.transpose(-1, -2))
                vals.append(float((gbar * stage(**{name: a})).sum()))
            probes.append((name, float(leaf[name].grad[idx]), (vals[0] - vals[1]) / (2 * FD_H)))
    scale = max(abs(a) for _, a, _ in probes)
    for name in idxs:
        if idxs[name]:
            e = max(abs(a - fd) for nm, a, fd in probes if nm == name) / scale
            print(f"DENSESTEP grad ({nx},{nu}) xbox={xbox} rows={poly}: d{name} vs central differences: {e:.2e} (of the largest "
                  f"probed {scale:.3g})")
    assert not poly or max(abs(a) for nm, a, _ in probes if nm == "h") > 0   # an active row was probed
    assert max(abs(a) for nm, a, _ in probes if nm == "C") > 0
    err = max(abs(a - fd) for _, a, fd in probes) / scale
    assert err < FD_TOL, (err, probes)


# ---- 7. host ------------------------------------------------------------------------------------------------------------
class _DenseRecordingBackend(RecordingBackend):
    """RecordingBackend with the three _dense methods and the dual updates with rows (records as its plain ones)."""

    def newton_step_dense(self, dims, z, xnext, F, x0, lam, rho, Cs, q, ulo, uhi, sb_u, st_u, xbnd, poly, d_out, g_out=None,
                          factor=None, info=None, **kw):
        assert not kw, kw   # no workspace, no obs
        assert Cs.dim() == 4
        self._note_factor(factor)
        self._lins.append(F)
        self.calls.append(["newton_step_dense", factor is not None, info is not None, xbnd is not None,
                           None if poly is None else tuple(poly[2:])])
        d_out.zero_()

    def merit_dense(self, dims, K, zc, xnext, x0, lam, rho, Cs, q, ulo, uhi, sb_u, st_u, xbnd, poly, phi, rnorm2=None):
        self.calls.append(["merit_dense", K])
        self._residual(rnorm2)

    def merit_pick_dense(self, dims, n_ls, d, xnext_all, x0, lam, rho, Cs, q, ulo, uhi, sb_u, st_u, xbnd, poly, z, phi_prev,
                         rnorm2=None, phi_all=None, k_out=None, accept_out=None):
        self.calls.append(["merit_pick_dense", n_ls])

    def dual_update_xbox(self, dims, z, xnext, x0, ulo, uhi, sb_u, st_u, xbnd, lam, rho, rho_scale=10.0):
        self.calls.append(["dual_update_xbox"])
        rho.mul_(rho_scale)

    def dual_update_rows(self, dims, z, xnext, x0, ulo, uhi, sb_u, st_u, xbnd, poly, lam, rho, rho_scale=10.0):
        self.calls.append(["dual_update_rows"])
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


@pytest.mark.parametrize("xbox,poly", COMBOS, ids=COMBO_IDS)
@pytest.mark.parametrize("grad", [False, True])
def test_no_quad_workspace_and_no_fused_model_with_a_dense_cost(grad, xbox, poly):
    """B = 5 >= QUAD_MIN_BATCH = 4 of the recording backend: the plain callable route takes the quad step there; with a
    dense cost the team step runs, with the packed factor when a backward pass follows. The recording backend has no
    solve_lin_gen: with a callable dx the combinations need newton_step_dense only."""
    from deq_mpc_corl_amd.dynamics import Pendulum1lDynamics
    from deq_mpc_corl_amd.qpth.AL_mpc import _SolveState
    pr, plant = _tiny()
    be = _DenseRecordingBackend()
    kw = dict(x_lower=-0.5, x_upper=0.5) if xbox else {}
    if poly:
        kw.update(ineqG=torch.tensor([[1.0, 1.0, 0.0], [0.0, 1.0, -1.0]], dtype=F64), ineqh=torch.tensor([0.3, 0.5], dtype=F64))
    # (the constructor's pairwise guard on rows with state bounds is for a backend handed to it; this one goes in behind it,
    # as the lazily resolved default does)
    mpc = _mpc(pr["dims"], pr["lo"], pr["hi"], None if xbox and poly else be, "fixed", al_iter=1, diag_cost=False, **kw)
    mpc._backend = be
    C = torch.diag_embed(pr["Qd"]).requires_grad_(grad)
    x, u, _ = _call(mpc, pr, plant, plant.jac, C=C)
    if grad:
        (x.sum() + u.sum()).backward()
    st = _SolveState()
    st.lin, st.stream_mode, st.dx = None, False, Pendulum1lDynamics()   # a provider with a compiled-in model
    assert mpc._fused_model(st) is False
    plain = _mpc(pr["dims"], pr["lo"], pr["hi"], be, "fixed", al_iter=1)
    assert plain._fused_model(st) is True
    names = [c[0] for c in be.calls]
    assert "_workspace" not in names and "new_workspace" not in names and "backward_ws" not in names
    dual = "dual_update_rows" if poly else "dual_update_xbox" if xbox else "dual_update"
    assert names[:-1 if grad else None] == ["merit_dense"] + ["newton_step_dense", "merit_pick_dense"] * 4 + ["merit_dense", dual]
    want = ["newton_step_dense", grad, True, xbox, (2, 0, 0, 0, 0) if poly else None]
    assert all(c == want for c in be.calls if c[0] == "newton_step_dense")
    if grad:
        assert be.calls[-1] == ["backward", "factor0", "last_linearisation"]
    T, nx, nu = pr["dims"][1:]
    assert mpc.lamda_prev.shape == (pr["dims"][0], grr.lam_width(T, nx, nu, xbox, 2 if poly else 0))


def test_plain_launch_trace_is_unchanged_without_a_dense_cost():
    """The recording backend WITH the _dense methods against the one without: identical records on the callable route."""
    pr, plant = _tiny()
    got = []
    for cls in (RecordingBackend, _DenseRecordingBackend):
        be = cls()
        mpc = _mpc(pr["dims"], pr["lo"], pr["hi"], be, "reference", al_iter=2)
        _call(mpc, pr, plant, plant.jac, C=torch.diag_embed(pr["Qd"]))
        got.append([c for c in be.calls if c[0] not in ("_workspace", "new_workspace")])
    assert got[0] == got[1] and got[0]


def test_old_errors_on_backends_without_the_dense_step():
    """Backends without newton_step_dense: the errors and messages of before, whatever other step twins they have."""
    from deq_mpc_corl_amd import MPC, PendulumDynamics, QuadCost
    nx, nu, B, T = 2, 1, 3, 4
    pr = sbr.xbox_problem(B, T, nx, nu, F64)
    dyn = PendulumDynamics()
    kw = dict(u_lower=pr["lo"], u_upper=pr["hi"], n_batch=B, dtype=F64, diag_cost=False)
    C = torch.diag_embed(pr["Qd"])
    xi, ui = pr["z0"][..., :nx].clone(), pr["z0"][..., nx:].clone()
    for be in (OracleBackend(), DenseOracleBackend(), grr.GenOracleBackend(), ssr.XboxStepOracleBackend(),
               rsr.RowsStepOracleBackend(), RecordingBackend()):
        mpc = MPC(nx, nu, T, backend=be, **kw)
        mpc.reinitialize(pr["x0"], None)
        with pytest.raises(NotImplementedError, match=OLD_MSG):
            mpc(pr["x0"], QuadCost(C, pr["q"]), dyn, dyn.jac, x_init=xi, u_init=ui)
    # with rows on a backend that has their step twins and solve_lin_gen, but not the dense step: still the old message
    rows = dict(ineqG=torch.ones(1, nx + nu, dtype=F64), ineqh=torch.ones(1, dtype=F64))
    for extra in (rows, dict(x_lower=-1.0, x_upper=1.0), dict(rows, x_lower=-1.0, x_upper=1.0)):
        mpc = MPC(nx, nu, T, backend=rsr.RowsStepOracleBackend(), **kw, **extra)
        mpc.reinitialize(pr["x0"], None)
        with pytest.raises(NotImplementedError, match=OLD_MSG):
            mpc(pr["x0"], QuadCost(C, pr["q"]), dyn, dyn.jac, x_init=xi, u_init=ui)
    # the constructor's pairwise guards for a backend with neither solve_lin_gen nor newton_step_dense
    with pytest.raises(NotImplementedError, match="x_lower / x_upper with diag_cost=False"):
        MPC(nx, nu, T, backend=ssr.XboxStepOracleBackend(), x_lower=-1.0, x_upper=1.0, **kw)
    with pytest.raises(NotImplementedError, match="ineqG / ineqh with diag_cost=False"):
        MPC(nx, nu, T, backend=prr.PolyOracleBackend(), **kw, **rows)
    # ... which a backend with newton_step_dense passes, and meets again in the solve when the dynamics are LinDx
    from deq_mpc_corl_amd.qpth.al_utils import LinDx
    be = _DenseRecordingBackend()
    for extra, msg in ((dict(x_lower=-1.0, x_upper=1.0), "x_lower / x_upper with diag_cost=False"),
                       (rows, "ineqG / ineqh with diag_cost=False")):
        mpc = MPC(nx, nu, T, backend=be, **kw, **extra)
        mpc.reinitialize(pr["x0"], None)
        with pytest.raises(NotImplementedError, match=msg):
            mpc(pr["x0"], QuadCost(C, pr["q"]), LinDx(pr["F"], pr["c"]), None, x_init=xi, u_init=ui)


def test_kept_guards_still_raise():
    from deq_mpc_corl_amd import MPC, PendulumDynamics, QuadCost
    from deq_mpc_corl_amd.qpth.AL_mpc_custom import Obstacle_MPC
    nx, nu, B, T = 2, 1, 3, 4
    pr = sbr.xbox_problem(B, T, nx, nu, F64)
    dyn = PendulumDynamics()
    kw = dict(u_lower=pr["lo"], u_upper=pr["hi"], n_batch=B, dtype=F64, diag_cost=False, backend=dsr.DenseStepOracleBackend())
    C = torch.diag_embed(pr["Qd"])
    xi, ui = pr["z0"][..., :nx].clone(), pr["z0"][..., nx:].clone()
    with pytest.raises(NotImplementedError, match="diag_cost=False with state_estimator"):
        MPC(nx, nu, T, state_estimator=True, **kw)
    with pytest.raises(NotImplementedError, match="Obstacle_MPC: diag_cost=False is not built"):
        Obstacle_MPC(3, nu, T, **kw)
    mpc = MPC(nx, nu, T, **kw)
    mpc.reinitialize(pr["x0"], None)
    mpc.linearize_once = True
    with pytest.raises(NotImplementedError, match="diag_cost=False with linearize_once"):
        mpc.al_solve_stream(xi, ui, dyn, dyn.jac, pr["x0"], QuadCost(C, pr["q"]))
    with pytest.raises(NotImplementedError, match="ineqG"):
        MPC(nx, nu, T, **kw, ineqG=torch.ones(1, nx + nu, dtype=F64, requires_grad=True), ineqh=torch.ones(1, dtype=F64))
    # a lamda of the plain width handed to a solve with rows / state bounds
    for extra in (dict(ineqG=torch.ones(1, nx + nu, dtype=F64), ineqh=torch.ones(1, dtype=F64)), dict(x_lower=-1.0, x_upper=1.0)):
        mpc = MPC(nx, nu, T, **kw, **extra)
        mpc.reinitialize(pr["x0"], None)
        with pytest.raises(ValueError, match="lamda"):
            mpc.al_solve(xi, ui, dyn, dyn.jac, pr["x0"], QuadCost(C, pr["q"]),
                         lamda_init=torch.zeros(B, T * nx + 2 * T * nu, dtype=F64))


def test_sharded_norm_is_the_rows_twins():
    """rn2 of merit_dense holds every row in use and nothing of the cost, so the batch-global exit of a sharded batch sees
    what it saw with a diagonal cost: equal to the diagonal twin's bit for bit, and to the direct statement's."""
    pr, plant = dsr.dense_problem(3, 4, 2, 1, 2, "per_stage", F64)
    be = dsr.DenseStepOracleBackend()
    B, T, nx, nu = pr["dims"]
    xn = ssr.true_next(plant, pr["z0"], nx)
    got = {}
    for xbox, poly in COMBOS:
        sb_u, st_u, xb, pl = dsr.args(pr, xbox, poly)
        lam, rho = torch.zeros(B, grr.lam_width(T, nx, nu, xbox, 2 if poly else 0), dtype=F64), torch.ones(B, dtype=F64)
        phi, rn2, rd = torch.zeros(B, dtype=F64), torch.zeros(B, dtype=F64), torch.zeros(B, dtype=F64)
        be.merit_dense(pr["dims"], 1, pr["z0"], xn, pr["x0"], lam, rho, pr["C"], pr["q"], pr["lo"], pr["hi"], sb_u, st_u, xb, pl,
                       phi, rn2)
        args = (pr["dims"], 1, pr["z0"], xn, pr["x0"], lam, rho, pr["Qd"], pr["q"], pr["lo"], pr["hi"], sb_u, st_u)
        if poly:
            be.merit_rows(*args, xb, pl, torch.zeros(B, dtype=F64), rd)
        elif xbox:
            be.merit_xbox(*args, xb, torch.zeros(B, dtype=F64), rd)
        else:
            OracleBackend.merit(be, *args, torch.zeros(B, dtype=F64), rd)
        assert torch.equal(rn2, rd)
        want = dsr.terms_numpy(pr, pr["z0"], xn, lam, rho, xbox, poly)["rp2"]
        assert np.allclose(rn2.numpy(), want, rtol=1e-13)
        got[(xbox, poly)] = rn2
    assert (got[(True, True)] > got[(False, True)]).all() and (got[(False, True)] > got[(False, False)]).all()


# ---- 8. the GPU tests' inputs, on the reference alone -------------------------------------------------------------------
@pytest.mark.parametrize("xbox,poly", COMBOS, ids=COMBO_IDS)
@pytest.mark.parametrize("nx,nu,T,B,m,layout", dsr.GPU_CASES, ids=lambda v: str(v))
def test_gpu_case_inputs(nx, nu, T, B, m, layout, xbox, poly):
    """After one reference AL iteration every instance has a row of each kind in use active with a nonzero multiplier, no
    row of any kind is within KINK_MARGIN of its kink, the cost is dense, and in NO instance are two of the 20 (or of the
    first 7) line-search merits the pick could confuse - the two smallest - closer than twice the fp32 merit tolerance:
    the GPU test demands the reference's index in every instance."""
    pr, plant, inp = dsr.gpu_case(nx, nu, T, B, m, layout, xbox, poly, F64)
    mm = m if poly else 0
    res = dsr.residuals(pr, inp["z"], xbox, poly)
    _, lxu, lxl, lp = grr.split_lam(inp["lam"].numpy(), T, nx, nu, xbox, mm)
    if poly:
        assert ((res["p"] > 0) & (lp > 0)).reshape(B, -1).any(1).all()
    if xbox:
        assert (res["x"] > 0).reshape(B, -1).any(1).all() and ((lxu > 0) | (lxl > 0)).reshape(B, -1).any(1).all()
    assert min(np.abs(v).min() for v in res.values() if v is not None) > dsr.KINK_MARGIN
    assert not np.isnan(inp["d"].numpy()).any() and (inp["rho"] == 10.0).all()
    off = pr["C"] - torch.diag_embed(pr["C"].diagonal(dim1=-2, dim2=-1))
    assert off.abs().amax((1, 2, 3)).min() > 0.05 and torch.equal(pr["C"], pr["C"].transpose(-1, -2))
    be = dsr.DenseStepOracleBackend()
    sb_u, st_u, xb, pl = dsr.args(pr, xbox, poly)
    al = (2.0 ** -torch.arange(20, dtype=F64)).view(20, 1, 1, 1)
    zc = (inp["z"].unsqueeze(0) + al * inp["d"].unsqueeze(0)).contiguous()
    xn_all = ssr.true_next(plant, zc, nx)
    phis = torch.empty(20, B, dtype=F64)
    be.merit_dense(pr["dims"], 20, zc, xn_all, pr["x0"], inp["lam"], inp["rho"], pr["C"], pr["q"], pr["lo"], pr["hi"], sb_u,
                   st_u, xb, pl, phis)
    zmag = inp["z"].abs().numpy()[None] + al.numpy() * inp["d"].abs().numpy()[None]
    A = np.stack([dsr.merit_magnitude_dense(pr, zc[k], xn_all[k], inp["lam"], inp["rho"], xbox, poly, zmag=zmag[k])[1]
                  for k in range(20)])
    tol32 = dsr.gamma_merit_dense(T, nx, nu, mm, cand=True) * ax.EPS[torch.float32] * A
    close = 0
    for n_ls in (20, 7):
        srt = np.sort(phis.numpy()[:n_ls], 0)
        close += int(((srt[1] - srt[0]) <= 2 * tol32[:n_ls].max(0)).sum())
    print(f"DENSESTEP inputs ({nx},{nu},{T},{B},m={m}) xbox={xbox} rows={poly}: near-ties of the two best merits at fp32 tolerance: "
          f"{close} of {2 * B}")
    assert close == 0


class _GapBackend(dsr.DenseStepOracleBackend):
    """Records, per line search, the smallest gap over the batch between the two best merits, relative to the merit."""

    def __init__(self):
        super().__init__()
        self.gaps = []

    def merit_pick_dense(self, dims, n_ls, d, xn_all, *a, **kw):
        pa = torch.empty(n_ls, dims[0], dtype=F64)
        super().merit_pick_dense(dims, n_ls, d, xn_all, *a, **{**kw, "phi_all": pa})
        srt = np.sort(pa.numpy(), 0)
        self.gaps.append(float(((srt[1] - srt[0]) / np.abs(srt[0]).clip(1)).min()))


def _whole_solve(be, nx, nu, T, B, mode, xbox, poly, al_iter=3, **kw):
    pr, plant = dsr.dense_whole_problem(B, T, nx, nu, xbox, poly, mode, **kw)
    mpc = _mpc(pr["dims"], pr["lo"], pr["hi"], be, mode, al_iter=al_iter, diag_cost=False, **dsr.mpc_kwargs(pr, xbox, poly))
    _call(mpc, pr, plant, plant.jac)
    return mpc


@pytest.mark.parametrize("xbox,poly", COMBOS, ids=COMBO_IDS)
@pytest.mark.parametrize("mode", ["reference", "fixed"])
def test_gpu_whole_solve_at_2_1_has_no_tied_line_search(mode, xbox, poly):
    """The (2,1) whole solve the GPU test compares (dense_step_reference.WHOLE_SOLVE_KW, on CurvedSinPlant): every line
    search of the reference solve is decided - the two best merits at least WHOLE_SOLVE_MIN_GAP apart, relative."""
    nx, nu = 2, 1
    T, B = dsr.WHOLE_SOLVE_DIMS[(nx, nu)]
    be = _GapBackend()
    mpc = _whole_solve(be, nx, nu, T, B, mode, xbox, poly, **dsr.WHOLE_SOLVE_KW[(nx, nu)])
    _, lxu, lxl, lp = grr.split_lam(mpc.lamda_prev.numpy(), T, nx, nu, xbox, 1 if poly else 0)
    assert (not poly or lp.max() > 0) and (poly or not xbox or max(lxu.max(), lxl.max()) > 0)   # (the row is the tighter one)
    print(f"DENSESTEP whole-solve gaps (2,1) {mode} xbox={xbox} rows={poly}: smallest relative gap of the two best merits: "
          f"{min(be.gaps):.2e}")
    assert min(be.gaps) > dsr.WHOLE_SOLVE_MIN_GAP


def _undecided(nx, nu, T, B, mode, xbox, poly, al_iter, **kw):
    """Per instance: does the reference whole solve have a line search float64 does not decide (dsr.DenseTieBackend)?"""
    be = dsr.DenseTieBackend()
    _whole_solve(be, nx, nu, T, B, mode, xbox, poly, al_iter, **kw)
    return be.undecided


def test_gpu_whole_solves_excused_shares():
    """What tests/test_gpu_dense_step.py may excuse by the near-tie rule, per instance, counted on the reference alone and
    capped at a quarter of the instances: the whole solves at (2,1) and (13,4) in both exit modes and the four
    combinations, and the large batch."""
    for (nx, nu), (_, B) in dsr.WHOLE_SOLVE_DIMS.items():
        for mode in ("reference", "fixed"):
            for xbox, poly in COMBOS:
                n = int(_undecided(nx, nu, 5, B, mode, xbox, poly, 3, **dsr.WHOLE_SOLVE_KW[(nx, nu)]).sum())
                print(f"DENSESTEP excused ({nx},{nu}) {mode} xbox={xbox} rows={poly}: {n} of {B}")
                assert n <= B // 4, (nx, nu, mode, xbox, poly, n)
    big = _undecided(2, 1, 3, 4096, "reference", False, False, 2, every_instance=False, **dsr.LARGE_BATCH_KW)
    print(f"DENSESTEP large batch: {int(big.sum())} of 4096 instances with an undecided line search")
    assert big.sum() <= 4096 // 4


@pytest.mark.parametrize("nx,nu", list(dsr.WHOLE_SOLVE_KW), ids=lambda v: str(v))
def test_gpu_whole_solves_reference_is_stable_at_the_twin_bound(nx, nu):
    """The whole solves the GPU test compares to the twin bound on lam: a one-ulp change of q, up or down, moves the
    REFERENCE's own lam by less than that bound in all eight solves (a comparison to the bound says nothing where the
    reference itself moves by more; a heavier sine does, dense_step_reference.WHOLE_SOLVE_KW)."""
    T, B = dsr.WHOLE_SOLVE_DIMS[(nx, nu)]
    worst = 0.0
    for mode in ("reference", "fixed"):
        for xbox, poly in COMBOS:
            pr, plant = dsr.dense_whole_problem(B, T, nx, nu, xbox, poly, mode, **dsr.WHOLE_SOLVE_KW[(nx, nu)])
            lams = []
            for way in (0.0, INF, -INF):
                q = pr["q"] if way == 0.0 else torch.from_numpy(np.nextafter(pr["q"].numpy(), way))
                mpc = _mpc(pr["dims"], pr["lo"], pr["hi"], dsr.DenseStepOracleBackend(), mode, al_iter=3, diag_cost=False,
                           **dsr.mpc_kwargs(pr, xbox, poly))
                _call(mpc, pr, plant, plant.jac, q=q)
                lams.append(mpc.lamda_prev.clone())
            bound = max(8 * dsr.INERT_TWIN[(nx, nu, xbox, poly)], 64 * EPS64 * float(lams[0].abs().max()))
            worst = max(worst, max(float((lams[0] - l).abs().max()) for l in lams[1:]) / bound)
    print(f"DENSESTEP whole-solve stability ({nx},{nu}): a one-ulp change of q moves the reference's lam by at most {worst:.2f} "
          f"of the twin bound")
    assert worst < 1.0
