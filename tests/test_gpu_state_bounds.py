"""GPU tests of the state-bound fused solve (k_solve_lin_gen<XBOX> behind alqp_solve_lin_xbox_*, MPC(x_lower=, x_upper=)).
The reference is tests/state_bounds_reference.py's backend (pinned on the CPU by tests/test_state_bounds_cpu.py), fed the
kernel's own inputs, in the kernel's dtype. Tolerances and the rule for comparing fp64 line-search decisions are
tests/test_gpu_dense_cost.py's (RT, PHI_EPS, G_FLOOR; 1e-10 / 2e-9 on z / lam of a full fp64 solve)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import state_bounds_reference as sbr
from tests.aux_cases import Guarded
from tests.dense_cost_reference import dense_w
from tests.test_gpu_dense_cost import G_FLOOR, PHI_EPS, RT, _GuardedU8, scale_err

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TD = {"f64": torch.float64, "f32": torch.float32}
INIT_MERIT, DUAL_UPDATE, SAVE_FACTOR = 1, 2, 4
# (nx, nu, T, B, state bounds per (b, t)): four teams per wavefront, the second wavefront ragged (a padding team with b
# clamped), T*NX = 4 below the team width 8; one instance, strided bounds; two teams per wavefront, ragged, T*NX = 32 =
# the team width; whole-wavefront teams with strided bounds, T*NX = 39 below 64; the largest n; the workload's horizon,
# T*NX = 260: four trips and a tail of the strided loops; the sizes at which Cfg's padding vanishes: n = 8 and n = 16
# (pad4(N) == N, no padding column behind a row; the second with strided bounds), and nx = 4 (pad4(NX) == NX) with odd
# n = 5 and NROWS = 15, one lane short of the 16-lane team
SHAPES = [(2, 1, 2, 5, False), (2, 1, 5, 1, True), (8, 2, 4, 3, False), (13, 4, 3, 2, True), (14, 4, 3, 2, False),
          (13, 4, 20, 2, False), (6, 2, 3, 5, False), (12, 4, 3, 3, True), (4, 1, 3, 9, False)]
ON_BOUND = (8, 2, 4, 3)   # the shape whose first traced iterate has a state exactly on its upper bound


def _be():
    from deq_mpc_corl_amd.backend import default_backend
    return default_backend()


def _problem(nx, nu, T, B, dtype, ps=False, seed=5):
    return sbr.xbox_problem(B, T, nx, nu, TD[dtype], ps, seed=seed, push=True)


def _state0(pr):
    B, T, nx, nu = pr["dims"]
    dt = pr["z0"].dtype
    return dict(z=pr["z0"].clone(), lam=torch.zeros(B, sbr.lam_width(T, nx, nu), dtype=dt), rho=torch.ones(B, dtype=dt),
                phi=torch.zeros(B, dtype=dt))


def _strides(pr):
    B, T, nx, nu = pr["dims"]
    return ((0, 0) if pr["lo"].dim() == 1 else (T * nu, nu)), ((0, 0) if pr["xlo"].dim() == 1 else (T * nx, nx))


def gpu_solve(pr, st, steps=0, want_factor=False, plain=False, **kw):
    """One alqp_solve_lin_xbox launch (`plain`: alqp_solve_lin on the team kernel, the state rows cut out of lam) from the
    state `st` (CPU tensors; not modified). Every output is a slice out of a sentinel-filled tensor whose guard bands must
    survive. -> dict of CPU tensors (+ tr, factor on the device)."""
    be = _be()
    B, T, nx, nu = pr["dims"]
    n = nx + nu
    dt = pr["z0"].dtype
    d = lambda a: a.to(DEV).contiguous()
    G = {k: Guarded(tuple(st[k].shape), dt, DEV, init=st[k]) for k in ("z", "lam", "rho", "phi")}
    G["rn2"] = Guarded((B,), dt, DEV)
    G["info"] = Guarded((B,), torch.int32, DEV, init=torch.zeros(B, dtype=torch.int32))
    G["status"] = _GuardedU8(B, DEV, torch.ones(B, dtype=torch.uint8))
    tr = None
    if steps:
        tr = {"g": Guarded((steps, B, T, n), dt, DEV), "d": Guarded((steps, B, T, n), dt, DEV),
              "phi": Guarded((steps, 20, B), dt, DEV), "phi_prev": Guarded((steps, B), dt, DEV),
              "k": Guarded((steps, B), torch.int32, DEV), "accept": Guarded((steps, B), torch.int32, DEV)}
        kw["trace"] = {k: v.t for k, v in tr.items()}
    if want_factor:
        G["factor"] = Guarded((B, T, n * (n + 1) // 2), dt, DEV)
        kw["factor"] = G["factor"].t
    (sb, stt), (sbx, stx) = _strides(pr)
    head = (pr["dims"], d(pr["Qd"]), d(pr["q"]), d(pr["F"]), d(pr["c"]), d(pr["x0"]), d(pr["lo"]), d(pr["hi"]), sb, stt)
    tail = (G["z"].t, G["lam"].t, G["rho"].t, G["phi"].t)
    okw = dict(rnorm2=G["rn2"].t, info=G["info"].t, status=G["status"].t)
    if plain:
        ok = be.solve_lin(*head, *tail, variant="team", **okw, **kw)
    else:
        ok = be.solve_lin_xbox(*head, d(pr["xlo"]), d(pr["xhi"]), sbx, stx, *tail, **okw, **kw)
    torch.cuda.synchronize()
    for name, g in list(G.items()) + list((tr or {}).items()):
        assert g.intact(), f"guard band of {name}"
    out = {k: v.t.cpu() for k, v in G.items() if k != "factor"}
    out["ok"] = ok
    if tr:
        out["tr"] = {k: v.t.cpu().numpy() for k, v in tr.items()}
    if want_factor:
        out["factor"] = G["factor"].t
    return out


def ref_solve(pr, st, **kw):
    return sbr.run_solve(sbr.XboxOracleBackend(), pr["Qd"], pr["q"], pr["F"], pr["c"], pr["x0"], pr["lo"], pr["hi"], pr["xlo"],
                         pr["xhi"], st["z"], st["lam"], st["rho"], st["phi"], **kw)


def _merit64(pr, z, lam, rho):
    """fp64 merit of the reference at (z, lam, rho) [B,...] numpy."""
    B, T, nx, nu = pr["dims"]
    f = lambda a: a.double().numpy()
    xl, xh = (f(pr[k]) if pr[k].dim() == 3 else f(pr[k]).reshape(1, 1, nx) for k in ("xlo", "xhi"))
    ll, lxu, lxl = sbr.split_lam(lam, T, nx, nu)
    xn = np.einsum("btij,btj->bti", f(pr["F"]), z[:, :-1]) + f(pr["c"])
    return sbr.merit_xbox("f64", z, xn, f(pr["x0"]), ll, lxu, lxl, rho, f(pr["Qd"]), f(pr["q"]), f(pr["lo"]), f(pr["hi"]), xl, xh)[0]


def _after_one_al_iteration(pr, on_bound=False):
    """(z, lam, rho, phi) after one AL iteration of the reference from lam = 0, rho = 1: nonzero state-row multipliers, and
    in every instance an upper and a lower state row active and one inactive - checked here. `on_bound`: one state per
    instance is then put exactly on its upper bound (its row counts in D, >= 0, and not in g, > 0)."""
    B, T, nx, nu = pr["dims"]
    o = ref_solve(pr, _state0(pr), al_iter=1, max_newton=4, flags=INIT_MERIT | DUAL_UPDATE)
    st = {k: o[k] for k in ("z", "lam", "rho", "phi")}
    if on_bound:
        st["z"][:, T - 1, 2] = pr["xhi"][:, T - 1, 2] if pr["xhi"].dim() == 3 else pr["xhi"][2]
    ru, rl = sbr.xbox_residuals(pr, st["z"])
    per = lambda m: m.reshape(B, -1).any(1).all()
    assert per(ru > 0) and per(rl > 0) and per((ru < 0) | (rl < 0)), "generator: active upper / lower and inactive state rows"
    assert not on_bound or per(ru == 0)
    _, lxu, lxl = sbr.split_lam(st["lam"].numpy(), T, nx, nu)
    assert per(lxu > 0) and per(lxl > 0), "generator: nonzero state-row multipliers"
    return st


# ---- per Newton step ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("nx,nu,T,B,ps", SHAPES)
def test_every_newton_step_vs_reference(nx, nu, T, B, ps, dtype):
    """One-step launches with an AlqpTrace; before each, the reference takes the same step from the kernel's own
    (z, lam, rho, phi). From (lam, rho = 10) after one reference AL iteration: four steps, the dual update, three more at
    rho = 100."""
    pr = _problem(nx, nu, T, B, dtype, ps)
    st = _after_one_al_iteration(pr, (nx, nu, T, B) == ON_BOUND)
    zs = float(pr["z0"].abs().max())
    rt, pe = RT[dtype], PHI_EPS[dtype]
    g0 = None
    worst = dict(g=0.0, d=0.0, phi=0.0)
    n_decided = 0
    for s in range(8):
        if s == 4:   # dual update alone
            h = gpu_solve(pr, st, al_iter=1, max_newton=0, flags=DUAL_UPDATE)
            o = ref_solve(pr, st, al_iter=1, max_newton=0, flags=DUAL_UPDATE)
            assert torch.equal(h["rho"], o["rho"])
            assert (h["lam"] - o["lam"]).abs().max() <= 10 * rt * max(1.0, float(o["lam"].abs().max()))
            st = {k: h[k] for k in ("z", "lam", "rho", "phi")}
            continue
        flags = INIT_MERIT if s in (0, 5) else 0
        h = gpu_solve(pr, st, steps=1, al_iter=1, max_newton=1, flags=flags)
        tr = {}
        o = ref_solve(pr, st, al_iter=1, max_newton=1, flags=flags, trace=tr)
        assert (h["info"] == 0).all() and (h["status"] == 1).all() and (o["info"] == 0).all()
        g, d, phi = h["tr"]["g"][0], h["tr"]["d"][0], h["tr"]["phi"][0]
        g0 = g0 or float(np.abs(tr["g"][0]).max())
        eg, ed = scale_err(g, tr["g"][0], G_FLOOR[dtype] * g0), scale_err(d, tr["d"][0], 1e-5 * zs)
        pp_ref = tr["phi_prev"][0]
        scale = np.maximum(np.abs(tr["phi"][0]), np.abs(pp_ref)[None]) + 1
        ep = float((np.abs(phi - tr["phi"][0]) / scale).max())
        worst = dict(g=max(worst["g"], eg), d=max(worst["d"], ed), phi=max(worst["phi"], ep))
        print(f"XBOX step {s} ({nx},{nu}) T={T} B={B} {dtype}: g {eg:.2e} d {ed:.2e} phi {ep:.2e}")
        assert eg < 10 * rt, ("g", s, eg)
        assert ed < 100 * rt, ("d", s, ed)
        assert ep < pe, ("phi", s, ep)
        assert (np.abs(h["tr"]["phi_prev"][0] - pp_ref) <= pe * (np.abs(pp_ref) + 1)).all(), ("phi_prev", s)
        # the decision, judged in fp64 at the kernel's own candidates z + 2^-k d
        kg, ag = h["tr"]["k"][0], h["tr"]["accept"][0]
        z64, lam64, rho64 = (st[k].double().numpy() for k in ("z", "lam", "rho"))
        p64 = np.stack([_merit64(pr, z64 + 2.0 ** -k * d.astype(np.float64), lam64, rho64) for k in range(20)])
        bi = np.arange(B)
        tol = pe * (np.abs(p64).min(0) + np.abs(pp_ref) + 1)
        if dtype == "f64":
            # equal to the reference's choice wherever its two best merits are further apart than the tolerance on a
            # merit itself (past convergence d ~ 1e-16 and all 20 merits tie: there only the criterion below holds)
            srt = np.sort(tr["phi"][0], axis=0)
            decided = srt[1] - srt[0] > 2 * pe * (np.abs(srt[0]) + 1)
            assert np.array_equal(kg[decided], tr["k"][0][decided]), ("k", s, kg, tr["k"][0])
            n_decided += int(decided.sum())
        assert (p64[kg, bi] - p64.min(0) <= 2 * tol).all(), ("k", s, kg, p64.argmin(0))
        sure = np.abs(p64.min(0) - pp_ref) > 2 * tol
        assert np.array_equal(ag[sure], (p64.min(0) < pp_ref)[sure].astype(np.int32)), ("accept", s)
        # z <- z + accept 2^-k d, merit <- the minimum
        step = torch.from_numpy(np.where(ag > 0, 2.0 ** -kg.astype(np.float64), 0.0)).to(st["z"].dtype)[:, None, None]
        ulp = torch.finfo(st["z"].dtype).eps * (zs + float(np.abs(d).max()))   # (the kernel may fuse the multiply-add)
        assert (h["z"] - (st["z"] + step * torch.from_numpy(d))).abs().max() <= 2 * ulp
        assert np.array_equal(h["phi"].numpy(), phi[kg, bi])
        st = {k: h[k] for k in ("z", "lam", "rho", "phi")}
    assert dtype == "f32" or n_decided >= 2 * B   # the fp64 comparison of k is not vacuous
    print(f"XBOX step ({nx},{nu}) T={T} B={B} {dtype}: worst g {worst['g']:.2e} d {worst['d']:.2e} (of the largest), "
          f"phi {worst['phi']:.2e} (of |phi| + 1)")


# ---- full solve -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,nu,T,B,ps", SHAPES)
def test_full_solve_f64(nx, nu, T, B, ps):
    pr = _problem(nx, nu, T, B, "f64", ps)
    st = _state0(pr)
    h = gpu_solve(pr, st, al_iter=2, max_newton=4, flags=INIT_MERIT | DUAL_UPDATE)
    o = ref_solve(pr, st, al_iter=2, max_newton=4, flags=INIT_MERIT | DUAL_UPDATE)
    assert (h["info"] == 0).all() and (h["status"] == 1).all()
    ez, el = float((h["z"] - o["z"]).abs().max()), float((h["lam"] - o["lam"]).abs().max())
    _, lxu, lxl = sbr.split_lam(o["lam"].numpy(), T, nx, nu)
    print(f"XBOX full f64 ({nx},{nu}) T={T} B={B}: max |z - ref| {ez:.2e}, |lam - ref| {el:.2e} (all rows; largest state-row "
          f"multiplier {max(lxu.max(), lxl.max()):.3g})")
    assert lxu.max() > 0 and lxl.max() > 0
    assert ez < 1e-10 and el < 2e-9 and torch.equal(h["rho"], o["rho"])   # test_every_compiled_dims_vs_oracle's
    assert (h["rn2"] - o["rn2"]).abs().max() <= 1e-8 * max(1.0, float(o["rn2"].abs().max()))


def _smoke_rule(pr, h, o, label):
    """__graft_entry__.smoke()'s fp32 rule, the reference being `o`."""
    B = pr["dims"][0]
    err = (h["z"] - o["z"]).abs().reshape(B, -1).max(1)[0].numpy()
    out = err >= 2e-3
    print(f"XBOX full f32 {label}: median per-instance error {np.median(err):.2e}, {int(out.sum())}/{B} beyond 2e-3")
    assert np.median(err) < 1e-5 and out.sum() <= 6, np.sort(err)[-8:]
    f = lambda a: a.double().numpy()
    if out.any():
        assert np.isfinite(f(h["z"])[out]).all() and np.isfinite(f(h["lam"])[out]).all()
        pg, po = _merit64(pr, f(h["z"]), f(h["lam"]), f(h["rho"])), _merit64(pr, f(o["z"]), f(o["lam"]), f(o["rho"]))
        assert ((pg - po)[out] <= 1e-3 * (np.abs(po[out]) + 1)).all(), (pg - po)[out]
    return ~out


@pytest.mark.parametrize("nx,nu,T", [(8, 2, 10), (13, 4, 5)])
def test_full_solve_f32(nx, nu, T):
    pr = _problem(nx, nu, T, 64, "f32", seed=3)
    st = _state0(pr)
    h = gpu_solve(pr, st, al_iter=2, max_newton=4, flags=INIT_MERIT | DUAL_UPDATE)
    o = ref_solve(pr, st, al_iter=2, max_newton=4, flags=INIT_MERIT | DUAL_UPDATE)
    assert (h["status"] == 1).all()
    ok = _smoke_rule(pr, h, o, f"({nx},{nu}) T={T} B=64")
    _lam_rn2_rule(pr, h, o, ok, f"({nx},{nu})")


def _lam_rn2_rule(pr, h, o, ok, label):
    """lam (state rows included), rho and rn2 of the instances `ok` that took the reference's steps (_smoke_rule's mask)."""
    # A row's residual moves by at most cF = 1 + max row sum |F| times the error dz of z, lam = max(0, lam + rho r) is built with rho = 1 and 10, and
    # rn2 = sum of M squares r^2: |dlam| <= 11 cF dz, |drn2| <= 2 sqrt(M rn2) cF dz + M (cF dz)^2; dz is the instance's own
    # error of z (not below the 1e-5 the rule asks of the median), with a factor 2 for the first iteration's iterate
    B = pr["dims"][0]
    assert torch.equal(h["rho"], o["rho"])
    dz = 2 * np.maximum((h["z"] - o["z"]).abs().reshape(B, -1).max(1)[0].numpy(), 1e-5)
    cF = 1 + float(pr["F"].abs().sum(-1).max())
    M = h["lam"].shape[1]
    el = (h["lam"] - o["lam"]).abs().reshape(B, -1).max(1)[0].numpy()
    er = (h["rn2"] - o["rn2"]).abs().numpy()
    rn = o["rn2"].numpy().astype(np.float64)
    print(f"XBOX full f32 {label}: |lam - ref| median {np.median(el):.2e} max {el[ok].max():.2e}, worst share of its bound "
          f"{(el / (11 * cF * dz))[ok].max():.2f}; rn2 {(er / (2 * np.sqrt(M * rn) * cF * dz + M * (cF * dz) ** 2))[ok].max():.2f}")
    assert (el <= 11 * cF * dz)[ok].all()
    assert (er <= 2 * np.sqrt(M * rn) * cF * dz + M * (cF * dz) ** 2)[ok].all()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_inert_twin_vs_plain_team_kernel(dtype):
    """Bounds no state reaches (+-1e20, what MPC makes of +-inf) through the xbox kernel against the plain team kernel."""
    nx, nu, T, B = (8, 2, 10, 64) if dtype == "f32" else (13, 4, 3, 5)
    pr = _problem(nx, nu, T, B, dtype, seed=3)
    pr["xlo"], pr["xhi"] = torch.full((nx,), -1e20, dtype=TD[dtype]), torch.full((nx,), 1e20, dtype=TD[dtype])
    st = _state0(pr)
    kw = dict(al_iter=2, max_newton=4, flags=INIT_MERIT | DUAL_UPDATE)
    h = gpu_solve(pr, st, **kw)
    stp = dict(st, lam=torch.zeros(B, T * nx + 2 * T * nu, dtype=TD[dtype]))
    o = gpu_solve(pr, stp, plain=True, **kw)
    plain, lxu, lxl = sbr.split_lam(h["lam"].numpy(), T, nx, nu)
    assert not lxu.any() and not lxl.any()   # exactly 0
    bitwise = torch.equal(h["z"], o["z"]) and np.array_equal(plain, o["lam"].numpy()) and torch.equal(h["rn2"], o["rn2"])
    print(f"XBOX inert twin {dtype}: bitwise equal to the plain team kernel: {bitwise}")
    if dtype == "f64":
        ez, el = float((h["z"] - o["z"]).abs().max()), float(np.abs(plain - o["lam"].numpy()).max())
        print(f"XBOX inert twin f64: max |z - plain| {ez:.2e}, |lam - plain| {el:.2e}")
        assert ez < 1e-10 and el < 2e-9
    else:
        zero = np.zeros((B, T, nx), np.float32)
        _smoke_rule(pr, h, dict(o, lam=torch.from_numpy(sbr.join_lam(o["lam"].numpy(), zero, zero, T, nx, nu))),
                    "inert twin (8,2) T=10 B=64")


# ---- exit routes through MPC ----------------------------------------------------------------------------------------
class _Recording:
    """HipBackend with its solve_lin_xbox calls noted: (al_iter, max_newton, in-kernel exit asked, launched)."""

    def __init__(self, inner):
        self._i, self.log = inner, []

    def __getattr__(self, k):
        return getattr(self._i, k)

    def solve_lin_xbox(self, *a, **kw):
        ok = self._i.solve_lin_xbox(*a, **kw)
        self.log.append((kw.get("al_iter"), kw.get("max_newton"), "newton_counts" in kw, ok is not False))
        return ok

    def solve_lin(self, *a, **kw):
        raise AssertionError("the plain kernel was reached with state bounds")


def _mpc_solve(pr, be, dev, requires_grad=False, **kw):
    from deq_mpc_corl_amd import MPC, QuadCost
    from deq_mpc_corl_amd.qpth.al_utils import LinDx
    B, T, nx, nu = pr["dims"]
    d = lambda a: a.to(dev)
    mpc = MPC(nx, nu, T, u_lower=d(pr["lo"]), u_upper=d(pr["hi"]), n_batch=B, dtype=pr["z0"].dtype, backend=be,
              x_lower=d(pr["xlo"]), x_upper=d(pr["xhi"]), **kw)
    mpc.reinitialize(d(pr["x0"]), None)
    leaf = {k: d(pr[k]).clone().requires_grad_(requires_grad) for k in ("Qd", "q", "F", "c", "x0")}
    x, u, _ = mpc(leaf["x0"], QuadCost(torch.diag_embed(leaf["Qd"]), leaf["q"]), LinDx(leaf["F"], leaf["c"]), None,
                  x_init=d(pr["z0"][..., :nx]).clone(), u_init=d(pr["z0"][..., nx:]).clone())
    return mpc, x, u, leaf


@pytest.mark.parametrize("in_kernel", [True, False])
@pytest.mark.parametrize("nx,nu,T,B,ps", [(2, 1, 5, 5, True), (13, 4, 3, 2, False)])
def test_reference_exit_routes(nx, nu, T, B, ps, in_kernel):
    pr = _problem(nx, nu, T, B, "f64", ps)
    m0, x0, u0, _ = _mpc_solve(pr, sbr.XboxOracleBackend(), "cpu", exit_mode="reference")
    be = _Recording(_be())
    m1, x1, u1, _ = _mpc_solve(pr, be, DEV, exit_mode="reference", exit_in_kernel=in_kernel)
    torch.cuda.synchronize()
    if in_kernel:   # one cooperative launch for the whole solve
        assert be.log == [(2, 4, True, True)], be.log
    else:           # per AL iteration: starting merit, four one-step launches, dual update
        assert [c[:2] for c in be.log] == [(1, 0), (1, 1), (1, 1), (1, 1), (1, 1), (1, 0)] * 2 and not any(c[2] for c in be.log)
    assert list(m1.last_newton_per_al) == list(m0.last_newton_per_al)
    # x, u are returned as float32: 1e-6 is the bound tests/test_dense_cost_cpu.py puts on that cast; lam stays fp64
    dev_xu = max(float((x1.cpu() - x0).abs().max()), float((u1.cpu() - u0).abs().max()))
    el = float((m1.lamda_prev.cpu() - m0.lamda_prev).abs().max())
    print(f"XBOX exit ({nx},{nu}) in_kernel={in_kernel}: Newton counts {list(m1.last_newton_per_al)}, |x,u - ref| {dev_xu:.2e}, "
          f"|lam - ref| {el:.2e}")
    assert m1.lamda_prev.shape == (B, sbr.lam_width(T, nx, nu))
    assert dev_xu < 1e-6 and el < 2e-9
    assert torch.equal(m1.rho_prev.cpu(), m0.rho_prev)


# ---- saved factor and backward --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("nx,nu,T,B,ps", [(2, 1, 5, 5, True), (13, 4, 3, 2, False)])
def test_saved_factor_feeds_backward(nx, nu, T, B, ps, dtype):
    pr = _problem(nx, nu, T, B, dtype, ps)
    st = _state0(pr)
    kw = dict(al_iter=1, max_newton=4, flags=INIT_MERIT | DUAL_UPDATE | SAVE_FACTOR)
    h = gpu_solve(pr, st, want_factor=True, **kw)
    tr = {}
    ref_solve(pr, st, trace=tr, **{**kw, "flags": INIT_MERIT | DUAL_UPDATE})
    i = np.arange(nx)
    assert (tr["Hd"][..., i, i] > pr["Qd"].numpy()[..., :nx] + 1.5).any()   # state rows are on the last Hessian's diagonal
    dt = TD[dtype]
    gbar = torch.randn(B, T, nx + nu, generator=torch.Generator().manual_seed(1), dtype=torch.float64).to(dt)
    qg, Qg = Guarded((B, T, nx + nu), dt, DEV), Guarded((B, T, nx + nu), dt, DEV)
    _be().backward(pr["dims"], h["factor"], pr["F"].to(DEV), st["rho"].to(DEV), h["z"].to(DEV), gbar.to(DEV), qg.t, Qg.t)
    torch.cuda.synchronize()
    assert qg.intact() and Qg.intact()
    w_ref = dense_w(tr["Hd"].astype(np.float64), tr["Hs"].astype(np.float64), gbar.double().numpy())
    e = scale_err(qg.t.cpu().double().numpy(), w_ref, 1e-30)
    print(f"XBOX backward ({nx},{nu}) {dtype}: w vs the dense solve with the reference's last Hessian {e:.2e} (of the largest)")
    assert e < 100 * RT[dtype]   # a Newton solve like d


@pytest.mark.parametrize("exit_mode", ["fixed", "reference"])
def test_gradients_through_mpc(exit_mode):
    from tests.test_state_bounds_cpu import _WiringBackend
    pr = _problem(4, 2, 5, 5, "f64", True, seed=7)
    be = _Recording(_be())
    mpc, x, u, leaf = _mpc_solve(pr, be, DEV, requires_grad=True, exit_mode=exit_mode)
    gen = torch.Generator().manual_seed(5)
    gx, gu = torch.randn(x.shape, generator=gen), torch.randn(u.shape, generator=gen)
    ((x * gx.to(DEV)).sum() + (u * gu.to(DEV)).sum()).backward()
    torch.cuda.synchronize()
    assert be.log and all(c[3] for c in be.log)
    _, x0, u0, leaf0 = _mpc_solve(pr, _WiringBackend(), "cpu", requires_grad=True, exit_mode=exit_mode)
    ((x0 * gx).sum() + (u0 * gu).sum()).backward()
    for k in ("Qd", "q", "F", "c", "x0"):
        assert leaf[k].grad is not None and float(leaf[k].grad.abs().max()) > 0, k
        e = scale_err(leaf[k].grad.cpu().numpy(), leaf0[k].grad.numpy(), 1e-30)
        print(f"XBOX grad ({exit_mode}): d{k} vs the reference backend {e:.2e} (of the largest)")
        assert e < 100 * RT["f64"], (k, e)   # every one is a product of w, a Newton solve like d


# ---- bad arguments ---------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_without_a_launch():
    from deq_mpc_corl_amd import _lib
    be = _be()
    pr = _problem(2, 1, 3, 2, "f64")
    B, T, nx, nu = pr["dims"]
    dv = {k: pr[k].to(DEV).contiguous() for k in ("Qd", "q", "F", "c", "x0", "lo", "hi", "xlo", "xhi")}
    z = Guarded((B, T, nx + nu), torch.float64, DEV, init=pr["z0"])
    lam, rho, phi = (torch.zeros(B, sbr.lam_width(T, nx, nu), dtype=torch.float64, device=DEV),
                     torch.ones(B, dtype=torch.float64, device=DEV), torch.zeros(B, dtype=torch.float64, device=DEV))
    P = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(xlo, xhi, variant, dims=(B, T, nx, nu), max_newton=1):
        d = _lib.AlqpDims(*dims)
        p = _lib.AlqpParams(1, max_newton, 20, 3, 10.0, variant, None)
        return be.lib.alqp_solve_lin_xbox_f64(ctypes.byref(d), ctypes.byref(p), P(dv["Qd"]), P(dv["q"]), P(dv["F"]), P(dv["c"]),
                                              P(dv["x0"]), P(dv["lo"]), P(dv["hi"]), 0, 0, xlo, xhi, 0, 0, P(z.t), P(lam),
                                              P(rho), P(phi), None, None, None, None, None, None)
    ok = (P(dv["xlo"]), P(dv["xhi"]))
    assert call(None, ok[1], 0) == -1 and call(ok[0], None, 0) == -1      # ALQP_E_BADARG: null bounds
    assert call(*ok, 2) == -1                                             # the quad variant
    assert call(*ok, 0, max_newton=-1) == -1
    assert call(*ok, 0, dims=(B, T, 3, 1)) == -2                          # ALQP_E_UNSUPPORTED: no (3, 1) instance
    assert call(*ok, 0, dims=(B, 100000, nx, nu)) == -2                   # a horizon whose factor does not fit the LDS image
    assert call(*ok, 0, dims=(0, T, nx, nu)) == -1                        # an empty batch
    torch.cuda.synchronize()
    assert torch.equal(z.t.cpu(), pr["z0"]) and z.intact()   # nothing ran
    # a lam of the plain width, too few bounds for the strides: refused by the backend before the library is reached
    args = (pr["dims"], dv["Qd"], dv["q"], dv["F"], dv["c"], dv["x0"], dv["lo"], dv["hi"], 0, 0)
    with pytest.raises(ValueError, match="lam"):
        be.solve_lin_xbox(*args, dv["xlo"], dv["xhi"], 0, 0, z.t, lam[:, :T * nx + 2 * T * nu].contiguous(), rho, phi)
    with pytest.raises(ValueError, match="x_lower"):
        be.solve_lin_xbox(*args, dv["xlo"], dv["xhi"], T * nx, nx, z.t, lam, rho, phi)
    with pytest.raises(RuntimeError, match="bad argument"):
        be.solve_lin_xbox(*args, dv["xlo"], dv["xhi"], 0, 0, z.t, lam, rho, phi, variant="quad")
    torch.cuda.synchronize()
    assert torch.equal(z.t.cpu(), pr["z0"]) and z.intact()
    assert call(*ok, 1) == 0 and call(*ok, 0) == 0
    torch.cuda.synchronize()
    assert not torch.equal(z.t.cpu(), pr["z0"]) and z.intact()
