"""GPU tests of the fused solve with general rows G_t z_t <= h_t (k_solve_lin_gen<POLY> behind alqp_solve_lin_poly_*,
MPC(ineqG=, ineqh=)). The reference is tests/poly_rows_reference.py's backend (pinned on the CPU by
tests/test_poly_rows_cpu.py), fed the kernel's own inputs, in the kernel's dtype. Structure and tolerances are
tests/test_gpu_state_bounds.py's: RT, PHI_EPS, G_FLOOR and scale_err of tests/test_gpu_dense_cost.py, 1e-10 / 2e-9 on z / lam
of a full fp64 solve."""
import ctypes

import numpy as np
import pytest
import torch

from tests import poly_rows_reference as prr
from tests.aux_cases import Guarded
from tests.dense_cost_reference import dense_w
from tests.test_gpu_dense_cost import G_FLOOR, PHI_EPS, RT, _GuardedU8, scale_err

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TD = {"f64": torch.float64, "f32": torch.float32}
INIT_MERIT, DUAL_UPDATE, SAVE_FACTOR = 1, 2, 4
# (nx, nu, T, B, m, layout of G and h): four teams per wavefront, the second wavefront ragged (a padding team with b
# clamped); m above the team width 8 (two trips of the residual loop), one instance, every stride in use; m no multiple of
# 4 (the hand-over region's padding), stage strides alone, a unit row exactly on its boundary; whole-wavefront teams;
# the largest n; the workload's horizon, T m = 140: two trips and a tail of the strided loops; the sizes at which Cfg's
# padding vanishes: n = 8 and n = 16 (pad4(N) == N, no padding column behind a row of G), and nx = 4 (pad4(NX) == NX) with
# odd n = 5 and NROWS = 15, one lane short of the 16-lane team
SHAPES = [(2, 1, 2, 5, 1, "shared"), (2, 1, 5, 1, 9, "per_instance"), (8, 2, 4, 3, 5, "per_stage"), (13, 4, 3, 2, 3, "per_instance"),
          (14, 4, 3, 2, 2, "shared"), (13, 4, 20, 2, 7, "shared"), (6, 2, 3, 5, 5, "per_instance"), (12, 4, 3, 3, 5, "per_instance"),
          (4, 1, 3, 9, 3, "shared")]
ON_BOUND = (8, 2, 4, 3)   # the shape whose traced iterates start with a unit row exactly on its boundary
# The iterate the traced steps start from has no row within KINK_MARGIN of its kink other than the one put there on
# purpose (_after_one_al_iteration asserts it): on a kink the order of a dot product decides [r >= 0] and with it the
# whole step, and kernel and reference may then both be right and differ.
KINK_MARGIN = 1e-4


def _be():
    from deq_mpc_corl_amd.backend import default_backend
    return default_backend()


def _problem(nx, nu, T, B, m, layout, dtype, seed=5):
    # rows shared by every (b, t) bind only with small slacks and scaled-down state columns (poly_problem says why)
    kw = dict(slack=(0.005, 0.02), state_scale=0.1) if layout == "shared" else {}
    kw["u_cost"] = 0.1   # (poly_problem says why: the per-step comparison of d and phi needs a Hessian without a 1e-8 eigenvalue)
    return prr.poly_problem(B, T, nx, nu, m, TD[dtype], layout, seed=seed, on_boundary=(nx, nu, T, B) == ON_BOUND, **kw)


def _state0(pr):
    B, T, nx, nu = pr["dims"]
    dt = pr["z0"].dtype
    return dict(z=pr["z0"].clone(), lam=torch.zeros(B, prr.lam_width(T, nx, nu, pr["m"]), dtype=dt), rho=torch.ones(B, dtype=dt),
                phi=torch.zeros(B, dtype=dt))


def gpu_solve(pr, st, steps=0, want_factor=False, plain=False, **kw):
    """One alqp_solve_lin_poly launch (`plain`: alqp_solve_lin on the team kernel, the general rows cut out of lam) from
    the state `st` (CPU tensors; not modified). Every output is a slice out of a sentinel-filled tensor whose guard bands
    must survive. -> dict of CPU tensors (+ tr, factor on the device)."""
    be = _be()
    B, T, nx, nu = pr["dims"]
    n, m = nx + nu, pr["m"]
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
    sb, stt = (0, 0) if pr["lo"].dim() == 1 else (T * nu, nu)
    head = (pr["dims"], d(pr["Qd"]), d(pr["q"]), d(pr["F"]), d(pr["c"]), d(pr["x0"]), d(pr["lo"]), d(pr["hi"]), sb, stt)
    tail = (G["z"].t, G["lam"].t, G["rho"].t, G["phi"].t)
    okw = dict(rnorm2=G["rn2"].t, info=G["info"].t, status=G["status"].t)
    if plain:
        ok = be.solve_lin(*head, *tail, variant="team", **okw, **kw)
    else:
        ok = be.solve_lin_poly(*head, d(pr["G"]), d(pr["h"]), m, *prr.strides(pr["G"], pr["h"], T, m, n), *tail, **okw, **kw)
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
    return prr.run_solve(prr.PolyOracleBackend(), pr["Qd"], pr["q"], pr["F"], pr["c"], pr["x0"], pr["lo"], pr["hi"], pr["G"],
                         pr["h"], st["z"], st["lam"], st["rho"], st["phi"], **kw)


def _merit64(pr, z, lam, rho):
    """fp64 merit of the reference at (z, lam, rho) [B,...] numpy."""
    B, T, nx, nu = pr["dims"]
    m = pr["m"]
    f = lambda a: a.double().numpy()
    Gr = np.broadcast_to(f(pr["G"]), (B, T, m, nx + nu))
    hr = np.broadcast_to(f(pr["h"]), (B, T, m))
    ll, lp = prr.split_lam(lam, T, nx, nu, m)
    xn = np.einsum("btij,btj->bti", f(pr["F"]), z[:, :-1]) + f(pr["c"])
    return prr.merit_poly("f64", z, xn, f(pr["x0"]), ll, lp, rho, f(pr["Qd"]), f(pr["q"]), f(pr["lo"]), f(pr["hi"]), Gr, hr)[0]


def _after_one_al_iteration(pr, on_bound=False):
    """(z, lam, rho, phi) after one AL iteration of the reference from lam = 0, rho = 1: nonzero row multipliers, and
    (T m >= 2) in every instance a row violated and a row slack - checked here. `on_bound`: the first control of stage 1
    is then put exactly on the boundary of its unit row (the row counts in H, >= 0, and not in g, > 0)."""
    B, T, nx, nu = pr["dims"]
    m = pr["m"]
    o = ref_solve(pr, _state0(pr), al_iter=1, max_newton=4, flags=INIT_MERIT | DUAL_UPDATE)
    st = {k: o[k] for k in ("z", "lam", "rho", "phi")}
    if on_bound:
        st["z"][:, 1, nx] = pr["h"].expand(B, T, m)[:, 1, m - 1]
    r = prr.poly_residuals(pr, st["z"])
    # (two rows per instance, T m = 2, under one shared h cannot be asked to split in every instance: there, over the batch)
    per = lambda a: a.reshape(B, -1).any(1).all() if T * m >= 4 else a.any()
    assert per(r > 0) and per(r < 0), "generator: a violated and a slack row in every instance"
    assert not on_bound or (r[:, 1, m - 1] == 0).all()
    off = np.abs(r)
    if on_bound:
        off[:, 1, m - 1] = 1
    assert off.min() > KINK_MARGIN, ("generator: a row rests on its kink", off.min())
    _, lp = prr.split_lam(st["lam"].numpy(), T, nx, nu, m)
    assert per(lp > 0), "generator: nonzero row multipliers"
    return st


# ---- per Newton step ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("nx,nu,T,B,m,layout", SHAPES)
def test_every_newton_step_vs_reference(nx, nu, T, B, m, layout, dtype):
    """One-step launches with an AlqpTrace; before each, the reference takes the same step from the kernel's own
    (z, lam, rho, phi). From (lam, rho = 10) after one reference AL iteration: four steps, the dual update alone, three
    more at rho = 100."""
    pr = _problem(nx, nu, T, B, m, layout, dtype)
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
            el = float((h["lam"] - o["lam"]).abs().max())
            print(f"POLY dual update ({nx},{nu}) T={T} B={B} m={m} {dtype}: |lam - ref| {el:.2e} (largest {float(o['lam'].abs().max()):.3g})")
            assert el <= 10 * rt * max(1.0, float(o["lam"].abs().max()))
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
        print(f"POLY step {s} ({nx},{nu}) T={T} B={B} m={m} {dtype}: g {eg:.2e} d {ed:.2e} phi {ep:.2e}")
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
    print(f"POLY step ({nx},{nu}) T={T} B={B} m={m} {dtype}: worst g {worst['g']:.2e} d {worst['d']:.2e} (of the largest), "
          f"phi {worst['phi']:.2e} (of |phi| + 1)")


# ---- full solve -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,nu,T,B,m,layout", SHAPES)
def test_full_solve_f64(nx, nu, T, B, m, layout):
    pr = _problem(nx, nu, T, B, m, layout, "f64")
    st = _state0(pr)
    h = gpu_solve(pr, st, al_iter=2, max_newton=4, flags=INIT_MERIT | DUAL_UPDATE)
    o = ref_solve(pr, st, al_iter=2, max_newton=4, flags=INIT_MERIT | DUAL_UPDATE)
    assert (h["info"] == 0).all() and (h["status"] == 1).all()
    ez, el = float((h["z"] - o["z"]).abs().max()), float((h["lam"] - o["lam"]).abs().max())
    _, lp = prr.split_lam(o["lam"].numpy(), T, nx, nu, m)
    print(f"POLY full f64 ({nx},{nu}) T={T} B={B} m={m}: max |z - ref| {ez:.2e}, |lam - ref| {el:.2e} (all rows; largest row "
          f"multiplier {lp.max():.3g})")
    assert lp.max() > 0
    assert ez < 1e-10 and el < 2e-9 and torch.equal(h["rho"], o["rho"])   # test_every_compiled_dims_vs_oracle's
    assert (h["rn2"] - o["rn2"]).abs().max() <= 1e-8 * max(1.0, float(o["rn2"].abs().max()))


def _smoke_rule(pr, h, o, label):
    """__graft_entry__.smoke()'s fp32 rule, the reference being `o`."""
    B = pr["dims"][0]
    err = (h["z"] - o["z"]).abs().reshape(B, -1).max(1)[0].numpy()
    out = err >= 2e-3
    print(f"POLY full f32 {label}: median per-instance error {np.median(err):.2e}, {int(out.sum())}/{B} beyond 2e-3")
    assert np.median(err) < 1e-5 and out.sum() <= 6, np.sort(err)[-8:]
    f = lambda a: a.double().numpy()
    if out.any():
        assert np.isfinite(f(h["z"])[out]).all() and np.isfinite(f(h["lam"])[out]).all()
        pg, po = _merit64(pr, f(h["z"]), f(h["lam"]), f(h["rho"])), _merit64(pr, f(o["z"]), f(o["lam"]), f(o["rho"]))
        assert ((pg - po)[out] <= 1e-3 * (np.abs(po[out]) + 1)).all(), (pg - po)[out]
    return ~out


@pytest.mark.parametrize("nx,nu,T", [(8, 2, 10), (13, 4, 5)])
def test_full_solve_f32(nx, nu, T):
    m = 5
    pr = _problem(nx, nu, T, 64, m, "per_instance", "f32", seed=3)
    st = _state0(pr)
    h = gpu_solve(pr, st, al_iter=2, max_newton=4, flags=INIT_MERIT | DUAL_UPDATE)
    o = ref_solve(pr, st, al_iter=2, max_newton=4, flags=INIT_MERIT | DUAL_UPDATE)
    assert (h["status"] == 1).all()
    ok = _smoke_rule(pr, h, o, f"({nx},{nu}) T={T} B=64 m={m}")
    _lam_rn2_rule(pr, h, o, ok, f"({nx},{nu})")


def _lam_rn2_rule(pr, h, o, ok, label):
    """lam (general rows included), rho and rn2 of the instances `ok` that took the reference's steps (_smoke_rule's mask)."""
    # A row's residual moves by at most cF times the error dz of z, cF = the largest absolute row sum over the dynamics rows (1 + |F|) and the
    # general rows (|G|); lam = max(0, lam + rho r) is built with rho = 1 and 10, and rn2 = sum of M squares r^2:
    # |dlam| <= 11 cF dz, |drn2| <= 2 sqrt(M rn2) cF dz + M (cF dz)^2; dz is the instance's own error of z (not below the
    # 1e-5 the rule asks of the median), with a factor 2 for the first iteration's iterate
    B = pr["dims"][0]
    assert torch.equal(h["rho"], o["rho"])
    dz = 2 * np.maximum((h["z"] - o["z"]).abs().reshape(B, -1).max(1)[0].numpy(), 1e-5)
    cF = max(1 + float(pr["F"].abs().sum(-1).max()), float(pr["G"].abs().sum(-1).max()))
    M = h["lam"].shape[1]
    el = (h["lam"] - o["lam"]).abs().reshape(B, -1).max(1)[0].numpy()
    er = (h["rn2"] - o["rn2"]).abs().numpy()
    rn = o["rn2"].numpy().astype(np.float64)
    print(f"POLY full f32 {label}: |lam - ref| median {np.median(el):.2e} max {el[ok].max():.2e}, worst share of its bound "
          f"{(el / (11 * cF * dz))[ok].max():.2f}; rn2 {(er / (2 * np.sqrt(M * rn) * cF * dz + M * (cF * dz) ** 2))[ok].max():.2f}")
    assert (el <= 11 * cF * dz)[ok].all()
    assert (er <= 2 * np.sqrt(M * rn) * cF * dz + M * (cF * dz) ** 2)[ok].all()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_inert_rows_vs_plain_team_kernel_bitwise(dtype):
    """Right-hand sides no stage reaches (1e20, what MPC makes of +inf) through the poly kernel against the plain team
    kernel: every term the rows add is an exact zero (weight fma(rho, 0, 0), activity 0, merit fma(0, r, 0)), so z, the
    plain part of lam, rho, phi and rn2 are the same bits, and every row multiplier is exactly 0."""
    nx, nu, T, B, m = (8, 2, 10, 64, 5) if dtype == "f32" else (13, 4, 3, 5, 9)
    pr = _problem(nx, nu, T, B, m, "per_stage", dtype, seed=3)
    pr["h"] = torch.full((m,), 1e20, dtype=TD[dtype])
    st = _state0(pr)
    kw = dict(al_iter=2, max_newton=4, flags=INIT_MERIT | DUAL_UPDATE)
    h = gpu_solve(pr, st, **kw)
    stp = dict(st, lam=torch.zeros(B, T * nx + 2 * T * nu, dtype=TD[dtype]))
    o = gpu_solve(pr, stp, plain=True, **kw)
    plain, lp = prr.split_lam(h["lam"].numpy(), T, nx, nu, m)
    assert not lp.any()   # exactly 0
    ez, el = float((h["z"] - o["z"]).abs().max()), float(np.abs(plain - o["lam"].numpy()).max())
    print(f"POLY inert rows {dtype}: max |z - plain| {ez:.2e}, |lam - plain| {el:.2e}")
    assert torch.equal(h["z"], o["z"]) and np.array_equal(plain, o["lam"].numpy())
    assert torch.equal(h["rn2"], o["rn2"]) and torch.equal(h["phi"], o["phi"]) and torch.equal(h["rho"], o["rho"])


# ---- exit routes through MPC ----------------------------------------------------------------------------------------
class _Recording:
    """HipBackend with its solve_lin_poly calls noted: (al_iter, max_newton, in-kernel exit asked, launched)."""

    def __init__(self, inner):
        self._i, self.log = inner, []

    def __getattr__(self, k):
        return getattr(self._i, k)

    def solve_lin_poly(self, *a, **kw):
        ok = self._i.solve_lin_poly(*a, **kw)
        self.log.append((kw.get("al_iter"), kw.get("max_newton"), "newton_counts" in kw, ok is not False))
        return ok

    def solve_lin(self, *a, **kw):
        raise AssertionError("the plain kernel was reached with general rows")


def _mpc_solve(pr, be, dev, requires_grad=False, **kw):
    from deq_mpc_corl_amd import MPC, QuadCost
    from deq_mpc_corl_amd.qpth.al_utils import LinDx
    B, T, nx, nu = pr["dims"]
    d = lambda a: a.to(dev)
    leaf = {k: d(pr[k]).clone().requires_grad_(requires_grad) for k in ("Qd", "q", "F", "c", "x0", "h")}
    mpc = MPC(nx, nu, T, u_lower=d(pr["lo"]), u_upper=d(pr["hi"]), n_batch=B, dtype=pr["z0"].dtype, backend=be,
              ineqG=d(pr["G"]), ineqh=leaf["h"], **kw)
    mpc.reinitialize(d(pr["x0"]), None)
    x, u, _ = mpc(leaf["x0"], QuadCost(torch.diag_embed(leaf["Qd"]), leaf["q"]), LinDx(leaf["F"], leaf["c"]), None,
                  x_init=d(pr["z0"][..., :nx]).clone(), u_init=d(pr["z0"][..., nx:]).clone())
    return mpc, x, u, leaf


@pytest.mark.parametrize("in_kernel", [True, False])
@pytest.mark.parametrize("nx,nu,T,B,m,layout", [(2, 1, 5, 5, 9, "per_instance"), (13, 4, 3, 2, 3, "shared")])
def test_reference_exit_routes(nx, nu, T, B, m, layout, in_kernel):
    pr = _problem(nx, nu, T, B, m, layout, "f64")
    m0, x0, u0, _ = _mpc_solve(pr, prr.PolyOracleBackend(), "cpu", exit_mode="reference")
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
    print(f"POLY exit ({nx},{nu}) m={m} in_kernel={in_kernel}: Newton counts {list(m1.last_newton_per_al)}, |x,u - ref| {dev_xu:.2e}, "
          f"|lam - ref| {el:.2e}")
    assert m1.lamda_prev.shape == (B, prr.lam_width(T, nx, nu, m))
    assert dev_xu < 1e-6 and el < 2e-9
    assert torch.equal(m1.rho_prev.cpu(), m0.rho_prev)


# ---- saved factor and backward --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("nx,nu,T,B,m,layout", [(2, 1, 5, 5, 9, "per_instance"), (13, 4, 3, 2, 3, "shared")])
def test_saved_factor_feeds_backward(nx, nu, T, B, m, layout, dtype):
    pr = _problem(nx, nu, T, B, m, layout, dtype)
    st = _state0(pr)
    kw = dict(al_iter=1, max_newton=4, flags=INIT_MERIT | DUAL_UPDATE | SAVE_FACTOR)
    h = gpu_solve(pr, st, want_factor=True, **kw)
    tr = {}
    ref_solve(pr, st, trace=tr, **{**kw, "flags": INIT_MERIT | DUAL_UPDATE})
    # the rows are in the last Hessian: an off-diagonal entry between a state and a control, which nothing else fills
    assert (np.abs(tr["Hd"][..., :nx, nx:]) > 0).any()
    dt = TD[dtype]
    gbar = torch.randn(B, T, nx + nu, generator=torch.Generator().manual_seed(1), dtype=torch.float64).to(dt)
    qg, Qg = Guarded((B, T, nx + nu), dt, DEV), Guarded((B, T, nx + nu), dt, DEV)
    _be().backward(pr["dims"], h["factor"], pr["F"].to(DEV), st["rho"].to(DEV), h["z"].to(DEV), gbar.to(DEV), qg.t, Qg.t)
    torch.cuda.synchronize()
    assert qg.intact() and Qg.intact()
    w_ref = dense_w(tr["Hd"].astype(np.float64), tr["Hs"].astype(np.float64), gbar.double().numpy())
    e = scale_err(qg.t.cpu().double().numpy(), w_ref, 1e-30)
    print(f"POLY backward ({nx},{nu}) m={m} {dtype}: w vs the dense solve with the reference's last Hessian {e:.2e} (of the largest)")
    assert e < 100 * RT[dtype]   # a Newton solve like d


@pytest.mark.parametrize("exit_mode", ["fixed", "reference"])
@pytest.mark.parametrize("layout", ["shared", "per_instance"])
def test_gradients_through_mpc(exit_mode, layout):
    from tests.test_poly_rows_cpu import _WiringBackend
    pr = _problem(4, 2, 5, 5, 3, layout, "f64", seed=7)
    be = _Recording(_be())
    mpc, x, u, leaf = _mpc_solve(pr, be, DEV, requires_grad=True, exit_mode=exit_mode)
    gen = torch.Generator().manual_seed(5)
    gx, gu = torch.randn(x.shape, generator=gen), torch.randn(u.shape, generator=gen)
    ((x * gx.to(DEV)).sum() + (u * gu.to(DEV)).sum()).backward()
    torch.cuda.synchronize()
    assert be.log and all(c[3] for c in be.log)
    _, x0, u0, leaf0 = _mpc_solve(pr, _WiringBackend(), "cpu", requires_grad=True, exit_mode=exit_mode)
    ((x0 * gx).sum() + (u0 * gu).sum()).backward()
    assert leaf["h"].grad.shape == pr["h"].shape
    for k in ("Qd", "q", "F", "c", "x0", "h"):
        assert leaf[k].grad is not None and float(leaf[k].grad.abs().max()) > 0, k
        e = scale_err(leaf[k].grad.cpu().numpy(), leaf0[k].grad.numpy(), 1e-30)
        print(f"POLY grad ({exit_mode}, {layout}): d{k} vs the reference backend {e:.2e} (of the largest)")
        assert e < 100 * RT["f64"], (k, e)   # every one is a product of w, a Newton solve like d


# ---- bad arguments ---------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_without_a_launch():
    from deq_mpc_corl_amd import _lib
    be = _be()
    m = 2
    pr = _problem(2, 1, 3, 2, m, "shared", "f64")
    B, T, nx, nu = pr["dims"]
    n = nx + nu
    dv = {k: pr[k].to(DEV).contiguous() for k in ("Qd", "q", "F", "c", "x0", "lo", "hi", "G", "h")}
    z = Guarded((B, T, n), torch.float64, DEV, init=pr["z0"])
    lam, rho, phi = (torch.zeros(B, prr.lam_width(T, nx, nu, m), dtype=torch.float64, device=DEV),
                     torch.ones(B, dtype=torch.float64, device=DEV), torch.zeros(B, dtype=torch.float64, device=DEV))
    big = torch.zeros(65 * n, dtype=torch.float64, device=DEV)       # room for m = 65, should a refusal fail
    biglam = torch.zeros(B, prr.lam_width(T, nx, nu, 65), dtype=torch.float64, device=DEV)
    P = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(Gp, hp, variant, rows=m, dims=(B, T, nx, nu), max_newton=1, lm=lam):
        d = _lib.AlqpDims(*dims)
        p = _lib.AlqpParams(1, max_newton, 20, 3, 10.0, variant, None)
        return be.lib.alqp_solve_lin_poly_f64(ctypes.byref(d), ctypes.byref(p), P(dv["Qd"]), P(dv["q"]), P(dv["F"]), P(dv["c"]),
                                              P(dv["x0"]), P(dv["lo"]), P(dv["hi"]), 0, 0, Gp, hp, rows, 0, 0, 0, 0, P(z.t), P(lm),
                                              P(rho), P(phi), None, None, None, None, None, None)
    ok = (P(dv["G"]), P(dv["h"]))
    assert call(None, ok[1], 0) == -1 and call(ok[0], None, 0) == -1      # ALQP_E_BADARG: null G, null h
    assert call(*ok, 2) == -1                                             # the quad variant
    assert call(P(big), P(big), 0, rows=0, lm=biglam) == -1               # m = 0
    assert call(P(big), P(big), 0, rows=65, lm=biglam) == -1              # m = 65
    assert call(*ok, 0, max_newton=-1) == -1
    assert call(*ok, 0, dims=(B, T, 3, 1)) == -2                          # ALQP_E_UNSUPPORTED: no (3, 1) instance
    assert call(*ok, 0, dims=(B, 100000, nx, nu)) == -2                   # a horizon whose factor does not fit the LDS image
    assert call(*ok, 0, dims=(0, T, nx, nu)) == -1                        # an empty batch
    torch.cuda.synchronize()
    assert torch.equal(z.t.cpu(), pr["z0"]) and z.intact()   # nothing ran
    # a lam of the plain width, too few rows for the strides: refused by the backend before the library is reached
    args = (pr["dims"], dv["Qd"], dv["q"], dv["F"], dv["c"], dv["x0"], dv["lo"], dv["hi"], 0, 0)
    with pytest.raises(ValueError, match="lam"):
        be.solve_lin_poly(*args, dv["G"], dv["h"], m, 0, 0, 0, 0, z.t, lam[:, :T * nx + 2 * T * nu].contiguous(), rho, phi)
    with pytest.raises(ValueError, match="ineqG"):
        be.solve_lin_poly(*args, dv["G"], dv["h"], m, T * m * n, m * n, 0, 0, z.t, lam, rho, phi)
    with pytest.raises(ValueError, match="ineqh"):
        be.solve_lin_poly(*args, dv["G"], dv["h"], m, 0, 0, T * m, m, z.t, lam, rho, phi)
    with pytest.raises(RuntimeError, match="bad argument"):
        be.solve_lin_poly(*args, dv["G"], dv["h"], m, 0, 0, 0, 0, z.t, lam, rho, phi, variant="quad")
    torch.cuda.synchronize()
    assert torch.equal(z.t.cpu(), pr["z0"]) and z.intact()
    assert call(*ok, 1) == 0 and call(*ok, 0) == 0
    torch.cuda.synchronize()
    assert not torch.equal(z.t.cpu(), pr["z0"]) and z.intact()
