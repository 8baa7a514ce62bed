"""GPU tests of the fused solve with two or three of dense cost, state box and general rows together (k_solve_lin_gen
behind alqp_solve_lin_gen_*, MPC(diag_cost=False, x_lower=, x_upper=, ineqG=, ineqh=)). The reference is
tests/gen_rows_reference.py's backend (pinned on the CPU by tests/test_gen_rows_cpu.py), fed the kernel's own inputs, in
the kernel's dtype. Method and tolerances are those of tests/test_gpu_state_bounds.py / tests/test_gpu_poly_rows.py: RT,
PHI_EPS, G_FLOOR and scale_err of tests/test_gpu_dense_cost.py, 1e-10 / 2e-9 on z / lam of a full fp64 solve, the fp32
rule of __graft_entry__.smoke() at B = 64."""
import numpy as np
import pytest
import torch

from tests import gen_rows_reference as grr
from tests import poly_rows_reference as prr
from tests.aux_cases import Guarded
from tests.dense_cost_reference import dense_w
from tests.test_gpu_dense_cost import G_FLOOR, PHI_EPS, RT, _GuardedU8, scale_err

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TD = {"f64": torch.float64, "f32": torch.float32}
INIT_MERIT, DUAL_UPDATE, SAVE_FACTOR = 1, 2, 4
COMBOS = grr.COMBOS
# (nx, nu, T, B, m, layout of G and h, form of the box): m above the team width of 8, so the in-place trips loop, the
# shortest horizon with a dynamics row, a padding team; 15 of 16 lanes; pad4(N) == N twice; the register edge twice; the
# full horizon
SHAPES = [(2, 1, 2, 5, 9, "per_instance", "shared"), (4, 1, 3, 3, 1, "shared", "per_stage"), (6, 2, 3, 2, 3, "per_stage", "shared"),
          (12, 4, 3, 2, 2, "shared", "per_stage"), (13, 4, 3, 2, 3, "per_instance", "shared"), (14, 4, 3, 2, 2, "shared", "per_stage"),
          (13, 4, 20, 2, 7, "per_instance", "per_stage")]
ALL_DIMS = [(2, 1), (4, 1), (4, 2), (6, 1), (6, 2), (8, 2), (10, 3), (12, 4), (13, 4), (14, 4)]
KINK_MARGIN = 1e-4   # tests/test_gpu_poly_rows.py: no row of the traced steps' starting iterate rests on its kink


def _be():
    from deq_mpc_corl_amd.backend import default_backend
    return default_backend()


def _problem(nx, nu, T, B, m, layout, box, dtype, seed=5):
    # rows shared by every (b, t) bind only with small slacks and scaled-down state columns (poly_problem says why);
    # control cost 0.1: the per-step comparison of d and phi needs a Hessian without a 1e-8 eigenvalue
    kw = dict(slack=(0.005, 0.02), state_scale=0.1) if layout == "shared" else {}
    return grr.gen_problem(B, T, nx, nu, m, TD[dtype], layout, box=box, seed=seed, u_cost=0.1, **kw)


def _width(pr, combo):
    B, T, nx, nu = pr["dims"]
    return grr.lam_width(T, nx, nu, "x" in combo, pr["m"] if "p" in combo else 0)


def _state0(pr, combo):
    B = pr["dims"][0]
    dt = pr["z0"].dtype
    return dict(z=pr["z0"].clone(), lam=torch.zeros(B, _width(pr, combo), dtype=dt), rho=torch.ones(B, dtype=dt),
                phi=torch.zeros(B, dtype=dt))


def gpu_solve(pr, combo, st, steps=0, want_factor=False, single=None, **kw):
    """One alqp_solve_lin_gen launch of `combo` (`single` "d" / "x" / "p": that feature's own entry point instead) from the
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
    cost, q, xbnd, poly = grr.gen_args(pr, single or combo)
    xbnd = None if xbnd is None else (d(xbnd[0]), d(xbnd[1]), *xbnd[2:])
    poly = None if poly is None else (d(poly[0]), d(poly[1]), *poly[2:])
    sb, stt = (0, 0) if pr["lo"].dim() == 1 else (T * nu, nu)
    head = (pr["dims"], d(cost), d(q), d(pr["F"]), d(pr["c"]), d(pr["x0"]), d(pr["lo"]), d(pr["hi"]), sb, stt)
    tail = (G["z"].t, G["lam"].t, G["rho"].t, G["phi"].t)
    okw = dict(rnorm2=G["rn2"].t, info=G["info"].t, status=G["status"].t)
    if single == "d":
        ok = be.solve_lin_dense(*head, *tail, **okw, **kw)
    elif single == "x":
        ok = be.solve_lin_xbox(*head, *xbnd, *tail, **okw, **kw)
    elif single == "p":
        ok = be.solve_lin_poly(*head, *poly, *tail, **okw, **kw)
    else:
        ok = be.solve_lin_gen(*head, xbnd, poly, *tail, **okw, **kw)
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


def ref_solve(pr, combo, st, **kw):
    return grr.run_solve(grr.GenOracleBackend(), pr, combo, st["z"], st["lam"], st["rho"], st["phi"], **kw)


def _terms64(pr, combo):
    p64 = {k: (v.double() if torch.is_tensor(v) else v) for k, v in pr.items()}
    cost, q, xbnd, poly = grr.gen_args(p64, combo)
    return grr.gen_terms(pr["dims"], cost, q, p64["F"], p64["c"], p64["x0"], p64["lo"], p64["hi"], 0, 0, xbnd, poly, "f64")


def _merit64(pr, combo, z, lam, rho):
    """fp64 merit of the reference at (z, lam, rho) [B,...] numpy."""
    B, T, nx, nu = pr["dims"]
    return _terms64(pr, combo).merit(z, *grr.split_lam(lam, T, nx, nu, "x" in combo, pr["m"] if "p" in combo else 0), rho)[0]


def _residuals(pr, combo, z):
    """Residuals of every extra row of `combo` at z (numpy, flat per instance), state rows then general rows."""
    B, T, nx, nu = pr["dims"]
    parts = []
    if "x" in combo:
        x = z.numpy()[..., :nx]
        parts += [(x - pr["xhi"].numpy()).reshape(B, -1), (pr["xlo"].numpy() - x).reshape(B, -1)]
    if "p" in combo:
        parts.append(prr.poly_residuals(pr, z).reshape(B, -1))
    return parts


def _after_one_al_iteration(pr, combo):
    """(z, lam, rho, phi) after one AL iteration of the reference from lam = 0, rho = 1, so that box rows and general rows
    are active with nonzero multipliers - checked here, over the batch - and none rests on its kink."""
    B, T, nx, nu = pr["dims"]
    o = ref_solve(pr, combo, _state0(pr, combo), al_iter=1, max_newton=4, flags=INIT_MERIT | DUAL_UPDATE)
    st = {k: o[k] for k in ("z", "lam", "rho", "phi")}
    for r in _residuals(pr, combo, st["z"]):
        assert np.abs(r).min() > KINK_MARGIN, ("generator: a row rests on its kink", np.abs(r).min())
    _, lxu, lxl, lp = grr.split_lam(st["lam"].numpy(), T, nx, nu, "x" in combo, pr["m"] if "p" in combo else 0)
    if "x" in combo:
        assert (lxu > 0).any() or (lxl > 0).any(), "generator: nonzero state-row multipliers"
    if "p" in combo:
        assert (lp > 0).any(), "generator: nonzero general-row multipliers"
    return st


# ---- per Newton step ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("combo", COMBOS)
@pytest.mark.parametrize("nx,nu,T,B,m,layout,box", SHAPES)
def test_every_newton_step_vs_reference(nx, nu, T, B, m, layout, box, combo, dtype):
    """One-step launches with an AlqpTrace; before each, the reference takes the same step from the kernel's own
    (z, lam, rho, phi). From (lam, rho = 10) after one reference AL iteration: four steps, the dual update alone, three
    more at rho = 100."""
    pr = _problem(nx, nu, T, B, m, layout, box, dtype)
    st = _after_one_al_iteration(pr, combo)
    zs = float(pr["z0"].abs().max())
    rt, pe = RT[dtype], PHI_EPS[dtype]
    tag = f"GEN {combo} ({nx},{nu}) T={T} B={B} m={m} {dtype}"
    g0 = None
    worst = dict(g=0.0, d=0.0, phi=0.0)
    n_decided = 0
    for s in range(8):
        if s == 4:   # dual update alone
            h = gpu_solve(pr, combo, st, al_iter=1, max_newton=0, flags=DUAL_UPDATE)
            o = ref_solve(pr, combo, st, al_iter=1, max_newton=0, flags=DUAL_UPDATE)
            assert torch.equal(h["rho"], o["rho"])
            el = float((h["lam"] - o["lam"]).abs().max())
            print(f"{tag} dual update: |lam - ref| {el:.2e} (largest {float(o['lam'].abs().max()):.3g})")
            assert el <= 10 * rt * max(1.0, float(o["lam"].abs().max()))
            st = {k: h[k] for k in ("z", "lam", "rho", "phi")}
            continue
        flags = INIT_MERIT if s in (0, 5) else 0
        h = gpu_solve(pr, combo, st, steps=1, al_iter=1, max_newton=1, flags=flags)
        tr = {}
        o = ref_solve(pr, combo, st, al_iter=1, max_newton=1, flags=flags, trace=tr)
        assert (h["info"] == 0).all() and (h["status"] == 1).all() and (o["info"] == 0).all()
        g, d, phi = h["tr"]["g"][0], h["tr"]["d"][0], h["tr"]["phi"][0]
        g0 = g0 or float(np.abs(tr["g"][0]).max())
        eg, ed = scale_err(g, tr["g"][0], G_FLOOR[dtype] * g0), scale_err(d, tr["d"][0], 1e-5 * zs)
        pp_ref = tr["phi_prev"][0]
        scale = np.maximum(np.abs(tr["phi"][0]), np.abs(pp_ref)[None]) + 1
        ep = float((np.abs(phi - tr["phi"][0]) / scale).max())
        worst = dict(g=max(worst["g"], eg), d=max(worst["d"], ed), phi=max(worst["phi"], ep))
        print(f"{tag} step {s}: g {eg:.2e} d {ed:.2e} phi {ep:.2e}")
        assert eg < 10 * rt, ("g", s, eg)
        assert ed < 100 * rt, ("d", s, ed)
        assert ep < pe, ("phi", s, ep)
        assert (np.abs(h["tr"]["phi_prev"][0] - pp_ref) <= pe * (np.abs(pp_ref) + 1)).all(), ("phi_prev", s)
        # the decision, judged in fp64 at the kernel's own candidates z + 2^-k d
        kg, ag = h["tr"]["k"][0], h["tr"]["accept"][0]
        z64, lam64, rho64 = (st[k].double().numpy() for k in ("z", "lam", "rho"))
        p64 = np.stack([_merit64(pr, combo, z64 + 2.0 ** -k * d.astype(np.float64), lam64, rho64) for k in range(20)])
        bi = np.arange(B)
        tol = pe * (np.abs(p64).min(0) + np.abs(pp_ref) + 1)
        if dtype == "f64":
            # equal to the reference's choice wherever its two best merits are further apart than the merit tolerance
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
    print(f"{tag}: worst g {worst['g']:.2e} d {worst['d']:.2e} (of the largest), phi {worst['phi']:.2e} (of |phi| + 1)")


# ---- full solves at all ten compiled sizes ----------------------------------------------------------------------------
def _full_shape(nx, nu):
    """Small full-solve shape per compiled size: T 4 (3 at the largest sizes), a ragged last wavefront where teams share one."""
    return (3 if nx >= 12 else 4), 3, 3


@pytest.mark.parametrize("combo", COMBOS)
@pytest.mark.parametrize("nx,nu", ALL_DIMS)
def test_full_solve_f64(nx, nu, combo):
    T, B, m = _full_shape(nx, nu)
    pr = _problem(nx, nu, T, B, m, "per_instance", "per_stage", "f64")
    st = _state0(pr, combo)
    kw = dict(al_iter=2, max_newton=4, flags=INIT_MERIT | DUAL_UPDATE)
    h = gpu_solve(pr, combo, st, **kw)
    o = ref_solve(pr, combo, st, **kw)
    assert (h["info"] == 0).all() and (h["status"] == 1).all()
    ez, el = float((h["z"] - o["z"]).abs().max()), float((h["lam"] - o["lam"]).abs().max())
    extra = o["lam"][:, T * nx:].reshape(B, T, -1)[..., 2 * nu:]
    print(f"GEN full f64 {combo} ({nx},{nu}) T={T} B={B} m={m}: max |z - ref| {ez:.2e}, |lam - ref| {el:.2e} (all rows; largest "
          f"extra multiplier {float(extra.max()) if extra.numel() else 0:.3g})")
    assert extra.max() > 0
    assert ez < 1e-10 and el < 2e-9 and torch.equal(h["rho"], o["rho"])   # test_every_compiled_dims_vs_oracle's
    assert (h["rn2"] - o["rn2"]).abs().max() <= 1e-8 * max(1.0, float(o["rn2"].abs().max()))


@pytest.mark.parametrize("combo", COMBOS)
@pytest.mark.parametrize("nx,nu", ALL_DIMS)
def test_full_solve_f32(nx, nu, combo):
    """B = 64 and the existing rule: median and count beyond 2e-3 on z, lam against each instance's own bound."""
    T, _, m = _full_shape(nx, nu)
    B = 64
    pr = _problem(nx, nu, T, B, m, "per_instance", "per_stage", "f32", seed=3)
    st = _state0(pr, combo)
    kw = dict(al_iter=2, max_newton=4, flags=INIT_MERIT | DUAL_UPDATE)
    h = gpu_solve(pr, combo, st, **kw)
    o = ref_solve(pr, combo, st, **kw)
    assert (h["status"] == 1).all()
    label = f"{combo} ({nx},{nu}) T={T} B={B} m={m}"
    err = (h["z"] - o["z"]).abs().reshape(B, -1).max(1)[0].numpy()
    out = err >= 2e-3
    print(f"GEN full f32 {label}: median per-instance error {np.median(err):.2e}, {int(out.sum())}/{B} beyond 2e-3")
    assert np.median(err) < 1e-5 and out.sum() <= 6, np.sort(err)[-8:]
    f = lambda a: a.double().numpy()
    if out.any():
        assert np.isfinite(f(h["z"])[out]).all() and np.isfinite(f(h["lam"])[out]).all()
        pg, po = (_merit64(pr, combo, f(v["z"]), f(v["lam"]), f(v["rho"])) for v in (h, o))
        assert ((pg - po)[out] <= 1e-3 * (np.abs(po[out]) + 1)).all(), (pg - po)[out]
    ok = ~out
    # tests/test_gpu_poly_rows.py:_lam_rn2_rule, with the state rows' unit row sum among the row sums
    assert torch.equal(h["rho"], o["rho"])
    dz = 2 * np.maximum(err, 1e-5)
    cF = max(1 + float(pr["F"].abs().sum(-1).max()), float(pr["G"].abs().sum(-1).max()) if "p" in combo else 1.0)
    M = h["lam"].shape[1]
    el = (h["lam"] - o["lam"]).abs().reshape(B, -1).max(1)[0].numpy()
    er = (h["rn2"] - o["rn2"]).abs().numpy()
    rn = o["rn2"].numpy().astype(np.float64)
    bound_r = 2 * np.sqrt(M * rn) * cF * dz + M * (cF * dz) ** 2
    print(f"GEN full f32 {label}: |lam - ref| median {np.median(el):.2e} max {el[ok].max():.2e}, worst share of its bound "
          f"{(el / (11 * cF * dz))[ok].max():.2f}; rn2 {(er / bound_r)[ok].max():.2f}")
    assert (el <= 11 * cF * dz)[ok].all()
    assert (er <= bound_r)[ok].all()


# ---- inert twins, bitwise -----------------------------------------------------------------------------------------
# (combination, what is made inert in it, the single-feature kernel it must then equal)
TWINS = [("dxp", "xp", "d"), ("xp", "p", "x"), ("xp", "x", "p"), ("dx", "x", "d"), ("dp", "p", "d")]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("combo,inert,single", TWINS)
def test_inert_twins_bitwise(combo, inert, single, dtype):
    """Bounds and right-hand sides no stage reaches (1e20, what MPC makes of an infinity) through the combined kernel
    against the single-feature kernel: every term the inert rows add is an exact zero, so z, the shared rows of lam, rho,
    phi and rn2 are the same bits, and every inert multiplier is exactly 0."""
    nx, nu, T, B, m = (8, 2, 10, 64, 5) if dtype == "f32" else (13, 4, 3, 5, 9)
    pr = _problem(nx, nu, T, B, m, "per_stage", "per_stage", dtype, seed=3)
    if "x" in inert:
        pr["xlo"], pr["xhi"] = torch.full((nx,), -1e20, dtype=TD[dtype]), torch.full((nx,), 1e20, dtype=TD[dtype])
    if "p" in inert:
        pr["h"] = torch.full((m,), 1e20, dtype=TD[dtype])
    kw = dict(al_iter=2, max_newton=4, flags=INIT_MERIT | DUAL_UPDATE)
    h = gpu_solve(pr, combo, _state0(pr, combo), **kw)
    o = gpu_solve(pr, combo, _state0(pr, single), single=single, **kw)
    plain, lxu, lxl, lp = grr.split_lam(h["lam"].numpy(), T, nx, nu, "x" in combo, m if "p" in combo else 0)
    if "x" in inert:
        assert not lxu.any() and not lxl.any()   # exactly 0
    if "p" in inert:
        assert not lp.any()
    shared = grr.join_lam(plain, lxu if single == "x" else None, lxl if single == "x" else None, lp if single == "p" else None,
                          T, nx, nu)
    ez, el = float((h["z"] - o["z"]).abs().max()), float(np.abs(shared - o["lam"].numpy()).max())
    print(f"GEN inert twin {combo} with {inert} inert vs {single} {dtype}: max |z - twin| {ez:.2e}, |lam - twin| {el:.2e}")
    assert torch.equal(h["z"], o["z"]) and np.array_equal(shared, o["lam"].numpy())
    assert torch.equal(h["rn2"], o["rn2"]) and torch.equal(h["phi"], o["phi"]) and torch.equal(h["rho"], o["rho"])


# ---- exit routes through MPC ----------------------------------------------------------------------------------------
class _Recording:
    """HipBackend with its solve_lin_gen calls noted: (al_iter, max_newton, in-kernel exit asked, launched)."""

    def __init__(self, inner):
        self._i, self.log = inner, []

    def __getattr__(self, k):
        return getattr(self._i, k)

    def solve_lin_gen(self, *a, **kw):
        ok = self._i.solve_lin_gen(*a, **kw)
        self.log.append((kw.get("al_iter"), kw.get("max_newton"), "newton_counts" in kw, ok is not False))
        return ok

    def _other(self, *a, **kw):
        raise AssertionError("another solve entry point was reached with a combination")

    solve_lin = solve_lin_dense = solve_lin_xbox = solve_lin_poly = _other


def _mpc_solve(pr, be, dev, requires_grad=False, **kw):
    from deq_mpc_corl_amd import MPC, QuadCost
    from deq_mpc_corl_amd.qpth.al_utils import LinDx
    B, T, nx, nu = pr["dims"]
    d = lambda a: a.to(dev)
    src = {"C": "C", "q": "qC", "F": "F", "c": "c", "x0": "x0", "h": "h"}
    leaf = {k: d(pr[v]).clone().requires_grad_(requires_grad) for k, v in src.items()}
    mpc = MPC(nx, nu, T, u_lower=d(pr["lo"]), u_upper=d(pr["hi"]), n_batch=B, dtype=pr["z0"].dtype, backend=be, diag_cost=False,
              x_lower=d(pr["xlo"]), x_upper=d(pr["xhi"]), ineqG=d(pr["G"]), ineqh=leaf["h"], **kw)
    mpc.reinitialize(d(pr["x0"]), None)
    x, u, _ = mpc(leaf["x0"], QuadCost(leaf["C"], leaf["q"]), LinDx(leaf["F"], leaf["c"]), None,
                  x_init=d(pr["z0"][..., :nx]).clone(), u_init=d(pr["z0"][..., nx:]).clone())
    return mpc, x, u, leaf


@pytest.mark.parametrize("in_kernel", [True, False])
@pytest.mark.parametrize("nx,nu,T,B,m,layout,box", [(2, 1, 5, 5, 9, "per_instance", "shared"), (13, 4, 3, 2, 3, "shared", "per_stage")])
def test_reference_exit_routes(nx, nu, T, B, m, layout, box, in_kernel):
    pr = _problem(nx, nu, T, B, m, layout, box, "f64")
    m0, x0, u0, _ = _mpc_solve(pr, grr.GenOracleBackend(), "cpu", exit_mode="reference")
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
    print(f"GEN exit dxp ({nx},{nu}) m={m} in_kernel={in_kernel}: Newton counts {list(m1.last_newton_per_al)}, |x,u - ref| "
          f"{dev_xu:.2e}, |lam - ref| {el:.2e}")
    assert m1.lamda_prev.shape == (B, grr.lam_width(T, nx, nu, True, m))
    assert dev_xu < 1e-6 and el < 2e-9
    assert torch.equal(m1.rho_prev.cpu(), m0.rho_prev)


# ---- saved factor and backward --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("combo", COMBOS)
@pytest.mark.parametrize("nx,nu,T,B,m,layout,box", [(2, 1, 5, 5, 9, "per_instance", "shared"), (13, 4, 3, 2, 3, "shared", "per_stage")])
def test_saved_factor_feeds_backward(nx, nu, T, B, m, layout, box, combo, dtype):
    pr = _problem(nx, nu, T, B, m, layout, box, dtype)
    st = _state0(pr, combo)
    kw = dict(al_iter=1, max_newton=4, flags=INIT_MERIT | DUAL_UPDATE | SAVE_FACTOR)
    h = gpu_solve(pr, combo, st, want_factor=True, **kw)
    tr = {}
    ref_solve(pr, combo, st, trace=tr, **{**kw, "flags": INIT_MERIT | DUAL_UPDATE})
    dt = TD[dtype]
    gbar = torch.randn(B, T, nx + nu, generator=torch.Generator().manual_seed(1), dtype=torch.float64).to(dt)
    qg, Qg = Guarded((B, T, nx + nu), dt, DEV), Guarded((B, T, nx + nu), dt, DEV)
    _be().backward(pr["dims"], h["factor"], pr["F"].to(DEV), st["rho"].to(DEV), h["z"].to(DEV), gbar.to(DEV), qg.t, Qg.t)
    torch.cuda.synchronize()
    assert qg.intact() and Qg.intact()
    w_ref = dense_w(tr["Hd"].astype(np.float64), tr["Hs"].astype(np.float64), gbar.double().numpy())
    e = scale_err(qg.t.cpu().double().numpy(), w_ref, 1e-30)
    print(f"GEN backward {combo} ({nx},{nu}) m={m} {dtype}: w vs the dense solve with the reference's last Hessian {e:.2e} (of the largest)")
    assert e < 100 * RT[dtype]   # a Newton solve like d


@pytest.mark.parametrize("exit_mode", ["fixed", "reference"])
@pytest.mark.parametrize("layout", ["shared", "per_instance"])
def test_gradients_through_mpc(exit_mode, layout):
    from tests.test_gen_rows_cpu import _WiringBackend
    pr = _problem(4, 2, 5, 5, 3, layout, "per_stage", "f64", seed=7)
    be = _Recording(_be())
    mpc, x, u, leaf = _mpc_solve(pr, be, DEV, requires_grad=True, exit_mode=exit_mode)
    gen = torch.Generator().manual_seed(5)
    gx, gu = torch.randn(x.shape, generator=gen), torch.randn(u.shape, generator=gen)
    ((x * gx.to(DEV)).sum() + (u * gu.to(DEV)).sum()).backward()
    torch.cuda.synchronize()
    assert be.log and all(c[3] for c in be.log)
    _, x0, u0, leaf0 = _mpc_solve(pr, _WiringBackend(), "cpu", requires_grad=True, exit_mode=exit_mode)
    ((x0 * gx).sum() + (u0 * gu).sum()).backward()
    assert leaf["h"].grad.shape == pr["h"].shape and leaf["C"].grad.shape == pr["C"].shape
    for k in ("C", "q", "F", "c", "x0", "h"):
        assert leaf[k].grad is not None and float(leaf[k].grad.abs().max()) > 0, k
        e = scale_err(leaf[k].grad.cpu().numpy(), leaf0[k].grad.numpy(), 1e-30)
        print(f"GEN grad dxp ({exit_mode}, {layout}): d{k} vs the reference backend {e:.2e} (of the largest)")
        assert e < 100 * RT["f64"], (k, e)   # every one is a product of w, a Newton solve like d


# ---- bad arguments ---------------------------------------------------------------------------------------------------
def test_backend_refuses_short_arguments_without_a_launch():
    be = _be()
    pr = _problem(2, 1, 3, 2, 2, "shared", "shared", "f64")
    B, T, nx, nu = pr["dims"]
    n, m = nx + nu, pr["m"]
    d = lambda a: a.to(DEV).contiguous()
    z = Guarded((B, T, n), torch.float64, DEV, init=pr["z0"])
    lam = torch.zeros(B, grr.lam_width(T, nx, nu, True, m), dtype=torch.float64, device=DEV)
    rho, phi = torch.ones(B, dtype=torch.float64, device=DEV), torch.zeros(B, dtype=torch.float64, device=DEV)
    head = (pr["dims"], d(pr["C"]), d(pr["qC"]), d(pr["F"]), d(pr["c"]), d(pr["x0"]), d(pr["lo"]), d(pr["hi"]), 0, 0)
    xb, pl = (d(pr["xlo"]), d(pr["xhi"]), 0, 0), (d(pr["G"]), d(pr["h"]), m, 0, 0, 0, 0)
    with pytest.raises(ValueError, match="lam"):   # the width of box + rows handed to all three... one short
        be.solve_lin_gen(*head, xb, pl, z.t, lam[:, :-1].contiguous(), rho, phi)
    with pytest.raises(ValueError, match="x_lower"):
        be.solve_lin_gen(*head, (xb[0], xb[1], T * nx, nx), pl, z.t, lam, rho, phi)
    with pytest.raises(ValueError, match="ineqG"):
        be.solve_lin_gen(*head, xb, (pl[0], pl[1], m, T * m * n, m * n, 0, 0), z.t, lam, rho, phi)
    with pytest.raises(ValueError, match="ineqh"):
        be.solve_lin_gen(*head, xb, (pl[0], pl[1], m, 0, 0, T * m, m), z.t, lam, rho, phi)
    with pytest.raises(RuntimeError, match="bad argument"):
        be.solve_lin_gen(*head, xb, pl, z.t, lam, rho, phi, variant="quad")
    with pytest.raises(RuntimeError, match="bad argument"):   # one feature alone
        be.solve_lin_gen(*head, None, None, z.t, lam, rho, phi)
    torch.cuda.synchronize()
    assert torch.equal(z.t.cpu(), pr["z0"]) and z.intact()   # nothing ran
    assert be.solve_lin_gen(*head, xb, pl, z.t, lam, rho, phi, al_iter=1, max_newton=1) is True
    torch.cuda.synchronize()
    assert not torch.equal(z.t.cpu(), pr["z0"]) and z.intact()
