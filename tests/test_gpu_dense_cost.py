"""GPU tests of the dense-cost fused solve (k_solve_lin_gen<DENSE> behind alqp_solve_lin_dense_*, MPC(diag_cost=False)).
The reference is tests/dense_cost_reference.py's backend (pinned on the CPU by tests/test_dense_cost_cpu.py), fed the
kernel's own inputs, in the kernel's dtype. Tolerances are those tests/test_gpu_parity.py applies to the plain team
kernel for the same quantities (RT, and 1e-10 / 2e-9 on z / lam of a full fp64 solve)."""
import ctypes

import numpy as np
import pytest
import torch

from tests.aux_cases import PAD, Guarded
from tests.dense_cost_reference import DenseOracleBackend, dense_w, run_solve, split_cost

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TD = {"f64": torch.float64, "f32": torch.float32}
RT = {"f64": 1e-8, "f32": 3e-4}            # test_fused_solve_vs_oracle: g within 10 RT, d within 100 RT (of the largest)
PHI_EPS = {"f64": 1e-10, "f32": 3e-5}      # its resolution of a merit, relative to |phi| + 1
# Floor under max |g| in the relative error of g, in units of g0 = max |g| of the first step. test_fused_solve_vs_oracle
# has 1e-5 for both dtypes. Kept in fp64. In fp32 it cannot hold here: from the third Newton step on these problems are
# stationary, |g| = 4e-7 .. 1e-4 (CPU run of the reference) is what is left when terms of size g0 = 3 .. 8 cancel, and
# 10 RT of a 1e-5 g0 floor is 3e-8 g0 - a quarter of an fp32 ulp of those terms. Two fp32 evaluations in different
# summation orders differ by more (measured: 3.4e-7 at g0 = 5.2, 0.55 ulp), and the order of the reference (the
# oracle's gradient, then offdiag(C) z on top) is set by how it is built, it is not the kernel's row dot product. The
# plain kernel meets 1e-5 because the oracle repeats its operation order. 1e-3: 10 RT of it is 3e-6 g0 = 25 ulps, the
# rounding of a 17-term dot product with a margin of 3; on every step with |g| >= 1e-3 g0 the floor is inactive.
G_FLOOR = {"f64": 1e-5, "f32": 1e-3}
INIT_MERIT, DUAL_UPDATE, SAVE_FACTOR = 1, 2, 4
# (nx, nu, T, B, bounds per (b, t)): four teams per wavefront + a ragged second wavefront + one dynamics stage; one
# instance; two teams per wavefront, ragged; n = 17 (odd row length, whole-wavefront team); the largest n; strided bounds;
# the sizes at which Cfg's padding vanishes: n = 8 and n = 16 (pad4(N) == N, no padding column behind a row), and nx = 4
# (pad4(NX) == NX) with odd n = 5 and NROWS = 15, one lane short of the 16-lane team
SHAPES = [(2, 1, 2, 5, False), (2, 1, 5, 1, False), (8, 2, 4, 3, False), (13, 4, 3, 2, False), (14, 4, 3, 2, False),
          (13, 4, 3, 2, True), (6, 2, 3, 5, False), (12, 4, 3, 3, False), (4, 1, 3, 9, False)]


class _GuardedU8:
    """tests/aux_cases.Guarded for the uint8 status array (its sentinel does not fit a byte)."""

    def __init__(self, numel, device, init):
        self.buf = torch.full((PAD + numel + PAD,), 0xA5, dtype=torch.uint8, device=device)
        self.t = self.buf[PAD:PAD + numel]
        self.t.copy_(init)

    def intact(self):
        return bool((self.buf[:PAD] == 0xA5).all()) and bool((self.buf[-PAD:] == 0xA5).all())


def _be():
    from deq_mpc_corl_amd.backend import default_backend
    return default_backend()


def _problem(nx, nu, T, B, dtype, bt_bounds=False, seed=5, diagonal=False):
    """CPU tensors of a synthetic problem with a dense cost (or, `diagonal`, the plain one's diag_embed)."""
    from deq_mpc_corl_amd import synthetic_dense_cost, synthetic_problem
    dt = TD[dtype]
    p = synthetic_problem(B, T, nx, nu, seed=seed, dtype=dt, active=True)
    C, q = (torch.diag_embed(p.Qd), p.q) if diagonal else synthetic_dense_cost(p, 1)
    lo, hi = p.u_lo, p.u_hi
    if bt_bounds:
        w = 1.0 + 0.5 * torch.rand(B, T, nu, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).to(dt)
        lo, hi = (-0.1 * w).contiguous(), (0.1 * w.flip(0)).contiguous()
    return dict(C=C, q=q, F=p.F, c=p.c, x0=p.x0, lo=lo, hi=hi, z0=p.z0, Qd=p.Qd, dims=(B, T, nx, nu))


def _state0(pr):
    B, T, nx, nu = pr["dims"]
    dt = pr["z0"].dtype
    return dict(z=pr["z0"].clone(), lam=torch.zeros(B, T * nx + 2 * T * nu, dtype=dt), rho=torch.ones(B, dtype=dt),
                phi=torch.zeros(B, dtype=dt))


def gpu_solve(pr, st, steps=0, want_factor=False, solve=None, **kw):
    """One alqp_solve_lin_dense launch from the state `st` (CPU tensors; not modified). Every output is a slice out of
    a sentinel-filled tensor whose guard bands must survive. -> dict of CPU tensors (+ tr, factor on the device)."""
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
    sb, stt = (0, 0) if pr["lo"].dim() == 1 else (T * nu, nu)
    solve = solve or be.solve_lin_dense
    cost = pr["C"] if solve == be.solve_lin_dense else pr["Qd"]
    ok = solve(pr["dims"], d(cost), d(pr["q"]), d(pr["F"]), d(pr["c"]), d(pr["x0"]), d(pr["lo"]), d(pr["hi"]), sb, stt,
               G["z"].t, G["lam"].t, G["rho"].t, G["phi"].t, rnorm2=G["rn2"].t, info=G["info"].t, status=G["status"].t,
               **kw)
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
    return run_solve(DenseOracleBackend(), pr["C"], pr["q"], pr["F"], pr["c"], pr["x0"], pr["lo"], pr["hi"], st["z"],
                     st["lam"], st["rho"], st["phi"], **kw)


def scale_err(a, b, floor):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), floor))


def _merit64(pr, z, lam, rho):
    """fp64 merit of the reference at (z, lam, rho) [B,...] numpy."""
    f = lambda a: a.double().numpy()
    Cd, off = split_cost(f(pr["C"]))
    xn = np.einsum("btij,btj->bti", f(pr["F"]), z[:, :-1]) + f(pr["c"])
    return DenseOracleBackend.merit_dense("f64", z, xn, f(pr["x0"]), lam, rho, Cd, off, f(pr["q"]), f(pr["lo"]), f(pr["hi"]))[0]


# ---- per Newton step ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("nx,nu,T,B,bt", SHAPES)
def test_every_newton_step_vs_reference(nx, nu, T, B, bt, dtype):
    """One-step launches with an AlqpTrace; before each, the reference takes the same step from the kernel's own
    (z, lam, rho, phi). Four steps at rho = 1, the dual update, three more at rho = 10."""
    pr = _problem(nx, nu, T, B, dtype, bt)
    st = _state0(pr)
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
    print(f"DENSE step ({nx},{nu}) T={T} B={B} {dtype}: worst g {worst['g']:.2e} d {worst['d']:.2e} (of the largest), "
          f"phi {worst['phi']:.2e} (of |phi| + 1)")


# ---- full solve -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,nu,T,B,bt", SHAPES)
def test_full_solve_f64(nx, nu, T, B, bt):
    pr = _problem(nx, nu, T, B, "f64", bt)
    st = _state0(pr)
    h = gpu_solve(pr, st, al_iter=2, max_newton=4, flags=INIT_MERIT | DUAL_UPDATE)
    o = ref_solve(pr, st, al_iter=2, max_newton=4, flags=INIT_MERIT | DUAL_UPDATE)
    assert (h["info"] == 0).all() and (h["status"] == 1).all()
    ez, el = float((h["z"] - o["z"]).abs().max()), float((h["lam"] - o["lam"]).abs().max())
    print(f"DENSE full f64 ({nx},{nu}) T={T} B={B}: max |z - ref| {ez:.2e}, |lam - ref| {el:.2e}")
    assert ez < 1e-10 and el < 2e-9 and torch.equal(h["rho"], o["rho"])   # test_every_compiled_dims_vs_oracle's
    assert (h["rn2"] - o["rn2"]).abs().max() <= 1e-8 * max(1.0, float(o["rn2"].abs().max()))


def _smoke_rule(pr, h, o, label):
    """__graft_entry__.smoke()'s fp32 rule, the reference being `o`."""
    B = pr["dims"][0]
    err = (h["z"] - o["z"]).abs().reshape(B, -1).max(1)[0].numpy()
    out = err >= 2e-3
    print(f"DENSE full f32 {label}: median per-instance error {np.median(err):.2e}, {int(out.sum())}/{B} beyond 2e-3")
    assert np.median(err) < 1e-5 and out.sum() <= 6, np.sort(err)[-8:]
    if out.any():
        f = lambda a: a.double().numpy()
        assert np.isfinite(f(h["z"])[out]).all() and np.isfinite(f(h["lam"])[out]).all()
        pg, po = _merit64(pr, f(h["z"]), f(h["lam"]), f(h["rho"])), _merit64(pr, f(o["z"]), f(o["lam"]), f(o["rho"]))
        assert ((pg - po)[out] <= 1e-3 * (np.abs(po[out]) + 1)).all(), (pg - po)[out]


@pytest.mark.parametrize("nx,nu,T", [(8, 2, 10), (13, 4, 5)])
def test_full_solve_f32(nx, nu, T):
    pr = _problem(nx, nu, T, 64, "f32", seed=3)
    st = _state0(pr)
    h = gpu_solve(pr, st, al_iter=2, max_newton=4, flags=INIT_MERIT | DUAL_UPDATE)
    o = ref_solve(pr, st, al_iter=2, max_newton=4, flags=INIT_MERIT | DUAL_UPDATE)
    assert (h["status"] == 1).all()
    _smoke_rule(pr, h, o, f"({nx},{nu}) T={T} B=64")


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_diagonal_twin_vs_plain_team_kernel(dtype):
    """diag_embed(Qd) through the dense kernel against the plain team kernel on Qd."""
    nx, nu, T, B = (8, 2, 10, 64) if dtype == "f32" else (13, 4, 3, 5)
    pr = _problem(nx, nu, T, B, dtype, seed=3, diagonal=True)
    st = _state0(pr)
    kw = dict(al_iter=2, max_newton=4, flags=INIT_MERIT | DUAL_UPDATE)
    h = gpu_solve(pr, st, **kw)
    o = gpu_solve(pr, st, solve=_be().solve_lin, variant="team", **kw)
    if dtype == "f64":
        ez, el = float((h["z"] - o["z"]).abs().max()), float((h["lam"] - o["lam"]).abs().max())
        print(f"DENSE twin f64: max |z - plain| {ez:.2e}, |lam - plain| {el:.2e}")
        assert ez < 1e-10 and el < 2e-9
    else:
        _smoke_rule(pr, h, o, "diagonal twin (8,2) T=10 B=64")


# ---- exit routes through MPC ----------------------------------------------------------------------------------------
class _Recording:
    """HipBackend with its solve_lin_dense calls noted: (al_iter, max_newton, in-kernel exit asked, launched)."""

    def __init__(self, inner):
        self._i, self.log = inner, []

    def __getattr__(self, k):
        return getattr(self._i, k)

    def solve_lin_dense(self, *a, **kw):
        ok = self._i.solve_lin_dense(*a, **kw)
        self.log.append((kw.get("al_iter"), kw.get("max_newton"), "newton_counts" in kw, ok is not False))
        return ok

    def solve_lin(self, *a, **kw):
        raise AssertionError("the diagonal kernel was reached with a dense cost")


def _mpc_solve(pr, be, dev, requires_grad=False, **kw):
    from deq_mpc_corl_amd import MPC, QuadCost
    from deq_mpc_corl_amd.qpth.al_utils import LinDx
    B, T, nx, nu = pr["dims"]
    d = lambda a: a.to(dev)
    mpc = MPC(nx, nu, T, u_lower=d(pr["lo"]), u_upper=d(pr["hi"]), n_batch=B, dtype=pr["z0"].dtype, backend=be,
              diag_cost=False, **kw)
    mpc.reinitialize(d(pr["x0"]), None)
    C, q = d(pr["C"]).requires_grad_(requires_grad), d(pr["q"]).requires_grad_(requires_grad)
    x, u, _ = mpc(d(pr["x0"]), QuadCost(C, q), LinDx(d(pr["F"]), d(pr["c"])), None, x_init=d(pr["z0"][..., :nx]).clone(),
                  u_init=d(pr["z0"][..., nx:]).clone())
    return mpc, x, u, C, q


@pytest.mark.parametrize("in_kernel", [True, False])
@pytest.mark.parametrize("nx,nu,T,B", [(2, 1, 5, 5), (13, 4, 3, 2)])
def test_reference_exit_routes(nx, nu, T, B, in_kernel):
    pr = _problem(nx, nu, T, B, "f64")
    m0, x0, u0, _, _ = _mpc_solve(pr, DenseOracleBackend(), "cpu", exit_mode="reference")
    be = _Recording(_be())
    m1, x1, u1, _, _ = _mpc_solve(pr, be, DEV, exit_mode="reference", exit_in_kernel=in_kernel)
    torch.cuda.synchronize()
    if in_kernel:   # one cooperative launch for the whole solve
        assert be.log == [(2, 4, True, True)], be.log
    else:           # per AL iteration: starting merit, four one-step launches, dual update
        assert [c[:2] for c in be.log] == [(1, 0), (1, 1), (1, 1), (1, 1), (1, 1), (1, 0)] * 2 and not any(c[2] for c in be.log)
    assert list(m1.last_newton_per_al) == list(m0.last_newton_per_al)
    # x, u are returned as float32: 1e-6 is the bound tests/test_dense_cost_cpu.py puts on that cast; lam stays fp64
    dev_xu = max(float((x1.cpu() - x0).abs().max()), float((u1.cpu() - u0).abs().max()))
    el = float((m1.lamda_prev.cpu() - m0.lamda_prev).abs().max())
    print(f"DENSE exit ({nx},{nu}) in_kernel={in_kernel}: Newton counts {list(m1.last_newton_per_al)}, |x,u - ref| {dev_xu:.2e}, "
          f"|lam - ref| {el:.2e}")
    assert dev_xu < 1e-6 and el < 2e-9
    assert torch.equal(m1.rho_prev.cpu(), m0.rho_prev)


# ---- saved factor and backward --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("nx,nu,T,B", [(2, 1, 5, 5), (13, 4, 3, 2)])
def test_saved_factor_feeds_backward(nx, nu, T, B, dtype):
    pr = _problem(nx, nu, T, B, dtype)
    st = _state0(pr)
    kw = dict(al_iter=1, max_newton=4, flags=INIT_MERIT | DUAL_UPDATE | SAVE_FACTOR)
    h = gpu_solve(pr, st, want_factor=True, **kw)
    tr = {}
    ref_solve(pr, st, trace=tr, **{**kw, "flags": INIT_MERIT | DUAL_UPDATE})
    dt = TD[dtype]
    gbar = torch.randn(B, T, nx + nu, generator=torch.Generator().manual_seed(1), dtype=torch.float64).to(dt)
    qg, Qg = Guarded((B, T, nx + nu), dt, DEV), Guarded((B, T, nx + nu), dt, DEV)
    _be().backward(pr["dims"], h["factor"], pr["F"].to(DEV), st["rho"].to(DEV), h["z"].to(DEV), gbar.to(DEV), qg.t, Qg.t)
    torch.cuda.synchronize()
    assert qg.intact() and Qg.intact()
    w_ref = dense_w(tr["Hd"].astype(np.float64), tr["Hs"].astype(np.float64), gbar.double().numpy())
    e = scale_err(qg.t.cpu().double().numpy(), w_ref, 1e-30)
    print(f"DENSE backward ({nx},{nu}) {dtype}: w vs the dense solve with the reference's last Hessian {e:.2e} (of the largest)")
    assert e < 100 * RT[dtype]   # a Newton solve like d


@pytest.mark.parametrize("exit_mode", ["fixed", "reference"])
def test_C_grad_through_mpc(exit_mode):
    pr = _problem(4, 2, 5, 5, "f64", seed=7)
    be = _Recording(_be())
    mpc, x, u, C, q = _mpc_solve(pr, be, DEV, requires_grad=True, exit_mode=exit_mode)
    gen = torch.Generator().manual_seed(5)
    gx, gu = torch.randn(x.shape, generator=gen).to(DEV), torch.randn(u.shape, generator=gen).to(DEV)
    ((x * gx).sum() + (u * gu).sum()).backward()
    torch.cuda.synchronize()
    assert C.grad is not None and torch.equal(C.grad, C.grad.transpose(-1, -2)) and float(q.grad.abs().max()) > 0
    w, z = q.grad.cpu(), torch.cat((x, u), -1).detach().double().cpu()
    want = 0.5 * (w.unsqueeze(-1) * z.unsqueeze(-2) + z.unsqueeze(-1) * w.unsqueeze(-2))
    e = float((C.grad.cpu() - want).abs().max() / want.abs().max())
    print(f"DENSE C.grad ({exit_mode}): vs 0.5 (w z' + z w') from q.grad and the returned float32 x, u: {e:.2e}")
    assert e < 1e-6   # z_final reaches the test through the float32 cast of x, u
    # w itself: the dense solve with the reference's Hessian of the last step, the same solve on the CPU backend
    cpu = DenseOracleBackend()
    _, x0, u0, C0, q0 = _mpc_solve(pr, cpu, "cpu", requires_grad=True, exit_mode=exit_mode)
    ((x0 * gx.cpu()).sum() + (u0 * gu.cpu()).sum()).backward()
    ew = scale_err(w.numpy(), q0.grad.numpy(), 1e-30)
    eC = scale_err(C.grad.cpu().numpy(), C0.grad.numpy(), 1e-30)
    print(f"DENSE C.grad ({exit_mode}): q.grad vs the reference backend {ew:.2e}, C.grad {eC:.2e}")
    assert ew < 100 * RT["f64"] and eC < 100 * RT["f64"]


# ---- bad arguments ---------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_without_a_launch():
    from deq_mpc_corl_amd import _lib
    be = _be()
    pr = _problem(2, 1, 3, 2, "f64")
    B, T, nx, nu = pr["dims"]
    dv = {k: pr[k].to(DEV).contiguous() for k in ("C", "q", "F", "c", "x0", "lo", "hi")}
    z = Guarded((B, T, nx + nu), torch.float64, DEV, init=pr["z0"])
    lam, rho, phi = (torch.zeros(B, T * nx + 2 * T * nu, dtype=torch.float64, device=DEV),
                     torch.ones(B, dtype=torch.float64, device=DEV), torch.zeros(B, dtype=torch.float64, device=DEV))
    P = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(Cptr, variant):
        d = _lib.AlqpDims(B, T, nx, nu)
        p = _lib.AlqpParams(1, 1, 20, 3, 10.0, variant, None)
        return be.lib.alqp_solve_lin_dense_f64(ctypes.byref(d), ctypes.byref(p), Cptr, P(dv["q"]), P(dv["F"]), P(dv["c"]),
                                               P(dv["x0"]), P(dv["lo"]), P(dv["hi"]), 0, 0, P(z.t), P(lam), P(rho), P(phi),
                                               None, None, None, None, None, None)
    assert call(None, 0) == -1      # ALQP_E_BADARG
    assert call(P(dv["C"]), 2) == -1
    torch.cuda.synchronize()
    assert torch.equal(z.t.cpu(), pr["z0"]) and z.intact()   # nothing ran
    assert call(P(dv["C"]), 1) == 0 and call(P(dv["C"]), 0) == 0
    torch.cuda.synchronize()
    assert not torch.equal(z.t.cpu(), pr["z0"]) and z.intact()
    with pytest.raises(RuntimeError, match="bad argument"):
        be.solve_lin_dense(pr["dims"], dv["C"], dv["q"], dv["F"], dv["c"], dv["x0"], dv["lo"], dv["hi"], 0, 0, z.t, lam, rho,
                           phi, variant="quad")
