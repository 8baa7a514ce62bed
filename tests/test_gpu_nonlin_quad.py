"""GPU tests of the compiled-in models' one-launch route on the plain row set: alqp_solve_nonlin_f32/_f64
(HipBackend.solve_nonlin), the four `Dyn` instantiations k_solve_lin_quad<real, NX, NU, false, Dyn> behind
dispatch_solve_nonlin: pendulum1l (2,1), cartpole1l and cartpole1l_v2 (4,1), cartpole2l (6,1). Their own paths:
Quad::linearize<Dyn> (the Jacobian by dual numbers over a quad's four lanes, rows gathered with sel4 and padded at NX = 2
and 6), merit_nonlin<Dyn> (candidates 4i+q per lane, exchanged), the Dyn branches of iter_end, stage_in(false, false), and
the F region of the workspace that k_backward_quad reads next to the records.

Oracle: tests/oracle_backend.OracleBackend's launch-per-step methods with the model restatements of oracle/dyn_py.py
(nonlin_reference.OraclePlant, al_iteration), the CPU route test_host_logic_with_restated_dynamics_vs_reference_mpc pins
against the reference's goldens. Second yardstick: the same driver over HipBackend's launch-per-step kernels with the
provider kernels, the route the parent runs for a plain callable.

Tolerance, per compared quantity (test_gpu_nonlin_rows._bound): the fused route's distance from the oracle may be at most the
larger of 8 times the launch-per-step GPU route's distance from the same oracle on the same problem and 64 eps of the
quantity's largest entry. F against the oracle's Jacobian: the same rule with the provider kernel's Jacobian as the
yardstick. backward_ws probes: BWD_TOL of tests/test_gpu_quad_sweep_traffic.py, relative to the largest entry, against the
fp64 oracle's Hessian of the step at the kernel's own pre-step iterate (nonlin_reference.backward_f64). Nothing is
calibrated on the kernel under test.

Line-search ties (the rules of test_gpu_nonlin_rows.py). nonlin_reference.SEED = 11 is chosen on the CPU so that the fp64
oracle decides every line search of both AL iterations of every case: fp64 excuses nothing. Counted on the CPU
(tests/test_nonlin_reference_cpu.py asserts the caps), the fp32 oracle's undecided picks per Newton step of the first / second AL
iteration are [0, 0, 1, 5] / none at cartpole1l T=9 B=17, [0, 0, 2, 8] / [0, 0, 1, 2] at cartpole1l_v2 T=2 B=33 and
[0, 0, 1, 5] / [0, 0, 1, 5] at cartpole2l T=2 B=17, none in the other seven cases and none in a one-instance case: at every
step at least three quarters of a batch (33 - 2, 17 - 1) enter with decided earlier picks. The per-step test starts every
step from the kernel's own iterate, so no instance is lost there; a pick the fp32 oracle does not decide is held to the
achieved merit in the oracle's own merits. Whole solves and gradients (fp32): an instance may miss the bound only if the
oracle marks one of its line searches undecided, at most a quarter of a batch may, and such an instance stays within 10
times the largest Newton step |d| of its undecided searches. No shape had to be kept out of the whole solves.

Shapes (nonlin_reference.CASES): all four models; T = 2 (one dynamics stage, T < KL), 5, 9 (above the KL cap of 8); B = 1, 17
(a wavefront of quads plus one, the last fp32 record pair half used), 33; control bounds [nu] and [B,T,nu]."""
import functools

import numpy as np
import pytest
import torch

from tests import nonlin_reference as nl
from tests.aux_cases import Guarded
from tests.oracle_backend import OracleBackend
from tests.test_gpu_nonlin_rows import _bound, _GuardedU8
from tests.test_gpu_quad_sweep_traffic import BWD_TOL

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TD, EPS = nl.TD, nl.EPS
INIT_MERIT, DUAL_UPDATE, FACTOR_IN_WS = 1, 2, 32   # include/mi_alqp.h (test_flags_are_the_librarys)
IDS = [nl.case_id(c) for c in nl.CASES]
ONE_AL = ((1, 0, INIT_MERIT),) + ((1, 1, 0),) * 4 + ((1, 0, DUAL_UPDATE),)   # MPC's reference-exit route (_al_iter_fused)
KEYS = ("z", "lam", "rho", "phi", "rn2", "info", "status")
GRAD_CASES = nl.GRAD_CASES
B17_CASE = nl.CASES[4]   # cartpole1l T=9 B=17: KL = 8 stages of the fp32 factor in LDS, the ninth in the records

cases = pytest.mark.parametrize("model,T,B,pbt", nl.CASES, ids=IDS)
dtypes = pytest.mark.parametrize("dtype", ["f64", "f32"])


def _be():
    from deq_mpc_corl_amd.backend import default_backend
    return default_backend()


def test_flags_are_the_librarys():
    from deq_mpc_corl_amd import _lib
    assert (_lib.ALQP_INIT_MERIT, _lib.ALQP_DUAL_UPDATE, _lib.ALQP_FACTOR_IN_WS) == (INIT_MERIT, DUAL_UPDATE, FACTOR_IN_WS)


@functools.lru_cache(maxsize=None)
def _oracle(model, T, B, pbt, dtype):
    """The oracle's whole solve of the case (two AL iterations, every step's trace): CPU, once per session, never modified."""
    return nl.oracle_solve(model, T, B, pbt, dtype, nl.SEED)


def _c(t):
    return t.detach().cpu().double().numpy()


def _state(z, lam, rho, phi=None, rn2=None):
    """(z, lam, rho[, phi, rn2]) as a launch's state on the device."""
    d = lambda t: t.detach().to(DEV).clone()
    zero = torch.zeros_like(rho, device=DEV)
    return dict(z=d(z), lam=d(lam), rho=d(rho), phi=d(phi) if phi is not None else zero, rn2=d(rn2) if rn2 is not None else zero.clone())


def _launch(be, prd, st, al_iter, max_newton, flags, ws, **kw):
    """One solve_nonlin launch from the state `st` into guarded outputs (z, lam, rho, phi, rn2, info and a guarded uint8
    status); the guard bands are asserted. -> (dict of Guarded, what the launch returned)."""
    B, T, nx, nu = prd["dims"]
    dt = st["z"].dtype
    out = dict(z=Guarded((B, T, nx + nu), dt, DEV, init=st["z"]), lam=Guarded(tuple(st["lam"].shape), dt, DEV, init=st["lam"]),
               rho=Guarded((B,), dt, DEV, init=st["rho"]), phi=Guarded((B,), dt, DEV, init=st["phi"]),
               rn2=Guarded((B,), dt, DEV, init=st["rn2"]),
               info=Guarded((B,), torch.int32, DEV, init=torch.zeros(B, dtype=torch.int32)), status=_GuardedU8(B))
    out["status"].t.fill_(7)   # (every launch that runs writes 0 or 1)
    ok = be.solve_nonlin(prd["dims"], prd["dyn_id"], nl.H_STEP, prd["Qd"], prd["q"], prd["x0"], prd["lo"], prd["hi"],
                         *nl.strides(prd), out["z"].t, out["lam"].t, out["rho"].t, out["phi"].t, rnorm2=out["rn2"].t,
                         info=out["info"].t, status=out["status"].t, al_iter=al_iter, max_newton=max_newton, flags=flags,
                         workspace=ws, **kw)
    torch.cuda.synchronize()
    assert all(g.intact() for g in out.values()), [k for k, g in out.items() if not g.intact()]
    return out, ok


def _next(out):
    return {k: out[k].t.clone() for k in ("z", "lam", "rho", "phi", "rn2")}


def _run(be, prd, st, calls, ws, extra_flags=0):
    """The launches (al_iter, max_newton, flags) in turn, the state carried. -> the last launch's outputs."""
    out = None
    for al_iter, max_newton, flags in calls:
        out, _ = _launch(be, prd, st, al_iter, max_newton, flags | extra_flags, ws)
        st = _next(out)
    return out


def _zero_ws(be, prd):
    return be.new_workspace_nonlin(prd["dims"], prd["z0"]).zero_()


def _bytes(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


def _same_bytes(label, a, b, keys=KEYS):
    for k in keys:
        assert _bytes(a[k].t) == _bytes(b[k].t), (label, k)


def _rule(label, figs, fails, fused, step, ref, dtype, keep=None):
    """The tolerance rule on arrays whose LAST axis is the instance axis; the figures go to the log."""
    dist, bnd = _bound(fused, step, ref, dtype, keep)
    sdist = _bound(step, step, ref, dtype, keep)[0]
    figs.append(f"{label} {dist:.1e}/{bnd:.1e} (step route {sdist:.1e})")
    if not dist <= bnd:
        fails.append((label, dist, bnd))


def _last(a):
    """[B, ...] -> instance axis last"""
    return np.moveaxis(_c(a), 0, -1)


def _backward_probe(be, pr, plant, ws, pre, z_after, dtype, seed):
    """backward_ws on a copy of the workspace a launch left behind, with a random gbar, against the dense solve with the fp64
    oracle's Hessian of the step taken at `pre` = (z, lam, rho) on the CPU. -> (q_grad error, Qd_grad error), relative to
    the reference's largest entry."""
    dims = pr["dims"]
    B, T, nx, nu = dims
    gen = torch.Generator(device="cpu").manual_seed(seed)
    gbar = torch.randn(B, T, nx + nu, generator=gen, dtype=torch.float64).to(TD[dtype])
    wsc = ws.clone()   # (the pass keeps w in the records' y/d field)
    qg, Qg = torch.full_like(z_after, float("nan")), torch.full_like(z_after, float("nan"))
    be.backward_ws(dims, wsc, be.nonlin_F_view(wsc, dims), pre[2].to(DEV), z_after, gbar.to(DEV), qg, Qg)
    torch.cuda.synchronize()
    rq, rQ = nl.backward_f64(pr, plant, pre[0], pre[1], pre[2], z_after, gbar)
    assert torch.isfinite(qg).all() and torch.isfinite(Qg).all()
    return float(np.abs(_c(qg) - rq).max() / np.abs(rq).max()), float(np.abs(_c(Qg) - rQ).max() / np.abs(rQ).max())


# ---- 1. per Newton step, by one-step launches on a private workspace ------------------------------------------------------
@dtypes
@cases
def test_newton_steps_by_one_step_launches(model, T, B, pbt, dtype):
    """From the state after one oracle AL iteration, the launches of MPC's reference-exit route: INIT_MERIT alone, four
    launches of one Newton step, DUAL_UPDATE alone. Every launch is compared with the oracle's and the launch-per-step GPU
    route's same operation from the kernel's own state before it."""
    pr, plant, its, _, _, _ = _oracle(model, T, B, pbt, dtype)
    (z1, lam1, rho1), ref_tr = its[1]
    be, prd, prov, obe = _be(), nl.to_dev(pr, DEV), nl.provider(model), OracleBackend()
    dims, nx = pr["dims"], pr["dims"][2]
    tol = nl.tie_tol(pr, dtype)
    if dtype == "f64":
        assert not nl.undecided_steps(ref_tr, tol).any()
    ws = _zero_ws(be, prd)
    Fv = be.nonlin_F_view(ws, dims)
    figs, fails = [], []
    cpu = lambda st: {k: v.cpu() for k, v in st.items()}

    # merit only: phi, rn2 against the oracle's merit at (z, lam, rho); z, lam, rho untouched. The launch linearises at z for
    # the true residuals (Quad::linearize writes F_t unconditionally): F is the Jacobian at z, and the same bits when repeated
    st = _state(z1, lam1, rho1)
    mo, _ = _launch(be, prd, st, 1, 0, INIT_MERIT, ws)
    assert (mo["info"].t == 0).all() and (mo["status"].t == 1).all()
    for k in ("z", "lam", "rho"):
        assert torch.equal(mo[k].t, st[k]), k
    o = nl.al_iteration(obe, pr, plant, z1.clone(), lam1.clone(), rho1.clone(), n_newton=0, dual=False)
    s = nl.al_iteration(be, prd, prov, st["z"].clone(), st["lam"].clone(), st["rho"].clone(), n_newton=0, dual=False)
    _rule("merit phi", figs, fails, _c(mo["phi"].t), _c(s["phi_end"]), _c(o["phi_end"]), dtype)
    _rule("merit rn2", figs, fails, _c(mo["rn2"].t), _c(s["rn2"]), _c(o["rn2"]), dtype)
    _, F_o = nl.ssr.linearize(plant, z1, nx)
    _, F_s = nl.ssr.linearize(prov, st["z"], nx)
    _rule("merit F", figs, fails, _last(Fv), _last(F_s), _last(F_o), dtype)
    F_before = Fv.clone()
    mo2, _ = _launch(be, prd, st, 1, 0, INIT_MERIT, ws)
    assert torch.equal(Fv, F_before)
    _same_bytes("merit only, repeated", mo, mo2)
    st = _next(mo)

    n_und = []
    for step_no in range(4):
        pre = cpu(st)
        out, _ = _launch(be, prd, st, 1, 1, 0, ws)
        assert (out["info"].t == 0).all() and (out["status"].t == 1).all()
        assert torch.equal(out["lam"].t, st["lam"]) and torch.equal(out["rho"].t, st["rho"])
        # the oracle's and the launch-per-step route's step from the kernel's own (z, lam, rho, phi)
        zo, po = pre["z"].clone(), pre["phi"].clone()
        o = nl.al_iteration(obe, pr, plant, zo, pre["lam"], pre["rho"], phi=po, n_newton=1, init=False, dual=False)
        zs, ps = st["z"].clone(), st["phi"].clone()
        s = nl.al_iteration(be, prd, prov, zs, st["lam"], st["rho"], phi=ps, n_newton=1, init=False, dual=False)
        und = nl.undecided_steps(o, tol)[0]
        n_und.append(int(und.sum()))
        if dtype == "f64":
            assert not und.any(), ("the fp64 oracle decides every line search of these cases", step_no, und.sum())
        lbl = f"s{step_no}"
        _rule(lbl + " F", figs, fails, _last(Fv), _last(s["F"][0]), _last(o["F"][0]), dtype)
        _rule(lbl + " phi", figs, fails, _c(out["phi"].t), _c(ps), _c(po), dtype)
        # the pick, from z_after - z_before = 2^-k d on the oracle's largest |d| entry of the instance
        dz, d_o = _c(out["z"].t).reshape(B, -1) - _c(pre["z"]).reshape(B, -1), _c(o["d"][0]).reshape(B, -1)
        j = np.abs(d_o).argmax(1)
        moved = np.abs(dz).max(1) > 0
        ratio = np.abs(d_o[np.arange(B), j]) / np.maximum(np.abs(dz[np.arange(B), j]), 1e-300)
        kf = np.where(moved, np.rint(np.log2(ratio)), -1).astype(int)
        kr, ar = _c(o["k"][0]).astype(int), _c(o["accept"][0]).astype(int)
        ph, prev = _c(o["phi"][0]), _c(o["phi_prev"][0])
        size = np.maximum(np.abs(ph).max(0), 1.0)
        same = (moved == (ar > 0)) & (~moved | (kf == kr))   # the kernel took the oracle's pick
        for b in np.nonzero(~same)[0]:
            if not und[b]:
                fails.append((lbl + " pick", int(b), int(kf[b]), int(kr[b]), bool(moved[b]), int(ar[b])))
            else:   # held to the achieved merit in the oracle's own merits
                if moved[b] and not (0 <= kf[b] < 20 and ph[kf[b], b] - ph[:, b].min() <= tol * size[b]):
                    fails.append((lbl + " tied pick worse than the tolerance", b, int(kf[b]), int(kr[b])))
                if moved[b] != bool(ar[b]) and abs(ph[:, b].min() - prev[b]) > tol * size[b]:
                    fails.append((lbl + " accept", b, bool(moved[b]), int(ar[b])))
        # the iterate and the residual after the step, where the pick is the oracle's
        _rule(lbl + " z", figs, fails, _last(out["z"].t), _last(zs), _last(zo), dtype, same)
        _rule(lbl + " rn2", figs, fails, _c(out["rn2"].t), _c(s["rn2"]), _c(o["rn2"]), dtype, same)
        # the factor and the F the step left behind (fp32: the LDS-held stages were written out by this one-step launch)
        eq, eQ = _backward_probe(be, pr, plant, ws, (pre["z"], pre["lam"], pre["rho"]), out["z"].t, dtype, 100 + step_no)
        figs.append(f"{lbl} backward_ws q {eq:.1e} Qd {eQ:.1e}")
        if not (eq < BWD_TOL[dtype] and eQ < BWD_TOL[dtype]):
            fails.append((lbl + " backward_ws", eq, eQ))
        st = _next(out)

    # dual update only: lam, rho, rn2 against the oracle's at the kernel's iterate; z, phi and F untouched, bit for bit
    pre = cpu(st)
    F_before = Fv.clone()
    du, _ = _launch(be, prd, st, 1, 0, DUAL_UPDATE, ws)
    assert (du["status"].t == 1).all()
    assert torch.equal(Fv, F_before)   # what the last Newton step left: backward_ws reads it after this launch
    assert torch.equal(du["z"].t, st["z"]) and torch.equal(du["phi"].t, st["phi"])
    lo_, ro_ = pre["lam"].clone(), pre["rho"].clone()
    o = nl.al_iteration(obe, pr, plant, pre["z"].clone(), lo_, ro_, n_newton=0, init=False)
    ls_, rs_ = st["lam"].clone(), st["rho"].clone()
    s = nl.al_iteration(be, prd, prov, st["z"].clone(), ls_, rs_, n_newton=0, init=False)
    _rule("dual lam", figs, fails, _last(du["lam"].t), _last(ls_), _last(lo_), dtype)
    _rule("dual rn2", figs, fails, _c(du["rn2"].t), _c(s["rn2"]), _c(o["rn2"]), dtype)
    assert torch.equal(du["rho"].t.cpu(), ro_)
    print(f"NLQUAD steps {model} T={T} B={B} bt={pbt} {dtype}: undecided picks {n_und}; fused/bound " + "; ".join(figs))
    assert not fails, fails[:4]


# ---- 2. one launch equals the step-by-step launches, and the oracle's whole solve ---------------------------------------
def _compare_solve(label, fused, step, ref, und, tied, dtype):
    """Per instance and quantity the rule; fp64 strict. fp32: an instance may fall outside only if the oracle marks one of
    its line searches undecided, at most a quarter of the batch may, and it stays within 10 times its largest tied step."""
    B = ref["z"].shape[0]
    bad = np.zeros(B, bool)
    figs = []
    for key in ref:
        f, s, r = (a[key].reshape(B, -1) for a in (fused, step, ref))
        dist_i = np.abs(f - r).max(1)
        bnd_i = np.maximum(8 * np.abs(s - r).max(1), 64 * EPS[dtype] * np.abs(r).max())
        bad |= ~(dist_i <= bnd_i)
        figs.append(f"{key} {dist_i.max():.1e}/{bnd_i.max():.1e} (step route {np.abs(s - r).max():.1e})")
    print(f"NLQUAD {label}: fused/bound " + "; ".join(figs) + f"; undecided {int(und.sum())}, instances outside {int(bad.sum())}/{B}")
    assert np.isfinite(fused["z"]).all()
    if dtype == "f64":
        assert not und.any() and not bad.any(), (label, int(und.sum()), np.nonzero(bad)[0])
        return
    assert not (bad & ~und).any(), (label, "outside the bound without an undecided line search", np.nonzero(bad & ~und)[0])
    assert bad.mean() <= 0.25, (label, int(bad.sum()), B)   # (none of a one-instance case)
    dz = np.abs(fused["z"] - ref["z"]).reshape(B, -1).max(1)
    lim = 10 * tied + 64 * EPS[dtype] * np.abs(ref["z"]).max()
    assert (dz[bad] <= lim[bad]).all(), (label, "excused instances beyond 10 x their tied step", dz[bad], lim[bad])


@dtypes
@cases
def test_one_launch_equals_the_one_step_launches_and_the_oracle(model, T, B, pbt, dtype):
    """al_iter = 2, max_newton = 4, INIT_MERIT | DUAL_UPDATE in one launch against the same solve as MPC's reference-exit
    route issues it, launch by launch: the same bits in both precisions (the one launch applies a chosen step in the next
    linearisation pass and the one-step launch in iter_end, both as fma(alpha, d, z); both evaluate the residuals with the
    true dynamics at that z; the fp32 factor the non-final steps keep in LDS holds the words the records would). Then the
    one launch against the oracle's whole solve."""
    pr, plant, its, (zr, lr, rr), phi_r, rn2_r = _oracle(model, T, B, pbt, dtype)
    be, prd = _be(), nl.to_dev(pr, DEV)
    z0, lam0, rho0 = nl.start(pr)
    one, _ = _launch(be, prd, _state(z0, lam0, rho0), 2, 4, INIT_MERIT | DUAL_UPDATE, _zero_ws(be, prd))
    steps = _run(be, prd, _state(z0, lam0, rho0), ONE_AL * 2, _zero_ws(be, prd))
    assert (one["info"].t == 0).all() and (one["status"].t == 1).all()
    assert float((one["z"].t - prd["z0"]).abs().max()) > 1e-3   # the solve moved z
    _same_bytes(f"one launch / one-step launches {model} T={T} B={B} {dtype}", one, steps)
    # the launch-per-step GPU route from the same start
    zs, ls, rs = (t.to(DEV) for t in (z0, lam0, rho0))
    ps = torch.zeros_like(rs)
    for _ in range(2):
        s = nl.al_iteration(be, prd, nl.provider(model), zs, ls, rs, phi=ps)
    und, undecided, tied = nl.solve_ties(its, pr, dtype)
    fused = dict(z=_c(one["z"].t), lam=_c(one["lam"].t), phi=_c(one["phi"].t), rn2=_c(one["rn2"].t))
    step = dict(z=_c(zs), lam=_c(ls), phi=_c(ps), rn2=_c(s["rn2"]))
    ref = dict(z=_c(zr), lam=_c(lr), phi=_c(phi_r), rn2=_c(rn2_r))
    _compare_solve(f"solve {model} T={T} B={B} bt={pbt} {dtype}", fused, step, ref, undecided, tied, dtype)
    assert torch.equal(one["rho"].t.cpu(), rr)
    # control rows ended active (the generator's purpose; asserted on the oracle in tests/test_nonlin_reference_cpu.py)
    assert (one["lam"].t[:, T * pr["dims"][2]:] > 0).any()


# ---- 3. ALQP_FACTOR_IN_WS on the Dyn instantiations; the factor a multi-step launch leaves behind ----------------------------
@dtypes
@cases
def test_factor_in_ws_same_bits_and_backward_on_the_workspace_left(model, T, B, pbt, dtype):
    """A (part A of test_gpu_quad_factor_lds.py): the fused nonlinear solve with and without ALQP_FACTOR_IN_WS (the entry
    point passes AlqpParams.flags through to the kernel, which reads the bit) from the same state on zeroed private
    workspaces: every output and the whole workspace as bytes. B (part B of that file): backward_ws on the workspace the
    unflagged solve left, against the dense solve with the oracle's Hessian at the iterate the launch's last Newton step
    started from - the state the same solve reaches by one-step launches, which test 2 shows to be the launch's own. It
    fails if a stage below KL was not written out on the last step."""
    pr, plant, _, _, _, _ = _oracle(model, T, B, pbt, dtype)
    be, prd = _be(), nl.to_dev(pr, DEV)
    z0, lam0, rho0 = nl.start(pr)
    wa, wb = _zero_ws(be, prd), _zero_ws(be, prd)
    a, _ = _launch(be, prd, _state(z0, lam0, rho0), 2, 4, INIT_MERIT | DUAL_UPDATE, wa)
    b, _ = _launch(be, prd, _state(z0, lam0, rho0), 2, 4, INIT_MERIT | DUAL_UPDATE | FACTOR_IN_WS, wb)
    label = f"factor in ws {model} T={T} B={B} {dtype}"
    _same_bytes(label, a, b)
    na, nb = wa.cpu().numpy(), wb.cpu().numpy()
    diff = np.flatnonzero(na.view(np.uint8) != nb.view(np.uint8))
    assert diff.size == 0, (label, "workspace", diff.size, diff[:8] // na.itemsize)
    # B: the launch's last step started from the state after ONE_AL and merit + three steps of the second iteration
    pre = _run(be, prd, _state(z0, lam0, rho0), ONE_AL + ONE_AL[:4], _zero_ws(be, prd))
    pre = (pre["z"].t.cpu(), pre["lam"].t.cpu(), pre["rho"].t.cpu())
    assert torch.equal(pre[2] * 10, a["rho"].t.cpu())   # (the launch's dual update came after its last step)
    eq, eQ = _backward_probe(be, pr, plant, wa, pre, a["z"].t, dtype, B + 1)
    print(f"NLQUAD {label}: backward_ws on the workspace left: q_grad {eq:.1e}, Qd_grad {eQ:.1e}")
    assert eq < BWD_TOL[dtype] and eQ < BWD_TOL[dtype], (eq, eQ)


# ---- 4. gradients through MPC on the fused route ------------------------------------------------------------------------
@dtypes
@pytest.mark.parametrize("mode", ["fixed", "reference"])
@pytest.mark.parametrize("model,T,B,pbt", GRAD_CASES, ids=[nl.case_id(c) for c in GRAD_CASES])
def test_gradients_through_mpc_on_the_fused_route(model, T, B, pbt, mode, dtype):
    """d/dq and d/dQd of a weighted sum of (x, u) through MPC with the compiled-in model (provider with fused_id) against
    the same MPC on OracleBackend with the plant on the CPU; yardstick: the provider without its fused_id. (MPC owns the
    launches' outputs here: the one test of this file without guard bands.)"""
    pr, ref, newton, und, tied = nl.oracle_grads(model, T, B, pbt, mode, dtype)
    prov = nl.provider(model)
    step, _, _ = nl.mpc_grads(pr, mode, nl.nr.Plain(prov), None, TD[dtype], DEV)
    fused, newton_f, mpc = nl.mpc_grads(pr, mode, prov, None, TD[dtype], DEV)
    assert mpc.backend.last_variant == "quad"
    assert newton_f == newton, (newton_f, newton)
    assert all(np.abs(fused[k]).max() > 0 for k in ("dq", "dQd"))
    _compare_solve(f"grad {model} T={T} B={B} {mode} {dtype}", fused, step, ref, und, tied, dtype)


# ---- 5. the reference exit inside one cooperative launch -------------------------------------------------------------------
@dtypes
def test_exit_inside_the_launch_equals_the_launch_per_step_exit(dtype):
    """ALQP_EXIT_IN_KERNEL (newton_counts) on a Dyn instantiation at B = 17: the same Newton counts and the same results as
    MPC's launch-per-step exit route (_newton_device_exit: alqp_exit_test on the launches' rnorm2 between one-step launches,
    each a no-op once the flag is set). With the in-kernel exit the kernel runs iter_end after every step, which is what
    the end of a one-step launch does: the same bits."""
    model, T, B, pbt = B17_CASE
    pr, _, _, _, _, _ = _oracle(model, T, B, pbt, dtype)
    be, prd = _be(), nl.to_dev(pr, DEV)
    z0, lam0, rho0 = nl.start(pr)
    cnt = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    one, ok = _launch(be, prd, _state(z0, lam0, rho0), 2, 4, INIT_MERIT | DUAL_UPDATE, _zero_ws(be, prd), newton_counts=cnt)
    if ok is False:   # no cooperative launch available: nothing was launched
        assert torch.equal(one["z"].t, prd["z0"]) and cnt.tolist() == [-7, -7]
        return
    ws, st, counts = _zero_ws(be, prd), _state(z0, lam0, rho0), []
    sumsq = lambda out: out["rn2"].t.sum(dtype=torch.float64).reshape(1)
    for _ in range(2):
        out, _ = _launch(be, prd, st, 1, 0, INIT_MERIT, ws)
        st = _next(out)
        ctl = torch.zeros(3, dtype=torch.float64, device=DEV)
        be.exit_test(sumsq(out), ctl, 0)
        for _ in range(4):
            out, _ = _launch(be, prd, st, 1, 1, 0, ws, skip=ctl)
            st = _next(out)
            be.exit_test(sumsq(out), ctl, 1)
        counts.append(int(ctl[1].item()))
        out, _ = _launch(be, prd, st, 1, 0, DUAL_UPDATE, ws)
        st = _next(out)
    print(f"NLQUAD in-kernel exit {model} T={T} B={B} {dtype}: Newton counts {cnt.tolist()} / launch per step {counts}")
    assert cnt.tolist() == counts and min(counts) >= 1
    assert (one["info"].t == 0).all() and (one["status"].t == 1).all()
    for k in ("z", "lam", "rho", "phi", "rn2"):
        assert _bytes(one[k].t) == _bytes(st[k]), k


# ---- 6. info / status / rnorm2 per instance: a NaN stays in its instance -------------------------------------------------
@dtypes
@pytest.mark.parametrize("bad", [5, 16])
def test_nan_in_one_instance_flags_its_status_and_leaves_the_others(bad, dtype):
    """A NaN in one instance's q: that instance's status is 0, every other instance - its neighbour in the fp32 record pair
    (4 next to 5), the rest of its wavefront, and with bad = B - 1 the instance the padding quads alias - keeps the bits of
    a clean run in z, lam, rho, phi, rnorm2, info and status."""
    model, T, B, pbt = B17_CASE
    pr, _, _, _, _, _ = _oracle(model, T, B, pbt, dtype)
    be, prd = _be(), nl.to_dev(pr, DEV)
    z0, lam0, rho0 = nl.start(pr)
    clean, _ = _launch(be, prd, _state(z0, lam0, rho0), 2, 4, INIT_MERIT | DUAL_UPDATE, _zero_ws(be, prd))
    prn = dict(prd, q=prd["q"].clone())
    prn["q"][bad, T // 2, 1] = float("nan")
    nan, _ = _launch(be, prn, _state(z0, lam0, rho0), 2, 4, INIT_MERIT | DUAL_UPDATE, _zero_ws(be, prd))
    assert (clean["status"].t == 1).all() and torch.isfinite(clean["z"].t).all()
    assert int(nan["status"].t[bad]) == 0
    keep = torch.arange(B, device=DEV) != bad
    for k in KEYS:
        assert _bytes(nan[k].t[keep]) == _bytes(clean[k].t[keep]), k
