"""GPU tests of the team solves at EVERY (nx, nu) of alqp_dims.hpp: the product builds of the dense-cost, state-bound and
general-row kernels (k_solve_lin_gen with one flag), the shared-dynamics kernels (k_solve_lin_shdyn and its quad
twin; product and TRACE builds), and the register-capped fp32 builds <float, NX, NU, false, 2> of k_solve_lin and
k_solve_lin_shdyn, which the dispatch rule launches only once the batch has more than one wavefront per SIMD.

The family test files run four sizes, n = 3, 10, 17, 18. The other six hold Cfg's layout edges: pad4(N) == N at (6,2) and
(12,4), pad4(NX) == NX with odd N and NROWS = 15 of 16 lanes at (4,1), the smallest 32-lane team at (4,2).

Problems, launchers, references, rules and tolerances are the family files' own, imported; nothing is restated here."""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle_py as orc
from tests import poly_rows_reference as prr
from tests import state_bounds_reference as sbr
from tests import test_gpu_dense_cost as dn
from tests import test_gpu_poly_rows as pl
from tests import test_gpu_state_bounds as xb
from tests.aux_cases import case
from tests.test_gpu_parity import NEAR_TIES_DIMS_F32, check_excluded, near_tie_instances
from tests.test_gpu_shared_dyn import _assert_equal, _dyn, _launch
from tests.test_quad_record_layout_cpu import _dims

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TD = {"f64": torch.float64, "f32": torch.float32}
DIMS = _dims()   # every (nx, nu) compiled into the library
INIT_MERIT, DUAL_UPDATE = 1, 2
FULL = dict(al_iter=2, max_newton=4, flags=INIT_MERIT | DUAL_UPDATE)
# family -> how its problem is drawn. xbox: bounds shared / per (b, t); poly: m = 5 is no multiple of 4 (the hand-over
# region's padding)
FAMILIES_F64 = ["dense", "xbox", "xbox_ps", "poly_m5_per_instance", "poly_m3_shared"]
FAMILIES_F32 = ["dense", "xbox", "poly_m5_per_instance"]


def _qpw(nx, nu):
    """Cfg::QPW: instances per wavefront."""
    nrows = 2 * (nx + nu) + nx + 1
    G = 8 if nrows <= 8 else 16 if nrows <= 16 else 32 if nrows <= 32 else 64
    return 64 // G


def _capped_batch(nx, nu, multiple_of=1):
    """The smallest batch, a multiple of `multiple_of`, at which the fp32 team dispatch takes the register-capped build."""
    simds = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    B = (simds * _qpw(nx, nu) // multiple_of + 1) * multiple_of
    # dispatch_solve / dispatch_solve_shdyn (alqp_team.hip): <float, NX, NU, false, 2> iff ceil(B / QPW) > 4 * CUs. Should
    # that rule change, this fails rather than let the tests below run the uncapped builds unnoticed
    assert -(-B // _qpw(nx, nu)) > simds and -(-(B - multiple_of) // _qpw(nx, nu)) <= simds, (B, simds)
    return B


def _family(fam, nx, nu, T, B, dtype, seed):
    """-> (the family's test module, its problem)"""
    if fam == "dense":
        return dn, dn._problem(nx, nu, T, B, dtype, seed=seed)
    if fam.startswith("xbox"):
        return xb, xb._problem(nx, nu, T, B, dtype, fam == "xbox_ps", seed=seed)
    _, m, layout = fam.split("_", 2)
    return pl, pl._problem(nx, nu, T, B, int(m[1:]), layout, dtype, seed=seed)


def _new_row_multipliers(mod, pr, lam):
    """The reference's multipliers of the rows the family adds, one array per kind of row."""
    B, T, nx, nu = pr["dims"]
    if mod is xb:
        return list(sbr.split_lam(lam.numpy(), T, nx, nu)[1:])
    if mod is pl:
        return [prr.split_lam(lam.numpy(), T, nx, nu, pr["m"])[1]]
    return []


# ---- 1. product builds of dense / xbox / poly -------------------------------------------------------------------------
@pytest.mark.parametrize("fam", FAMILIES_F64)
@pytest.mark.parametrize("nx,nu", DIMS)
def test_full_solve_f64_every_size(nx, nu, fam):
    """Two full wavefronts of teams and a ragged third; each family's test_full_solve_f64, its bounds unchanged."""
    T, B = 3, 2 * _qpw(nx, nu) + 1
    mod, pr = _family(fam, nx, nu, T, B, "f64", 5)
    st = mod._state0(pr)
    h = mod.gpu_solve(pr, st, **FULL)   # (asserts the guard bands of every output)
    o = mod.ref_solve(pr, st, **FULL)
    assert (o["info"] == 0).all()
    assert (h["info"] == 0).all() and (h["status"] == 1).all()
    ez, el = float((h["z"] - o["z"]).abs().max()), float((h["lam"] - o["lam"]).abs().max())
    new = _new_row_multipliers(mod, pr, o["lam"])
    print(f"{fam} full f64 ({nx},{nu}) T={T} B={B}: max |z - ref| {ez:.2e}, |lam - ref| {el:.2e}; largest multipliers of the "
          f"new rows {[float(a.max()) for a in new]}")
    assert all(a.max() > 0 for a in new)
    assert ez < 1e-10 and el < 2e-9 and torch.equal(h["rho"], o["rho"])
    assert (h["rn2"] - o["rn2"]).abs().max() <= 1e-8 * max(1.0, float(o["rn2"].abs().max()))


@pytest.mark.parametrize("fam", FAMILIES_F32)
@pytest.mark.parametrize("nx,nu", DIMS)
def test_full_solve_f32_every_size(nx, nu, fam):
    """Each family's test_full_solve_f32: its _smoke_rule (at most 6 of 64 instances beyond 2e-3, those finite and no worse
    in merit) and, where the family has one, its bound on lam and rn2."""
    T, B = 5, 64
    mod, pr = _family(fam, nx, nu, T, B, "f32", 3)
    st = mod._state0(pr)
    h = mod.gpu_solve(pr, st, **FULL)
    o = mod.ref_solve(pr, st, **FULL)
    assert (h["status"] == 1).all()
    ok = mod._smoke_rule(pr, h, o, f"({nx},{nu}) T={T} B={B} {fam}")
    if mod is not dn:
        mod._lam_rn2_rule(pr, h, o, ok, f"({nx},{nu})")


# ---- 2. the register-capped fp32 builds -------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,nu", DIMS)
def test_capped_f32_replicas_bitwise_and_vs_oracle(nx, nu):
    """The 19 problems of test_gpu_parity.py::test_every_compiled_dims_vs_oracle, tiled along the batch until the dispatch
    takes k_solve_lin<float, NX, NU, false, 2>: every replica the same bits as the first (same inputs, same kernel: the
    place in the grid must not matter), and the first against the oracle with that test's checks and budgets."""
    from deq_mpc_corl_amd import synthetic_problem
    from deq_mpc_corl_amd.backend import default_backend
    be = default_backend()
    dt = torch.float32
    B0, T = 19, 7
    B = _capped_batch(nx, nu, multiple_of=B0)
    k = B // B0
    p = synthetic_problem(B0, T, nx, nu, seed=5, dtype=dt, device=DEV)
    rep = lambda a: a.repeat(k, *([1] * (a.dim() - 1))).contiguous()
    z = rep(p.z0)
    lam = torch.zeros(B, T * nx + 2 * T * nu, dtype=dt, device=DEV)
    rho, phi, rn2 = torch.ones(B, dtype=dt, device=DEV), torch.zeros(B, dtype=dt, device=DEV), torch.zeros(B, dtype=dt, device=DEV)
    info = torch.zeros(B, dtype=torch.int32, device=DEV)
    st = torch.zeros(B, dtype=torch.uint8, device=DEV)
    be.solve_lin((B, T, nx, nu), rep(p.Qd), rep(p.q), rep(p.F), rep(p.c), rep(p.x0), p.u_lo, p.u_hi, 0, 0, z, lam, rho, phi, rn2,
                 info, st, al_iter=2, max_newton=4, n_ls=20, flags=3, variant="team")
    torch.cuda.synchronize()
    assert be.last_variant == "team"
    for name, a in (("z", z), ("lam", lam), ("rho", rho), ("rn2", rn2), ("info", info), ("status", st)):
        r = a.view(k, B0, -1)
        differ = (r != r[:1]).any(2).any(1)   # (a NaN differs from itself)
        assert not differ.any(), (name, "replicas", differ.nonzero().flatten()[:8].tolist(), "of", k)
    c = lambda a: a[:B0].cpu().numpy()
    n = lambda a: a.cpu().numpy()
    o = orc.solve_lin("f32", n(p.Qd), n(p.q), n(p.F), n(p.c), n(p.x0), n(p.u_lo), n(p.u_hi), n(p.z0), al_iter=2,
                      exit_mode="fixed", trace_steps=8)
    assert int(info.abs().sum()) == 0 and int(st.sum()) == B
    ok = ~near_tie_instances(o, "f32")
    prob = dict(Qd=n(p.Qd), q=n(p.q), F=n(p.F), c=n(p.c), x0=n(p.x0), u_lo=n(p.u_lo), u_hi=n(p.u_hi))
    check_excluded("f32", ~ok, c(z), c(lam), c(rho), o, prob, max_count=NEAR_TIES_DIMS_F32[(nx, nu)] + 1,
                   label=f"({nx},{nu})/f32/team capped, B={B}")
    ez, el = np.abs(c(z) - o["z"])[ok].max(), np.abs(c(lam) - o["lam"])[ok].max()
    print(f"capped team ({nx},{nu}) B={B}: |z - oracle| {ez:.2e}, |lam - oracle| {el:.2e}")
    assert ez < 2e-3
    assert el < 2e-3 * 20


@functools.lru_cache(maxsize=2)
def _case(dims, dtype):
    return case(dims, TD[dtype])   # CPU tensors; the launches copy them


def _shared_equals_plain(dims, dtype, kernel, Fform, cform, traced=False):
    """test_gpu_shared_dyn.py::test_shared_equals_plain_on_expanded_bitwise at `dims`. `traced`: both launches get an
    AlqpTrace, which selects the TRACE builds, and the traces are compared too."""
    cs = _case(dims, dtype)
    dyn = _dyn(cs, Fform, cform)
    B, T, nx, nu = dims
    S, dt = FULL["al_iter"] * FULL["max_newton"], TD[dtype]
    nan = lambda *s: torch.full(s, float("nan"), dtype=dt, device=DEV)
    new_trace = lambda: {"g": nan(S, B, T, nx + nu), "d": nan(S, B, T, nx + nu), "phi": nan(S, 20, B), "phi_prev": nan(S, B),
                         "k": torch.full((S, B), -1, dtype=torch.int32, device=DEV),
                         "accept": torch.full((S, B), -1, dtype=torch.int32, device=DEV)}
    trs = [new_trace(), new_trace()] if traced else [None, None]
    got = _launch(cs, dyn, True, kernel, **({"trace": trs[0]} if traced else {}))
    want = _launch(cs, dyn, False, kernel, **({"trace": trs[1]} if traced else {}))
    assert torch.isfinite(want["z"]).all() and not torch.equal(want["z"], cs.z.to(DEV))   # the solve moved z
    _assert_equal(got, want)
    if traced:
        for name in trs[1]:
            assert torch.equal(trs[0][name], trs[1][name]), name   # (every entry was written: a NaN left over fails here)
        assert (trs[1]["k"] >= 0).all() and (trs[1]["accept"] >= 0).all()
    # the caller's data was only read
    assert torch.equal(dyn["Fv"], dyn["Fe"][0, 0] if Fform == "lti" else dyn["Fe"][0] if Fform == "ltv" else dyn["Fe"])
    assert torch.isnan(dyn["F"][dyn["Fv"].numel():]).all() and torch.isnan(dyn["c"][dyn["cv"].numel():]).all()


@pytest.mark.parametrize("Fform,cform", [("lti", "lti"), ("ltv", "pi")])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("kernel", ["team", "quad"])
@pytest.mark.parametrize("nx,nu", DIMS)
def test_shared_dyn_every_size_bitwise(nx, nu, kernel, dtype, Fform, cform):
    """team: two full wavefronts of teams and a ragged third; quad: 16 instances per wavefront plus one."""
    B = 2 * _qpw(nx, nu) + 1 if kernel == "team" else 17
    _shared_equals_plain((B, 3, nx, nu), dtype, kernel, Fform, cform)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("kernel", ["team", "quad"])
@pytest.mark.parametrize("nx,nu", DIMS)
def test_shared_dyn_trace_builds_bitwise(nx, nu, kernel, dtype):
    """The TRACE builds of k_solve_lin_shdyn / k_solve_lin_quad_shdyn, which no other test launches: outputs and every
    array of the AlqpTrace against the plain entry point's TRACE build, one sequence F_t and a per-instance c."""
    B = 2 * _qpw(nx, nu) + 1 if kernel == "team" else 17
    _shared_equals_plain((B, 3, nx, nu), dtype, kernel, "ltv", "pi", traced=True)


@pytest.mark.parametrize("Fform,cform", [("lti", "lti"), ("ltv", "pi")])
@pytest.mark.parametrize("nx,nu", DIMS)
def test_capped_f32_shared_dyn_bitwise(nx, nu, Fform, cform):
    """k_solve_lin_shdyn<float, NX, NU, false, 2> against k_solve_lin<float, NX, NU, false, 2>: both entry points at a
    batch at which both dispatch rules take the capped build."""
    _shared_equals_plain((_capped_batch(nx, nu), 3, nx, nu), "f32", "team", Fform, cform)
