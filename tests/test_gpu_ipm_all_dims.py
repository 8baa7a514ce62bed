"""GPU tests of the interior-point kernels at EVERY (nx, nu) of alqp_dims.hpp and at the horizons where they take
another path: the register/LDS-resident kernel k_ipm_g4 / k_ipm_g4_backward (FULLT at T = 20, the masked build below;
the two elimination chains of its twisted factorisation have equal length for odd T, differ by one block for even T, and
the bottom one is empty at T = 2; T % 4 decides which of the 4 x 5 stage slots stay empty) and the size-generic kernel
k_ipm / k_ipm_backward with its Schur factor in LDS and in the workspace, which is all there is beyond T = 20.

Only the public outputs of HipBackend.ipm_solve / ipm_backward are compared, with the C oracle's structured solver
(oracle/ipm_oracle_impl.h, solver 0, per-instance exit) in float64. The fixtures, the headline shape and the 4 GiB tests
run (2,1), (8,2), (12,4), (13,4), (14,4) at T = 5, 10, 20; this file adds the other five sizes and every other horizon.

One problem per (size, T): synthetic_problem(B = 5, seed = T), control bounds widened 4x. At the drawn bounds the
interior-point solution has 85-95 % of its controls on a bound; at 4x between a fifth and three quarters are, so both the
active and the inactive branch of every bound row carry weight (asserted per case from the oracle's solution alone)."""
import functools

import numpy as np
import pytest
import torch

from tests.test_quad_record_layout_cpu import _dims

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TD = {"f64": torch.float64, "f32": torch.float32}
ND = {"f64": np.float64, "f32": np.float32}
DIMS = _dims()   # every (nx, nu) compiled into the library
B = 5
RES_T = [2, 3, 4, 5, 7, 8, 19, 20]    # resident: empty / single-block / unequal chains, every T % 4, FULLT at 20
GEN_T = [2, 3, 8, 20, 21, 33]         # generic: the smallest, and past the resident kernel's 20 slots
GRID = ([("resident", T) for T in RES_T] + [(v, T) for v in ("generic_lds", "generic_ws") for T in GEN_T] +
        [("auto", T) for T in (21, 33)])
SUB_T = [4, 20]
VARIANTS = ["resident", "generic_lds", "generic_ws"]
KEYS = ("zhat", "nus", "lams", "slacks")
TOL_F64 = 1e-8                             # tests/test_ip_golden.py::test_ip_at_scale_properties, test_ip_beyond_4gib.py
TOL_F32_MAX = 1e-2                         # the same tests' fp32 bound: the ceiling of the per-case bound below
TOL_BW = {"f64": 1e-12, "f32": 5e-6}       # tests/test_ip_beyond_4gib.py
FORCED = dict(exit_mode="reference", eps=0.0, not_improved_lim=10**9)   # INIT, (RESID, STEP) x 20, FINAL: no exit fires


def fac_fits_lds(dtype, nx, nu, T):
    """alqp_ipm.hip:34-36 (lds_words with the factor) against kLdsLimit = 64 KB (fac_fits_lds, :628): whether the generic
    kernel can hold its Schur factor in LDS. "generic_lds" takes the workspace where it cannot."""
    words = 2 * T * nx * nx + nx * (nx + nu) + 2 * (nx + nu) + 2 * nx * nx + T * nx + 64
    return words * (8 if dtype == "f64" else 4) <= 64 * 1024


def _same_kernel_as(variant, dtype, nx, nu, T):
    """The variant whose launch `variant` must repeat bit for bit, or None. "auto" beyond 20 stages is the generic kernel
    with fac_in_lds's placement (alqp_ipm.hip:630-639): at B = 5 < 2048, LDS whenever the factor fits."""
    fits = fac_fits_lds(dtype, nx, nu, T)
    if variant == "auto":
        assert T > 20
        return "generic_lds" if fits else "generic_ws"
    return "generic_ws" if variant == "generic_lds" and not fits else None


@functools.lru_cache(maxsize=None)
def _be():
    from deq_mpc_corl_amd.backend import HipBackend
    return HipBackend()


def _frozen(d):
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def _problem(nx, nu, T, dtype):
    """Batch-major numpy arrays in float64 holding the problem as `dtype` sees it (drawn in float64, cast, cast back): the
    float64 oracle and an fp32 kernel then solve the same problem and differ by arithmetic alone."""
    from deq_mpc_corl_amd import synthetic_problem
    p = synthetic_problem(B, T, nx, nu, seed=T, dtype=torch.float64, device="cpu")
    c = lambda a: a.numpy().astype(ND[dtype]).astype(np.float64)
    return _frozen(dict(Qd=c(p.Qd), q=c(p.q), F=c(p.F), f=c(p.c), x0=c(p.x0), uhi=c(4 * p.u_hi), ulo=c(4 * p.u_lo)))


def _oracle_args(pr):
    return pr["Qd"], pr["q"], pr["F"], pr["f"], pr["x0"], pr["uhi"], pr["ulo"]


@functools.lru_cache(maxsize=None)
def _converged(nx, nu, T, dtype):
    """The float64 oracle's 20 iterations on _problem(.., dtype), and from that solution alone the proof that the case is
    not degenerate: 10-90 % of its control entries within 1e-6 of a bound."""
    from oracle import ipm_py
    pr = _problem(nx, nu, T, dtype)
    o = ipm_py.forward("f64", *_oracle_args(pr), solver=0, exit_mode=1)
    assert int(np.abs(o["info"]).max()) == 0
    u = o["zhat"].reshape(B, T, nx + nu)[:, :, nx:]
    share = float(((np.abs(u - pr["uhi"]) < 1e-6) | (np.abs(u - pr["ulo"]) < 1e-6)).mean())
    assert 0.1 <= share <= 0.9, ("share of controls on a bound", share)
    return _frozen({k: o[k] for k in KEYS}), share


@functools.lru_cache(maxsize=None)
def _reference(nx, nu, T, dtype, max_iter):
    """The float64 oracle's solve of _problem(.., dtype), stopped after max_iter iterations."""
    from oracle import ipm_py
    conv, _ = _converged(nx, nu, T, dtype)
    if max_iter == 20:
        return conv
    o = ipm_py.forward("f64", *_oracle_args(_problem(nx, nu, T, dtype)), solver=0, exit_mode=1, max_iter=max_iter)
    assert int(np.abs(o["info"]).max()) == 0
    return _frozen({k: o[k] for k in KEYS})


@functools.lru_cache(maxsize=None)
def _e_ref(nx, nu, T, max_iter):
    """The fp32 oracle's own distance from the float64 oracle on the fp32 case (largest of the four outputs)."""
    from oracle import ipm_py
    ref = _reference(nx, nu, T, "f32", max_iter)
    o = ipm_py.forward("f32", *_oracle_args(_problem(nx, nu, T, "f32")), solver=0, exit_mode=1, max_iter=max_iter)
    assert int(np.abs(o["info"]).max()) == 0
    return max(_rel(o[k], ref[k]) for k in KEYS)


def _rel(got, ref):
    """tests/test_ip_beyond_4gib.py::_check_forward's error of one output."""
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / max(1.0, np.abs(ref).max()))


def _device_args(pr, dtype):
    """ipm_solve's arguments, time-major as qp_wrapper.MPC hands them over: Cd, c [T,B,n]; F [T-1,B,nx,n]; f [T-1,B,nx]."""
    dev = lambda a: torch.tensor(a, dtype=TD[dtype], device=DEV)   # (a copy: the cached arrays are read-only)
    tm = lambda a: dev(a).transpose(0, 1).contiguous()
    return (tm(pr["Qd"]), tm(pr["q"]), tm(pr["F"]), tm(pr["f"]), dev(pr["x0"])), dev(pr["uhi"]), dev(pr["ulo"])


def _solve(nx, nu, T, dtype, variant, pr=None, batch=B, **kw):
    pr = pr or _problem(nx, nu, T, dtype)
    args, uhi, ulo = _device_args(pr, dtype)
    o = _be().ipm_solve((batch, T, nx, nu), *args, uhi, ulo, variant=variant, **kw)
    torch.cuda.synchronize()
    out = {k: o[k].cpu().numpy() for k in KEYS + ("info",)}
    out["iters"] = o["iters"]
    return out


def _assert_same_bits(a, b, keys, what):
    for k in keys:
        assert np.array_equal(a[k], b[k]), (what, k, float(np.abs(a[k] - b[k]).max()))


def _forward_case(nx, nu, T, dtype, variant, max_iter):
    got = _solve(nx, nu, T, dtype, variant, exit_mode="fixed", max_iter=max_iter)
    twin = _same_kernel_as(variant, dtype, nx, nu, T)
    if twin is not None:
        _assert_same_bits(got, _solve(nx, nu, T, dtype, twin, exit_mode="fixed", max_iter=max_iter), KEYS + ("info",),
                          f"{variant} is {twin} here")
    ref = _reference(nx, nu, T, dtype, max_iter)
    return got, {k: _rel(got[k], ref[k]) for k in KEYS}


# ---- 1. forward, fp64: every size x horizon x kernel -------------------------------------------------------------------
@pytest.mark.parametrize("variant,T", GRID)
@pytest.mark.parametrize("nx,nu", DIMS)
def test_forward_f64_every_size_and_horizon(nx, nu, variant, T):
    """All 20 iterations in one launch against the float64 oracle. Every compiled size fits the resident kernel's 64 KB at
    T = 20 in fp64 ((14,4): 60.5 KB), so "unsupported" is an error here. "auto" at T > 20 and "generic_lds" without room
    for the factor must repeat the generic kernel they stand for bit for bit."""
    got, errs = _forward_case(nx, nu, T, "f64", variant, 20)
    print(f"IPM fwd f64 {variant} ({nx},{nu}) T={T}: err {max(errs.values()):.2e} {errs}")
    assert int(np.abs(got["info"]).max()) == 0
    for k, e in errs.items():
        assert e < TOL_F64, (k, e)


@pytest.mark.parametrize("T", SUB_T)
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("nx,nu", DIMS)
def test_forward_f64_three_iterations(nx, nu, variant, T):
    """max_iter = 3: "the best of k iterates" for a small k, where the iterates are far apart and a wrong choice shows."""
    got, errs = _forward_case(nx, nu, T, "f64", variant, 3)
    print(f"IPM fwd3 f64 {variant} ({nx},{nu}) T={T}: err {max(errs.values()):.2e} {errs}")
    assert int(np.abs(got["info"]).max()) == 0
    for k, e in errs.items():
        assert e < 1e-10, (k, e)


# ---- 2. forward, fp32: the truncated solve -----------------------------------------------------------------------------
@pytest.mark.parametrize("variant,T", GRID)
@pytest.mark.parametrize("nx,nu", DIMS)
def test_forward_f32_truncated_every_size_and_horizon(nx, nu, variant, T):
    """fp32 kernels against the FLOAT64 oracle, both stopped after three iterations. (Solved to convergence at these bounds
    the fp32 oracle is itself up to 8.9e-3 from the float64 one and trips non-positive pivots in a third of the instances,
    which leaves the project's 1e-2 no room to show a kernel error; after three iterations it is within 8.4e-4 and trips
    none.) The bound of a case is ten times the fp32 oracle's own error on it, e_ref, at least 2e-5 and at most 1e-2: the
    factor covers another summation order and the resident kernel's hardware reciprocals."""
    got, errs = _forward_case(nx, nu, T, "f32", variant, 3)
    e_ref = _e_ref(nx, nu, T, 3)
    bound = min(max(10 * e_ref, 2e-5), TOL_F32_MAX)
    err = max(errs.values())
    print(f"IPM fwd3 f32 {variant} ({nx},{nu}) T={T}: err {err:.2e} e_ref {e_ref:.2e} ratio {err / e_ref:.2f} "
          f"bound {bound:.2e} {errs}")
    assert int(np.abs(got["info"]).max()) == 0
    for k, e in errs.items():
        assert e < bound, (k, e, bound, e_ref)


# ---- 3. backward: every size x horizon x kernel, both dtypes -----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _backward_case(nx, nu, T, dtype):
    """Multipliers and slacks in [0.5, 1.5], gbar in [-1, 1] (tests/test_ip_beyond_4gib.py::_check_backward), seed T, cast
    to `dtype`; the float64 oracle's solve of exactly those numbers."""
    from oracle import ipm_py
    pr = _problem(nx, nu, T, dtype)
    _converged(nx, nu, T, dtype)   # (the case is not degenerate)
    gen = torch.Generator(device="cpu")
    gen.manual_seed(T)
    draw = lambda *shape: torch.rand(*shape, generator=gen, dtype=torch.float64)
    c = lambda a: a.numpy().astype(ND[dtype]).astype(np.float64)
    lams, slacks = c(0.5 + draw(B, 2 * T * nu)), c(0.5 + draw(B, 2 * T * nu))
    g = c(2 * draw(B, T * (nx + nu)) - 1)
    ref = ipm_py.backward("f64", pr["Qd"], pr["F"], lams, slacks, g, solver=0)
    return _frozen(dict(lams=lams, slacks=slacks, g=g, dx=ref[0], dlam=ref[1], dnu=ref[2]))


def _backward(nx, nu, T, dtype, variant):
    pr, cs = _problem(nx, nu, T, dtype), _backward_case(nx, nu, T, dtype)
    args, _, _ = _device_args(pr, dtype)
    dev = lambda a: torch.tensor(a, dtype=TD[dtype], device=DEV)
    out = _be().ipm_backward((B, T, nx, nu), args[0], args[2], dev(cs["lams"]), dev(cs["slacks"]), dev(cs["g"]),
                             variant=variant)
    torch.cuda.synchronize()
    return dict(zip(("dx", "dlam", "dnu"), (a.cpu().numpy() for a in out)))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("variant,T", GRID)
@pytest.mark.parametrize("nx,nu", DIMS)
def test_backward_every_size_and_horizon(nx, nu, variant, T, dtype):
    got = _backward(nx, nu, T, dtype, variant)
    twin = _same_kernel_as(variant, dtype, nx, nu, T)
    if twin is not None:
        _assert_same_bits(got, _backward(nx, nu, T, dtype, twin), ("dx", "dlam", "dnu"), f"{variant} is {twin} here")
    cs = _backward_case(nx, nu, T, dtype)
    errs = {k: _rel(got[k], cs[k]) for k in ("dx", "dlam", "dnu")}
    print(f"IPM bwd {dtype} {variant} ({nx},{nu}) T={T}: err {max(errs.values()):.2e} {errs}")
    assert max(errs.values()) < TOL_BW[dtype], errs


# ---- 4. one launch against one launch per iteration ---------------------------------------------------------------------
@pytest.mark.parametrize("T", SUB_T)
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("nx,nu", DIMS)
def test_one_launch_equals_launch_per_iteration(nx, nu, variant, T):
    """INIT, (RESID, STEP) x 20, FINAL through the workspace (the reference exit mode with its exit rule disarmed) against
    the whole solve in one launch. The resident kernel keeps its iterate in registers in the one case and hands it over
    through the workspace in the other: all four outputs bit for bit (tests/test_ipm_g4_emu.py asserts it of the same
    source in the emulator). The generic kernel keeps every vector in the workspace either way, and the same inlined
    resid() / step() run on it: bit for bit as well."""
    one = _solve(nx, nu, T, "f64", variant, exit_mode="fixed")
    many = _solve(nx, nu, T, "f64", variant, **FORCED)
    assert one["iters"] == 20 and many["iters"] == 20
    ref = _reference(nx, nu, T, "f64", 20)
    errs = {k: _rel(many[k], ref[k]) for k in KEYS}
    same = all(np.array_equal(one[k], many[k]) for k in KEYS)
    print(f"IPM launches f64 {variant} ({nx},{nu}) T={T}: bitwise {same} err {max(errs.values()):.2e}")
    assert int(np.abs(many["info"]).max()) == 0
    for k, e in errs.items():
        assert e < TOL_F64, (k, e)
    _assert_same_bits(one, many, KEYS, "one launch / one per iteration")


# ---- 5. the pivot flag ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_non_positive_pivot_is_reported(variant):
    """tests/test_ipm_g4_emu.py::test_resident_kernel_emulated_reports_a_non_positive_pivot on the device: a stage with
    negative curvature makes a pivot of the Schur complement non-positive; the kernels replace it by its magnitude and
    report the first as block * nx + column + 1 (a numeric flag; nothing faults). The resident kernel's top chain meets
    the oracle's pivots, so a bad stage in the first half gives the oracle's index; one in the second half is met from
    below, through other pivots: flagged, with the twisted order's own index. The generic kernel eliminates block 0
    (initial state), then dynamics 0 .. T-2, top-down like the oracle (alqp_ipm.hip:176, :241 - ipm_oracle_impl.h:121,
    :158) and must report the oracle's index in both."""
    from deq_mpc_corl_amd import synthetic_problem
    from oracle import ipm_py
    T, nx, nu = 12, 4, 2
    p = synthetic_problem(3, T, nx, nu, seed=3, dtype=torch.float64, device="cpu")
    Qd = p.Qd.numpy().copy()
    Qd[1, 3, :nx] = -50.0        # instance 1: stage 3 (top chain)
    Qd[2, 9, :nx] = -50.0        # instance 2: stage 9 (bottom chain)
    c = lambda a: a.numpy()
    pr = dict(Qd=Qd, q=c(p.q), F=c(p.F), f=c(p.c), x0=c(p.x0), uhi=c(p.u_hi), ulo=c(p.u_lo))
    orc = ipm_py.forward("f64", *_oracle_args(pr), solver=0, exit_mode=1, max_iter=2)
    got = _solve(nx, nu, T, "f64", variant, pr=pr, batch=3, exit_mode="fixed", max_iter=2)
    print(f"IPM pivot {variant}: info {got['info'].tolist()} oracle {orc['info'].tolist()}")
    assert int(got["info"][0]) == 0 and int(orc["info"][0]) == 0
    assert int(orc["info"][1]) != 0 and int(orc["info"][2]) != 0
    assert int(got["info"][1]) == int(orc["info"][1])
    if variant == "resident":
        assert int(got["info"][2]) != 0
    else:
        assert int(got["info"][2]) == int(orc["info"][2])


# ---- 6. the caller's equality residual ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fixed", "forced20"])
@pytest.mark.parametrize("variant", ["resident", "generic_lds"])
@pytest.mark.parametrize("nx,nu", DIMS)
def test_external_residual_every_size(nx, nu, variant, mode):
    """ry_fn (one launch per iteration, the residual read from ry_ext) given the affine residual A z - b of the same
    problem, evaluated in PyTorch: the ry_fn = None solve again. Rows as qp_wrapper.MPC.dyn_res builds them and
    ipm_oracle_impl.h:468-471 reads them: F_t tau_t + f_t - x_{t+1} for t = 0 .. T-2, then x_0 - x0."""
    T = 5
    pr = _problem(nx, nu, T, "f64")
    dev = lambda a: torch.tensor(a, dtype=torch.float64, device=DEV)
    F, f, x0 = dev(pr["F"]), dev(pr["f"]), dev(pr["x0"])
    calls = []

    def ry_fn(z):
        assert z.shape == (B, T * (nx + nu)) and z.dtype == torch.float64
        calls.append(1)
        tau = z.reshape(B, T, nx + nu)
        dyn = torch.einsum("btij,btj->bti", F, tau[:, :-1]) + f - tau[:, 1:, :nx]
        return torch.cat((dyn.reshape(B, -1), tau[:, 0, :nx] - x0), dim=1)

    kw = dict(exit_mode="fixed") if mode == "fixed" else FORCED
    got = _solve(nx, nu, T, "f64", variant, ry_fn=ry_fn, **kw)
    assert got["iters"] == 20 and len(calls) == 20
    plain = _solve(nx, nu, T, "f64", variant, exit_mode="fixed")
    ref = _reference(nx, nu, T, "f64", 20)
    errs = {k: _rel(got[k], plain[k]) for k in KEYS}
    errs_orc = {k: _rel(got[k], ref[k]) for k in KEYS}
    print(f"IPM ry_ext f64 {variant} {mode} ({nx},{nu}) T={T}: vs ry_fn=None {max(errs.values()):.2e}, vs oracle "
          f"{max(errs_orc.values()):.2e}")
    assert int(np.abs(got["info"]).max()) == 0
    for k in KEYS:   # (against the oracle too: two runs of one kernel would share a defect outside the residual)
        assert errs[k] < TOL_F64 and errs_orc[k] < TOL_F64, (k, errs[k], errs_orc[k])
