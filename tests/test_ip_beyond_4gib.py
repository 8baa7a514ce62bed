"""The interior-point path at batches whose time-major inputs pass 4 GiB per array (qp_wrapper.MPC hands ipm_solve
time-major data: F [T-1, B, nx, n], stage stride B nx n). The register-resident kernel addresses its inputs with
32-bit byte offsets from an instance's base; beyond 2^32 bytes the late stages' offsets would wrap silently into
earlier stages of the same array. Its launch guard (alqp_ipm_g4_launch.hpp: resident_addressable, checked on the host
by tests/test_ipm_g4_guard.py) then refuses, "auto" falls through to the generic kernel and "resident" reports
unsupported. Just below the limit the resident kernel must still run: the guard sits at the last legal stage.

(20, 13, 4) as bench.py times it, exit mode "fixed". F is ~5.4 GB in both cases above the limit. The batch tiles the
instances of one synthetic_problem draw (generating several 100 k instances on the host takes minutes); the initial
states are drawn per instance, so no two instances of a sample share a problem. Runs alone: tens of GB of device
memory."""
import ctypes as C

import numpy as np
import pytest
import torch

DEV = "cuda:0"
T, NX, NU = 20, 13, 4
N = NX + NU
B0 = 8192          # distinct instances of the synthetic draw
TOL = {"f64": 1e-8, "f32": 1e-2}   # as test_ip_at_scale_properties
# backward at well-conditioned multipliers (the fp32 C oracle is within 2e-7 of the float64 one there); measured on the
# MI355X: fp64 5e-16, fp32 2.8e-7 (both kernels)
TOL_BW = {"f64": 1e-12, "f32": 5e-6}
TD = {"f64": torch.float64, "f32": torch.float32}


def _problem(B, dtype):
    """Time-major arguments of ipm_solve (batch-major copies freed), plus the batch-major data of a 32-instance sample
    (first and last instance included) for the CPU oracle."""
    from deq_mpc_corl_amd import synthetic_problem
    dt = TD[dtype]
    p = synthetic_problem(B0, T, NX, NU, seed=0, dtype=dt, device=DEV)
    reps = (B + B0 - 1) // B0
    tile = lambda a: a.repeat((reps,) + (1,) * (a.dim() - 1))[:B]
    gen = torch.Generator(device=DEV)
    gen.manual_seed(1)
    x0 = torch.randn(B, NX, generator=gen, dtype=torch.float64, device=DEV).to(dt)
    sel = torch.from_numpy(np.linspace(0, B - 1, 32).round().astype(np.int64)).to(DEV)
    assert int(sel[0]) == 0 and int(sel[-1]) == B - 1 and len(torch.unique(sel)) == 32
    c = lambda a: a.index_select(0, sel).cpu().numpy()
    Qd, q, F, f = tile(p.Qd), tile(p.q), tile(p.F), tile(p.c)
    sample = dict(Qd=c(Qd), q=c(q), F=c(F), f=c(f), x0=c(x0), uhi=p.u_hi.cpu().numpy(), ulo=p.u_lo.cpu().numpy())
    tm = lambda a: a.transpose(0, 1).contiguous()
    args = [tm(Qd), tm(q)]
    del Qd, q
    args.append(tm(F))
    del F
    args += [tm(f), x0]
    del f
    uhi, ulo = p.u_hi, p.u_lo
    del p
    return args, uhi, ulo, sel, sample


def _check_forward(o, sel, sample, dtype):
    from oracle import ipm_py
    s = sample
    ref = ipm_py.forward(dtype, s["Qd"], s["q"], s["F"], s["f"], s["x0"], s["uhi"], s["ulo"], solver=0, exit_mode=1)
    errs = {}
    for k in ("zhat", "nus", "lams", "slacks"):
        got = o[k].index_select(0, sel).cpu().numpy()
        errs[k] = float(np.abs(got - ref[k]).max() / max(1.0, np.abs(ref[k]).max()))
    print(f"{dtype} forward vs oracle (32-instance sample), relative: {errs}")
    for k, e in errs.items():
        assert e < TOL[dtype], (k, e)


def _check_backward(be, dims, args, sel, sample, dtype, variant):
    """ipm_backward (same launcher, same problem load as the forward kernel) against the float64 oracle. The multipliers
    and slacks are drawn in [0.5, 1.5] rather than taken from the solve: at an fp32 solution they reach 1e-16 and the
    unregularised KKT solve is not representable in fp32 (the fp32 oracle returns NaN there as well)."""
    from oracle import ipm_py
    B = dims[0]
    dt = args[0].dtype
    gen = torch.Generator(device=DEV)
    gen.manual_seed(2)
    draw = lambda *shape: torch.rand(*shape, generator=gen, dtype=torch.float64, device=DEV)
    lams, slacks = (0.5 + draw(B, 2 * T * NU)).to(dt), (0.5 + draw(B, 2 * T * NU)).to(dt)
    g = (2 * draw(B, T * N) - 1).to(dt)
    dx, dlam, dnu = be.ipm_backward(dims, args[0], args[2], lams, slacks, g, variant=variant)
    torch.cuda.synchronize()
    c = lambda a: a.index_select(0, sel).cpu().numpy().astype(np.float64)
    d = lambda a: a.astype(np.float64)
    ref = ipm_py.backward("f64", d(sample["Qd"]), d(sample["F"]), c(lams), c(slacks), c(g), solver=0)
    errs = [float(np.abs(got - want).max() / max(1.0, np.abs(want).max()))
            for got, want in zip((c(dx), c(dlam), c(dnu)), ref)]
    print(f"{dtype} backward ({variant}) vs float64 oracle (32-instance sample), relative dx / dlam / dnu: {errs}")
    assert max(errs) < TOL_BW[dtype], errs


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,B", [("f64", 160000), ("f32", 320000)])
def test_ip_above_4gib_takes_the_generic_kernel(dtype, B):
    from deq_mpc_corl_amd import _lib
    from deq_mpc_corl_amd.backend import HipBackend
    be = HipBackend()
    dims = (B, T, NX, NU)
    try:
        args, uhi, ulo, sel, sample = _problem(B, dtype)
        assert args[2].numel() * args[2].element_size() > 1 << 32
        d = _lib.AlqpDims(B, T, NX, NU)
        print(f"{dtype} B = {B}: F {args[2].numel() * args[2].element_size() / 1e9:.2f} GB, generic workspace "
              f"alqp_ipm_workspace_bytes = {be.lib.alqp_ipm_workspace_bytes(C.byref(d), int(dtype == 'f64')) / 1e9:.2f} GB")
        o = be.ipm_solve(dims, *args, uhi, ulo, exit_mode="fixed", variant="auto")
        torch.cuda.synchronize()
        _check_forward(o, sel, sample, dtype)
        _check_backward(be, dims, args, sel, sample, dtype, "auto")
        with pytest.raises(RuntimeError, match="unsupported"):
            be.ipm_solve(dims, *args, uhi, ulo, exit_mode="fixed", variant="resident")
    finally:
        args = o = None
        be._ws.clear()
        torch.cuda.empty_cache()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,B", [("f64", 128000), ("f32", 256000)])
def test_ip_below_4gib_limit_resident(dtype, B):
    from deq_mpc_corl_amd.backend import HipBackend
    be = HipBackend()
    dims = (B, T, NX, NU)
    try:
        args, uhi, ulo, sel, sample = _problem(B, dtype)
        o = be.ipm_solve(dims, *args, uhi, ulo, exit_mode="fixed", variant="resident")
        torch.cuda.synchronize()
        _check_forward(o, sel, sample, dtype)
        _check_backward(be, dims, args, sel, sample, dtype, "resident")
    finally:
        args = o = None
        be._ws.clear()
        torch.cuda.empty_cache()
