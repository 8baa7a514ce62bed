"""The fp32 quad fused solve keeps the factor of its first KL stages in LDS between the forward and the backward sweep
(csrc/alqp_quad.hpp, QCfg::KL: 3 stages at (13,4), 5 at (10,3), 8 - the cap - at (8,2) and (2,1)) and writes those stages to the
workspace records only on the launch's last Newton step, or on every step with the in-kernel exit. ALQP_FACTOR_IN_WS
switches that off inside the same binary: every stage's factor goes through the records, as in fp64 and in the other
quad kernels.

Shapes: (13,4), (2,1), (8,2), (10,3) (last slot of the factor with 1, 3, 2 and 1 owning lanes per quad: the compact LDS
chunks); T = 2, 3, 4, 8, 9: below, at and above KL = 3 and the cap of 8, across KL = 5, and T < KL, where every stage
is in LDS;
B = 1, 17, 33 (a lone instance, an odd pair count, padding quads); both dtypes; synthetic_problem(seed=11).

A. Bit identity against the switch: the same launches from the same state with and without the flag; z, lam, rho, phi,
   rnorm2, info, status and the whole workspace tensor compared as bytes, no exclusions, no tolerance. Routes: the fused
   solve (al_iter = 2, max_newton = 4, flags 3), one Newton step per launch on a primed workspace, and the in-kernel
   exit at B = 17 with equal Newton counts. fp64 holds no factor in LDS: identical trivially, the flag is inert there.
B. k_backward_quad on the workspace the fused solve (without the flag) left behind, against the oracle's backward:
   fails if a stage below KL was not written out on the last step. Tolerances: BWD_TOL of test_gpu_quad_sweep_traffic.py.
C. The fused solve without the flag against the CPU oracle. fp64: 1e-9 (_compare of that file). fp32: the instances the
   oracle's own trace marks as line-search near-ties (near_tie_instances, test_gpu_parity.py) are left out, at most
   B // 4 of them (0 of 1, 4 of 17, 8 of 33; counted on the CPU for every case here: at most 0, 3 and 8, the maximum at
   (13,4), T = 9); on the rest the median z error is below 1e-5, at most B // 17 instances are at or above 2e-3, and
   rho, info, status are exact on the instances below 2e-3."""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle_py as orc
from tests.test_gpu_parity import near_tie_instances
from tests.test_gpu_quad_sweep_traffic import (BWD_TOL, DEV, FUSED, RHO_SCALE, STEPWISE, TD, _compare, _launches,
                                               _problem_cpu, _reference, _state, _to_dev)

pytestmark = pytest.mark.gpu
DIMS = [(13, 4), (2, 1), (8, 2), (10, 3)]
HORIZONS = [2, 3, 4, 8, 9]
BATCHES = [1, 17, 33]
FACTOR_IN_WS = 32   # ALQP_FACTOR_IN_WS (include/mi_alqp.h)
KEYS = ("z", "lam", "rho", "phi", "rn2", "info", "st")

grid = pytest.mark.parametrize("nx,nu,T,B,dtype", [(nx, nu, T, B, dt) for (nx, nu) in DIMS for T in HORIZONS
                                                   for B in BATCHES for dt in ("f32", "f64")])
grid17 = pytest.mark.parametrize("nx,nu,T,dtype", [(nx, nu, T, dt) for (nx, nu) in DIMS for T in HORIZONS
                                                   for dt in ("f32", "f64")])


def test_flag_is_the_headers():
    import os
    import re
    from deq_mpc_corl_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mi_alqp.h")).read()
    assert int(re.search(r"#define ALQP_FACTOR_IN_WS\s+(\d+)", hdr).group(1)) == _lib.ALQP_FACTOR_IN_WS == FACTOR_IN_WS


def _run(nx, nu, T, B, dtype, calls, extra_flags, **kw):
    """The launches on a zeroed private workspace -> (state as numpy, the workspace tensor, the state on the device)."""
    from deq_mpc_corl_amd.backend import default_backend
    be = default_backend()
    dt, dims = TD[dtype], (B, T, nx, nu)
    p = _to_dev(_problem_cpu(nx, nu, T, B, dtype))
    s = _state(p, B, T, nx, nu, dt, DEV)
    ws = be.new_workspace(dims, s["z"]).zero_()
    _launches(be, p, dims, s, tuple((a, m, f | extra_flags) for a, m, f in calls), variant="quad", workspace=ws, **kw)
    assert be.last_variant == "quad"
    torch.cuda.synchronize()
    return {k: s[k].cpu().numpy() for k in KEYS}, ws, s


def _same_bytes(label, a, wa, b, wb):
    for k in KEYS:
        assert a[k].tobytes() == b[k].tobytes(), (label, k)
    wa, wb = wa.cpu().numpy(), wb.cpu().numpy()
    diff = np.flatnonzero(wa.view(np.uint8) != wb.view(np.uint8))
    assert diff.size == 0, (label, "workspace", diff.size, diff[:8] // wa.itemsize)


@grid
def test_fused_solve_same_bits_as_with_the_factor_in_the_records(nx, nu, T, B, dtype):
    a, wa, _ = _run(nx, nu, T, B, dtype, FUSED, 0)
    b, wb, _ = _run(nx, nu, T, B, dtype, FUSED, FACTOR_IN_WS)
    assert np.isfinite(a["z"]).all()
    _same_bytes(f"fused ({nx},{nu}) T={T} B={B} {dtype}", a, wa, b, wb)


@grid
def test_step_per_launch_same_bits_as_with_the_factor_in_the_records(nx, nu, T, B, dtype):
    a, wa, _ = _run(nx, nu, T, B, dtype, STEPWISE, 0)
    b, wb, _ = _run(nx, nu, T, B, dtype, STEPWISE, FACTOR_IN_WS)
    assert float(np.abs(a["z"] - _problem_cpu(nx, nu, T, B, dtype).z0.numpy()).max()) > 1e-3   # the steps moved z
    _same_bytes(f"stepwise ({nx},{nu}) T={T} B={B} {dtype}", a, wa, b, wb)


@grid17
def test_exit_inside_the_launch_same_bits_as_with_the_factor_in_the_records(nx, nu, T, dtype):
    B = 17
    ca, cb = (torch.full((2,), -7, dtype=torch.int32, device=DEV) for _ in range(2))
    a, wa, _ = _run(nx, nu, T, B, dtype, FUSED, 0, newton_counts=ca)
    b, wb, _ = _run(nx, nu, T, B, dtype, FUSED, FACTOR_IN_WS, newton_counts=cb)
    assert ca.tolist() == cb.tolist() and min(ca.tolist()) >= 1, (ca.tolist(), cb.tolist())
    _same_bytes(f"in-kernel exit ({nx},{nu}) T={T} {dtype}", a, wa, b, wb)


@functools.lru_cache(maxsize=None)
def _oracle(nx, nu, T, B, dtype):
    """The oracle's fused solve with its line-search trace and its factor: once per case, shared, never written to."""
    pc = _problem_cpu(nx, nu, T, B, dtype)
    c = lambda a: a.numpy()
    return orc.solve_lin(dtype, c(pc.Qd), c(pc.q), c(pc.F), c(pc.c), c(pc.x0), c(pc.u_lo), c(pc.u_hi), c(pc.z0), al_iter=2,
                         exit_mode="fixed", trace_steps=8 if dtype == "f32" else 0, save_factor=True)


@grid
def test_backward_pass_on_the_workspace_the_fused_solve_left(nx, nu, T, B, dtype):
    from deq_mpc_corl_amd.backend import default_backend
    be = default_backend()
    dt, dims = TD[dtype], (B, T, nx, nu)
    pc = _problem_cpu(nx, nu, T, B, dtype)
    g, ws, s = _run(nx, nu, T, B, dtype, FUSED, 0)
    gen = torch.Generator(device="cpu").manual_seed(B + 1)
    gbar = torch.randn(B, T, nx + nu, generator=gen, dtype=torch.float64).to(dt)
    qg, Qg = torch.full_like(s["z"], float("nan")), torch.full_like(s["z"], float("nan"))
    be.backward_ws(dims, ws, pc.F.to(DEV), s["rho"] / RHO_SCALE, s["z"], gbar.to(DEV), qg, Qg)
    torch.cuda.synchronize()
    o = _oracle(nx, nu, T, B, dtype)
    rq, rQ = orc.backward(dtype, o["L"], pc.F.numpy(), o["rho"] / RHO_SCALE, g["z"], gbar.numpy())
    ok = np.abs(g["z"] - o["z"]).reshape(B, -1).max(1) < (1e-9 if dtype == "f64" else 2e-3)
    if dtype == "f32":
        ok &= ~near_tie_instances(o, dtype)   # another step there: another factor
    qg, Qg = qg.cpu().numpy(), Qg.cpu().numpy()
    assert np.isfinite(qg).all() and np.isfinite(Qg).all()
    assert ok.sum() >= B - B // 4 - B // 17, int(ok.sum())
    if ok.any():
        eq = np.abs(qg - rq).reshape(B, -1).max(1)[ok].max() / np.abs(rq).max()
        eQ = np.abs(Qg - rQ).reshape(B, -1).max(1)[ok].max() / np.abs(rQ).max()
        print(f"backward pass ({nx},{nu}) T={T} B={B} {dtype}: q_grad {eq:.2e}, Qd_grad {eQ:.2e} ({int(ok.sum())} instances)")
        assert eq < BWD_TOL[dtype] and eQ < BWD_TOL[dtype], (eq, eQ)


@grid
def test_fused_solve_against_the_oracle(nx, nu, T, B, dtype):
    pc = _problem_cpu(nx, nu, T, B, dtype)
    g, _, _ = _run(nx, nu, T, B, dtype, FUSED, 0)
    ref = _reference(nx, nu, T, B, dtype, FUSED)
    label = f"fused, factor in LDS ({nx},{nu}) T={T} B={B} {dtype}"
    if dtype == "f64":
        _compare(label, dtype, B, g, ref, pc.F.numpy())
        return
    tie = near_tie_instances(_oracle(nx, nu, T, B, dtype), dtype)
    err = np.abs(g["z"] - ref["z"]).reshape(B, -1).max(1)
    keep = ~tie
    print(f"{label}: {int(tie.sum())} of {B} left out as near-ties; z median "
          f"{np.median(err[keep]) if keep.any() else float('nan'):.3e}, {int((err[keep] >= 2e-3).sum())} at or above 2e-3")
    assert np.isfinite(g["z"]).all() and np.isfinite(g["lam"]).all()
    assert tie.sum() <= B // 4, (int(tie.sum()), B)
    assert np.median(err[keep]) < 1e-5 and (err[keep] >= 2e-3).sum() <= B // 17, np.sort(err[keep])[-4:]
    ok = keep & (err < 2e-3)
    assert np.array_equal(g["rho"][ok], ref["rho"][ok])
    assert np.array_equal(g["info"][ok], ref["info"][ok]) and np.array_equal(g["st"][ok], ref["st"][ok])
