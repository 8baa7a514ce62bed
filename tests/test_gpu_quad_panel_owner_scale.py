"""The quad forward sweep scales a pivot column on the lanes that own its rows and broadcasts the product
(csrc/alqp_quad.hpp, Quad::forward, QCfg::OWNER_SCALE) where it used to broadcast the entry and multiply on all four
lanes. Identical operands reach every multiply and fma (emulated in test_quad_panel_owner_scale_emulation.py), so the
kernels must give the bits they gave before.

Shapes by how many lanes own a row in the last slot of the panel: (13,4) n = 17, one; (8,2) n = 10, two; (2,1) n = 3,
three, in a single slot; (12,4) n = 16, a full slot. T = 2, 3 (without and with a middle stage), B = 1, 17 (a lone
instance; an odd pair count with padding quads), both dtypes; synthetic_problem(seed=11).

A. Bit identity with the commit before the change. tests/golden/quad_panel/bits_<dtype>.npz (a directory of its own:
   test_oracle_golden.py takes every .npz directly under tests/golden for a fixture of the reference) was written by
   tools/gen_golden_quad_panel.py on an MI355X with that commit's library (MI_ALQP_LIB): the fused solve (FUSED), one
   Newton step per launch on a primed workspace (STEPWISE) and one newton_step with a workspace, each on a zeroed
   workspace. z, lam, rho, phi, rnorm2, info, status and the step d are stored whole and compared as bytes. The
   workspace tensors of the 48 launches per dtype come to 1.1 MB (fp32) + 2.1 MB (fp64), more than a fixture may hold:
   the file keeps a 128-bit BLAKE2b digest of every 256-byte chunk of each (the last chunk may be shorter), and the test
   compares the digests of all chunks: every byte of the workspace takes part, no tolerance, no exclusions, and a
   difference is reported as the chunk's word range.
B. backward_ws on the workspace the fused solve left behind, against the oracle's backward, at BWD_TOL.
C. The fused solve against the CPU oracle: fp64 1e-9 (_compare); fp32 with the oracle's line-search near-ties left
   out, at most B // 4 of them, as in test_gpu_quad_factor_lds.py."""
import functools
import hashlib
import os

import numpy as np
import pytest
import torch

from oracle import oracle_py as orc
from tests.test_gpu_parity import near_tie_instances
from tests.test_gpu_quad_sweep_traffic import (BWD_TOL, DEV, FUSED, RHO_SCALE, STEPWISE, TD, _compare, _launches,
                                               _problem_cpu, _reference, _state, _to_dev)

pytestmark = pytest.mark.gpu
DIMS = [(13, 4), (8, 2), (2, 1), (12, 4)]
HORIZONS = [2, 3]
BATCHES = [1, 17]
KEYS = ("z", "lam", "rho", "phi", "rn2", "info", "st")
ROUTES = {"fused": FUSED, "stepwise": STEPWISE}
CHUNK = 256   # bytes of workspace per digest
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quad_panel", "bits_{}.npz")

grid = pytest.mark.parametrize("nx,nu,T,B,dtype", [(nx, nu, T, B, dt) for (nx, nu) in DIMS for T in HORIZONS
                                                   for B in BATCHES for dt in ("f32", "f64")])


def chunk_digests(ws):
    """[number of chunks, 16] uint8: BLAKE2b-128 of every CHUNK bytes of the workspace tensor."""
    raw = ws.cpu().numpy().tobytes()
    return np.frombuffer(b"".join(hashlib.blake2b(raw[i:i + CHUNK], digest_size=16).digest()
                                  for i in range(0, len(raw), CHUNK)), np.uint8).reshape(-1, 16).copy()


def _solve(nx, nu, T, B, dtype, calls):
    """The launches on a zeroed private workspace -> (state as numpy, the workspace tensor, the state on the device)."""
    from deq_mpc_corl_amd.backend import default_backend
    be = default_backend()
    dt, dims = TD[dtype], (B, T, nx, nu)
    p = _to_dev(_problem_cpu(nx, nu, T, B, dtype))
    s = _state(p, B, T, nx, nu, dt, DEV)
    ws = be.new_workspace(dims, s["z"]).zero_()
    _launches(be, p, dims, s, calls, variant="quad", workspace=ws)
    assert be.last_variant == "quad"
    torch.cuda.synchronize()
    return {k: s[k].cpu().numpy() for k in KEYS}, ws, s


def _newton_step(nx, nu, T, B, dtype):
    """One k_newton_step_quad launch (forward and backward sweep, d to the caller) on a zeroed workspace, away from
    the solve's starting point. The inputs are drawn on the CPU generator and formed with element-wise operations
    only, so that they are the same bits wherever the file runs. -> (d, info, the workspace tensor)"""
    from deq_mpc_corl_amd.backend import default_backend
    be = default_backend()
    dt, dims = TD[dtype], (B, T, nx, nu)
    pc = _problem_cpu(nx, nu, T, B, dtype)
    g = torch.Generator(device="cpu").manual_seed(1000 * nx + 10 * T + B)
    r = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)
    lam = (0.3 * r(B, T * nx + 2 * T * nu)).to(dt)
    lam[:, T * nx:].clamp_(min=0)
    rho = (1.0 + 9.0 * torch.rand(B, generator=g, dtype=torch.float64)).to(dt)
    z = (pc.z0 + (0.2 * r(B, T, nx + nu)).to(dt)).contiguous()
    xn = (pc.c + (0.05 * r(B, T - 1, nx)).to(dt)).contiguous()
    p = _to_dev(pc)
    d = torch.full((B, T, nx + nu), float("nan"), dtype=dt, device=DEV)
    info = torch.zeros(B, dtype=torch.int32, device=DEV)
    ws = be.new_workspace(dims, d).zero_()
    be.newton_step(dims, z.to(DEV), xn.to(DEV), p.F, p.x0, lam.to(DEV), rho.to(DEV), p.Qd, p.q, p.u_lo, p.u_hi, 0, 0, d,
                   info=info, workspace=ws)
    torch.cuda.synchronize()
    return d.cpu().numpy(), info.cpu().numpy(), ws


def bits_of_case(nx, nu, T, B, dtype):
    """Every array the golden file holds for one case, under the key it has there."""
    out = {}
    tag = f"{nx}_{nu}_T{T}_B{B}"
    for route, calls in ROUTES.items():
        g, ws, _ = _solve(nx, nu, T, B, dtype, calls)
        for k in KEYS:
            out[f"{tag}.{route}.{k}"] = g[k]
        out[f"{tag}.{route}.ws_digests"] = chunk_digests(ws)
    d, info, ws = _newton_step(nx, nu, T, B, dtype)
    out[f"{tag}.step.d"], out[f"{tag}.step.info"], out[f"{tag}.step.ws_digests"] = d, info, chunk_digests(ws)
    return out


@functools.lru_cache(maxsize=None)
def _golden(dtype):
    with np.load(GOLDEN.format(dtype)) as f:
        return {k: f[k] for k in f.files}


@grid
def test_same_bits_as_before_the_change(nx, nu, T, B, dtype):
    gold = _golden(dtype)
    got = bits_of_case(nx, nu, T, B, dtype)
    assert np.isfinite(got[f"{nx}_{nu}_T{T}_B{B}.fused.z"]).all() and np.isfinite(got[f"{nx}_{nu}_T{T}_B{B}.step.d"]).all()
    assert not got[f"{nx}_{nu}_T{T}_B{B}.step.info"].any()
    for key, a in got.items():
        b = gold[key]
        assert a.dtype == b.dtype and a.shape == b.shape, (key, a.dtype, b.dtype, a.shape, b.shape)
        if key.endswith("ws_digests"):
            bad = np.flatnonzero((a != b).any(1))
            per = CHUNK // (4 if dtype == "f32" else 8)
            assert bad.size == 0, (key, f"{bad.size} chunks differ; words", [(int(i) * per, int(i) * per + per) for i in bad[:8]])
        else:
            assert a.tobytes() == b.tobytes(), (key, int((a != b).sum()))


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
    g, ws, s = _solve(nx, nu, T, B, dtype, FUSED)
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
    g, _, _ = _solve(nx, nu, T, B, dtype, FUSED)
    ref = _reference(nx, nu, T, B, dtype, FUSED)
    label = f"fused, owner-scaled panel ({nx},{nu}) T={T} B={B} {dtype}"
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
