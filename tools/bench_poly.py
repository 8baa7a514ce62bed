#!/usr/bin/env python3
"""What the general rows G_t z_t <= h_t cost in the team kernel: ms per launch of alqp_solve_lin_poly against the kernel
that solves the nearest problem without them. (T, nx, nu) = (20, 13, 4), al_iter = 2, fixed exit (4 Newton steps per AL
iteration), HIP events, median of 30 launches; the two kernels alternated, three runs each. Three configurations:
    box    the state box |x| <= 0.6 as m = 26 rows G = [I 0; -I 0] against alqp_solve_lin_xbox on the same box
    m4     m = 4 dense rows coupling states and controls, h = G z0 (about half violated at the start), against
           alqp_solve_lin (variant "team") on the problem without rows
    m16    the same with m = 16
One JSON line per (configuration, batch, dtype):
    python tools/bench_poly.py [--bsz 200 16384] [--dtypes f32 f64] [--out profiles/r11/bench_poly.jsonl]
Above 1024 wavefronts (B = 16384) the plain fp32 launch runs the register-capped build; the poly kernel has none."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deq_mpc_corl_amd import synthetic_problem  # noqa: E402
from deq_mpc_corl_amd.backend import default_backend  # noqa: E402

T, NX, NU = 20, 13, 4
N = NX + NU
WIDTH = 0.6
DEV = "cuda:0"


def timed(p, launch, M, reps=30, warmup=3):
    B = p.B
    dt = p.q.dtype
    z, lam = p.z0.clone(), torch.zeros(B, M, dtype=dt, device=DEV)
    rho, phi = torch.ones(B, dtype=dt, device=DEV), torch.zeros(B, dtype=dt, device=DEV)
    ms = []
    for i in range(warmup + reps):
        z.copy_(p.z0); lam.zero_(); rho.fill_(1.0); phi.zero_()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch(z, lam, rho, phi)
        e1.record()
        e1.synchronize()
        if i >= warmup:
            ms.append(e0.elapsed_time(e1))
    assert bool(torch.isfinite(z).all())
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bsz", type=int, nargs="+", default=[200, 16384])
    ap.add_argument("--dtypes", nargs="+", default=["f32", "f64"])
    ap.add_argument("--configs", nargs="+", default=["box", "m4", "m16"])
    ap.add_argument("--out")
    a = ap.parse_args()
    be = default_backend()
    rows = []
    for B in a.bsz:
        for name in a.dtypes:
            dt = {"f32": torch.float32, "f64": torch.float64}[name]
            p = synthetic_problem(B, T, NX, NU, seed=0, dtype=dt, active=True, device=DEV)
            head = ((B, T, NX, NU), p.Qd, p.q, p.F, p.c, p.x0, p.u_lo, p.u_hi, 0, 0)
            kw = dict(al_iter=2, max_newton=4, variant="team")
            for cfg in a.configs:
                if cfg == "box":
                    m = 2 * NX
                    G = torch.zeros(m, N, dtype=dt, device=DEV)
                    G[:NX, :NX], G[NX:, :NX] = torch.eye(NX, dtype=dt, device=DEV), -torch.eye(NX, dtype=dt, device=DEV)
                    h = torch.full((m,), WIDTH, dtype=dt, device=DEV)
                    xhi = torch.full((NX,), WIDTH, dtype=dt, device=DEV)
                    xlo = -xhi
                    base_name, base_M = "xbox", T * NX + T * (2 * NU + 2 * NX)
                    base = lambda z, lam, rho, phi: be.solve_lin_xbox(*head, xlo, xhi, 0, 0, z, lam, rho, phi, **kw)
                    sg = (0, 0, 0, 0)
                else:
                    m = int(cfg[1:])
                    gen = torch.Generator().manual_seed(1)
                    G = (torch.randn(m, N, generator=gen, dtype=torch.float64) / N ** 0.5).to(dt).to(DEV)
                    h = torch.einsum("kj,btj->btk", G, p.z0).contiguous()   # rows through the starting iterate
                    base_name, base_M = "team_plain", T * NX + 2 * T * NU
                    base = lambda z, lam, rho, phi: be.solve_lin(*head, z, lam, rho, phi, **kw)
                    sg = (0, 0, T * m, m)
                poly = lambda z, lam, rho, phi: be.solve_lin_poly(*head, G, h, m, *sg, z, lam, rho, phi, **kw)
                runs = {"poly": [], base_name: []}
                for _ in range(3):   # alternated
                    runs["poly"].append(timed(p, poly, T * NX + T * (2 * NU + m)))
                    runs[base_name].append(timed(p, base, base_M))
                row = dict(config=cfg, B=B, dtype=name, T=T, nx=NX, nu=NU, m=m, al_iter=2, newton=4, poly_ms=runs["poly"],
                           base=base_name, base_ms=runs[base_name],
                           ratio=statistics.median(runs["poly"]) / statistics.median(runs[base_name]))
                rows.append(row)
                print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in rows)


if __name__ == "__main__":
    main()
