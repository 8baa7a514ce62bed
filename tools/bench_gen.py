#!/usr/bin/env python3
"""What the combined instances of the team kernel cost: ms per launch of alqp_solve_lin_gen against the single-feature
kernel on the same problem with the other features removed. (T, nx, nu) = (20, 13, 4), al_iter = 2, fixed exit (4 Newton
steps per AL iteration), HIP events, median of 30 launches; the two kernels alternated, three runs each. Configurations:
    dxp_vs_d, dxp_vs_x, dxp_vs_p   dense cost + state box |x| <= 0.6 + m = 4 rows against alqp_solve_lin_dense / _xbox /
                                   _poly with the other two features removed: the price of each addition
    xp_vs_rows                     box as bounds + m = 4 rows against alqp_solve_lin_poly with the box as 26 more rows
                                   (the rewrite the old error message recommended)
    dp_vs_p_m4, dp_vs_p_m16        dense cost + rows against alqp_solve_lin_poly on the diagonal cost: what the in-place
                                   fetches of C_t and of G_t's first trip cost
The diagonal cost has 0.1 on the controls (the synthetic problem's 1e-8 leaves these problems ill-conditioned in fp32).
One JSON line per (configuration, batch, dtype):
    python tools/bench_gen.py [--bsz 200 16384] [--dtypes f32 f64] [--out profiles/r14/bench_gen.jsonl]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deq_mpc_corl_amd import synthetic_dense_cost, synthetic_problem  # noqa: E402
from deq_mpc_corl_amd.backend import default_backend  # noqa: E402

T, NX, NU = 20, 13, 4
N = NX + NU
WIDTH = 0.6
DEV = "cuda:0"
CONFIGS = ["dxp_vs_d", "dxp_vs_x", "dxp_vs_p", "xp_vs_rows", "dp_vs_p_m4", "dp_vs_p_m16"]


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


def rows_through_z0(p, m, dt):
    gen = torch.Generator().manual_seed(1)
    G = (torch.randn(m, N, generator=gen, dtype=torch.float64) / N ** 0.5).to(dt).to(DEV)
    h = torch.einsum("kj,btj->btk", G, p.z0).contiguous()   # about half violated at the start
    return (G, h, m, 0, 0, T * m, m)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bsz", type=int, nargs="+", default=[200, 16384])
    ap.add_argument("--dtypes", nargs="+", default=["f32", "f64"])
    ap.add_argument("--configs", nargs="+", default=CONFIGS)
    ap.add_argument("--out")
    a = ap.parse_args()
    be = default_backend()
    rows = []
    for B in a.bsz:
        for name in a.dtypes:
            dt = {"f32": torch.float32, "f64": torch.float64}[name]
            p = synthetic_problem(B, T, NX, NU, seed=0, dtype=dt, active=True, device=DEV)
            # control cost 0.1 in place of the synthetic problem's 1e-8 (DESIGN section 20 says why): with 1e-8, a box and
            # rows through z0 the fp32 reference itself meets non-positive pivots in a quarter of the instances and
            # the iterates stop being finite; the cost's value changes no instruction count
            Qd = p.Qd.clone()
            Qd[..., NX:] = 0.1
            p = p._replace(Qd=Qd, q=-(Qd * p.xref))
            C, qC = synthetic_dense_cost(p, seed=0)
            dims = (B, T, NX, NU)
            tail = (p.F, p.c, p.x0, p.u_lo, p.u_hi, 0, 0)
            kw = dict(al_iter=2, max_newton=4, variant="team")
            xhi = torch.full((NX,), WIDTH, dtype=dt, device=DEV)
            xb = (-xhi, xhi, 0, 0)
            W = lambda x, m: T * NX + T * (2 * NU + (2 * NX if x else 0) + m)
            for cfg in a.configs:
                m = 16 if cfg.endswith("m16") else 4
                pl = rows_through_z0(p, m, dt)
                if cfg.startswith("dxp"):
                    gen_M = W(True, m)
                    gen = lambda z, lam, rho, phi: be.solve_lin_gen(dims, C, qC, *tail, xb, pl, z, lam, rho, phi, **kw)
                    base_name = {"d": "dense", "x": "xbox", "p": "poly"}[cfg[-1]]
                    if base_name == "dense":
                        base_M = W(False, 0)
                        base = lambda z, lam, rho, phi: be.solve_lin_dense(dims, C, qC, *tail, z, lam, rho, phi, **kw)
                    elif base_name == "xbox":
                        base_M = W(True, 0)
                        base = lambda z, lam, rho, phi: be.solve_lin_xbox(dims, p.Qd, p.q, *tail, *xb, z, lam, rho, phi, **kw)
                    else:
                        base_M = W(False, m)
                        base = lambda z, lam, rho, phi: be.solve_lin_poly(dims, p.Qd, p.q, *tail, *pl, z, lam, rho, phi, **kw)
                elif cfg == "xp_vs_rows":
                    gen_M = W(True, m)
                    gen = lambda z, lam, rho, phi: be.solve_lin_gen(dims, p.Qd, p.q, *tail, xb, pl, z, lam, rho, phi, **kw)
                    Gb = torch.zeros(2 * NX, N, dtype=dt, device=DEV)
                    Gb[:NX, :NX], Gb[NX:, :NX] = torch.eye(NX, dtype=dt, device=DEV), -torch.eye(NX, dtype=dt, device=DEV)
                    G2 = torch.cat((Gb, pl[0]), 0).contiguous()
                    h2 = torch.cat((torch.full((B, T, 2 * NX), WIDTH, dtype=dt, device=DEV), pl[1]), 2).contiguous()
                    m2 = 2 * NX + m
                    base_name, base_M = "poly_box_as_rows", W(False, m2)
                    base = lambda z, lam, rho, phi: be.solve_lin_poly(dims, p.Qd, p.q, *tail, G2, h2, m2, 0, 0, T * m2, m2, z, lam,
                                                                      rho, phi, **kw)
                else:
                    gen_M = W(False, m)
                    gen = lambda z, lam, rho, phi: be.solve_lin_gen(dims, C, qC, *tail, None, pl, z, lam, rho, phi, **kw)
                    base_name, base_M = "poly", W(False, m)
                    base = lambda z, lam, rho, phi: be.solve_lin_poly(dims, p.Qd, p.q, *tail, *pl, z, lam, rho, phi, **kw)
                runs = {"gen": [], base_name: []}
                for _ in range(3):   # alternated
                    runs["gen"].append(timed(p, gen, gen_M))
                    runs[base_name].append(timed(p, base, base_M))
                row = dict(config=cfg, B=B, dtype=name, T=T, nx=NX, nu=NU, m=m, al_iter=2, newton=4, gen_ms=runs["gen"],
                           base=base_name, base_ms=runs[base_name],
                           ratio=statistics.median(runs["gen"]) / statistics.median(runs[base_name]))
                rows.append(row)
                print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in rows)


if __name__ == "__main__":
    main()
