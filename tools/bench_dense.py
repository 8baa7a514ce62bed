#!/usr/bin/env python3
"""What the dense stage cost costs in the team kernel: ms per launch of alqp_solve_lin_dense on synthetic_dense_cost
against alqp_solve_lin (variant "team") on the diagonal problem, same dynamics, bounds and start. (T, nx, nu) =
(20, 13, 4), al_iter = 2, fixed exit (4 Newton steps per AL iteration), HIP events, median of 30 launches; the two
kernels alternated, three runs each. One JSON line per (batch, dtype):
    python tools/bench_dense.py [--bsz 200 16384] [--dtypes f32 f64] [--out profiles/r09/bench_dense.jsonl]"""
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
DEV = "cuda:0"


def timed(be, solve, cost, p, q, reps=30, warmup=3):
    B = p.B
    dt = p.q.dtype
    z0 = p.z0
    z, lam = z0.clone(), torch.zeros(B, T * NX + 2 * T * NU, dtype=dt, device=DEV)
    rho, phi = torch.ones(B, dtype=dt, device=DEV), torch.zeros(B, dtype=dt, device=DEV)
    ms = []
    for i in range(warmup + reps):
        z.copy_(z0); lam.zero_(); rho.fill_(1.0); phi.zero_()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        solve((B, T, NX, NU), cost, q, p.F, p.c, p.x0, p.u_lo, p.u_hi, 0, 0, z, lam, rho, phi, al_iter=2, max_newton=4,
              variant="team")
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
    ap.add_argument("--out")
    a = ap.parse_args()
    be = default_backend()
    rows = []
    for B in a.bsz:
        for name in a.dtypes:
            dt = {"f32": torch.float32, "f64": torch.float64}[name]
            p = synthetic_problem(B, T, NX, NU, seed=0, dtype=dt, active=True, device=DEV)
            C, qd = synthetic_dense_cost(p, 0)
            runs = {"dense": [], "team_diag": []}
            for _ in range(3):   # alternated
                runs["dense"].append(timed(be, be.solve_lin_dense, C, p, qd))
                runs["team_diag"].append(timed(be, be.solve_lin, p.Qd, p, p.q))
            row = dict(B=B, dtype=name, T=T, nx=NX, nu=NU, al_iter=2, newton=4,
                       lds_bytes_per_team=be.lds_bytes(B, T, NX, NU, dt) // be.qps_per_wave(B, T, NX, NU, dt),
                       dense_ms=runs["dense"], team_diag_ms=runs["team_diag"],
                       ratio=statistics.median(runs["dense"]) / statistics.median(runs["team_diag"]))
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in rows)


if __name__ == "__main__":
    main()
