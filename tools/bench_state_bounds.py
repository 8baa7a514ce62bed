#!/usr/bin/env python3
"""What the state box rows cost in the team kernel: ms per launch of alqp_solve_lin_xbox (|x| <= 0.6 on every state and
stage of the active-bound synthetic problem: about half of the rows bind) against alqp_solve_lin (variant "team") on the
same problem with the state bounds removed. (T, nx, nu) = (20, 13, 4), al_iter = 2, fixed exit (4 Newton steps per AL
iteration), HIP events, median of 30 launches; the two kernels alternated, three runs each. One JSON line per
(batch, dtype):
    python tools/bench_state_bounds.py [--bsz 200 16384] [--dtypes f32 f64] [--out profiles/r10/bench_state_bounds.jsonl]
Above 1024 wavefronts (B = 16384) the plain fp32 launch runs the register-capped build; the xbox kernel has none."""
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
    ap.add_argument("--out")
    a = ap.parse_args()
    be = default_backend()
    rows = []
    for B in a.bsz:
        for name in a.dtypes:
            dt = {"f32": torch.float32, "f64": torch.float64}[name]
            p = synthetic_problem(B, T, NX, NU, seed=0, dtype=dt, active=True, device=DEV)
            xhi = torch.full((NX,), WIDTH, dtype=dt, device=DEV)
            xlo = -xhi
            head = ((B, T, NX, NU), p.Qd, p.q, p.F, p.c, p.x0, p.u_lo, p.u_hi, 0, 0)
            kw = dict(al_iter=2, max_newton=4, variant="team")
            xbox = lambda z, lam, rho, phi: be.solve_lin_xbox(*head, xlo, xhi, 0, 0, z, lam, rho, phi, **kw)
            plain = lambda z, lam, rho, phi: be.solve_lin(*head, z, lam, rho, phi, **kw)
            runs = {"xbox": [], "team_plain": []}
            for _ in range(3):   # alternated
                runs["xbox"].append(timed(p, xbox, T * NX + T * (2 * NU + 2 * NX)))
                runs["team_plain"].append(timed(p, plain, T * NX + 2 * T * NU))
            row = dict(B=B, dtype=name, T=T, nx=NX, nu=NU, al_iter=2, newton=4, width=WIDTH,
                       xbox_ms=runs["xbox"], team_plain_ms=runs["team_plain"],
                       ratio=statistics.median(runs["xbox"]) / statistics.median(runs["team_plain"]))
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in rows)


if __name__ == "__main__":
    main()
