#!/usr/bin/env python3
"""What batch-shared dynamics cost or buy in the fused solve: ms per launch of alqp_solve_lin_shared with one F for the
whole batch (lti: F [nx,n], c [nx]) and with one sequence F_t (ltv: F [T-1,nx,n], c [T-1,nx]) against alqp_solve_lin on
the same dynamics expanded to [B,T-1,nx,n] (plain). (T, nx, nu) = (20, 13, 4), al_iter = 2, fixed exit (4 Newton steps per
AL iteration), HIP events, median of 30 launches; the three configurations alternated, three runs each. The kernel is the
one the batch picks ("auto": team at bsz 200, quad at B = 16384). One JSON line per (batch, dtype), with the device
memory the dynamics occupy in either form:
    python tools/bench_shared_dyn.py [--bsz 200 16384] [--dtypes f32 f64] [--out profiles/r12/bench_shared_dyn.jsonl]
The noise floor of a comparison is the spread of `plain` over its own three runs."""
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
DEV = "cuda:0"


def timed(p, launch, reps=30, warmup=3):
    B = p.B
    dt = p.q.dtype
    z, lam = p.z0.clone(), torch.zeros(B, T * NX + 2 * T * NU, dtype=dt, device=DEV)
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
    return statistics.median(ms), z.clone()


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
            kw = dict(al_iter=2, max_newton=4)
            F_ltv, c_ltv = p.F[0].contiguous(), p.c[0].contiguous()     # instance 0's model for everyone
            F_lti, c_lti = p.F[0, 0].contiguous(), p.c[0, 0].contiguous()
            full = lambda F, c: (F.expand(B, T - 1, NX, N).contiguous(), c.expand(B, T - 1, NX).contiguous())
            head, tail = ((B, T, NX, NU), p.Qd, p.q), (p.x0, p.u_lo, p.u_hi, 0, 0)
            cfgs = {}
            for form, F, c, s in (("lti", F_lti, c_lti, (0, 0, 0, 0)), ("ltv", F_ltv, c_ltv, (0, NX * N, 0, NX))):
                Fe, ce = full(F, c)
                cfgs[form] = lambda z, lam, rho, phi, F=F, c=c, s=s: be.solve_lin_shared(*head, F, c, *s, *tail, z, lam, rho, phi, **kw)
                cfgs["plain_" + form] = lambda z, lam, rho, phi, Fe=Fe, ce=ce: be.solve_lin(*head, Fe, ce, *tail, z, lam, rho, phi, **kw)
            runs = {k: [] for k in cfgs}
            zs = {}
            for _ in range(3):   # alternated
                for k, fn in cfgs.items():
                    ms, zs[k] = timed(p, fn)
                    runs[k].append(ms)
            for form in ("lti", "ltv"):   # the same bits, whichever entry point
                assert torch.equal(zs[form], zs["plain_" + form]), form
            esz = p.q.element_size()
            med = {k: statistics.median(v) for k, v in runs.items()}
            row = dict(B=B, dtype=name, T=T, nx=NX, nu=NU, al_iter=2, newton=4, kernel=be.last_variant, ms=runs,
                       lti_over_plain=med["lti"] / med["plain_lti"], ltv_over_plain=med["ltv"] / med["plain_ltv"],
                       plain_spread={k: (max(v) - min(v)) / statistics.median(v) for k, v in runs.items() if k.startswith("plain")},
                       dyn_bytes=dict(per_instance=(B * (T - 1) * NX * (N + 1)) * esz, ltv=((T - 1) * NX * (N + 1)) * esz,
                                      lti=(NX * (N + 1)) * esz))
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in rows)


if __name__ == "__main__":
    main()
