#!/usr/bin/env python3
"""ms per launch of the three launch-per-step kernels with a dense stage cost (alqp_newton_step_dense, alqp_merit_dense,
alqp_merit_pick_dense) in their four combinations - alone, with state bounds, with general rows, with both - next to their
plain / _xbox / _rows twins on the same problem with diag(C). T = 20, (nx, nu) = (13, 4), m = 4 rows
per stage given per stage ([T,m,n], [T,m]), B = 200 and B = 16384, fp32 and fp64, |x| <= 0.6 on every state and stage
(the [nx] form), C = synthetic_dense_cost's.

HIP events around each launch, median of 30 after 5 warm-up launches, three runs with the kernels alternated (one run
times every kernel once before the next run starts). One JSON line per (dtype, B, kernel) with the three medians.
    python tools/bench_dense_step.py [--reps 30] [--runs 3]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    from deq_mpc_corl_amd import synthetic_dense_cost, synthetic_problem
    from deq_mpc_corl_amd.backend import default_backend
    be = default_backend()
    dev = "cuda:0"
    T, nx, nu, m = 20, 13, 4, 4
    n = nx + nu
    for dt in (torch.float32, torch.float64):
        for B in (200, 16384):
            p = synthetic_problem(B, T, nx, nu, seed=3, dtype=dt, device=dev, active=True)
            C, qC = synthetic_dense_cost(p, seed=3)
            Qd = C.diagonal(dim1=-2, dim2=-1).contiguous()
            dims = (B, T, nx, nu)
            g = torch.Generator(device="cpu").manual_seed(11)
            rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).to(dt).to(dev)
            z = (p.z0 + 0.2 * rnd(B, T, n)).contiguous()
            xn = (torch.einsum("btij,btj->bti", p.F, z[:, :-1]) + p.c + 0.05 * rnd(B, T - 1, nx)).contiguous()
            rho = torch.full((B,), 10.0, dtype=dt, device=dev)
            xb = (torch.full((nx,), -0.6, dtype=dt, device=dev), torch.full((nx,), 0.6, dtype=dt, device=dev), 0, 0)
            G = (rnd(T, m, n) / n ** 0.5).contiguous()   # rows per stage, about half of them violated at z
            h = (torch.einsum("tkj,btj->btk", G, z).median(0).values).contiguous()
            poly = (G, h, m, 0, m * n, 0, m)
            d = torch.empty(B, T, n, dtype=dt, device=dev)
            fac = torch.empty(B, T, n * (n + 1) // 2, dtype=dt, device=dev)
            phi, rn2 = torch.zeros(B, dtype=dt, device=dev), torch.zeros(B, dtype=dt, device=dev)

            def lam_of(xr, mm):
                lam = (0.3 * rnd(B, T * nx + T * (2 * nu + xr + mm))).contiguous()
                lam[:, T * nx:].clamp_(min=0)
                return lam
            pd = lambda lam: (p.x0, lam, rho, Qd, qC, p.u_lo, p.u_hi, 0, 0)   # the twins: diag(C)
            pc = lambda lam: (p.x0, lam, rho, C, qC, p.u_lo, p.u_hi, 0, 0)
            be.newton_step_dense(dims, z, xn, p.F, *pc(lam_of(0, 0)), None, None, d)
            al = (2.0 ** -torch.arange(20, device=dev, dtype=dt)).view(20, 1, 1, 1)
            xn_all = (torch.einsum("btij,kbtj->kbti", p.F, (z.unsqueeze(0) + al * d.unsqueeze(0))[:, :, :-1]) + p.c).contiguous()
            zw = z.clone()
            # phi_prev below every merit at the first launch and the minimum itself from then on: the pick never moves z
            low = lambda: torch.full((B,), -1e30, dtype=dt, device=dev)
            kernels = {}

            def add(xbox, rows):
                lam = lam_of(2 * nx if xbox else 0, m if rows else 0)
                xbnd, pl = (xb if xbox else None), (poly if rows else None)
                pv, pw = low(), low()
                tag = ("+xbox" if xbox else "") + ("+rows" if rows else "")
                if rows:
                    tw, ex = "_rows", (xbnd, pl)
                elif xbox:
                    tw, ex = "_xbox", (xbnd,)
                else:
                    tw, ex = "", ()
                kernels[f"newton_step{tw}{'+xbox' if xbox and rows else ''}"] = \
                    lambda: getattr(be, "newton_step" + tw)(dims, z, xn, p.F, *pd(lam), *ex, d, factor=fac)
                kernels["newton_step_dense" + tag] = lambda: be.newton_step_dense(dims, z, xn, p.F, *pc(lam), xbnd, pl, d, factor=fac)
                kernels[f"merit{tw}{'+xbox' if xbox and rows else ''}"] = \
                    lambda: getattr(be, "merit" + tw)(dims, 1, z, xn, *pd(lam), *ex, phi, rn2)
                kernels["merit_dense" + tag] = lambda: be.merit_dense(dims, 1, z, xn, *pc(lam), xbnd, pl, phi, rn2)
                kernels[f"merit_pick{tw}{'+xbox' if xbox and rows else ''}"] = \
                    lambda: getattr(be, "merit_pick" + tw)(dims, 20, d, xn_all, *pd(lam), *ex, zw, pv, rnorm2=rn2)
                kernels["merit_pick_dense" + tag] = \
                    lambda: be.merit_pick_dense(dims, 20, d, xn_all, *pc(lam), xbnd, pl, zw, pw, rnorm2=rn2)
            for xbox, rows in ((False, False), (True, False), (False, True), (True, True)):
                add(xbox, rows)
            res = {k: [] for k in kernels}
            for _ in range(a.runs):
                for k, fn in kernels.items():
                    res[k].append(timed(fn, a.reps))
            for k, v in res.items():
                print(json.dumps(dict(dtype=str(dt).replace("torch.", ""), B=B, T=T, nx=nx, nu=nu, m=m, kernel=k,
                                      ms_median_per_run=[round(x, 5) for x in v])), flush=True)


if __name__ == "__main__":
    main()
