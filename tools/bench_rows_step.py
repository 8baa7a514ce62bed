#!/usr/bin/env python3
"""ms per launch of the four launch-per-step kernels with general rows (alqp_newton_step_rows, alqp_merit_rows,
alqp_merit_pick_rows, alqp_dual_update_rows), without and with state bounds, against their plain and their _xbox twins on
the same problem without the rows. T = 20, (nx, nu) = (13, 4), m = 4 and m = 16 rows per stage given
per stage ([T,m,n], [T,m]), B = 200 and B = 16384, fp32 and fp64, |x| <= 0.6 on every state and stage (the [nx] form).

HIP events around each launch, median of 30 after 5 warm-up launches, three runs with the kernels alternated (one run
times every kernel once before the next run starts). One JSON line per (dtype, B, kernel) with the three medians.
    python tools/bench_rows_step.py [--reps 30] [--runs 3]"""
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
    from deq_mpc_corl_amd import synthetic_problem
    from deq_mpc_corl_amd.backend import default_backend
    be = default_backend()
    dev = "cuda:0"
    T, nx, nu = 20, 13, 4
    n = nx + nu
    for dt in (torch.float32, torch.float64):
        for B in (200, 16384):
            p = synthetic_problem(B, T, nx, nu, seed=3, dtype=dt, device=dev, active=True)
            dims = (B, T, nx, nu)
            g = torch.Generator(device="cpu").manual_seed(11)
            rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).to(dt).to(dev)
            z = (p.z0 + 0.2 * rnd(B, T, n)).contiguous()
            xn = (torch.einsum("btij,btj->bti", p.F, z[:, :-1]) + p.c + 0.05 * rnd(B, T - 1, nx)).contiguous()
            rho = torch.full((B,), 10.0, dtype=dt, device=dev)
            xb = (torch.full((nx,), -0.6, dtype=dt, device=dev), torch.full((nx,), 0.6, dtype=dt, device=dev), 0, 0)
            d = torch.empty(B, T, n, dtype=dt, device=dev)
            fac = torch.empty(B, T, n * (n + 1) // 2, dtype=dt, device=dev)
            phi, rn2 = torch.zeros(B, dtype=dt, device=dev), torch.zeros(B, dtype=dt, device=dev)

            def lam_of(xr, m):
                lam = (0.3 * rnd(B, T * nx + T * (2 * nu + xr + m))).contiguous()
                lam[:, T * nx:].clamp_(min=0)
                return lam
            pp = lambda lam: (p.x0, lam, rho, p.Qd, p.q, p.u_lo, p.u_hi, 0, 0)
            lam_p, lam_x = lam_of(0, 0), lam_of(2 * nx, 0)
            be.newton_step(dims, z, xn, p.F, *pp(lam_p), d)
            al = (2.0 ** -torch.arange(20, device=dev, dtype=dt)).view(20, 1, 1, 1)
            xn_all = (torch.einsum("btij,kbtj->kbti", p.F, (z.unsqueeze(0) + al * d.unsqueeze(0))[:, :, :-1]) + p.c).contiguous()
            zw = z.clone()
            # phi_prev below every merit at the first launch and the minimum itself from then on: the pick never moves z
            low = lambda: torch.full((B,), -1e30, dtype=dt, device=dev)

            def dual(fn, lam, *extra):
                lam, r = lam.clone(), rho.clone()
                return lambda: fn(dims, z, xn, p.x0, p.u_lo, p.u_hi, 0, 0, *extra, lam, r, 1.0)
            prev = {k: low() for k in ("p", "x")}
            kernels = {
                "newton_step": lambda: be.newton_step(dims, z, xn, p.F, *pp(lam_p), d, factor=fac),
                "newton_step_xbox": lambda: be.newton_step_xbox(dims, z, xn, p.F, *pp(lam_x), xb, d, factor=fac),
                "merit": lambda: be.merit(dims, 1, z, xn, *pp(lam_p), phi, rn2),
                "merit_xbox": lambda: be.merit_xbox(dims, 1, z, xn, *pp(lam_x), xb, phi, rn2),
                "merit_pick": lambda: be.merit_pick(dims, 20, d, xn_all, *pp(lam_p), zw, prev["p"], rnorm2=rn2),
                "merit_pick_xbox": lambda: be.merit_pick_xbox(dims, 20, d, xn_all, *pp(lam_x), xb, zw, prev["x"], rnorm2=rn2),
                "dual_update": dual(be.dual_update, lam_p),
                "dual_update_xbox": dual(be.dual_update_xbox, lam_x, xb),
            }

            def add_rows(m, xbox):
                # rows per stage, about half of them violated at z
                G = (rnd(T, m, n) / n ** 0.5).contiguous()
                h = (torch.einsum("tkj,btj->btk", G, z).median(0).values).contiguous()
                poly = (G, h, m, 0, m * n, 0, m)
                lam = lam_of(2 * nx if xbox else 0, m)
                xbnd = xb if xbox else None
                pv = low()
                tag = f"_rows{'+xbox' if xbox else ''} m={m}"
                kernels["newton_step" + tag] = lambda: be.newton_step_rows(dims, z, xn, p.F, *pp(lam), xbnd, poly, d, factor=fac)
                kernels["merit" + tag] = lambda: be.merit_rows(dims, 1, z, xn, *pp(lam), xbnd, poly, phi, rn2)
                kernels["merit_pick" + tag] = lambda: be.merit_pick_rows(dims, 20, d, xn_all, *pp(lam), xbnd, poly, zw, pv, rnorm2=rn2)
                kernels["dual_update" + tag] = dual(be.dual_update_rows, lam, xbnd, poly)
            for m in (4, 16):
                for xbox in (False, True):
                    add_rows(m, xbox)
            res = {k: [] for k in kernels}
            for _ in range(a.runs):
                for k, fn in kernels.items():
                    res[k].append(timed(fn, a.reps))
            for k, v in res.items():
                print(json.dumps(dict(dtype=str(dt).replace("torch.", ""), B=B, T=T, nx=nx, nu=nu, kernel=k,
                                      ms_median_per_run=[round(x, 5) for x in v])), flush=True)


if __name__ == "__main__":
    main()
