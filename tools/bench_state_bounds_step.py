#!/usr/bin/env python3
"""ms per launch of the four state-bound launch-per-step kernels (alqp_newton_step_xbox, alqp_merit_xbox,
alqp_merit_pick_xbox, alqp_dual_update_xbox) against their plain twins on the same problem without state bounds
(DESIGN section 24). T = 20, (nx, nu) = (13, 4), B = 200 and B = 16384, fp32 and fp64, |x| <= 0.6 on every state and
stage (the [nx] form). Also, for information, the plain QUAD step at B = 16384 (alqp_newton_step with a workspace): the
kernel a large batch gives up when it has state bounds.

HIP events around each launch, median of 30 after 5 warm-up launches, three runs with the kernels alternated (one run
times every kernel once before the next run starts). One JSON line per (dtype, B, kernel) with the three medians.
    python tools/bench_state_bounds_step.py [--reps 30] [--runs 3]"""
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
            Mp, Mx = T * nx + 2 * T * nu, T * nx + T * (2 * nu + 2 * nx)
            lam_x = (0.3 * rnd(B, Mx)).contiguous()
            lam_x[:, T * nx:].clamp_(min=0)
            li = lam_x[:, T * nx:].reshape(B, T, 2 * nu + 2 * nx)
            lam_p = torch.cat([lam_x[:, :T * nx], li[..., :2 * nu].reshape(B, -1)], 1).contiguous()
            assert lam_p.shape[1] == Mp
            rho = torch.full((B,), 10.0, dtype=dt, device=dev)
            xb = (torch.full((nx,), -0.6, dtype=dt, device=dev), torch.full((nx,), 0.6, dtype=dt, device=dev), 0, 0)
            d = torch.empty(B, T, n, dtype=dt, device=dev)
            fac = torch.empty(B, T, n * (n + 1) // 2, dtype=dt, device=dev)
            phi, rn2 = torch.zeros(B, dtype=dt, device=dev), torch.zeros(B, dtype=dt, device=dev)
            pp = lambda lam: (p.x0, lam, rho, p.Qd, p.q, p.u_lo, p.u_hi, 0, 0)
            be.newton_step(dims, z, xn, p.F, *pp(lam_p), d)
            al = (2.0 ** -torch.arange(20, device=dev, dtype=dt)).view(20, 1, 1, 1)
            xn_all = (torch.einsum("btij,kbtj->kbti", p.F, (z.unsqueeze(0) + al * d.unsqueeze(0))[:, :, :-1]) + p.c).contiguous()
            # phi_prev below every merit at the first launch and the minimum itself from then on: the pick never moves z
            prev_p, prev_x = (torch.full((B,), -1e30, dtype=dt, device=dev) for _ in range(2))
            zw = z.clone()

            def dual(xbox):
                lam = (lam_x if xbox else lam_p).clone()
                r = rho.clone()
                if xbox:
                    return lambda: be.dual_update_xbox(dims, z, xn, p.x0, p.u_lo, p.u_hi, 0, 0, xb, lam, r, 1.0)
                return lambda: be.dual_update(dims, z, xn, p.x0, p.u_lo, p.u_hi, 0, 0, lam, r, 1.0)
            kernels = {
                "newton_step": lambda: be.newton_step(dims, z, xn, p.F, *pp(lam_p), d, factor=fac),
                "newton_step_xbox": lambda: be.newton_step_xbox(dims, z, xn, p.F, *pp(lam_x), xb, d, factor=fac),
                "merit": lambda: be.merit(dims, 1, z, xn, *pp(lam_p), phi, rn2),
                "merit_xbox": lambda: be.merit_xbox(dims, 1, z, xn, *pp(lam_x), xb, phi, rn2),
                "merit_pick": lambda: be.merit_pick(dims, 20, d, xn_all, *pp(lam_p), zw, prev_p, rnorm2=rn2),
                "merit_pick_xbox": lambda: be.merit_pick_xbox(dims, 20, d, xn_all, *pp(lam_x), xb, zw, prev_x, rnorm2=rn2),
                "dual_update": dual(False),
                "dual_update_xbox": dual(True),
            }
            if B == 16384:
                ws = be.new_workspace(dims, z)
                kernels["newton_step_quad (information)"] = lambda: be.newton_step(dims, z, xn, p.F, *pp(lam_p), d, workspace=ws)
            res = {k: [] for k in kernels}
            for _ in range(a.runs):
                for k, fn in kernels.items():
                    res[k].append(timed(fn, a.reps))
            for k, v in res.items():
                print(json.dumps(dict(dtype=str(dt).replace("torch.", ""), B=B, T=T, nx=nx, nu=nu, kernel=k,
                                      ms_median_per_run=[round(x, 5) for x in v])), flush=True)


if __name__ == "__main__":
    main()
