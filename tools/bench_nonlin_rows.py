#!/usr/bin/env python3
"""ms per MPC.__call__ with state bounds on a provider with a compiled-in model: the launch-per-step route (the provider
wrapped so that it has no fused_id: provider kernels between the four launch-per-step kernels, what the library ran
before DESIGN section 28) against the one-launch route on the team kernel (HipBackend.solve_nonlin_rows).

pendulum1l and cartpole1l, T = 20, |x| bounded on every stage (the [nx] form), bsz 200 and B = 4096, fp32 and fp64, both
exit modes. HIP events around each call, median of 30 after 5 warm-up calls, the two routes alternated three times. One
JSON line per (model, dtype, B, exit mode) with the three medians of each route; the routing rule of section 28 reads the
medians of these rows.
    python tools/bench_nonlin_rows.py [--reps 30] [--runs 3] [--modes fixed,reference]"""
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


class Plain:
    """The provider without its fused_id: the launch-per-step route."""

    def __init__(self, prov):
        self.prov = prov

    def __call__(self, x, u):
        return self.prov(x, u)

    def jac(self, x, u):
        return self.prov.jac(x, u)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--modes", default="fixed,reference")
    a = ap.parse_args()
    from deq_mpc_corl_amd import MPC, QuadCost
    from deq_mpc_corl_amd.dynamics import Cartpole1lDynamics, Pendulum1lDynamics
    dev, T = "cuda:0", 20
    for model, cls, nx in (("pendulum1l", Pendulum1lDynamics, 2), ("cartpole1l", Cartpole1lDynamics, 4)):
        n = nx + 1
        for dt in (torch.float32, torch.float64):
            for B in (200, 4096):
                g = torch.Generator().manual_seed(7)
                x0 = (0.2 * torch.randn(B, nx, generator=g)).to(dt).to(dev)
                Qd = (1.0 + torch.rand(B, T, n, generator=g)).to(dt).to(dev)
                q = (0.5 * torch.randn(B, T, n, generator=g)).to(dt).to(dev)
                xb = torch.full((nx,), 0.5, dtype=dt, device=dev)   # |x| <= 0.5 on every stage; x0 is inside
                prov = cls(0.05)
                cost = QuadCost(torch.diag_embed(Qd), q, torch.zeros(B, T, dtype=dt, device=dev))
                for mode in a.modes.split(","):
                    calls = {}
                    for name, dyn in (("per_step", Plain(prov)), ("one_launch", prov)):
                        mpc = MPC(nx, 1, T, u_lower=-3.0, u_upper=3.0, x_lower=-xb, x_upper=xb, n_batch=B, dtype=dt,
                                  exit_mode=mode, prefer_fused=True)

                        def call(mpc=mpc, dyn=dyn):
                            mpc.reinitialize(x0, None)
                            mpc(x0, cost, dyn, dyn.jac)
                        calls[name] = call
                    med = {k: [] for k in calls}
                    for _ in range(a.runs):
                        for k, fn in calls.items():
                            med[k].append(round(timed(fn, a.reps), 4))
                    print(json.dumps(dict(model=model, dtype=str(dt).split(".")[-1], B=B, T=T, exit_mode=mode, ms=med)), flush=True)


if __name__ == "__main__":
    main()
