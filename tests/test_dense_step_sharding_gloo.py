"""Dense stage cost (with state bounds and general rows) on the callable-dynamics route with a SHARDED batch, on the CPU:
two gloo processes, each owning a slab, the test-only DenseStepOracleBackend standing in for the GPU. The reference exit is
batch-global: the norm each rank reduces is the rn2 the _dense merit kernels return, so both ranks take the Newton counts
of the unsharded solve and the gathered x, u, lam equal it bit for bit. A rank deciding on its own slab takes other counts
(asserted: that is what makes the comparison tell)."""
import os

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.test_sharding_gloo import _free_port

F64 = torch.float64
DIMS = (6, 5, 2, 1)   # B, T, nx, nu


def _solve(pr, plant, sl, **mk):
    """One MPC call on the instances of slice `sl` through DenseStepOracleBackend -> (mpc, x, u)."""
    from deq_mpc_corl_amd import QuadCost
    from deq_mpc_corl_amd.sharding import make_sharded_mpc
    from tests import dense_step_reference as dsr
    B, T, nx, nu = pr["dims"]
    c = lambda a: a[sl].contiguous()
    mpc = make_sharded_mpc(nx, nu, T, pr["lo"], pr["hi"], mk.pop("total"), mk.pop("rank"), mk.pop("world"), dtype=F64,
                           exit_mode="reference", backend=dsr.DenseStepOracleBackend(), al_iter=3, diag_cost=False,
                           ineqG=pr["G"], ineqh=c(pr["h"]), x_lower=pr["xlo"], x_upper=pr["xhi"])
    mpc.reinitialize(c(pr["x0"]), None)
    x, u, _ = mpc(c(pr["x0"]), QuadCost(c(pr["C"]), c(pr["q"])), plant, plant.jac,
                  x_init=c(pr["z0"])[..., :nx].clone(), u_init=c(pr["z0"])[..., nx:].clone())
    return mpc, x, u


def _problem():
    from tests import dense_step_reference as dsr
    B, T, nx, nu = DIMS
    pr, plant = dsr.dense_whole_problem(B, T, nx, nu, True, True, "reference")
    # the second slab is easy: no pull (q = 0), the row out of reach, a start near the origin - alone it converges sooner
    for k in ("q", "h", "x0", "z0"):
        pr[k] = pr[k].clone()
    pr["q"][B // 2:] = 0
    pr["h"][B // 2:] = 1e3
    pr["x0"][B // 2:] *= 0.01
    pr["z0"][B // 2:] *= 0.01
    return pr, plant


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)
    from deq_mpc_corl_amd.sharding import gather_batch, shard_range
    pr, plant = _problem()
    B = DIMS[0]
    lo, hi = shard_range(B, rank, world)
    mpc, x, u = _solve(pr, plant, slice(lo, hi), total=B, rank=rank, world=world)
    xg, ug, lg = gather_batch(x, B), gather_batch(u, B), gather_batch(mpc.lamda_prev, B)
    if rank == 0:
        np.savez(os.path.join(out_dir, "out.npz"), x=xg.numpy(), u=ug.numpy(), lam=lg.numpy(), npa=np.array(mpc.last_newton_per_al))
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_reference_exit_with_a_dense_cost_equals_the_unsharded_solve(tmp_path):
    from deq_mpc_corl_amd.sharding import shard_range
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    out = np.load(tmp_path / "out.npz")
    pr, plant = _problem()
    B, T, nx, nu = DIMS
    whole, x, u = _solve(pr, plant, slice(0, B), total=B, rank=0, world=1)
    assert list(out["npa"]) == list(whole.last_newton_per_al)
    assert np.array_equal(out["x"], x.numpy()) and np.array_equal(out["u"], u.numpy())
    assert np.array_equal(out["lam"], whole.lamda_prev.numpy())
    assert out["lam"].shape[1] == T * nx + T * (2 * nu + 2 * nx + 1)
    # a slab on its own decides otherwise: without the all-reduce of rn2 the counts would differ
    alone = []
    for rank in range(2):
        lo, hi = shard_range(B, rank, 2)
        alone.append(list(_solve(pr, plant, slice(lo, hi), total=hi - lo, rank=0, world=1)[0].last_newton_per_al))
    print(f"DENSESTEP sharded: Newton counts {list(out['npa'])}; the slabs alone {alone}")
    assert any(a != list(out["npa"]) for a in alone), alone
