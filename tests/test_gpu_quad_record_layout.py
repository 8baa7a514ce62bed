"""Quad solve through the wave-interleaved workspace records: a full headline-size batch and a ragged one (B not a
multiple of 16 or of 2: the last record pair is half used), a sample of instances checked against the CPU oracle."""
import numpy as np
import pytest
import torch

from oracle import oracle_py as orc

DEV = "cuda:0"
TD = {"f32": torch.float32, "f64": torch.float64}


@pytest.mark.gpu
@pytest.mark.parametrize("B", [16384, 4099])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_quad_layout_batch_against_oracle_sample(dtype, B):
    from deq_mpc_corl_amd import synthetic_problem
    from deq_mpc_corl_amd.backend import default_backend
    be = default_backend()
    dt = TD[dtype]
    T, nx, nu = 20, 13, 4
    p = synthetic_problem(B, T, nx, nu, seed=11, dtype=dt, device=DEV)
    M = T * nx + 2 * T * nu
    z = p.z0.clone()
    lam = torch.zeros(B, M, dtype=dt, device=DEV)
    rho = torch.ones(B, dtype=dt, device=DEV)
    phi = torch.zeros(B, dtype=dt, device=DEV)
    rn2 = torch.zeros(B, dtype=dt, device=DEV)
    info = torch.zeros(B, dtype=torch.int32, device=DEV)
    st = torch.zeros(B, dtype=torch.uint8, device=DEV)
    be.solve_lin((B, T, nx, nu), p.Qd, p.q, p.F, p.c, p.x0, p.u_lo, p.u_hi, 0, 0, z, lam, rho, phi, rn2,
                 info, st, al_iter=2, max_newton=4, n_ls=20, flags=3, variant="quad")
    torch.cuda.synchronize()
    assert be.last_variant == "quad"
    # both halves of the first pairs, the last (half-used) pair, the last wave, and a spread in between
    idx = np.unique(np.concatenate([np.arange(4), np.arange(B - 18, B), np.linspace(4, B - 19, 10).astype(int)]))
    assert len(idx) == 32
    c = lambda a: a.cpu().numpy()
    s = lambda a: c(a)[idx]
    u_lo = s(p.u_lo) if p.u_lo.dim() > 0 and p.u_lo.shape[0] == B else c(p.u_lo)
    u_hi = s(p.u_hi) if p.u_hi.dim() > 0 and p.u_hi.shape[0] == B else c(p.u_hi)
    o = orc.solve_lin(dtype, s(p.Qd), s(p.q), s(p.F), s(p.c), s(p.x0), u_lo, u_hi, s(p.z0), al_iter=2,
                      exit_mode="fixed")
    assert int(info.abs().sum()) == 0
    assert bool(st.all())
    err = np.abs(s(z) - o["z"]).reshape(len(idx), -1).max(1)
    assert np.isfinite(s(z)).all() and np.isfinite(s(lam)).all()
    if dtype == "f64":
        assert err.max() < 1e-9, err
    else:
        # fp32: an instance whose line search has a near-tie may take another step than the oracle
        assert np.median(err) < 1e-5 and (err >= 2e-3).sum() <= 3, np.sort(err)[-6:]
