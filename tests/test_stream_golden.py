"""Streaming / warm-start route against fixtures made by RUNNING the reference
(tools/gen_golden_stream.py): `al_solve_stream` (qpth/AL_mpc.py:342-423), `warm_start_initialize`
(:581-592), `linearize_once` (:370-391, qpth/al_utils_lin.py:140-189) and the same sequence
through `policies.Tracking_MPC` (policies.py:1236-1310).

Each fixture is replayed twice: on the CPU with the TEST-ONLY oracle backend (checks the host logic
and the oracle; not gpu) and on the MI355X through the C ABI (`-m gpu`). Compared per stream call:
number of AL iterations executed, Newton steps per AL iteration, x, u, status, lamda, rho.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import golden_util as gu

TD = {"f64": torch.float64, "f32": torch.float32}

STREAM = ["pend_stream_f64", "pend_stream_lin_f64", "cart_stream_f64", "cart_stream_lin_f64",
          "cart_stream_active_f64", "quad13_stream_lin_f64", "pend1l_casadi_stream_lin_f64",
          "cart1l_casadi_stream_f64", "cart1l_casadi_stream_lin_f64"]


def _load(name):
    g = gu.load(name)
    for k in ("linearize_once", "al_iter_first", "al_iter_stream", "stream_calls"):
        if k in g:
            g[k] = int(g[k])
    if "kind" in g:
        g["kind"] = str(g["kind"])
    return g


def _dynamics(kind, g, dt, dev):
    """The fixture's dynamics: on the GPU the provider kernels (the product), on the CPU the
    restated models of oracle/dyn_oracle.c (test infrastructure)."""
    from deq_mpc_corl_amd import AffineDynamics, PendulumDynamics
    tt = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dt).to(dev)
    if kind == "affine":
        return AffineDynamics(tt(g["F"]), tt(g["c"]))
    if kind == "pendulum":
        return PendulumDynamics()
    if dev != "cpu":
        from deq_mpc_corl_amd import Cartpole1lDynamics, Pendulum1lDynamics
        return Pendulum1lDynamics(0.05) if kind == "casadi_pendulum1l" else Cartpole1lDynamics(0.05)
    from oracle import dyn_py
    dyn_py.build()

    class Dyn:
        def __call__(self, x, u):
            return self.jac(x, u)[0]

        def jac(self, x, u):
            xn_, un_ = x.detach().double().numpy(), u.detach().double().numpy()
            if kind == "casadi_pendulum1l":
                xn, A, Bm = dyn_py.pendulum1l(xn_, un_, 0.05)
            else:
                xn, J = dyn_py.cartpole1l(xn_, np.concatenate([un_, np.zeros((un_.shape[0], 1))], 1), 0.05)
                A, Bm = J[:, :, :4].copy(), J[:, :, 4:5].copy()
            return torch.from_numpy(xn).to(x.dtype), (torch.from_numpy(A).to(x.dtype), torch.from_numpy(Bm).to(x.dtype))

    return Dyn()


def _replay_stream(name, backend, dev, newton_rho_max=None):
    from deq_mpc_corl_amd import MPC, QuadCost
    g = _load(name)
    dt = TD[g["dtype"]]
    B, T, nx, nu = g["B"], g["T"], g["nx"], g["nu"]
    tt = lambda a, d=dt: torch.as_tensor(np.ascontiguousarray(a)).to(d).to(dev)
    c = lambda a: a.detach().cpu().numpy()
    dyn = _dynamics(g["kind"], g, dt, dev)
    mpc = MPC(nx, nu, T, u_lower=tt(g["u_lo"]), u_upper=tt(g["u_hi"]), n_batch=B, dtype=dt, backend=backend)
    x0 = tt(g["x0"])
    Qd = tt(g["Qd"])
    zeros = torch.zeros(B, T, dtype=dt, device=dev)
    mpc.reinitialize(x0, None)
    mpc.al_iter = g["al_iter_first"]
    z0 = tt(g["z0"])
    x, u, st = mpc(x0, QuadCost(torch.diag_embed(Qd), tt(g["q0"]), zeros), dyn, dyn.jac,
                   x_init=z0[..., :nx].clone(), u_init=z0[..., nx:].clone())
    f64 = g["dtype"] == "f64"
    tol = 2e-5 if f64 else 5e-3
    assert st is False
    assert list(mpc.last_newton_per_al) == g["newton_first"].tolist()
    assert np.abs(c(x) - g["x_first"]).max() < tol and np.abs(c(u) - g["u_first"]).max() < tol
    assert np.array_equal(c(mpc.rho_prev), g["rho_first"])
    # warm start exactly as recorded (the reference's own fp32 iterate with the last stage replaced)
    mpc.warm_start_initialize(tt(g["x_warm"], torch.float32), tt(g["u_warm"], torch.float32),
                              SimpleNamespace(rho_init_max=float(g["rho_init_max"])))
    assert mpc.warm_starting is True
    assert float(mpc.lamda_prev.abs().max()) == 0.0
    assert np.array_equal(c(mpc.rho_prev), g["rho_after_warm"])
    mpc.linearize_once = bool(g["linearize_once"])
    for ci in range(g["stream_calls"]):
        mpc.al_iter = g["al_iter_stream"]
        x, u, st = mpc(x0, QuadCost(torch.diag_embed(Qd), tt(g["q"][ci]), zeros), dyn, dyn.jac)
        want_newton = g["newton"][g["ap_call"] == ci].tolist()
        assert len(mpc.last_newton_per_al) == int(g["n_al"][ci]), (ci, mpc.last_newton_per_al, want_newton)
        got_newton = list(mpc.last_newton_per_al)
        if newton_rho_max is not None:   # fp32: Newton counts are only comparable while rho is fp32-meaningful
            keep = (g["ap_rho"][g["ap_call"] == ci].reshape(len(want_newton), -1).max(1) <= newton_rho_max).tolist()
            got_newton = [a for a, k in zip(got_newton, keep) if k]
            want_newton = [a for a, k in zip(want_newton, keep) if k]
        assert got_newton == want_newton, (ci, mpc.last_newton_per_al, want_newton)
        assert st is bool(g["status"][ci])
        assert x.dtype == torch.float32 and u.dtype == torch.float32
        assert np.array_equal(c(mpc.rho_prev), g["rho"][ci])
        if f64:
            ex, eu = np.abs(c(x) - g["x"][ci]).max(), np.abs(c(u) - g["u"][ci]).max()
            assert ex < 2e-5 and eu < 2e-5, (ci, ex, eu)
            lam, lam_ref = c(mpc.lamda_prev), g["lam"][ci]
            assert np.abs(lam - lam_ref).max() < 1e-4 * max(1.0, np.abs(lam_ref).max()), (ci, np.abs(lam - lam_ref).max())
        else:
            assert np.isfinite(c(x)).all() and np.isfinite(c(u)).all()
    return mpc


@pytest.mark.parametrize("name", STREAM)
def test_stream_host_logic_vs_reference_cpu(name):
    from tests.oracle_backend import OracleBackend
    _replay_stream(name, OracleBackend(), "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("name", STREAM)
def test_stream_hip_vs_reference(name):
    """The same fixtures through HipBackend (team kernels at these batch sizes)."""
    _replay_stream(name, None, "cuda:0")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cart_stream_f64", "cart_stream_lin_f64", "quad13_stream_lin_f64",
                                  "cart_stream_active_f64"])
def test_stream_hip_quad_variant_vs_reference(name):
    """...and with the headline (quad) kernel forced, as it runs from B = 4096 on."""
    from deq_mpc_corl_amd.backend import HipBackend
    be = HipBackend()
    be.default_variant = "quad"
    _replay_stream(name, be, "cuda:0")


def test_stream_lin_f32_iteration_counts_cpu():
    """fp32 at rho up to 1e10 is numerically meaningless for x/u, but the control
    flow - iterations until the batch-mean residual stops decreasing or rho passes 1e8 - is the
    reference's own fp32 run."""
    from tests.oracle_backend import OracleBackend
    g = _load("pend_stream_lin_f32")
    assert g["status"].tolist() == [1, 1]
    # AL-iteration counts, status and rho exactly; Newton-step counts while rho <= 1e5 (beyond that the
    # batch-global 1e-3 tests are decided by fp32 rounding: 4 vs 3 steps at rho = 1e8 in this fixture)
    _replay_stream("pend_stream_lin_f32", OracleBackend(), "cpu", newton_rho_max=1e5)


@pytest.mark.gpu
def test_stream_lin_f32_iteration_counts_hip():
    _replay_stream("pend_stream_lin_f32", None, "cuda:0", newton_rho_max=1e5)


def test_linearize_once_outside_stream_raises_like_the_reference():
    """al_solve with linearize_once=True dies in the reference with TypeError ('dict' object is not
    callable, al_utils.py:237 reached from AL_mpc.py:303); the linearize_once stream route cannot be
    differentiated there (al_utils_lin.NewtonAL.backward: wrong number of gradients)."""
    from deq_mpc_corl_amd import MPC, QuadCost, PendulumDynamics
    from tests.oracle_backend import OracleBackend
    g = _load("pend_stream_lin_f64")
    dt = torch.float64
    tt = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dt)
    B, T, nx, nu = g["B"], g["T"], g["nx"], g["nu"]
    dyn = PendulumDynamics()
    mpc = MPC(nx, nu, T, u_lower=tt(g["u_lo"]), u_upper=tt(g["u_hi"]), n_batch=B, dtype=dt, backend=OracleBackend())
    mpc.reinitialize(tt(g["x0"]), None)
    mpc.linearize_once = True
    cost = QuadCost(torch.diag_embed(tt(g["Qd"])), tt(g["q0"]), torch.zeros(B, T, dtype=dt))
    with pytest.raises(TypeError):
        mpc(tt(g["x0"]), cost, dyn, dyn.jac)
    mpc.linearize_once = False
    mpc(tt(g["x0"]), cost, dyn, dyn.jac)
    mpc.warm_start_initialize(mpc.x_init, mpc.u_init, SimpleNamespace(rho_init_max=1e4))
    mpc.linearize_once = True
    q = tt(g["q"][0]).requires_grad_(True)
    with pytest.raises(RuntimeError):
        mpc(tt(g["x0"]), QuadCost(torch.diag_embed(tt(g["Qd"])), q, torch.zeros(B, T, dtype=dt)), dyn, dyn.jac)


# ---- the adapter: policies.Tracking_MPC's call sequence, restated in a few lines -----------------
class _TrackingAdapter:
    """What the reference's Tracking_MPC does around the solver (policies.py:1236-1310), so that the
    recorded traces can be replayed without the reference. The traces were recorded from the unchanged
    reference class (tools/gen_golden.py, tools/gen_golden_stream.py)."""

    def __init__(self, ctrl, B, T, nx, nu, dt, dev):
        self.ctrl, self.x_init, self.u_init = ctrl, None, None
        qd = torch.cat([torch.full((nx,), 10.0), torch.full((nu,), 1e-8)]).to(dt).to(dev)
        self.Q = torch.diag(qd).repeat(B, T, 1, 1)

    def reinitialize(self, x, mask):
        self.x_init = None
        self.ctrl.reinitialize(x, mask)

    def warm_start_initialize(self, x_ref, u_ref, args):
        self.u_init, self.x_init = self.ctrl.u_init, self.ctrl.x_init
        self.u_init[:, -1:] = u_ref[:, -1:]
        self.x_init[:, -1:] = x_ref[:, -1:]
        self.ctrl.warm_start_initialize(self.x_init, self.u_init, args)

    def __call__(self, x0, x_ref, u_ref, dyn, al_iters=2):
        from deq_mpc_corl_amd import QuadCost
        xu_ref = torch.cat([x_ref, u_ref], -1)
        if self.x_init is None:
            self.x_init = self.ctrl.x_init = x_ref.detach().clone()
            self.u_init = self.ctrl.u_init = u_ref.detach().clone()
        p = -(self.Q * xu_ref.unsqueeze(-2)).sum(-1)
        f = 0.5 * (xu_ref * (self.Q * xu_ref.unsqueeze(-2)).sum(-1)).sum(-1)
        self.ctrl.al_iter = al_iters
        x, u, st = self.ctrl(x0, QuadCost(self.Q, p, f), dyn, dyn.jac, None)
        self.u_init = u.clone().detach()
        return x, u, st


def _replay_tracking(name, backend, dev):
    from deq_mpc_corl_amd import MPC, AffineDynamics
    g = gu.load(name)
    dt = torch.float64
    B, T, nx, nu = int(g["B"]), int(g["T"]), int(g["nx"]), int(g["nu"])
    tt = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dt).to(dev)
    dyn = AffineDynamics(tt(g["F"]), tt(g["c"]))
    ctrl = MPC(nx, nu, T, u_lower=torch.full((nu,), -0.5, device=dev), u_upper=torch.full((nu,), 0.5, device=dev),
               exit_unconverged=False, eps=1e-2, n_batch=B, backprop=False, verbose=0,
               u_init=torch.randn(B, T, nu, dtype=dt, device=dev), solver_type="dense", dtype=dt,
               state_estimator=False, backend=backend)
    tm = _TrackingAdapter(ctrl, B, T, nx, nu, dt, dev)
    x0, u_ref = tt(g["x0"]), tt(g["u_ref"])
    tm.reinitialize(tt(g["x_ref"][0]), torch.ones(B, T, 1, dtype=dt, device=dev))
    phase = g["phase"].tolist() if "phase" in g else [0] * g["x"].shape[0]
    warmed = False
    for i, ph in enumerate(phase):
        if ph == 1 and not warmed:
            tm.warm_start_initialize(tt(g["x_ref_warm"]), u_ref, SimpleNamespace(rho_init_max=float(g["rho_init_max"])))
            ctrl.linearize_once = bool(int(g["linearize_once"]))
            warmed = True
        x, u, st = tm(x0, tt(g["x_ref"][i]), u_ref, dyn)
        if "status" in g:
            assert st is bool(g["status"][i]), (i, st)
            assert np.array_equal(ctrl.rho_prev.cpu().numpy(), g["rho"][i]), i
        ex = np.abs(x.cpu().numpy() - g["x"][i]).max()
        eu = np.abs(u.cpu().numpy() - g["u"][i]).max()
        assert ex < 1e-4 and eu < 1e-4, (i, ex, eu)
    lam, lam_ref = ctrl.lamda_prev.cpu().numpy(), g["lam"]
    assert np.abs(lam - lam_ref).max() < 1e-4 * max(1.0, np.abs(lam_ref).max())


TRACKING = ["cart_tracking_f64", "cart_tracking_stream_f64", "cart_tracking_stream_lin_f64"]


@pytest.mark.parametrize("name", TRACKING)
def test_tracking_adapter_trace_cpu(name):
    from tests.oracle_backend import OracleBackend
    _replay_tracking(name, OracleBackend(), "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("name", TRACKING)
@pytest.mark.parametrize("variant", ["auto", "quad"])
def test_tracking_adapter_trace_hip(name, variant):
    """Tracking_MPC's recorded traces (plain, streaming, streaming + linearize_once) through HipBackend."""
    from deq_mpc_corl_amd.backend import HipBackend
    be = HipBackend()
    be.default_variant = variant
    _replay_tracking(name, be, "cuda:0")
