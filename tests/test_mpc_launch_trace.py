"""Which backend calls a solve makes, in what order and on which workspace, pinned per configuration.

The MPC class runs on tests/recording_backend.py (a fake that computes nothing and records every call) over a cross
product of batch size, exit mode, exit_in_kernel, gradient, warm start, cooperative-launch outcome and dynamics kind,
plus single cases for the routes the product does not cover. Every trace is compared with
tests/golden/mpc_launch_traces.json, which holds the distinct traces and a configuration -> trace index. Two host
routes that compute the same numbers but launch differently (an extra copy-in pass, a lost ALQP_WS_PRIMED flag, the
cached workspace where the private one belongs) differ here.

`python tests/test_mpc_launch_trace.py --write` regenerates the fixture; pytest never writes it."""
import contextlib
import itertools
import json
import os
import sys
import tempfile
import warnings
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import pytest
import torch

from tests.recording_backend import RecordingBackend

FIXTURE = os.path.join(ROOT, "tests", "golden", "mpc_launch_traces.json")
T, NU = 3, 1
DT = torch.float64


class _Callable:
    """dx / dx_jac as plain callables: x_next = x."""

    def __init__(self, nx):
        self._nx = nx

    def __call__(self, x, u):
        return x.clone()

    def jac(self, x, u):
        K = x.shape[0]
        return x.clone(), (torch.eye(self._nx, dtype=DT).expand(K, -1, -1), torch.zeros(K, self._nx, NU, dtype=DT))


def _dynamics(kind, be, B, nx, fused_default=True):
    if kind == "affine":
        from deq_mpc_corl_amd import AffineDynamics
        F = torch.zeros(B, T - 1, nx, nx + NU, dtype=DT)
        be.note_caller_F(F)
        return AffineDynamics(F, torch.zeros(B, T - 1, nx, dtype=DT))
    dyn = _Callable(nx)
    if kind == "fused":
        dyn.fused_id, dyn.dt, dyn.nx, dyn.nu, dyn.fused_default = 1, 0.05, nx, NU, fused_default
    return dyn


def run_case(B=2, exit_mode="reference", exit_in_kernel="auto", grad=False, stream=False, coop_ok=True,
             dynamics="affine", fused_default=True, prefer_fused=False, state_estimator=False, obstacles=False,
             linearize_once=False, al_iter=2, rho_start=None, barrier_timeout=False, bad_info=False,
             check_numerics=None, sharded=False):
    """One solve (and its backward pass when `grad`) -> the record the fixture holds."""
    from deq_mpc_corl_amd import MPC, QuadCost
    nx = 3 if obstacles else 2   # the obstacle rows act on x[0:3]
    be = RecordingBackend(coop_ok=coop_ok, barrier_timeout=barrier_timeout, bad_info=bad_info)
    kw = dict(u_lower=torch.tensor([-1.0]), u_upper=torch.tensor([1.0]), n_batch=B, dtype=DT, exit_mode=exit_mode,
              backend=be, exit_in_kernel=exit_in_kernel, prefer_fused=prefer_fused, check_numerics=check_numerics,
              state_estimator=state_estimator)
    if obstacles:
        from deq_mpc_corl_amd.qpth.AL_mpc_custom import Obstacle_MPC
        env = SimpleNamespace(obstacle_radius=0.2, obstacle_positions=torch.arange(120, dtype=DT).reshape(40, 3))
        mpc = Obstacle_MPC(nx, NU, T, env=env, **kw)
    else:
        mpc = MPC(nx, NU, T, **kw)
    if sharded:
        mpc.process_group = torch.distributed.group.WORLD
    dyn = _dynamics(dynamics, be, B, nx, fused_default)
    x0 = torch.zeros(B, nx, dtype=DT)
    xs, us = torch.zeros(B, T, nx, dtype=DT), torch.zeros(B, T, NU, dtype=DT)
    mpc.reinitialize(xs, None)
    mpc.linearize_once = linearize_once
    if rho_start is not None:
        mpc.rho_prev = torch.full((B, 1), rho_start, dtype=DT)
    if stream:
        mpc.warm_start_initialize(xs.clone(), us.clone(), SimpleNamespace(rho_init_max=rho_start or 50.0))
    mpc.al_iter = al_iter
    Qd = torch.ones(B, T, nx + NU, dtype=DT, requires_grad=grad)
    q = torch.zeros(B, T, nx + NU, dtype=DT, requires_grad=grad)
    cost = QuadCost(torch.diag_embed(Qd), q, torch.zeros(B, T, dtype=DT))
    rec = {"calls": be.calls, "newton_per_al": None, "status": None, "rho_prev": None, "error": None, "warnings": []}
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        try:
            x, u, status = mpc(x0, cost, dyn, dyn.jac, x_init=xs.clone(), u_init=us.clone())
            rec.update(newton_per_al=list(mpc.last_newton_per_al), status=status,
                       rho_prev=mpc.rho_prev.reshape(-1).tolist())
            if grad:
                (x.sum() + u.sum()).backward()
        except Exception as e:  # noqa: BLE001  (the type is what the fixture pins)
            rec["error"] = type(e).__name__
    rec["warnings"] = sorted(w.category.__name__ for w in caught)
    return json.loads(json.dumps(rec))


def _cases():
    """name -> run_case keyword arguments; `sharded` cases need the one-rank process group."""
    cases = {}
    for B, em, eik, grad, stream, ok, dyn in itertools.product(
            (2, 8), ("fixed", "reference"), (True, False, "auto"), (False, True), (False, True), (True, False),
            ("affine", "callable", "fused")):
        name = f"B{B}/{em}/eik_{eik}/{'grad' if grad else 'nograd'}/{'stream' if stream else 'plain'}/" \
               f"{'coop' if ok else 'nocoop'}/{dyn}"
        cases[name] = dict(B=B, exit_mode=em, exit_in_kernel=eik, grad=grad, stream=stream, coop_ok=ok, dynamics=dyn)
    for em, prefer in itertools.product(("fixed", "reference"), (False, True)):
        cases[f"fused_default_False/{em}/prefer_{prefer}"] = dict(
            exit_mode=em, dynamics="fused", fused_default=False, prefer_fused=prefer, grad=True)
    for B, grad in itertools.product((2, 8), (False, True)):
        g = "grad" if grad else "nograd"
        cases[f"state_estimator/B{B}/{g}"] = dict(B=B, grad=grad, dynamics="callable", state_estimator=True)
        cases[f"obstacles/B{B}/{g}"] = dict(B=B, grad=grad, dynamics="callable", obstacles=True)
    # rho from 3e-5: it passes rho_max = 1e8 in the 13th AL iteration, so the loop's own bound (100) and al_iter = 10,
    # which this route ignores, give different traces
    for B in (2, 8):
        cases[f"linearize_once/B{B}/stream"] = dict(B=B, dynamics="callable", linearize_once=True, stream=True,
                                                    al_iter=10, rho_start=3e-5)
    for grad in (False, True):   # B == QUAD_MIN_BATCH: the first batch whose Newton direction the quad kernels give
        cases[f"quad_min_batch/{'grad' if grad else 'nograd'}"] = dict(B=4, grad=grad, dynamics="callable")
    for dyn, ok in (("affine", True), ("affine", False), ("callable", True)):
        cases[f"rho_max/{dyn}/{'coop' if ok else 'nocoop'}"] = dict(
            dynamics=dyn, coop_ok=ok, stream=True, rho_start=1e8, exit_in_kernel=True)
    # the four configurations _run rejects
    cases["reject/state_estimator_affine"] = dict(state_estimator=True, dynamics="affine")
    cases["reject/linearize_once_stream_grad"] = dict(dynamics="callable", linearize_once=True, stream=True, grad=True)
    cases["reject/linearize_once_plain"] = dict(dynamics="callable", linearize_once=True)
    cases["reject/obstacles_linearize_once"] = dict(dynamics="callable", obstacles=True, linearize_once=True,
                                                    stream=True)
    for dyn in ("affine", "fused"):
        cases[f"barrier_timeout/{dyn}"] = dict(dynamics=dyn, exit_in_kernel=True, barrier_timeout=True)
    for cn in ("warn", "raise"):
        cases[f"check_numerics/{cn}"] = dict(dynamics="affine", exit_mode="fixed", bad_info=True, check_numerics=cn)
    for dyn, stream in (("affine", False), ("affine", True), ("callable", False), ("fused", False)):
        cases[f"sharded/{dyn}/{'stream' if stream else 'plain'}"] = dict(
            dynamics=dyn, stream=stream, exit_in_kernel=True, sharded=True)
    return cases


CASES = _cases()


@contextlib.contextmanager
def one_rank_group(directory):
    """A one-rank gloo group from a file store (no network, no spawn): MPC._sharded() is true with it."""
    import torch.distributed as dist
    dist.init_process_group("gloo", store=dist.FileStore(os.path.join(str(directory), "store"), 1), rank=0,
                            world_size=1)
    try:
        yield
    finally:
        dist.destroy_process_group()


def _run_all(names, directory):
    out = {n: run_case(**CASES[n]) for n in names if not CASES[n].get("sharded")}
    sharded = [n for n in names if CASES[n].get("sharded")]
    if sharded:
        with one_rank_group(directory):
            out.update((n, run_case(**CASES[n])) for n in sharded)
    return out


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def traces(tmp_path_factory):
    return _run_all(list(CASES), tmp_path_factory.mktemp("gloo"))


def test_fixture_covers_exactly_these_configurations(golden):
    assert sorted(golden["configs"]) == sorted(CASES)
    assert sorted(set(golden["configs"].values())) == list(range(len(golden["traces"])))


@pytest.mark.parametrize("group", sorted({n.split("/")[0] for n in CASES}))
def test_launch_trace_matches_fixture(group, golden, traces):
    bad = []
    for name in (n for n in CASES if n.split("/")[0] == group):
        want, got = golden["traces"][golden["configs"][name]], traces[name]
        if got != want:
            diff = [k for k in want if k != "calls" and got[k] != want[k]]
            first = next((i for i, (a, b) in enumerate(zip(got["calls"], want["calls"])) if a != b),
                         min(len(got["calls"]), len(want["calls"])))
            bad.append(f"{name}: differs in {diff}, calls {len(got['calls'])} vs {len(want['calls'])} in the fixture, "
                       f"first difference at call {first}: {got['calls'][first:first + 1]} vs "
                       f"{want['calls'][first:first + 1]}")
    assert not bad, "\n".join(bad)


def test_cases_reach_what_they_are_named_for(traces):
    """Guards the test's own set-up: a case that died early for another reason would pin nothing."""
    err = {n: t["error"] for n, t in traces.items()}
    assert all(err[n] is None for n in CASES if n.startswith("B")), {n: e for n, e in err.items() if n[0] == "B" and e}
    assert err["reject/state_estimator_affine"] == "NotImplementedError"
    assert err["reject/linearize_once_stream_grad"] == "RuntimeError"
    assert err["reject/linearize_once_plain"] == "TypeError"
    assert err["reject/obstacles_linearize_once"] == "NotImplementedError"
    assert err["barrier_timeout/affine"] == err["barrier_timeout/fused"] == "RuntimeError"
    assert err["check_numerics/raise"] == "FloatingPointError"
    assert traces["check_numerics/warn"]["warnings"] == ["RuntimeWarning"] and err["check_numerics/warn"] is None
    assert all(traces[n]["status"] is True for n in CASES if n.startswith("rho_max/"))
    assert all(err[n] is None for n in CASES if n.split("/")[0] in (
        "sharded", "rho_max", "state_estimator", "obstacles", "linearize_once", "fused_default_False",
        "quad_min_batch"))
    for B in (2, 8):   # the frozen-linearisation loop runs past al_iter = 10 and ends on rho_max
        t = traces[f"linearize_once/B{B}/stream"]
        assert len(t["newton_per_al"]) == 13 and t["status"] is True
    # B = 8 launches on the quad kernels' cached workspace: primed within an AL iteration, and not after the PyTorch
    # dual update that changed lam / rho behind its records
    calls = traces["linearize_once/B8/stream"]["calls"]
    lin = [i for i, c in enumerate(calls) if c[0] == "solve_lin"]
    second = next(k for k, i in enumerate(lin) if calls[i - 1][0] == "dual_update")   # first of AL iteration 2
    assert "WS_PRIMED" in calls[lin[1]][3] and "WS_PRIMED" in calls[lin[second + 1]][3]
    assert "WS_PRIMED" not in calls[lin[second]][3]
    assert traces["quad_min_batch/nograd"]["calls"] != traces["B2/reference/eik_auto/nograd/plain/coop/callable"]["calls"]


def write_fixture():
    with tempfile.TemporaryDirectory() as d:
        traces = _run_all(list(CASES), d)
    index, configs = {}, {}
    for name in CASES:
        configs[name] = index.setdefault(json.dumps(traces[name]), len(index))
    with open(FIXTURE, "w") as f:
        f.write('{"traces": [\n' + ",\n".join(index) + '\n],\n"configs": {\n')
        f.write(",\n".join(f"{json.dumps(n)}: {i}" for n, i in configs.items()) + "\n}}\n")
    print(f"{len(configs)} configurations, {len(index)} distinct traces -> {FIXTURE}")


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_mpc_launch_trace.py --write")
    write_fixture()
