"""CPU checks of the C-ABI boundary: the shared library loads without a GPU, exports
every symbol include/mi_alqp.h declares, and rejects bad input before any launch."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    txt = open(os.path.join(ROOT, "include", "mi_alqp.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(alqp_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol():
    from deq_mpc_corl_amd import _lib
    lib = _lib.load()
    syms = declared_symbols()
    assert len(syms) >= 17
    for s in syms:
        assert hasattr(lib, s), s
    assert sorted(syms) == sorted(_lib.EXPORTED_SYMBOLS)
    assert lib.alqp_abi_version() == _lib.ABI_VERSION
    # the suffix variants that became nullable arguments: neither declared nor exported any more
    for op, suffixes in (("newton_step", ("obs", "ws", "ws_obs")), ("merit", ("obs",)), ("dual_update", ("obs",)),
                         ("backward", ("ws", "dyn", "ws_dyn"))):
        for stem in (f"alqp_{op}_{x}" for x in suffixes):
            for s in (stem + "_f32", stem + "_f64"):
                assert s not in syms and s not in _lib.EXPORTED_SYMBOLS and not hasattr(lib, s), s


def test_supported_dims_and_lds_budget():
    from deq_mpc_corl_amd import _lib
    lib = _lib.load()
    q = lambda *d: (lib.alqp_supported(C.byref(_lib.AlqpDims(*d)), 0), lib.alqp_supported(C.byref(_lib.AlqpDims(*d)), 1))
    assert q(16384, 20, 13, 4) == (1, 1)
    assert q(128, 5, 2, 1) == (1, 1)
    assert q(8192, 10, 8, 2) == (1, 1)
    assert q(65536, 50, 13, 4) == (1, 1)
    assert q(4, 20, 7, 3) == (0, 0)            # not instantiated
    assert q(4, 1, 13, 4) == (0, 0)            # T < 2
    assert q(4, 400, 13, 4) == (1, 1)          # too long for the team's LDS image, but the quad variant runs it
    v = lambda var, *d: lib.alqp_supported_variant(C.byref(_lib.AlqpDims(*d)), 0, var)
    assert v(1, 4, 400, 13, 4) == 0 and v(2, 4, 400, 13, 4) == 1
    assert v(1, 4, 20, 13, 4) == 1 and v(2, 4, 20, 13, 4) == 1 and v(3, 4, 20, 13, 4) == 0
    d = _lib.AlqpDims(1, 20, 13, 4)
    assert 0 < lib.alqp_lds_bytes(C.byref(d), 0) <= 160 * 1024
    assert lib.alqp_qps_per_wave(C.byref(d), 0) == 1
    assert lib.alqp_qps_per_wave(C.byref(_lib.AlqpDims(1, 5, 2, 1)), 0) == 4
    # quad variant workspace: one record per (instance, stage)
    w = lib.alqp_workspace_bytes(C.byref(_lib.AlqpDims(16384, 20, 13, 4)), 0)
    assert w == 16384 * 20 * 352 * 4
    assert lib.alqp_workspace_bytes(C.byref(_lib.AlqpDims(4, 20, 7, 3)), 0) == 0


# (dims, is_f64, flags, expected) at quad_min_batch = -1: alqp_pick_variant's table on both sides of each threshold
# (ALQP_SAVE_FACTOR -> team; else quad from the table's batch on, or when the team's LDS image does not fit; the
# whole-wavefront team (13,4) and the shared-wavefront team (8,2) have thresholds of their own, (8,2) one per dtype)
SAVE_FACTOR = 4
PICK_TABLE = (
    [((B, 20, 13, 4), f64, 0, v) for f64 in (0, 1) for B, v in ((4096, 1), (4097, 2))] +
    [((4095, 10, 8, 2), 0, 0, 1), ((4096, 10, 8, 2), 0, 0, 2), ((4607, 10, 8, 2), 1, 0, 1), ((4608, 10, 8, 2), 1, 0, 2),
     ((16384, 20, 13, 4), 0, SAVE_FACTOR, 1),
     ((4, 400, 13, 4), 0, 0, 2)] +                                      # the team image does not fit
    [((B, 20, 7, 3), f64, fl, 0) for B in (4, 16384) for f64 in (0, 1) for fl in (0, SAVE_FACTOR)])   # no instance


def test_pick_variant_table_and_override():
    from deq_mpc_corl_amd import _lib
    lib = _lib.load()
    assert _lib.ALQP_SAVE_FACTOR == SAVE_FACTOR
    pick = lambda dims, f64, flags, qmin: lib.alqp_pick_variant(C.byref(_lib.AlqpDims(*dims)), f64, flags, qmin)
    for dims, f64, flags, want in PICK_TABLE:
        assert pick(dims, f64, flags, -1) == want, (dims, f64, flags)
    # quad_min_batch >= 0 replaces the table's threshold, nothing else
    assert pick((1, 20, 13, 4), 0, 0, 0) == 2
    assert pick((16384, 20, 13, 4), 0, 0, 1 << 40) == 1
    assert pick((4, 400, 13, 4), 0, 0, 1 << 40) == 2


def test_backend_pick_variant_agrees_with_the_library():
    """HipBackend._pick_variant: the library's table at the default QUAD_MIN_BATCH, the attribute as override otherwise.
    The constructor only loads the library: no device needed."""
    import torch
    from deq_mpc_corl_amd import _lib
    from deq_mpc_corl_amd.backend import HipBackend
    be = HipBackend()
    assert be.QUAD_MIN_BATCH == 4096
    dtype = lambda f64: torch.float64 if f64 else torch.float32
    for dims, f64, flags, want in PICK_TABLE:
        assert be._pick_variant(dims, dtype(f64), flags) == want, (dims, f64, flags)
    try:
        for qmin in (0, 1, 1 << 40):
            be.QUAD_MIN_BATCH = qmin
            for dims, f64, flags, _ in PICK_TABLE + [((1, 20, 13, 4), 0, 0, None), ((16384, 20, 13, 4), 1, 0, None)]:
                want = be.lib.alqp_pick_variant(C.byref(_lib.AlqpDims(*dims)), f64, flags, qmin)
                assert be._pick_variant(dims, dtype(f64), flags) == want, (qmin, dims, f64, flags)
            assert be._pick_variant((1, 20, 13, 4), torch.float32, 0) == (2 if qmin <= 1 else 1)
            assert be._pick_variant((16384, 20, 13, 4), torch.float32, 0) == (1 if qmin == 1 << 40 else 2)
            assert be._pick_variant((4, 400, 13, 4), torch.float32, 0) == 2
            assert be._pick_variant((16384, 20, 13, 4), torch.float32, SAVE_FACTOR) == 1
    finally:
        del be.QUAD_MIN_BATCH   # back to the class default
    assert be.QUAD_MIN_BATCH == 4096


def test_bad_arguments_are_rejected_without_a_launch():
    from deq_mpc_corl_amd import _lib
    lib = _lib.load()
    d = _lib.AlqpDims(4, 20, 13, 4)
    p = _lib.AlqpParams(2, 4, 20, 3, 10.0, 0)
    rc = lib.alqp_solve_lin_f32(C.byref(d), C.byref(p), *([None] * 7), 0, 0, *([None] * 8), None, None, 0, None)
    assert rc == -1
    rc = lib.alqp_backward_f64(C.byref(d), None, None, 0, *([None] * 6), None, None)
    assert rc == -1
    fake = C.c_void_p(16)
    bad = _lib.AlqpParams(2, 4, 21, 3, 10.0, 0)  # n_ls > 20
    rc = lib.alqp_solve_lin_f32(C.byref(d), C.byref(bad), *([fake] * 7), 0, 0, *([fake] * 8), None, None, 0, None)
    assert rc == -1
    fake = C.c_void_p(64)   # every required argument below is this non-null pointer: each call is refused before a launch
    for sfx in ("f32", "f64"):
        f = lambda name: getattr(lib, name + sfx)
        # alqp_backward: exactly one of factor and workspace
        assert f("alqp_backward_")(C.byref(d), fake, fake, 1 << 40, *([fake] * 6), None, None) == -1
        assert f("alqp_backward_")(C.byref(d), None, None, 0, *([fake] * 6), None, None) == -1
        # the quad Newton step leaves its factor in the workspace: no packed factor_out next to it
        assert f("alqp_newton_step_")(C.byref(d), *([fake] * 10), 0, 0, None, fake, 1 << 40, fake, fake, fake, None,
                                      None) == -1
        # obstacle rows without their centres
        obs = _lib.AlqpObstacles(None, 0.5, 1, 0)
        assert f("alqp_newton_step_")(C.byref(d), *([fake] * 10), 0, 0, C.byref(obs), None, 0, fake, None, None, None,
                                      None) == -1
        assert f("alqp_merit_")(C.byref(d), 1, *([fake] * 9), 0, 0, C.byref(obs), fake, None, None) == -1
        assert f("alqp_dual_update_")(C.byref(d), *([fake] * 5), 0, 0, C.byref(obs), fake, fake, 10.0, None) == -1
        assert f("alqp_merit_pick_")(C.byref(d), 20, *([fake] * 9), 0, 0, C.byref(obs), fake, fake, None, None, None,
                                     None, None) == -1


def test_product_path_fails_loudly_on_cpu_tensors():
    """No CPU fallback: CPU tensors reach the HIP backend and raise."""
    import torch
    from deq_mpc_corl_amd import MPC, AffineDynamics, QuadCost, synthetic_problem
    p = synthetic_problem(4, 5, 2, 1, dtype=torch.float32)
    mpc = MPC(2, 1, 5, u_lower=p.u_lo, u_upper=p.u_hi, n_batch=4, dtype=torch.float32, exit_mode="fixed")
    with pytest.raises(RuntimeError, match="reinitialize"):
        mpc(p.x0, QuadCost(torch.diag_embed(p.Qd), p.q, torch.zeros(4, 5)), None, None)
    mpc.reinitialize(p.x0, None)
    dyn = AffineDynamics(p.F, p.c)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mpc(p.x0, QuadCost(torch.diag_embed(p.Qd), p.q, torch.zeros(4, 5)), dyn, dyn.jac,
            x_init=p.z0[..., :2], u_init=p.z0[..., 2:])
