"""CPU checks of the four state-bound launch-per-step entry points at the C-ABI boundary (include/mi_alqp.h:
alqp_newton_step_xbox, alqp_merit_xbox, alqp_merit_pick_xbox, alqp_dual_update_xbox, each _f32 / _f64): exported, ABI
version still 17 (symbols were added, no signature changed), and every refusal the header lists comes back with its code
before any launch (null or fake device pointers, no GPU)."""
import ctypes as C

import pytest

BADARG, UNSUPPORTED = -1, -2
FAKE = C.c_void_p(64)   # a non-null pointer nothing dereferences: every call below is refused before a launch
NAMES = ("alqp_newton_step_xbox", "alqp_merit_xbox", "alqp_merit_pick_xbox", "alqp_dual_update_xbox")


def _args(name, dims, xlo=FAKE, xhi=FAKE, sb_x=0, st_x=0, n_ls=20, K=1):
    """The argument list of one entry point with FAKE for every required pointer."""
    from deq_mpc_corl_amd import _lib
    d = C.byref(_lib.AlqpDims(*dims))
    box = (FAKE, FAKE, 0, 0, xlo, xhi, sb_x, st_x)   # u_lo, u_hi, sb_u, st_u, x_lo, x_hi, sb_x, st_x
    if name == "alqp_newton_step_xbox":   # z xnext F x0 lam rho Qd q | bounds | d_out g_out factor info stream
        return (d, *([FAKE] * 8), *box, FAKE, None, None, None, None)
    if name == "alqp_merit_xbox":         # K zc xnext x0 lam rho Qd q | bounds | phi rnorm2 stream
        return (d, K, *([FAKE] * 7), *box, FAKE, None, None)
    if name == "alqp_merit_pick_xbox":    # n_ls d xnext_all x0 lam rho Qd q | bounds | z phi_prev rnorm2 phi_all k acc stream
        return (d, n_ls, *([FAKE] * 7), *box, FAKE, FAKE, None, None, None, None, None)
    return (d, FAKE, FAKE, FAKE, *box, FAKE, FAKE, 10.0, None)   # z xnext x0 | bounds | lam rho rho_scale stream


def _call(lib, name, sfx, dims=(4, 20, 13, 4), **kw):
    return getattr(lib, f"{name}_{sfx}")(*_args(name, dims, **kw))


def test_exported_and_abi_version_still_17():
    from deq_mpc_corl_amd import _lib
    lib = _lib.load()
    for n in NAMES:
        for sfx in ("f32", "f64"):
            assert hasattr(lib, f"{n}_{sfx}") and f"{n}_{sfx}" in _lib.EXPORTED_SYMBOLS
    assert _lib.ABI_VERSION == 17 and lib.alqp_abi_version() == 17


@pytest.mark.parametrize("sfx", ["f32", "f64"])
@pytest.mark.parametrize("name", NAMES)
def test_refusals_come_back_without_a_launch(name, sfx):
    from deq_mpc_corl_amd import _lib
    lib = _lib.load()
    # a null bound, either side
    assert _call(lib, name, sfx, xlo=None) == BADARG
    assert _call(lib, name, sfx, xhi=None) == BADARG
    # a negative stride, either one
    assert _call(lib, name, sfx, sb_x=-1) == BADARG
    assert _call(lib, name, sfx, st_x=-13) == BADARG
    # an empty batch
    assert _call(lib, name, sfx, dims=(0, 20, 13, 4)) == BADARG
    if name == "alqp_merit_pick_xbox":
        for n_ls in (0, 21, -1):
            assert _call(lib, name, sfx, n_ls=n_ls) == BADARG
    if name == "alqp_merit_xbox":
        assert _call(lib, name, sfx, K=0) == BADARG
    if name == "alqp_newton_step_xbox":
        # an (nx, nu) that is not compiled; a horizon whose LDS image does not fit (no quad kernel to fall back on)
        assert _call(lib, name, sfx, dims=(4, 20, 7, 3)) == UNSUPPORTED
        assert _call(lib, name, sfx, dims=(4, 400, 13, 4)) == UNSUPPORTED
        assert lib.alqp_supported_variant(C.byref(_lib.AlqpDims(4, 400, 13, 4)), int(sfx == "f64"), 1) == 0


def test_backend_refuses_a_narrow_lam_and_short_bounds():
    """HipBackend's host-side checks of the four methods (the C entry points see pointers only): lam at least
    M = T nx + T (2 nu + 2 nx) wide, bounds as long as their strides reach. Nothing is launched."""
    import torch
    from deq_mpc_corl_amd.backend import HipBackend
    B, T, nx, nu = 3, 4, 2, 1
    M = T * nx + T * (2 * nu + 2 * nx)
    lo, hi = torch.zeros(nx), torch.ones(nx)
    assert HipBackend._row_checks((B, T, nx, nu), torch.zeros(B, M), None, (lo, hi, 0, 0), None)[:4] == (lo, hi, 0, 0)
    with pytest.raises(ValueError, match="state-bound rows need"):
        HipBackend._row_checks((B, T, nx, nu), torch.zeros(B, T * nx + 2 * T * nu), None, (lo, hi, 0, 0), None)
    with pytest.raises(ValueError, match="too few for strides"):
        HipBackend._row_checks((B, T, nx, nu), torch.zeros(B, M), None, (lo, hi, T * nx, nx), None)
    with pytest.raises(ValueError, match="x_upper is required"):
        HipBackend._row_checks((B, T, nx, nu), torch.zeros(B, M), None, (lo, None, 0, 0), None)
