"""CPU checks of the four launch-per-step entry points with general rows at the C-ABI boundary (include/mi_alqp.h:
alqp_newton_step_rows, alqp_merit_rows, alqp_merit_pick_rows, alqp_dual_update_rows, each _f32 / _f64): exported, ABI
version still 17 (symbols were added, no signature changed), and every refusal the header lists comes back with its code
before any launch (null or fake device pointers, no GPU)."""
import ctypes as C

import pytest

BADARG, UNSUPPORTED = -1, -2
FAKE = C.c_void_p(64)   # a non-null pointer nothing dereferences: every call below is refused before a launch
NAMES = ("alqp_newton_step_rows", "alqp_merit_rows", "alqp_merit_pick_rows", "alqp_dual_update_rows")


def _args(name, dims, xlo=FAKE, xhi=FAKE, sb_x=0, st_x=0, G=FAKE, h=FAKE, m=3, sg=(0, 0, 0, 0), n_ls=20, K=1):
    """The argument list of one entry point with FAKE for every required pointer."""
    from deq_mpc_corl_amd import _lib
    d = C.byref(_lib.AlqpDims(*dims))
    # u_lo, u_hi, sb_u, st_u, x_lo, x_hi, sb_x, st_x, G, h, m, sb_g, st_g, sb_h, st_h
    rows = (FAKE, FAKE, 0, 0, xlo, xhi, sb_x, st_x, G, h, m, *sg)
    if name == "alqp_newton_step_rows":   # z xnext F x0 lam rho Qd q | rows | d_out g_out factor info stream
        return (d, *([FAKE] * 8), *rows, FAKE, None, None, None, None)
    if name == "alqp_merit_rows":         # K zc xnext x0 lam rho Qd q | rows | phi rnorm2 stream
        return (d, K, *([FAKE] * 7), *rows, FAKE, None, None)
    if name == "alqp_merit_pick_rows":    # n_ls d xnext_all x0 lam rho Qd q | rows | z phi_prev rnorm2 phi_all k acc stream
        return (d, n_ls, *([FAKE] * 7), *rows, FAKE, FAKE, None, None, None, None, None)
    return (d, FAKE, FAKE, FAKE, *rows, FAKE, FAKE, 10.0, None)   # z xnext x0 | rows | lam rho rho_scale stream


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
    # null rows or right-hand sides
    assert _call(lib, name, sfx, G=None) == BADARG
    assert _call(lib, name, sfx, h=None) == BADARG
    # m outside 1..64
    for m in (0, 65, -1):
        assert _call(lib, name, sfx, m=m) == BADARG
    # one state bound null alone (both null means "no state bounds": refused for nothing but what follows)
    assert _call(lib, name, sfx, xlo=None) == BADARG
    assert _call(lib, name, sfx, xhi=None) == BADARG
    # a negative stride, any of the six - with and without state bounds
    for xb in (dict(), dict(xlo=None, xhi=None)):
        for i in range(4):
            sg = [0, 0, 0, 0]
            sg[i] = -1
            assert _call(lib, name, sfx, sg=tuple(sg), **xb) == BADARG
        assert _call(lib, name, sfx, sb_x=-1, **xb) == BADARG
        assert _call(lib, name, sfx, st_x=-13, **xb) == BADARG
        # an empty batch
        assert _call(lib, name, sfx, dims=(0, 20, 13, 4), **xb) == BADARG
        if name == "alqp_merit_pick_rows":
            for n_ls in (0, 21, -1):
                assert _call(lib, name, sfx, n_ls=n_ls, **xb) == BADARG
        if name == "alqp_merit_rows":
            assert _call(lib, name, sfx, K=0, **xb) == BADARG
        if name == "alqp_newton_step_rows":
            # an (nx, nu) that is not compiled; a horizon whose LDS image does not fit (no quad kernel to fall back on)
            assert _call(lib, name, sfx, dims=(4, 20, 7, 3), **xb) == UNSUPPORTED
            assert _call(lib, name, sfx, dims=(4, 400, 13, 4), **xb) == UNSUPPORTED


def test_lds_limit_counts_the_hand_over_region():
    """The image is the team image plus 2 pad4(m) words per team: at the longest horizon whose team image still fits, m = 64
    no longer does, while alqp_newton_step_xbox (no hand-over region) is not refused for its size there."""
    from deq_mpc_corl_amd import _lib
    lib = _lib.load()
    for sfx, is64 in (("f32", 0), ("f64", 1)):
        fits = lambda T: 0 < lib.alqp_lds_bytes(C.byref(_lib.AlqpDims(4, T, 13, 4)), is64) <= 160 * 1024
        T = max(t for t in range(2, 400) if fits(t))
        img = lib.alqp_lds_bytes(C.byref(_lib.AlqpDims(4, T, 13, 4)), is64)
        qpw = lib.alqp_qps_per_wave(C.byref(_lib.AlqpDims(4, T, 13, 4)), is64)
        word = 8 if is64 else 4
        refused = [m for m in (1, 4, 16, 64) if img + qpw * 2 * ((m + 3) & ~3) * word > 160 * 1024]
        assert refused, (T, img, qpw)   # the longest horizon leaves less room than the widest hand-over region needs
        for m in refused:
            assert _call(lib, "alqp_newton_step_rows", sfx, dims=(4, T, 13, 4), m=m) == UNSUPPORTED


def test_backend_refuses_a_narrow_lam_and_short_rows():
    """HipBackend's host-side checks of the four methods (the C entry points see pointers only): lam at least
    M = T nx + T (2 nu + [2 nx] + m) wide, bounds and rows as long as their strides reach. Nothing is launched."""
    import torch
    from deq_mpc_corl_amd.backend import HipBackend
    B, T, nx, nu, m = 3, 4, 2, 1, 2
    n = nx + nu
    lo, hi = torch.zeros(nx), torch.ones(nx)
    G, h = torch.zeros(m, n), torch.zeros(m)
    poly = (G, h, m, 0, 0, 0, 0)
    dims = (B, T, nx, nu)
    M0, M1 = T * nx + T * (2 * nu + m), T * nx + T * (2 * nu + 2 * nx + m)
    assert HipBackend._row_checks(dims, torch.zeros(B, M0), None, None, poly) == (None, None, 0, 0, *poly)
    assert HipBackend._row_checks(dims, torch.zeros(B, M1), None, (lo, hi, 0, 0), poly) == (lo, hi, 0, 0, *poly)
    with pytest.raises(ValueError, match=f"these rows need \\[B, {M1}\\]"):
        HipBackend._row_checks(dims, torch.zeros(B, M0), None, (lo, hi, 0, 0), poly)
    with pytest.raises(ValueError, match=f"these rows need \\[B, {M0}\\]"):
        HipBackend._row_checks(dims, torch.zeros(B, T * nx + 2 * T * nu), None, None, poly)
    with pytest.raises(ValueError, match="ineqG has .* too few for strides"):
        HipBackend._row_checks(dims, torch.zeros(B, M0), None, None, (G, h, m, 0, m * n, 0, 0))
    with pytest.raises(ValueError, match="ineqh has .* too few for strides"):
        HipBackend._row_checks(dims, torch.zeros(B, M0), None, None, (G, h, m, 0, 0, T * m, m))
    with pytest.raises(ValueError, match="x_lower has .* too few for strides"):
        HipBackend._row_checks(dims, torch.zeros(B, M1), None, (lo, hi, T * nx, nx), poly)
    with pytest.raises(ValueError, match="x_upper is required"):
        HipBackend._row_checks(dims, torch.zeros(B, M1), None, (lo, None, 0, 0), poly)
