"""CPU checks of the three launch-per-step entry points with a dense stage cost at the C-ABI boundary (include/mi_alqp.h:
alqp_newton_step_dense, alqp_merit_dense, alqp_merit_pick_dense, each _f32 / _f64): exported, ABI version still 17
(symbols were added, no signature changed), and every refusal the header lists comes back with its code before any launch
(null or fake device pointers, no GPU)."""
import ctypes as C

import pytest

BADARG, UNSUPPORTED = -1, -2
FAKE = C.c_void_p(64)   # a non-null pointer nothing dereferences: every call below is refused before a launch
NAMES = ("alqp_newton_step_dense", "alqp_merit_dense", "alqp_merit_pick_dense")
NO_XB = dict(xlo=None, xhi=None)
NO_PL = dict(G=None, h=None, m=0)


def _args(name, dims, Cm=FAKE, xlo=FAKE, xhi=FAKE, sb_x=0, st_x=0, G=FAKE, h=FAKE, m=3, sg=(0, 0, 0, 0), n_ls=20, K=1):
    """The argument list of one entry point with FAKE for every required pointer."""
    from deq_mpc_corl_amd import _lib
    d = C.byref(_lib.AlqpDims(*dims))
    # C, q, u_lo, u_hi, sb_u, st_u, x_lo, x_hi, sb_x, st_x, G, h, m, sb_g, st_g, sb_h, st_h
    rows = (Cm, FAKE, FAKE, FAKE, 0, 0, xlo, xhi, sb_x, st_x, G, h, m, *sg)
    if name == "alqp_newton_step_dense":   # z xnext F x0 lam rho | C q rows | d_out g_out factor info stream
        return (d, *([FAKE] * 6), *rows, FAKE, None, None, None, None)
    if name == "alqp_merit_dense":         # K zc xnext x0 lam rho | C q rows | phi rnorm2 stream
        return (d, K, *([FAKE] * 5), *rows, FAKE, None, None)
    # n_ls d xnext_all x0 lam rho | C q rows | z phi_prev rnorm2 phi_all k acc stream
    return (d, n_ls, *([FAKE] * 5), *rows, FAKE, FAKE, None, None, None, None, None)


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
    # every combination of rows: state bounds or none (both null), general rows or none (both null with m == 0)
    combos = [dict(), NO_XB, NO_PL, {**NO_XB, **NO_PL}]
    for base in combos:
        rows = base.get("G", FAKE) is not None
        assert _call(lib, name, sfx, Cm=None, **base) == BADARG   # a null C
        # an empty batch
        assert _call(lib, name, sfx, dims=(0, 20, 13, 4), **base) == BADARG
        # a negative stride, any of the six
        for i in range(4):
            sg = [0, 0, 0, 0]
            sg[i] = -1
            assert _call(lib, name, sfx, sg=tuple(sg), **base) == BADARG
        assert _call(lib, name, sfx, sb_x=-1, **base) == BADARG
        assert _call(lib, name, sfx, st_x=-13, **base) == BADARG
        if rows:
            # G without h, h without G; m outside 1..64 with G
            assert _call(lib, name, sfx, **{**base, "G": None}) == BADARG
            assert _call(lib, name, sfx, **{**base, "h": None}) == BADARG
            for m in (0, 65, -1):
                assert _call(lib, name, sfx, **{**base, "m": m}) == BADARG
        else:
            # a nonzero m without G
            for m in (1, 3, -1):
                assert _call(lib, name, sfx, **{**base, "m": m}) == BADARG
        if base.get("xlo", FAKE) is not None:
            # one state bound null alone (both null means "no state bounds")
            assert _call(lib, name, sfx, **{**base, "xlo": None}) == BADARG
            assert _call(lib, name, sfx, **{**base, "xhi": None}) == BADARG
        if name == "alqp_merit_pick_dense":
            for n_ls in (0, 21, -1):
                assert _call(lib, name, sfx, n_ls=n_ls, **base) == BADARG
        if name == "alqp_merit_dense":
            assert _call(lib, name, sfx, K=0, **base) == BADARG
        if name == "alqp_newton_step_dense":
            # an (nx, nu) that is not compiled; a horizon whose LDS image does not fit (no quad kernel to fall back on)
            assert _call(lib, name, sfx, dims=(4, 20, 7, 3), **base) == UNSUPPORTED
            assert _call(lib, name, sfx, dims=(4, 400, 13, 4), **base) == UNSUPPORTED


def test_lds_limit_counts_the_hand_over_region():
    """With general rows the image is the team image plus 2 pad4(m) words per team: at the longest horizon whose team image
    still fits, m = 64 no longer does, with state bounds or without. One horizon further the team image itself does not
    fit, with general rows or without."""
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
        for xb in (dict(), NO_XB):
            for m in refused:
                assert _call(lib, "alqp_newton_step_dense", sfx, dims=(4, T, 13, 4), m=m, **xb) == UNSUPPORTED
            # one horizon further the team image itself no longer fits, general rows or none
            assert _call(lib, "alqp_newton_step_dense", sfx, dims=(4, T + 1, 13, 4), **xb, **NO_PL) == UNSUPPORTED
            assert _call(lib, "alqp_newton_step_dense", sfx, dims=(4, T + 1, 13, 4), m=1, **xb) == UNSUPPORTED


def test_backend_checks_c_lam_and_rows():
    """HipBackend's host-side checks of the three methods (the C entry points see pointers only): C [B,T,n,n] as
    solve_lin_dense asks, lam at least M = T nx + T (2 nu + [2 nx] + [m]) wide, bounds and rows as long as their strides
    reach. Nothing is launched: the checks raise before a pointer is taken."""
    import torch
    from deq_mpc_corl_amd.backend import HipBackend
    B, T, nx, nu, m = 3, 4, 2, 1, 2
    n = nx + nu
    be = HipBackend.__new__(HipBackend)   # (no library handle: none of the checks needs one)
    lo, hi = torch.zeros(nx), torch.ones(nx)
    poly = (torch.zeros(m, n), torch.zeros(m), m, 0, 0, 0, 0)
    xb = (lo, hi, 0, 0)
    dims = (B, T, nx, nu)
    Cs = torch.zeros(B, T, n, n)
    width = lambda x, p: T * nx + T * (2 * nu + (2 * nx if x else 0) + (m if p else 0))
    dt = torch.float32
    assert be._fam_cargs("dense", dims, torch.zeros(B, width(0, 0)), Cs, None, None, dt) == (None, None, 0, 0, None, None, 0, 0, 0, 0, 0)
    with pytest.raises(ValueError, match=r"C has shape .* expected \(3, 4, 3, 3\)"):
        be._fam_cargs("dense", dims, torch.zeros(B, width(0, 0)), torch.zeros(B, T, n), None, None, dt)
    with pytest.raises(ValueError, match=f"expected \\[B, {width(0, 0)}\\]"):
        be._fam_cargs("dense", dims, torch.zeros(B, width(0, 0) - 1), Cs, None, None, dt)
    with pytest.raises(ValueError, match=f"the state-bound rows need \\[B, {width(1, 0)}\\]"):
        be._fam_cargs("dense", dims, torch.zeros(B, width(0, 0)), Cs, xb, None, dt)
    with pytest.raises(ValueError, match=f"these rows need \\[B, {width(0, 1)}\\]"):
        be._fam_cargs("dense", dims, torch.zeros(B, width(0, 0)), Cs, None, poly, dt)
    with pytest.raises(ValueError, match=f"these rows need \\[B, {width(1, 1)}\\]"):
        be._fam_cargs("dense", dims, torch.zeros(B, width(0, 1)), Cs, xb, poly, dt)
    with pytest.raises(ValueError, match="x_lower has .* too few for strides"):
        be._fam_cargs("dense", dims, torch.zeros(B, width(1, 0)), Cs, (lo, hi, T * nx, nx), None, dt)
    with pytest.raises(ValueError, match="ineqG has .* too few for strides"):
        be._fam_cargs("dense", dims, torch.zeros(B, width(0, 1)), Cs, None, (poly[0], poly[1], m, 0, m * n, 0, 0), dt)
    # past the checks the first thing asked is a device pointer: CPU tensors are refused there, nothing is launched
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        be._fam_cargs("dense", dims, torch.zeros(B, width(1, 1)), Cs, xb, poly, dt)
