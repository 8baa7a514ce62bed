"""CPU checks of alqp_solve_lin_gen_{f32,f64} at the C-ABI boundary (include/mi_alqp.h): exported, ABI version 17, and
every refusal the header lists comes back with its code before any launch (null or fake device pointers, no GPU)."""
import ctypes as C

import pytest

BADARG, UNSUPPORTED = -1, -2
FAKE = C.c_void_p(64)   # a non-null pointer nothing dereferences: every call below is refused before a launch


def _call(lib, sfx, dims=(4, 20, 13, 4), variant=0, Qd=FAKE, C_=None, xlo=None, xhi=None, G=None, h=None, m=0,
          strides=(0, 0, 0, 0, 0, 0), n_ls=20):
    from deq_mpc_corl_amd import _lib
    d = _lib.AlqpDims(*dims)
    p = _lib.AlqpParams(2, 4, n_ls, 3, 10.0, variant)
    sb_x, st_x, sb_g, st_g, sb_h, st_h = strides
    return getattr(lib, "alqp_solve_lin_gen_" + sfx)(
        C.byref(d), C.byref(p), Qd, *([FAKE] * 6), 0, 0, *([FAKE] * 4), None, None, None, None, None, None, 0, None,
        C_, xlo, xhi, sb_x, st_x, G, h, m, sb_g, st_g, sb_h, st_h)


def test_exported_and_abi_version_17():
    from deq_mpc_corl_amd import _lib
    lib = _lib.load()
    for s in ("alqp_solve_lin_gen_f32", "alqp_solve_lin_gen_f64"):
        assert hasattr(lib, s) and s in _lib.EXPORTED_SYMBOLS
    assert _lib.ABI_VERSION == 17 and lib.alqp_abi_version() == _lib.ABI_VERSION


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_refusals_come_back_without_a_launch(sfx):
    from deq_mpc_corl_amd import _lib
    lib = _lib.load()
    box = dict(xlo=FAKE, xhi=FAKE)
    rows = dict(G=FAKE, h=FAKE, m=4)
    # fewer than two features: none, and each alone (the single-feature entry points stay the way to run those)
    assert _call(lib, sfx) == BADARG
    assert _call(lib, sfx, C_=FAKE) == BADARG
    assert _call(lib, sfx, **box) == BADARG
    assert _call(lib, sfx, **rows) == BADARG
    # one half of a pair
    assert _call(lib, sfx, C_=FAKE, xlo=FAKE) == BADARG
    assert _call(lib, sfx, C_=FAKE, xhi=FAKE) == BADARG
    assert _call(lib, sfx, C_=FAKE, G=FAKE, m=4) == BADARG
    assert _call(lib, sfx, C_=FAKE, h=FAKE, m=4) == BADARG
    assert _call(lib, sfx, **box, G=FAKE, m=4) == BADARG
    # m outside 1..64 while G is given
    for m in (0, -1, 65):
        assert _call(lib, sfx, C_=FAKE, G=FAKE, h=FAKE, m=m) == BADARG
        assert _call(lib, sfx, **box, G=FAKE, h=FAKE, m=m) == BADARG
    # variant not 0 / 1
    for v in (2, 3, -1):
        assert _call(lib, sfx, C_=FAKE, **box, **rows, variant=v) == BADARG
    # negative strides, a missing Qd where no C stands in for it, the siblings' parameter checks, an empty batch
    assert _call(lib, sfx, C_=FAKE, **box, strides=(-1, 0, 0, 0, 0, 0)) == BADARG
    assert _call(lib, sfx, C_=FAKE, **rows, strides=(0, 0, 0, -1, 0, 0)) == BADARG
    assert _call(lib, sfx, Qd=None, **box, **rows) == BADARG
    assert _call(lib, sfx, C_=FAKE, **box, n_ls=21) == BADARG
    assert _call(lib, sfx, dims=(0, 20, 13, 4), C_=FAKE, **box) == BADARG
    # an (nx, nu) that is not compiled; a horizon whose image does not fit (with rows: the hand-over region counts)
    for kw in (dict(C_=FAKE, **box), dict(C_=FAKE, **rows), dict(**box, **rows), dict(C_=FAKE, **box, **rows)):
        assert _call(lib, sfx, dims=(4, 20, 7, 3), **kw) == UNSUPPORTED
        assert _call(lib, sfx, dims=(4, 400, 13, 4), **kw) == UNSUPPORTED


def test_the_hand_over_region_counts_towards_the_image():
    """The longest (13,4) horizon whose team image fits: still taken by the box + dense pair's check, refused with 64 rows
    when their 2 pad4(m) words per team pass the budget. Found from alqp_lds_bytes; nothing is launched (the refused
    side), and the accepted side is not called."""
    from deq_mpc_corl_amd import _lib
    lib = _lib.load()
    T = 2
    while lib.alqp_lds_bytes(C.byref(_lib.AlqpDims(4, T + 1, 13, 4)), 1) <= 160 * 1024:
        T += 1
    img = lib.alqp_lds_bytes(C.byref(_lib.AlqpDims(4, T, 13, 4)), 1)
    assert img <= 160 * 1024 < img + 2 * 64 * 8   # (T = 91: 224 bytes to spare, 64 rows need 1024)
    assert _call(lib, "f64", dims=(4, T, 13, 4), xlo=FAKE, xhi=FAKE, G=FAKE, h=FAKE, m=64) == UNSUPPORTED
    assert _call(lib, "f64", dims=(4, T, 13, 4), C_=FAKE, G=FAKE, h=FAKE, m=64) == UNSUPPORTED
