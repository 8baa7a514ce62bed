"""CPU checks of the nonlinear fused solve with state bounds and / or general rows at the C-ABI boundary (include/mi_alqp.h:
alqp_solve_nonlin_rows_f32 / _f64, alqp_workspace_bytes_nonlin_rows): exported, ABI version still 17 (symbols were added, no
signature changed), every refusal the header lists comes back with its code before any launch (null or fake device
pointers, no GPU), and the backend's host checks."""
import ctypes as C

import pytest

BADARG, UNSUPPORTED = -1, -2
FAKE = C.c_void_p(64)   # a non-null pointer nothing dereferences: every call below is refused before a launch
EXIT_IN_KERNEL, WS_PRIMED = 16, 8


def _call(lib, sfx, dims=(4, 10, 4, 1), dyn_id=2, n_ls=20, flags=3, xlo=FAKE, xhi=FAKE, sx=(0, 0), G=FAKE, h=FAKE, m=3,
          sg=(0, 0, 0, 0), ws=FAKE, ws_bytes=None, factor=None, al_iter=2, max_newton=4):
    from deq_mpc_corl_amd import _lib
    d = _lib.AlqpDims(*dims)
    if ws_bytes is None:
        ws_bytes = lib.alqp_workspace_bytes_nonlin_rows(C.byref(d), int(sfx == "f64"))
    p = _lib.AlqpParams(al_iter, max_newton, n_ls, flags, 10.0, 0, None)
    return getattr(lib, "alqp_solve_nonlin_rows_" + sfx)(
        C.byref(d), C.byref(p), dyn_id, 0.05, FAKE, FAKE, FAKE, FAKE, FAKE, 0, 0, xlo, xhi, *sx, G, h, m, *sg,
        FAKE, FAKE, FAKE, FAKE, None, None, None, factor, None, ws, ws_bytes, None)


def test_exported_and_abi_version_still_17():
    from deq_mpc_corl_amd import _lib
    lib = _lib.load()
    for n in ("alqp_solve_nonlin_rows_f32", "alqp_solve_nonlin_rows_f64", "alqp_workspace_bytes_nonlin_rows"):
        assert hasattr(lib, n) and n in _lib.EXPORTED_SYMBOLS
    assert _lib.ABI_VERSION == 17 and lib.alqp_abi_version() == 17


def test_workspace_bytes():
    from deq_mpc_corl_amd import _lib
    lib = _lib.load()
    q = lambda dims, f64: lib.alqp_workspace_bytes_nonlin_rows(C.byref(_lib.AlqpDims(*dims)), f64)
    # per instance F[T-1][nx][n], then xnext[T-1][nx]
    assert q((7, 14, 2, 1), 0) == 7 * 13 * 2 * 4 * 4 and q((7, 14, 4, 1), 1) == 7 * 13 * 4 * 6 * 8
    # no model of that size on this route ((6,1): cartpole2l has no instance here), no batch, no dynamics stage
    for dims in ((7, 14, 13, 4), (7, 14, 6, 1), (7, 14, 4, 2), (0, 14, 2, 1), (7, 1, 2, 1)):
        assert q(dims, 0) == 0 and q(dims, 1) == 0


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_refusals_come_back_without_a_launch(sfx):
    from deq_mpc_corl_amd import _lib
    lib = _lib.load()
    none = dict(xlo=None, xhi=None)
    norows = dict(G=None, h=None, m=0)
    # neither row family; one half of a pair null
    assert _call(lib, sfx, **none, **norows) == BADARG
    for kw in (dict(xlo=None), dict(xhi=None), dict(G=None), dict(h=None), dict(G=None, m=0), dict(h=None, m=0)):
        assert _call(lib, sfx, **kw) == BADARG
    # m outside 1..64 with rows, m != 0 without
    for m in (0, 65, -1):
        assert _call(lib, sfx, m=m) == BADARG and _call(lib, sfx, m=m, **none) == BADARG
    assert _call(lib, sfx, G=None, h=None, m=3) == BADARG
    # a negative stride, any of the six
    for i in range(4):
        sg = [0, 0, 0, 0]
        sg[i] = -1
        assert _call(lib, sfx, sg=tuple(sg)) == BADARG and _call(lib, sfx, sg=tuple(sg), **none) == BADARG
    assert _call(lib, sfx, sx=(-1, 0)) == BADARG and _call(lib, sfx, sx=(0, -4), **norows) == BADARG
    for xb in (dict(), none, norows):
        # an empty batch; n_ls != 20; workspace null or too small; the cooperative exit; a factor asked for without its array
        assert _call(lib, sfx, dims=(0, 10, 4, 1), ws_bytes=1 << 20, **xb) == BADARG
        for n_ls in (19, 21, 1, 0):
            assert _call(lib, sfx, n_ls=n_ls, **xb) == BADARG
        assert _call(lib, sfx, ws=None, **xb) == BADARG
        need = lib.alqp_workspace_bytes_nonlin_rows(C.byref(_lib.AlqpDims(4, 10, 4, 1)), int(sfx == "f64"))
        assert need > 0 and _call(lib, sfx, ws_bytes=need - 1, **xb) == BADARG
        assert _call(lib, sfx, flags=3 | EXIT_IN_KERNEL, **xb) == BADARG
        assert _call(lib, sfx, flags=3 | 4, factor=None, **xb) == BADARG
        # unknown dyn_id, a model without an instance on this route, (nx, nu) not the model's, no such size at all
        for dyn_id in (0, 5, 3):
            assert _call(lib, sfx, dyn_id=dyn_id, **xb) == UNSUPPORTED
        assert _call(lib, sfx, dyn_id=1, **xb) == UNSUPPORTED                        # pendulum1l is (2,1)
        assert _call(lib, sfx, dyn_id=2, dims=(4, 10, 2, 1), **xb) == UNSUPPORTED    # cartpole1l is (4,1)
        assert _call(lib, sfx, dyn_id=3, dims=(4, 10, 6, 1), ws_bytes=1 << 20, **xb) == UNSUPPORTED
        assert _call(lib, sfx, dims=(4, 10, 13, 4), ws_bytes=1 << 20, **xb) == UNSUPPORTED
        # a horizon whose LDS image does not fit
        assert _call(lib, sfx, dims=(4, 6000, 4, 1), **xb) == UNSUPPORTED


def test_lds_limit_counts_the_hand_over_region():
    from deq_mpc_corl_amd import _lib
    lib = _lib.load()
    for sfx, is64 in (("f32", 0), ("f64", 1)):
        lds = lambda T: lib.alqp_lds_bytes(C.byref(_lib.AlqpDims(4, T, 4, 1)), is64)
        T = max(t for t in range(2, 6000) if 0 < lds(t) <= 160 * 1024)
        qpw = lib.alqp_qps_per_wave(C.byref(_lib.AlqpDims(4, T, 4, 1)), is64)
        word = 8 if is64 else 4
        refused = [m for m in (1, 4, 16, 64) if lds(T) + qpw * 2 * ((m + 3) & ~3) * word > 160 * 1024]
        assert refused, (T, lds(T), qpw)
        for m in refused:
            assert _call(lib, sfx, dims=(4, T, 4, 1), m=m) == UNSUPPORTED


def test_backend_host_checks():
    """HipBackend.solve_nonlin_rows refuses on the host, before any pointer is taken: no rows at all, a narrow lam, bounds or
    rows shorter than their strides reach, a size without a model."""
    import torch
    from deq_mpc_corl_amd.backend import HipBackend
    be = HipBackend()
    B, T, nx, nu, m = 3, 4, 2, 1, 2
    n = nx + nu
    dims = (B, T, nx, nu)
    z = torch.zeros(B, T, n)
    lo, hi = torch.zeros(nx), torch.ones(nx)
    G, h = torch.zeros(m, n), torch.zeros(m)
    poly, xb = (G, h, m, 0, 0, 0, 0), (lo, hi, 0, 0)
    M1 = T * nx + T * (2 * nu + 2 * nx + m)
    call = lambda dims, xbnd, poly, lam: be.solve_nonlin_rows(dims, 1, 0.05, None, None, None, None, None, 0, 0, xbnd, poly,
                                                              z, lam, None, None)
    with pytest.raises(ValueError, match="needs state bounds or general rows"):
        call(dims, None, None, torch.zeros(B, M1))
    with pytest.raises(ValueError, match=f"these rows need \\[B, {M1}\\]"):
        call(dims, xb, poly, torch.zeros(B, M1 - 1))
    with pytest.raises(ValueError, match="ineqG has .* too few for strides"):
        call(dims, xb, (G, h, m, 0, m * n, 0, 0), torch.zeros(B, M1))
    with pytest.raises(ValueError, match="x_lower has .* too few for strides"):
        call(dims, (lo, hi, T * nx, nx), poly, torch.zeros(B, M1))
    with pytest.raises(RuntimeError, match="not available for these sizes"):
        call((B, T, 6, 1), None, (torch.zeros(m, 7), h, m, 0, 0, 0, 0), torch.zeros(B, T * 6 + T * (2 + m)))
    assert be.nonlin_rows_workspace_bytes(dims, torch.float64) == B * (T - 1) * nx * (n + 1) * 8
    # the F view of a workspace: instance b's first (T-1) nx n words
    ws = torch.arange(B * (T - 1) * nx * (n + 1), dtype=torch.float64)
    Fv = be.nonlin_rows_F_view(ws, dims)
    per = (T - 1) * nx * (n + 1)
    assert Fv.shape == (B, T - 1, nx, n) and Fv.data_ptr() == ws.data_ptr()
    assert torch.equal(Fv[1].reshape(-1), ws[per:per + (T - 1) * nx * n])
