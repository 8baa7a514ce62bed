"""The launch guard of the register-resident interior-point kernel (alqp_ipm_g4_launch.hpp: resident_addressable),
compiled on the host and called through ctypes. The kernel reads Cd / c, F and f as (instance base) + (unsigned 32-bit
byte offset); the guard must accept exactly the strides whose highest offset stays below 2^32, so that `auto` falls
through to the generic kernel before an offset wraps (tests/test_ip_beyond_4gib.py runs both sides of the limit on the
GPU). Only the predicate is called here: no solve entry point sees a pointer."""
import ctypes as C
import os
import subprocess

import pytest

from tests.test_quad_record_layout_cpu import _dims

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "deq-mpc-corl_amd", "csrc")
SRC = os.path.join(HERE, "emu", "ipm_g4_guard.cpp")
LIB = os.path.join(HERE, "emu", "libipm_g4_guard.so")

DIMS = _dims()   # every (nx, nu) compiled into the library
SIZE = {"f32": 4, "f64": 8}
LIM = 1 << 32

_lib = None


def _guard():
    global _lib
    if _lib is None:
        deps = [SRC] + [os.path.join(CSRC, f) for f in ("alqp_ipm_g4_launch.hpp", "alqp_ipm_args.hpp")]
        if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(s) for s in deps):
            subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-I" + CSRC, SRC, "-o", LIB])
        lib = C.CDLL(LIB)
        fn = lib.g4_resident_addressable
        fn.restype = C.c_int
        fn.argtypes = [C.c_int] * 4 + [C.c_long] * 3
        _lib = fn
    return _lib


def ok(T, nx, nu, dt, sC_t, sF_t, sf_t):
    return bool(_guard()(T, nx, nu, SIZE[dt], sC_t, sF_t, sf_t))


def tm_strides(B, nx, nu):
    """What backend.ipm_solve passes for time-major data: sC_t = B n, sF_t = B nx n, sf_t = B nx."""
    n = nx + nu
    return B * n, B * nx * n, B * nx


def top_byte(T, nx, nu, dt, sC_t, sF_t, sf_t):
    """Highest byte offset the kernel forms from an instance's base: the last element it reads of each array."""
    n = nx + nu
    last = [(T - 1) * sC_t + n - 1, (T - 2) * sF_t + nx * n - 1, (T - 2) * sf_t + nx - 1]
    return max(last) * SIZE[dt]


def b_limit(T, nx, nu, dt):
    """Largest B whose time-major strides keep every offset below 2^32 (bisection on top_byte)."""
    lo, hi = 1, 1 << 40
    assert top_byte(T, nx, nu, dt, *tm_strides(lo, nx, nu)) < LIM <= top_byte(T, nx, nu, dt, *tm_strides(hi, nx, nu))
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if top_byte(T, nx, nu, dt, *tm_strides(mid, nx, nu)) < LIM:
            lo = mid
        else:
            hi = mid
    return lo


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("T", [2, 3, 19, 20])
@pytest.mark.parametrize("nx,nu", DIMS)
def test_guard_switches_at_the_byte_limit(nx, nu, T, dt):
    B = b_limit(T, nx, nu, dt)
    assert ok(T, nx, nu, dt, *tm_strides(B, nx, nu))
    assert not ok(T, nx, nu, dt, *tm_strides(B + 1, nx, nu))
    assert ok(T, nx, nu, dt, *tm_strides(8192, nx, nu))   # bench.py's batch stays on the resident kernel
    # batch-major data (strides of one instance's own slab) never reach the limit
    n = nx + nu
    assert ok(T, nx, nu, dt, n, nx * n, nx)


def test_guard_limit_at_bench_dims():
    """(20,13,4) time-major: the batches at which the kernel's offsets used to wrap silently (the old guard counted
    elements, T max(sC_t, sF_t) < 2^31, and accepted B up to ~486 k)."""
    assert b_limit(20, 13, 4, "f64") == 134959
    assert b_limit(20, 13, 4, "f32") == 269919
    for dt, B in (("f64", 160000), ("f32", 320000)):
        s = tm_strides(B, 13, 4)
        assert 20 * max(s[0], s[1]) < 1 << 31       # what the old guard let through
        assert not ok(20, 13, 4, dt, *s)
    for dt, B in (("f64", 128000), ("f32", 256000)):
        assert ok(20, 13, 4, dt, *tm_strides(B, 13, 4))


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_guard_each_stride_binds(dt):
    """Every stride the kernel multiplies by a stage index is checked on its own, not only sF_t."""
    T, nx, nu = 20, 13, 4
    n = nx + nu
    E = LIM // SIZE[dt]          # elements that start below 2^32 bytes
    small = (n, nx * n, nx)      # batch-major strides
    # Cd / c: (T-1) sC_t + n - 1 < E
    sC = (E - n) // (T - 1)
    assert ok(T, nx, nu, dt, sC, small[1], small[2])
    assert not ok(T, nx, nu, dt, sC + 1, small[1], small[2])
    # F: (T-2) sF_t + nx n - 1 < E
    sF = (E - nx * n) // (T - 2)
    assert ok(T, nx, nu, dt, small[0], sF, small[2])
    assert not ok(T, nx, nu, dt, small[0], sF + 1, small[2])
    # f: (T-2) sf_t + nx - 1 < E (f padded to a wide stride: neither sC_t nor sF_t is anywhere near the limit)
    sf = (E - nx) // (T - 2)
    assert ok(T, nx, nu, dt, small[0], small[1], sf)
    assert not ok(T, nx, nu, dt, small[0], small[1], sf + 1)
    # T = 2 reads F and f of stage 0 only: their stage strides do not matter, the cost's does
    assert ok(2, nx, nu, dt, (E - n) // 1, 1 << 40, 1 << 40)
    assert not ok(2, nx, nu, dt, E - n + 1, small[1], small[2])


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_guard_element_limit_and_bad_input(dt):
    """Strides at the old element limit (T max(sC_t, sF_t) = 2^31) are far beyond the byte limit and stay rejected;
    so do strides whose product would overflow 64 bits, negative strides and degenerate sizes."""
    T, nx, nu = 20, 13, 4
    n = nx + nu
    el = (1 << 31) // T
    assert not ok(T, nx, nu, dt, el, nx * n, nx)
    assert not ok(T, nx, nu, dt, n, el, nx)
    assert not ok(T, nx, nu, dt, n, nx * n, el)
    assert not ok(T, nx, nu, dt, n, (1 << 62) + 1, nx)
    assert not ok(T, nx, nu, dt, -n, nx * n, nx)
    assert not ok(1, nx, nu, dt, n, nx * n, nx)
    assert not ok(T, 0, nu, dt, n, 0, 0)
