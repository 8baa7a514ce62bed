"""The quad workspace record layout (alqp_quad.hpp: QCfg), checked on the host for every compiled (nx, nu) and both
dtypes. tests/emu/quad_layout_probe.cpp dumps the workspace word of every element a quad kernel addresses - L chunks
per (slot, chunk, lane), vector field slots per (field, lane, slot), the bound-row chunks - through the layout's own
accessors; this file asserts properties of that mapping without restating its offsets:
  * no two elements of any (instance, stage) share a word, and all words lie below ws_words(B, T);
  * ws_words * sizeof(real) is what alqp_workspace_bytes reports (the library loads without a GPU);
  * every 4-word per-lane access starts at w % 16 <= 12 and stays inside one 64-byte block;
  * a lane's head and tail words of a vector field sit at the same lane offset (16 q bytes in fp32) from a group start,
    and the whole-field read (fw / lp) finds every element where the per-lane access (ld_slots / st_slots) put it;
  * fp32: instances 2i and 2i + 1 alternate in the 64-byte halves of each 128-byte line, and RECW is whole lines.
Odd and even B (the last pair half used), T = 2 and 7."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "deq-mpc-corl_amd", "csrc")
SRC = os.path.join(HERE, "emu", "quad_layout_probe.cpp")
LIB = os.path.join(HERE, "emu", "libquad_layout_probe.so")


def _dims():
    src = open(os.path.join(CSRC, "alqp_dims.hpp")).read()
    return [(int(a), int(b)) for a, b in re.findall(r"X\((\d+),\s*(\d+)\)", src)]


DIMS = _dims()
BS = [1, 2, 3, 17, 33]
TS = [2, 7]
_probe = None


def _lib():
    global _probe
    if _probe is None:
        deps = [SRC] + [os.path.join(CSRC, f) for f in ("alqp_quad.hpp", "alqp_dims.hpp", "alqp_team.hpp", "alqp_dyn.hpp")]
        if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(s) for s in deps):
            subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-std=c++17", "-O1", "-shared", "-fPIC", "-w",
                                   "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), SRC, "-o", LIB])
        lib = C.CDLL(LIB)
        lib.quad_layout_probe.restype = C.c_int
        lib.quad_layout_probe.argtypes = [C.c_int] * 5 + [C.c_void_p] * 4
        _probe = lib.quad_layout_probe
    return _probe


def probe(dt, nx, nu, B, T):
    """-> meta dict, elements [E, 8] (kind, a, b, lane, i, rel, alt, chunk), words [B, T, E], ws_words"""
    f64 = int(dt == "f64")
    meta = np.zeros(9, np.int64)
    assert _lib()(f64, nx, nu, 0, 0, meta.ctypes.data, None, None, None) == 0
    m = dict(zip(("RECW", "RSTR", "IL", "SH", "SW", "SY", "NLAST", "E", "size"), meta.tolist()))
    E = m["E"]
    el = np.zeros((E, 8), np.int32)
    words = np.zeros((B, T, E), np.int64)
    ws = np.zeros(1, np.int64)
    assert _lib()(f64, nx, nu, B, T, None, el.ctypes.data, words.ctypes.data, ws.ctypes.data) == 0
    return m, el, words, int(ws[0])


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("nx,nu", DIMS)
def test_quad_record_layout_invariants(nx, nu, dt):
    from deq_mpc_corl_amd import _lib as alqp
    lib = alqp.load()
    for B in BS:
        for T in TS:
            m, el, words, ws_words = probe(dt, nx, nu, B, T)
            tag = (dt, nx, nu, B, T)
            flat = words.reshape(-1)
            # injective over all (instance, stage, element), inside the allocation
            assert len(np.unique(flat)) == flat.size, tag
            assert flat.min() >= 0 and flat.max() < ws_words, (tag, int(flat.max()), ws_words)
            # the size the library reports for the allocation
            d = alqp.AlqpDims(B, T, nx, nu)
            assert lib.alqp_workspace_bytes(C.byref(d), int(dt == "f64")) == ws_words * m["size"], tag
            # 4-word per-lane accesses: start at w % 16 <= 12, inside one 64-byte block
            ch = words[:, :, el[:, 7] == 1].reshape(-1)
            assert (ch % 16 <= 12).all(), tag
            assert ((ch * m["size"]) // 64 == ((ch + 3) * m["size"] + m["size"] - 1) // 64).all(), tag
            # the chunk's four words are the element list's next three L words / head slots: consecutive words
            idx = np.nonzero(el[:, 7] == 1)[0]
            for k in range(1, 4):
                assert (words[:, :, idx + k] == words[:, :, idx] + k).all(), (tag, k)
            vec = el[:, 0] >= 1
            # a lane's head and tail words of a vector field: the same lane offset from a 16-word group start
            assert ((words[:, :, vec] % 16) // 4 == el[vec, 3]).all(), tag
            # whole-field read (fw / lp) == per-lane access (ld_slots / st_slots) for every element
            assert (el[vec, 6] == el[vec, 5]).all(), (tag, el[vec][el[vec, 6] != el[vec, 5]][:4])
            if dt == "f32":
                assert m["IL"] == 2 and m["RECW"] % 32 == 0, (tag, m)
                # instance b's words sit in the (b % 2) half of every 128-byte line
                half = (words // 16) % 2
                assert (half == (np.arange(B) % 2)[:, None, None]).all(), tag
            else:
                assert m["IL"] == 1, (tag, m)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_quad_record_layout_covers_the_slots_of_every_field(dt):
    """The probe enumerates what the kernels address: L has SH slots of s + 1 chunks, each with one chunk per lane that
    owns a row of the slot (4, or NLAST in the last); every field has 4 lanes x its slot count. Pins the edge cases the
        layout has: (2,1) has no head chunks of an n-vector (SY < 4); the last L slot holds 1, 2, 3 or 4 lanes (NLAST, each
    with its own chunk stride) across the compiled sizes."""
    seen = {}
    for nx, nu in DIMS:
        m, el, _, _ = probe(dt, nx, nu, 1, 2)
        n = nx + nu
        assert m["SH"] == (n + 3) // 4 and m["SY"] == m["SH"] and m["SW"] == (nx + 3) // 4
        L = el[el[:, 0] == 0]
        lanes = lambda s: m["NLAST"] if s == m["SH"] - 1 else 4
        assert len(L) == 4 * sum((s + 1) * lanes(s) for s in range(m["SH"]))
        assert m["NLAST"] == n - 4 * (m["SH"] - 1)
        slots = [m["SY"], m["SY"], m["SW"], m["SW"], m["SW"], 4, m["SY"], m["SY"], m["SW"]]
        for f, S in enumerate(slots):
            assert (el[:, 0] == 1 + f).sum() == 4 * S, (nx, nu, f)
        seen[(nx, nu)] = m
    assert seen[(2, 1)]["SY"] // 4 == 0
    assert seen[(10, 3)]["NLAST"] == 1 and seen[(13, 4)]["NLAST"] == 1 and seen[(6, 1)]["NLAST"] == 3
    assert {m["NLAST"] for m in seen.values()} == {1, 2, 3, 4}
