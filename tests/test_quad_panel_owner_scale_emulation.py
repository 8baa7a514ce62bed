"""Four-lane emulation of one stage's panel factorisation plus Schur accumulation of the quad forward sweep
(csrc/alqp_quad.hpp, Quad::forward), indexed as the kernel indexes it (QCfg::hidx, lanes_of, qbv; the helpers of
tests/test_quad_own_solves_emulation.py): lane q holds row 4m + q of H in slot m of its panel and row 4s + q of W in
slot s; Y is replicated on the four lanes; S and Sy are own rows.

The stage is emulated twice. `broadcast_then_scale` is the source -DALQP_PANEL_OWNER_SCALE=0 compiles: the multiplier
l_kj = qbv(H[k][j], k) * (1/p_j) is formed on all four lanes behind the broadcast and the updates negate their
multiplicand, fma(-a, l, c). `owner_scales` is the product: the owner of row k multiplies its entry of column j by
-1/p_j, the broadcast carries the product, the updates are fma(a, -l, c); likewise W[b][j] / p_j for the Schur sums.
Both must give the same BITS in every word, since identical operands reach every multiply and every fma:
x * (-y) == -(x * y) exactly and (-a) * l == a * (-l) exactly, whatever the rounding of the fma around them.

Every panel word the kernel may not use is NaN here: above the diagonal inside the 4 x 4 diagonal blocks, and the whole
panel row of a lane without a row in the last slot. The owner-scaled column is made of those words too (the kernel scales
whole slots); none of them may reach a defined word. W's slots of lanes without a row hold zeros, as in the kernel
(its quad sums run over all four lanes).

fma: fp32 as one fp64 product (exact) and sum, rounded to fp32; fp64 as product then sum. The identity under test does
not depend on the fusion. That the emulation is the kernel's algorithm is checked against a dense factorisation:
Hh[k][j] = L[k][j] p_j, 1/p_k on the diagonal, S = W A^-1 W', Sy = W A^-1 y.
No GPU: numpy only."""
import numpy as np
import pytest

from tests.test_quad_own_solves_emulation import LANES, Panel, hidx, qbv

# (nx, nu) of every compiled size (ALQP_FOR_EACH_DIMS): n = 3, 5, 6, 7, 8, 10, 13, 16, 17, 18
DIMS = [(2, 1), (4, 1), (4, 2), (6, 1), (6, 2), (8, 2), (10, 3), (12, 4), (13, 4), (14, 4)]
BITS = {np.float32: np.uint32, np.float64: np.uint64}


def fma(a, b, c):
    if a.dtype == np.float32:
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    return a * b + c


def pack(P, nx, A, F, y, dt):
    """The stage's registers in front of the panel: (H, W, Y, S, Sy), NaN wherever the kernel may not look."""
    sw = (nx + 3) // 4
    H = np.full((4, P.ht), np.nan, dt)
    for s in range(P.sh):
        for q in range(4):
            k = 4 * s + q
            if k < P.n:
                for j in range(k + 1):
                    H[q, hidx(s, j)] = A[k, j]
    W = np.zeros((4, sw, P.n), dt)
    for r in range(nx):
        W[r & 3, r >> 2] = F[r]
    Y = np.tile(y.astype(dt), (4, 1))
    return H, W, Y, np.zeros((4, 2 * sw * (sw + 1)), dt), np.zeros((4, sw), dt)


def stage(P, nx, regs, owner_scales):
    H, W, Y, S, Sy = (a.copy() for a in regs)
    dt = H.dtype.type
    sw = W.shape[1]
    with np.errstate(invalid="ignore"):
        for j in range(P.n):
            dj = hidx(j >> 2, j)
            p = qbv(H[:, dj], j)
            assert (p > 0).all()
            ip = dt(1) / np.abs(p)
            if owner_scales:
                nip = -ip
                hs = {m: H[:, hidx(m, j)] * nip for m in range(j >> 2, P.sh)}   # whole slots, poison included
            for k in range(j + 1, P.n):
                if owner_scales:
                    nlkj = qbv(hs[k >> 2], k)
                    for s in range(k >> 2, P.sh):
                        H[:, hidx(s, k)] = fma(H[:, hidx(s, j)], nlkj, H[:, hidx(s, k)])
                    for s in range(sw):
                        W[:, s, k] = fma(W[:, s, j], nlkj, W[:, s, k])
                    Y[:, k] = fma(Y[:, j], nlkj, Y[:, k])
                else:
                    lkj = qbv(H[:, hidx(k >> 2, j)], k) * ip
                    for s in range(k >> 2, P.sh):
                        H[:, hidx(s, k)] = fma(-H[:, hidx(s, j)], lkj, H[:, hidx(s, k)])
                    for s in range(sw):
                        W[:, s, k] = fma(-W[:, s, j], lkj, W[:, s, k])
                    Y[:, k] = fma(-Y[:, j], lkj, Y[:, k])
            if owner_scales:
                wsc = [W[:, s, j] * ip for s in range(sw)]
            for b in range(nx):
                wbj = qbv(wsc[b >> 2], b) if owner_scales else qbv(W[:, b >> 2, j], b) * ip
                for s in range(b >> 2, sw):
                    S[:, hidx(s, b)] = fma(W[:, s, j], wbj, S[:, hidx(s, b)])
            yip = Y[:, j] * ip
            for s in range(sw):
                Sy[:, s] = fma(W[:, s, j], yip, Sy[:, s])
            H[:, dj] = np.where(LANES == (j & 3), ip, H[:, dj])
    return H, W, Y, S, Sy


def readable(P):
    """The words of H the kernel may read behind the panel: row k = 4s + q < n, columns j <= k."""
    m = np.zeros((4, P.ht), bool)
    for s in range(P.sh):
        for q in range(4):
            k = 4 * s + q
            if k < P.n:
                m[q, [hidx(s, j) for j in range(k + 1)]] = True
    return m


def _problem(n, nx, seed):
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((n, n))
    return M @ M.T + n * np.eye(n), rng.standard_normal((nx, n)), rng.standard_normal(n)


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("nx,nu", DIMS)
def test_owner_scaled_panel_gives_the_same_bits(nx, nu, dt):
    n = nx + nu
    P = Panel(n)
    ok = readable(P)
    for seed in range(3):
        A, F, y = _problem(n, nx, 1000 * n + seed)
        regs = pack(P, nx, A.astype(dt), F.astype(dt), y, dt)
        assert np.isnan(regs[0]).any() and not np.isnan(regs[0][ok]).any()   # the poison is there, and only there
        old = stage(P, nx, regs, owner_scales=False)
        new = stage(P, nx, regs, owner_scales=True)
        for name, a, b in zip(("H", "W", "Y", "S", "Sy"), old, new):
            assert a.dtype == dt and b.dtype == dt
            sel = ok if name == "H" else np.ones(a.shape, bool)
            assert np.isfinite(a[sel]).all() and np.isfinite(b[sel]).all(), name   # no NaN reached a defined word
            assert np.array_equal(a[sel].view(BITS[dt]), b[sel].view(BITS[dt])), name


@pytest.mark.parametrize("nx,nu", DIMS)
def test_emulated_stage_is_the_factorisation(nx, nu):
    """fp64, owner-scaled form against a dense factorisation (1e-12 relative: n <= 18 well-conditioned rows)."""
    n = nx + nu
    P = Panel(n)
    A, F, y = _problem(n, nx, 7 * n)
    H, W, Y, S, Sy = stage(P, nx, pack(P, nx, A, F, y, np.float64), owner_scales=True)
    Lc = np.linalg.cholesky(A)
    dg = np.diag(Lc)
    L, p = Lc / dg, dg * dg
    Sref, Syref = F @ np.linalg.solve(A, F.T), F @ np.linalg.solve(A, y)
    for k in range(n):
        q, s = k & 3, k >> 2
        for j in range(k + 1):
            ref = 1.0 / p[k] if j == k else L[k, j] * p[j]
            assert abs(H[q, hidx(s, j)] - ref) <= 1e-12 * np.abs(A).max()
    for r in range(nx):
        q, s = r & 3, r >> 2
        assert abs(Sy[q, s] - Syref[r]) <= 1e-12 * max(1.0, np.abs(Syref).max())
        for b in range(r + 1):
            assert abs(S[q, hidx(s, b)] - Sref[r, b]) <= 1e-12 * max(1.0, np.abs(Sref).max())
