"""Four-lane emulation of the quad kernels' triangular solves on own elements (csrc/alqp_quad.hpp: lsolve_own,
ltsolve_own), indexed exactly as the kernel indexes them: lane q holds row 4m + q of the factor in slot m of its panel
(QCfg::hidx), element 4m + q of a vector in slot m; the diagonal slot of a column is masked lane by lane and the last
slot may hold fewer than four rows.

Every panel word the kernel must not use is NaN here: the words on the upper side of the diagonal inside the 4 x 4
diagonal blocks (the forward sweep leaves arbitrary values there) and the whole panel row of a lane that owns no row
in the last slot (the kernel re-reads lane 0's words there). The solves must still return the solution of
L D L' x = b, on every lane (the replicated copy) and as own elements with zeros where a lane owns nothing.
No GPU: numpy only."""
import numpy as np
import pytest

# n = nx + nu of every compiled size (ALQP_FOR_EACH_DIMS)
SIZES = [3, 5, 6, 7, 8, 10, 13, 16, 17, 18]
LANES = np.arange(4)


def hidx(s, j):
    return 2 * s * (s + 1) + j


class Panel:
    def __init__(self, n):
        self.n = n
        self.sh = (n + 3) // 4
        self.ht = 2 * self.sh * (self.sh + 1)
        self.nlast = n - 4 * (self.sh - 1)

    def lanes_of(self, s):
        return self.nlast if s == self.sh - 1 else 4

    def pack(self, L, p):
        """Hh[k][j] = L[k][j] p_j below the diagonal, 1 / p_k on it; NaN wherever the kernel may not look."""
        H = np.full((4, self.ht), np.nan)
        for s in range(self.sh):
            for q in range(4):
                k = 4 * s + q
                if k >= self.n:
                    continue
                for j in range(4 * (s + 1)):
                    if j < k:
                        H[q, hidx(s, j)] = L[k, j] * p[j]
                    elif j == k:
                        H[q, hidx(s, j)] = 1.0 / p[k]
        return H

    def own_of(self, v):
        o = np.zeros((4, self.sh))
        for k in range(self.n):
            o[k & 3, k >> 2] = v[k]
        return o


def qbv(v, src):
    return np.full(4, v[src & 3])


def qsum(v):
    v = v + v[[1, 0, 3, 2]]
    return v + v[[2, 3, 0, 1]]


def lane_lo(m, j):
    return (j & 3) + 1 if m == (j >> 2) else 0


def in_lanes(lo, hi):
    return (LANES >= lo) & (LANES < hi)


def lsolve_own(P, H, u):
    """u <- Lh^{-1} u, column form; the last slot's lanes without a row are not masked (their slots hold garbage)."""
    u = u.copy()
    for j in range(P.n):
        mj = j >> 2
        wj = qbv(u[:, mj] * H[:, hidx(mj, j)], j)
        for m in range(mj, P.sh):
            lo = lane_lo(m, j)
            if lo >= P.lanes_of(m):
                continue
            v = -H[:, hidx(m, j)] * wj + u[:, m]
            u[:, m] = v if lo == 0 else np.where(LANES >= lo, v, u[:, m])
    return u


def ltsolve_own(P, H, y):
    """d <- Lh^{-T} D^{-1} y, dot form; returns (own elements, replicated copy)."""
    d = np.zeros((4, P.sh))
    rep = np.zeros((4, P.n))
    for i in range(P.n - 1, -1, -1):
        mi = i >> 2
        p, have = np.zeros(4), False
        for m in range(mi, P.sh):
            lo, hi = lane_lo(m, i), P.lanes_of(m)
            if lo >= hi:
                continue
            h = H[:, hidx(m, i)]
            if not (lo == 0 and hi == 4):
                h = np.where(in_lanes(lo, hi), h, 0.0)
            p = h * d[:, m] + p if have else h * d[:, m]
            have = True
        r = y[:, mi]
        if have:
            r = r - qsum(p)
        di = qbv(r * H[:, hidx(mi, i)], i)
        rep[:, i] = di
        d[:, mi] = np.where(LANES == (i & 3), di, d[:, mi])
    return d, rep


def _problem(n, seed):
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((n, n))
    A = M @ M.T + n * np.eye(n)
    Lc = np.linalg.cholesky(A)
    dg = np.diag(Lc)
    return A, Lc / dg, dg * dg, rng.standard_normal(n)


@pytest.mark.parametrize("n", SIZES)
def test_own_element_solves_match_dense_solve(n):
    P = Panel(n)
    for seed in range(3):
        A, L, p, b = _problem(n, 100 * n + seed)
        H = P.pack(L, p)
        assert np.isnan(H).any()   # the poison is really there
        u = lsolve_own(P, H, P.own_of(b))
        # forward substitution: own elements of L^{-1} b (lanes without a row are not looked at)
        u_ref = np.linalg.solve(L, b)
        for k in range(n):
            assert np.isfinite(u[k & 3, k >> 2])
            assert abs(u[k & 3, k >> 2] - u_ref[k]) <= 1e-12 * np.abs(u_ref).max()
        d, rep = ltsolve_own(P, H, u)
        x = np.linalg.solve(A, b)
        scale = np.abs(x).max()
        assert np.isfinite(rep).all() and np.isfinite(d).all()
        for q in range(4):
            assert np.abs(rep[q] - x).max() <= 1e-12 * scale
        for s in range(P.sh):
            for q in range(4):
                k = 4 * s + q
                assert d[q, s] == (rep[0, k] if k < n else 0.0)


@pytest.mark.parametrize("n", SIZES)
def test_slot_masks_cover_exactly_the_rows_below_the_diagonal(n):
    """Over all slots, the lanes a column step may touch are the rows j < k < n, each once."""
    P = Panel(n)
    for j in range(n):
        rows = []
        for m in range(j >> 2, P.sh):
            lo, hi = lane_lo(m, j), P.lanes_of(m)
            if lo >= hi:
                continue
            rows += [4 * m + q for q in range(4) if in_lanes(lo, hi)[q]]
        assert rows == list(range(j + 1, n))
