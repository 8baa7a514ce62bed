"""TEST-ONLY reference for the dense stage cost 1/2 z_t' C_t z_t + q_t' z_t (MPC(diag_cost=False),
alqp_solve_lin_dense): OracleBackend plus `solve_lin_dense`, built from the oracle's own building blocks the way
OracleBackend.solve_lin is. The oracle sees diag(C); the off-diagonal part is added around it:

    gradient   g_t   += offdiag(C_t) z_t
    Hessian    H_tt  += offdiag(C_t)
    merit      phi   += 1/2 sum_t z_t' offdiag(C_t) z_t          (per line-search candidate)

Newton direction, line-search decision and dual update are the oracle's, unchanged. The reference the oracle is pinned
to cannot run this case, so the pin is tests/test_dense_cost_cpu.py's rotated-states test: a diagonal problem in rotated
coordinates is a dense problem here, and must give the oracle's own iterates."""
import numpy as np
import torch

from oracle import oracle_py as orc
from tests.oracle_backend import DUAL_UPDATE, INIT_MERIT, SAVE_FACTOR, OracleBackend, _bounds, _n, _sfx


def split_cost(C):
    """C [B,T,n,n] -> (diag(C) [B,T,n], offdiag(C) [B,T,n,n])."""
    Cd = np.diagonal(C, axis1=-2, axis2=-1).copy()
    off = C.copy()
    idx = np.arange(C.shape[-1])
    off[..., idx, idx] = 0
    return Cd, off


class DenseOracleBackend(OracleBackend):
    """`calls` records the solve entry points MPC reached. `trace` (a dict, optional argument of solve_lin_dense) gets
    one entry per Newton step under g, d, phi [n_ls,B], phi_prev, k, accept, and Hd / Hs of the last step."""

    name = "oracle-test-dense"

    def __init__(self):
        self.calls = []

    def solve_lin(self, *a, **kw):
        self.calls.append("solve_lin")
        return super().solve_lin(*a, **kw)

    @staticmethod
    def merit_dense(s, zz, xn, x0, ll, rr, Cd, off, q, lo, hi):
        npdt = zz.dtype.type
        ph, rp2 = orc.merit(s, zz, xn, x0, ll, rr, Cd, q, lo, hi)
        return (ph + npdt(0.5) * np.einsum("bti,btij,btj->b", zz, off, zz)).astype(npdt), rp2

    @staticmethod
    def grad_hess_dense(s, zz, xn, F, x0, ll, rr, Cd, off, q, lo, hi):
        g, Hd, Hs = orc.grad_hess(s, zz, xn, F, x0, ll, rr, Cd, q, lo, hi)
        return (g + np.einsum("btij,btj->bti", off, zz)).astype(g.dtype), (Hd + off).astype(g.dtype), Hs

    def solve_lin_dense(self, dims, Cs, q, F, c, x0, ulo, uhi, sb_u, st_u, z, lam, rho, phi, rnorm2=None,
                        info=None, status=None, factor=None, al_iter=2, max_newton=4, n_ls=20, flags=3,
                        rho_scale=10.0, trace=None, variant=None, skip=None):
        self.calls.append("solve_lin_dense")
        if skip is not None and float(skip[0]) != 0.0:
            return
        B, T, nx, nu = dims
        s = _sfx(z)
        npdt = np.float64 if s == "f64" else np.float32
        lo, hi = _bounds(ulo, uhi, sb_u, st_u, B, T, nu)
        C_, q_, F_, c_, x0_ = _n(Cs), _n(q), _n(F), _n(c), _n(x0)
        assert np.array_equal(C_, C_.transpose(0, 1, 3, 2)), "the host hands the solve a symmetric C"
        Cd, off = split_cost(C_)
        zz, ll, rr, ph = _n(z).copy(), _n(lam).copy(), _n(rho).copy(), _n(phi).copy()

        def xnext(v):
            return (np.einsum("btij,btj->bti", F_, v[:, :-1]) + c_).astype(npdt)

        L = None
        inf_acc = np.zeros(B, np.int32)
        for _ in range(al_iter):
            if flags & INIT_MERIT:
                ph, _ = self.merit_dense(s, zz, xnext(zz), x0_, ll, rr, Cd, off, q_, lo, hi)
            for _ in range(max_newton):
                g, Hd, Hs = self.grad_hess_dense(s, zz, xnext(zz), F_, x0_, ll, rr, Cd, off, q_, lo, hi)
                d, inf, L, _ = orc.newton_dir(s, g, Hd, Hs, nx, want_factor=True)
                inf_acc = np.where(inf_acc == 0, inf, inf_acc)
                phis = []
                for k in range(n_ls):
                    zc = (zz + npdt(2.0 ** -k) * d).astype(npdt)
                    phis.append(self.merit_dense(s, zc, xnext(zc), x0_, ll, rr, Cd, off, q_, lo, hi)[0])
                kk, acc, pm = orc.linesearch_pick(s, np.stack(phis), ph)
                if trace is not None:
                    for key, v in (("g", g), ("d", d), ("phi", np.stack(phis)), ("phi_prev", ph.copy()), ("k", kk),
                                   ("accept", acc)):
                        trace.setdefault(key, []).append(v)
                    trace["Hd"], trace["Hs"] = Hd, Hs
                alpha = np.where(acc > 0, 2.0 ** -kk.astype(np.float64), 0.0).astype(npdt)
                zz = np.where((acc > 0)[:, None, None], zz + alpha[:, None, None] * d, zz).astype(npdt)
                ph = pm
            if flags & DUAL_UPDATE:
                ll, rr = orc.dual_update(s, zz, xnext(zz), x0_, lo, hi, ll, rr)
                if rho_scale != 10.0:
                    rr = rr / 10.0 * rho_scale
        _, rp2 = self.merit_dense(s, zz, xnext(zz), x0_, ll, rr, Cd, off, q_, lo, hi)
        z.copy_(torch.from_numpy(zz)); lam.copy_(torch.from_numpy(ll)); rho.copy_(torch.from_numpy(rr))
        phi.copy_(torch.from_numpy(ph))
        if rnorm2 is not None:
            rnorm2.copy_(torch.from_numpy(rp2))
        if info is not None:
            cur = _n(info)
            info.copy_(torch.from_numpy(np.where(cur == 0, inf_acc, cur).astype(np.int32)))
        if status is not None:
            status.copy_(torch.from_numpy(np.isfinite(zz).all(axis=(1, 2)).astype(np.uint8)))
        if factor is not None and (flags & SAVE_FACTOR) and L is not None:
            factor.copy_(torch.from_numpy(self._pack_X(L)))


def dense_w(Hd, Hs, gbar):
    """w = -H^{-1} gbar with H assembled densely from the blocks of a Newton step (float64)."""
    B, T, n = gbar.shape
    w = np.empty((B, T, n))
    for b in range(B):
        H = np.zeros((T * n, T * n))
        for t in range(T):
            H[t * n:(t + 1) * n, t * n:(t + 1) * n] = Hd[b, t]
        for t in range(T - 1):
            H[(t + 1) * n:(t + 2) * n, t * n:(t + 1) * n] = Hs[b, t]
            H[t * n:(t + 1) * n, (t + 1) * n:(t + 2) * n] = Hs[b, t].T
        w[b] = -np.linalg.solve(H, np.asarray(gbar[b], np.float64).reshape(-1)).reshape(T, n)
    return w


def run_solve(be, C, q, F, c, x0, lo, hi, z0, lam0=None, rho0=None, phi0=None, **kw):
    """One solve_lin_dense call on tensors of any backend: -> dict(z, lam, rho, phi, rn2, info, status) (copies)."""
    B, T, n = z0.shape
    nx = x0.shape[1]
    nu = n - nx
    dev, dt = z0.device, z0.dtype
    z = z0.clone()
    lam = torch.zeros(B, T * nx + 2 * T * nu, dtype=dt, device=dev) if lam0 is None else lam0.clone()
    rho = torch.ones(B, dtype=dt, device=dev) if rho0 is None else rho0.clone()
    phi = torch.zeros(B, dtype=dt, device=dev) if phi0 is None else phi0.clone()   # (the merit carried between calls)
    rn2 = torch.zeros(B, dtype=dt, device=dev)
    info = torch.zeros(B, dtype=torch.int32, device=dev)
    status = torch.ones(B, dtype=torch.uint8, device=dev)
    sb, st = (0, 0) if lo.dim() == 1 else (T * nu, nu)
    ok = be.solve_lin_dense((B, T, nx, nu), C, q, F, c, x0, lo, hi, sb, st, z, lam, rho, phi, rnorm2=rn2, info=info,
                            status=status, **kw)
    return dict(z=z, lam=lam, rho=rho, phi=phi, rn2=rn2, info=info, status=status, ok=ok)
