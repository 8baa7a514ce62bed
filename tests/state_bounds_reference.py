"""TEST-ONLY reference for the state box rows xlo[t] <= x_t <= xhi[t] (MPC(x_lower=, x_upper=), alqp_solve_lin_xbox):
OracleBackend plus `solve_lin_xbox`, built from the oracle's own building blocks the way OracleBackend.solve_lin is. The
oracle sees the plain problem and the plain part of lam; the state rows are added around it by ONE function, `box_rows`,
which states every term a box row r_u = v - hi, r_l = -v + lo contributes (conventions of the control rows,
oracle/alqp_oracle_impl.h: merit_one, grad_hess_one, orc_dual_update):

    gradient     g     += (lam_u + rho max(r_u, 0)) - (lam_l + rho max(r_l, 0))
    Hessian      H_ii  += rho ([r_u >= 0] + [r_l >= 0])
    merit        phi   += lam_u r_u + lam_l r_l + rho/2 (max(r_u, 0)^2 + max(r_l, 0)^2)     (per line-search candidate)
    |r+|^2             += max(r_u, 0)^2 + max(r_l, 0)^2
    dual update  lam_u <- max(0, lam_u + rho r_u), lam_l <- max(0, lam_l + rho r_l)

Newton direction and line-search decision are the oracle's. The reference the oracle is pinned to cannot run this case
(its rows are commented out, al_utils.py:294-302), so the pins are tests/test_state_bounds_cpu.py's: `box_rows` applied
to the CONTROL rows equals what the oracle adds for them, and a problem whose bounded states are last stage's controls
is a control-bounded problem the oracle solves.

Multiplier layout: [B, T nx + T (2 nu + 2 nx)], the T nx equality rows, then per stage
[u - uhi | -u + ulo | x - xhi | -x + xlo]."""
import numpy as np
import torch

from oracle import oracle_py as orc
from tests.oracle_backend import DUAL_UPDATE, INIT_MERIT, SAVE_FACTOR, OracleBackend, _bounds, _n, _sfx


def box_rows(v, lo, hi, lam_u, lam_l, rho):
    """Every term of the box rows r_u = v - hi, r_l = -v + lo on the entries v [B,T,m] (lo, hi broadcast against v;
    lam_u, lam_l [B,T,m]; rho [B]), in v's dtype:
    -> g [B,T,m], Hd [B,T,m] (diagonal entries), phi [B], rp2 [B], (lam_u, lam_l) after the dual update."""
    dt = v.dtype.type
    lo, hi = np.broadcast_to(np.asarray(lo, v.dtype), v.shape), np.broadcast_to(np.asarray(hi, v.dtype), v.shape)
    r = np.reshape(rho, (-1, 1, 1)).astype(v.dtype)
    ru, rl = v - hi, -v + lo
    pu, pl = np.maximum(ru, dt(0)), np.maximum(rl, dt(0))
    g = (lam_u + r * pu) - (lam_l + r * pl)
    Hd = r * ((ru >= 0).astype(v.dtype) + (rl >= 0).astype(v.dtype))
    rp2 = (pu * pu + pl * pl).reshape(len(v), -1).sum(1)
    phi = (lam_u * ru + lam_l * rl).reshape(len(v), -1).sum(1) + dt(0.5) * np.reshape(rho, (-1,)).astype(v.dtype) * rp2
    new = (np.maximum(lam_u + r * ru, dt(0)), np.maximum(lam_l + r * rl, dt(0)))
    return g.astype(v.dtype), Hd.astype(v.dtype), phi.astype(v.dtype), rp2.astype(v.dtype), new


def lam_width(T, nx, nu):
    return T * nx + T * (2 * nu + 2 * nx)


def split_lam(lam, T, nx, nu):
    """lam [B, T nx + T (2 nu + 2 nx)] -> (plain lam [B, T nx + 2 T nu], lam_xu [B,T,nx], lam_xl [B,T,nx]) (copies)."""
    B = lam.shape[0]
    neq = T * nx
    li = lam[:, neq:].reshape(B, T, 2 * nu + 2 * nx)
    plain = np.concatenate([lam[:, :neq], li[..., :2 * nu].reshape(B, -1)], 1)
    return np.ascontiguousarray(plain), li[..., 2 * nu:2 * nu + nx].copy(), li[..., 2 * nu + nx:].copy()


def join_lam(plain, lxu, lxl, T, nx, nu):
    B = plain.shape[0]
    neq = T * nx
    li = np.concatenate([plain[:, neq:].reshape(B, T, 2 * nu), lxu, lxl], 2)
    return np.ascontiguousarray(np.concatenate([plain[:, :neq], li.reshape(B, -1)], 1))


def _xbounds(xlo, xhi, sb, st, B, T, nx):
    lo, hi = _n(xlo), _n(xhi)
    if sb == 0 and st == 0:
        return lo.reshape(1, 1, nx), hi.reshape(1, 1, nx)
    return lo.reshape(B, T, nx), hi.reshape(B, T, nx)


def merit_xbox(s, zz, xn, x0, ll, lxu, lxl, rr, Qd, q, lo, hi, xlo, xhi):
    """(phi, rp2) with the state rows: the oracle's on the plain problem plus box_rows' on the states."""
    nx = x0.shape[1]
    ph, rp2 = orc.merit(s, zz, xn, x0, ll, rr, Qd, q, lo, hi)
    _, _, px, rx, _ = box_rows(zz[..., :nx], xlo, xhi, lxu, lxl, rr)
    return (ph + px).astype(zz.dtype), (rp2 + rx).astype(zz.dtype)


def grad_hess_xbox(s, zz, xn, F, x0, ll, lxu, lxl, rr, Qd, q, lo, hi, xlo, xhi):
    nx = x0.shape[1]
    g, Hd, Hs = orc.grad_hess(s, zz, xn, F, x0, ll, rr, Qd, q, lo, hi)
    gx, hx, _, _, _ = box_rows(zz[..., :nx], xlo, xhi, lxu, lxl, rr)
    g, Hd = g.copy(), Hd.copy()
    g[..., :nx] += gx
    i = np.arange(nx)
    Hd[..., i, i] += hx
    return g, Hd, Hs


class XboxOracleBackend(OracleBackend):
    """`calls` records the solve entry points MPC reached. `trace` (a dict, optional argument of solve_lin_xbox) gets one
    entry per Newton step under g, d, phi [n_ls,B], phi_prev, k, accept, z (the iterate the step started from), and
    Hd / Hs of the last step."""

    name = "oracle-test-xbox"

    def __init__(self):
        self.calls = []

    def solve_lin(self, *a, **kw):
        self.calls.append("solve_lin")
        return super().solve_lin(*a, **kw)

    def solve_lin_xbox(self, dims, Qd, q, F, c, x0, ulo, uhi, sb_u, st_u, xlo, xhi, sb_x, st_x, z, lam, rho, phi,
                       rnorm2=None, info=None, status=None, factor=None, al_iter=2, max_newton=4, n_ls=20, flags=3,
                       rho_scale=10.0, trace=None, variant=None, skip=None):
        self.calls.append("solve_lin_xbox")
        if skip is not None and float(skip[0]) != 0.0:
            return
        B, T, nx, nu = dims
        assert tuple(lam.shape) == (B, lam_width(T, nx, nu)), tuple(lam.shape)
        s = _sfx(z)
        npdt = np.float64 if s == "f64" else np.float32
        lo, hi = _bounds(ulo, uhi, sb_u, st_u, B, T, nu)
        xl, xh = _xbounds(xlo, xhi, sb_x, st_x, B, T, nx)
        assert np.isfinite(xl).all() and np.isfinite(xh).all(), "the host hands the solve finite bounds"
        Qd_, q_, F_, c_, x0_ = _n(Qd), _n(q), _n(F), _n(c), _n(x0)
        zz, rr, ph = _n(z).copy(), _n(rho).copy(), _n(phi).copy()
        ll, lxu, lxl = split_lam(_n(lam), T, nx, nu)

        def xnext(v):
            return (np.einsum("btij,btj->bti", F_, v[:, :-1]) + c_).astype(npdt)

        def merit(v):
            return merit_xbox(s, v, xnext(v), x0_, ll, lxu, lxl, rr, Qd_, q_, lo, hi, xl, xh)

        L = None
        inf_acc = np.zeros(B, np.int32)
        for _ in range(al_iter):
            if flags & INIT_MERIT:
                ph, _ = merit(zz)
            for _ in range(max_newton):
                g, Hd, Hs = grad_hess_xbox(s, zz, xnext(zz), F_, x0_, ll, lxu, lxl, rr, Qd_, q_, lo, hi, xl, xh)
                d, inf, L, _ = orc.newton_dir(s, g, Hd, Hs, nx, want_factor=True)
                inf_acc = np.where(inf_acc == 0, inf, inf_acc)
                phis = np.stack([merit((zz + npdt(2.0 ** -k) * d).astype(npdt))[0] for k in range(n_ls)])
                kk, acc, pm = orc.linesearch_pick(s, phis, ph)
                if trace is not None:
                    for key, v in (("g", g), ("d", d), ("phi", phis), ("phi_prev", ph.copy()), ("k", kk), ("accept", acc),
                                   ("z", zz.copy())):
                        trace.setdefault(key, []).append(v)
                    trace["Hd"], trace["Hs"] = Hd, Hs
                alpha = np.where(acc > 0, 2.0 ** -kk.astype(np.float64), 0.0).astype(npdt)
                zz = np.where((acc > 0)[:, None, None], zz + alpha[:, None, None] * d, zz).astype(npdt)
                ph = pm
            if flags & DUAL_UPDATE:
                _, _, _, _, (lxu, lxl) = box_rows(zz[..., :nx], xl, xh, lxu, lxl, rr)   # (with the rho of this iteration)
                ll, rr = orc.dual_update(s, zz, xnext(zz), x0_, lo, hi, ll, rr)
                if rho_scale != 10.0:
                    rr = rr / 10.0 * rho_scale
        _, rp2 = merit(zz)
        z.copy_(torch.from_numpy(zz)); rho.copy_(torch.from_numpy(rr)); phi.copy_(torch.from_numpy(ph))
        lam.copy_(torch.from_numpy(join_lam(ll, lxu, lxl, T, nx, nu)))
        if rnorm2 is not None:
            rnorm2.copy_(torch.from_numpy(rp2))
        if info is not None:
            cur = _n(info)
            info.copy_(torch.from_numpy(np.where(cur == 0, inf_acc, cur).astype(np.int32)))
        if status is not None:
            status.copy_(torch.from_numpy(np.isfinite(zz).all(axis=(1, 2)).astype(np.uint8)))
        if factor is not None and (flags & SAVE_FACTOR) and L is not None:
            factor.copy_(torch.from_numpy(self._pack_X(L)))


def run_solve(be, Qd, q, F, c, x0, lo, hi, xlo, xhi, z0, lam0=None, rho0=None, phi0=None, **kw):
    """One solve_lin_xbox call on tensors of any backend: -> dict(z, lam, rho, phi, rn2, info, status) (copies)."""
    B, T, n = z0.shape
    nx = x0.shape[1]
    nu = n - nx
    dev, dt = z0.device, z0.dtype
    z = z0.clone()
    lam = torch.zeros(B, lam_width(T, nx, nu), dtype=dt, device=dev) if lam0 is None else lam0.clone()
    rho = torch.ones(B, dtype=dt, device=dev) if rho0 is None else rho0.clone()
    phi = torch.zeros(B, dtype=dt, device=dev) if phi0 is None else phi0.clone()
    rn2 = torch.zeros(B, dtype=dt, device=dev)
    info = torch.zeros(B, dtype=torch.int32, device=dev)
    status = torch.ones(B, dtype=torch.uint8, device=dev)
    sb, st = (0, 0) if lo.dim() == 1 else (T * nu, nu)
    sbx, stx = (0, 0) if xlo.dim() == 1 else (T * nx, nx)
    ok = be.solve_lin_xbox((B, T, nx, nu), Qd, q, F, c, x0, lo, hi, sb, st, xlo, xhi, sbx, stx, z, lam, rho, phi,
                           rnorm2=rn2, info=info, status=status, **kw)
    return dict(z=z, lam=lam, rho=rho, phi=phi, rn2=rn2, info=info, status=status, ok=ok)


def xbox_problem(B, T, nx, nu, dtype, per_stage=False, seed=5, width=0.6, push=False):
    """CPU tensors of the active-bound synthetic problem plus state bounds that bind: |x| <= width (the reference
    trajectory and x0 are N(0,1) draws, so at width 0.6 about half of the states want to be outside), per (b, t) entry
    widened by its own factor in [1, 1.5) with `per_stage`, where stage 0 is relaxed to contain x0. `push`: the
    reference trajectory of state 0 is moved above +width + 0.5 and that of state 1 below -width - 0.5 on every stage of
    every instance, so that each instance keeps an upper and a lower state row active."""
    from deq_mpc_corl_amd import synthetic_problem
    p = synthetic_problem(B, T, nx, nu, seed=seed, dtype=dtype, active=True)
    f64 = torch.float64
    if push:
        xref = p.xref.clone()
        xref[..., 0] = xref[..., 0].abs() + width + 0.5
        xref[..., 1] = -xref[..., 1].abs() - width - 0.5
        p = p._replace(xref=xref, z0=xref.clone(), q=-(p.Qd * xref))
    if per_stage:
        g = torch.Generator().manual_seed(seed + 11)
        w = width * (1.0 + 0.5 * torch.rand(B, T, nx, generator=g, dtype=f64))
        xhi, xlo = w.clone(), -w.flip(0)
        xhi[:, 0] = torch.maximum(xhi[:, 0], p.x0.double() + 0.05)
        xlo[:, 0] = torch.minimum(xlo[:, 0], p.x0.double() - 0.05)
        xhi, xlo = xhi.to(dtype).contiguous(), xlo.to(dtype).contiguous()
    else:
        xhi = torch.full((nx,), width, dtype=dtype)
        xlo = -xhi
    return dict(Qd=p.Qd, q=p.q, F=p.F, c=p.c, x0=p.x0, lo=p.u_lo, hi=p.u_hi, xlo=xlo, xhi=xhi, z0=p.z0.clone(),
                dims=(B, T, nx, nu))


def xbox_residuals(pr, z):
    """State-row residuals (x - xhi, -x + xlo) [B,T,nx] each, numpy in z's dtype."""
    nx = pr["dims"][2]
    x = _n(z)[..., :nx]
    return x - _n(pr["xhi"]), -x + _n(pr["xlo"])
