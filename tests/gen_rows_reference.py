"""TEST-ONLY reference for the dense cost, the state box and the general rows TOGETHER (alqp_solve_lin_gen,
HipBackend.solve_lin_gen): OracleBackend plus `solve_lin_gen`, composed from what the three single-feature references
pin and nothing else - `split_cost` and the dense merit / Hessian of tests/dense_cost_reference.py, `box_rows` of
tests/state_bounds_reference.py, `poly_rows` of tests/poly_rows_reference.py. The only arithmetic here is the sum of
their terms on top of the oracle's plain problem:

    g   = oracle + offdiag(C) z        + box_rows.g on the states   + poly_rows.g
    H   = oracle + offdiag(C)          + box_rows.Hd on the diagonal + poly_rows.H
    phi = oracle + 1/2 z' offdiag(C) z + box_rows.phi               + poly_rows.phi
    |r+|^2 and the dual update likewise, each feature's own.

Multiplier layout: [B, T nx + T (2 nu + [2 nx] + [m])], the T nx equality rows, then per stage
[u - uhi | -u + ulo | x - xhi | -x + xlo | G_t z_t - h_t], a feature's rows present exactly when the feature is."""
import numpy as np
import torch

from oracle import oracle_py as orc
from tests.dense_cost_reference import DenseOracleBackend, split_cost
from tests.oracle_backend import DUAL_UPDATE, INIT_MERIT, SAVE_FACTOR, OracleBackend, _bounds, _n, _sfx
from tests.poly_rows_reference import _rows, poly_problem, poly_rows
from tests.poly_rows_reference import strides as poly_strides
from tests.state_bounds_reference import _xbounds, box_rows


def lam_width(T, nx, nu, xbox, m):
    return T * nx + T * (2 * nu + (2 * nx if xbox else 0) + m)


def split_lam(lam, T, nx, nu, xbox, m):
    """lam [B, lam_width] -> (plain lam [B, T nx + 2 T nu], lam_xu, lam_xl [B,T,nx] or None, row multipliers [B,T,m] or
    None) (copies)."""
    B = lam.shape[0]
    neq, xr = T * nx, 2 * nx if xbox else 0
    li = lam[:, neq:].reshape(B, T, 2 * nu + xr + m)
    plain = np.ascontiguousarray(np.concatenate([lam[:, :neq], li[..., :2 * nu].reshape(B, -1)], 1))
    lxu = li[..., 2 * nu:2 * nu + nx].copy() if xbox else None
    lxl = li[..., 2 * nu + nx:2 * nu + 2 * nx].copy() if xbox else None
    lp = li[..., 2 * nu + xr:].copy() if m else None
    return plain, lxu, lxl, lp


def join_lam(plain, lxu, lxl, lp, T, nx, nu):
    B = plain.shape[0]
    neq = T * nx
    parts = [plain[:, neq:].reshape(B, T, 2 * nu)] + ([lxu, lxl] if lxu is not None else []) + ([lp] if lp is not None else [])
    return np.ascontiguousarray(np.concatenate([plain[:, :neq], np.concatenate(parts, 2).reshape(B, -1)], 1))


class GenTerms:
    """The composed merit and gradient / Hessian of one problem: the oracle's plain problem plus each present
    feature's terms. `off` offdiag(C) or None, (xl, xh) broadcastable state bounds or None, (Gr, hr) rows or None."""

    def __init__(self, s, nx, Cd, off, q, F, c, x0, lo, hi, xb, rows):
        self.s, self.nx, self.Cd, self.off, self.q, self.F, self.c, self.x0 = s, nx, Cd, off, q, F, c, x0
        self.lo, self.hi, self.xb, self.rows = lo, hi, xb, rows
        self.npdt = np.float64 if s == "f64" else np.float32

    def xnext(self, v):
        return (np.einsum("btij,btj->bti", self.F, v[:, :-1]) + self.c).astype(self.npdt)

    def merit(self, v, ll, lxu, lxl, lp, rr):
        """(phi, rp2)."""
        xn = self.xnext(v)
        if self.off is not None:
            ph, rp2 = DenseOracleBackend.merit_dense(self.s, v, xn, self.x0, ll, rr, self.Cd, self.off, self.q, self.lo, self.hi)
        else:
            ph, rp2 = orc.merit(self.s, v, xn, self.x0, ll, rr, self.Cd, self.q, self.lo, self.hi)
        if self.xb is not None:
            _, _, px, rx, _ = box_rows(v[..., :self.nx], *self.xb, lxu, lxl, rr)
            ph, rp2 = (ph + px).astype(v.dtype), (rp2 + rx).astype(v.dtype)
        if self.rows is not None:
            _, _, pp, rx, _ = poly_rows(v, *self.rows, lp, rr)
            ph, rp2 = (ph + pp).astype(v.dtype), (rp2 + rx).astype(v.dtype)
        return ph, rp2

    def grad_hess(self, v, ll, lxu, lxl, lp, rr):
        xn = self.xnext(v)
        if self.off is not None:
            g, Hd, Hs = DenseOracleBackend.grad_hess_dense(self.s, v, xn, self.F, self.x0, ll, rr, self.Cd, self.off, self.q,
                                                           self.lo, self.hi)
        else:
            g, Hd, Hs = orc.grad_hess(self.s, v, xn, self.F, self.x0, ll, rr, self.Cd, self.q, self.lo, self.hi)
        if self.xb is not None:
            gx, hx, _, _, _ = box_rows(v[..., :self.nx], *self.xb, lxu, lxl, rr)
            g, Hd = g.copy(), Hd.copy()
            g[..., :self.nx] += gx
            i = np.arange(self.nx)
            Hd[..., i, i] += hx
        if self.rows is not None:
            gp, Hp, _, _, _ = poly_rows(v, *self.rows, lp, rr)
            g, Hd = (g + gp).astype(v.dtype), (Hd + Hp).astype(v.dtype)
        return g, Hd, Hs

    def dual_update(self, v, ll, lxu, lxl, lp, rr):
        if self.xb is not None:
            _, _, _, _, (lxu, lxl) = box_rows(v[..., :self.nx], *self.xb, lxu, lxl, rr)   # (with the rho of this iteration)
        if self.rows is not None:
            _, _, _, _, lp = poly_rows(v, *self.rows, lp, rr)
        ll, rr = orc.dual_update(self.s, v, self.xnext(v), self.x0, self.lo, self.hi, ll, rr)
        return ll, lxu, lxl, lp, rr


def gen_terms(dims, Qd_or_C, q, F, c, x0, ulo, uhi, sb_u, st_u, xbnd, poly, s):
    B, T, nx, nu = dims
    lo, hi = _bounds(ulo, uhi, sb_u, st_u, B, T, nu)
    Cn = _n(Qd_or_C)
    Cd, off = (Cn, None)
    if Cn.ndim == 4:
        assert np.array_equal(Cn, Cn.transpose(0, 1, 3, 2)), "the host hands the solve a symmetric C"
        Cd, off = split_cost(Cn)
    xb = rows = None
    if xbnd is not None:
        xb = _xbounds(*xbnd, B, T, nx)
        assert np.isfinite(xb[0]).all() and np.isfinite(xb[1]).all(), "the host hands the solve finite bounds"
    if poly is not None:
        G, h, m, sb_g, st_g, sb_h, st_h = poly
        rows = _rows(G, h, sb_g, st_g, sb_h, st_h, B, T, m, nx + nu)
        assert np.isfinite(rows[0]).all() and np.isfinite(rows[1]).all(), "the host hands the solve finite rows"
    return GenTerms(s, nx, Cd, off, _n(q), _n(F), _n(c), _n(x0), lo, hi, xb, rows)


class GenOracleBackend(OracleBackend):
    """`calls` records the solve entry points MPC reached. `trace` (a dict, optional argument of solve_lin_gen) gets one
    entry per Newton step under g, d, phi [n_ls,B], phi_prev, k, accept, z (the iterate the step started from), and
    Hd / Hs of the last step; `newton_counts` (a list) the Newton steps per AL iteration when `exit_tol` is given
    (the batch-global exit test of al_utils.py:551-564 on the composed |r+|)."""

    name = "oracle-test-gen"

    def __init__(self):
        self.calls = []

    def solve_lin(self, *a, **kw):
        self.calls.append("solve_lin")
        return super().solve_lin(*a, **kw)

    def solve_lin_gen(self, dims, Qd_or_C, q, F, c, x0, ulo, uhi, sb_u, st_u, xbnd, poly, z, lam, rho, phi,
                      rnorm2=None, info=None, status=None, factor=None, al_iter=2, max_newton=4, n_ls=20, flags=3,
                      rho_scale=10.0, trace=None, variant=None, skip=None, ref_exit_counts=None, exit_tol=1e-3):
        self.calls.append("solve_lin_gen")
        if skip is not None and float(skip[0]) != 0.0:
            return
        B, T, nx, nu = dims
        m = poly[2] if poly is not None else 0
        assert tuple(lam.shape) == (B, lam_width(T, nx, nu, xbnd is not None, m)), tuple(lam.shape)
        s = _sfx(z)
        npdt = np.float64 if s == "f64" else np.float32
        tm = gen_terms(dims, Qd_or_C, q, F, c, x0, ulo, uhi, sb_u, st_u, xbnd, poly, s)
        zz, rr, ph = _n(z).copy(), _n(rho).copy(), _n(phi).copy()
        ll, lxu, lxl, lp = split_lam(_n(lam), T, nx, nu, xbnd is not None, m)

        def norm(v):
            return float(np.sqrt(tm.merit(v, ll, lxu, lxl, lp, rr)[1].astype(np.float64).sum()))

        L = None
        inf_acc = np.zeros(B, np.int32)
        for _ in range(al_iter):
            if flags & INIT_MERIT:
                ph, _ = tm.merit(zz, ll, lxu, lxl, lp, rr)
            old = norm(zz) if ref_exit_counts is not None else None
            done = 0
            for _ in range(max_newton):
                g, Hd, Hs = tm.grad_hess(zz, ll, lxu, lxl, lp, rr)
                d, inf, L, _ = orc.newton_dir(s, g, Hd, Hs, nx, want_factor=True)
                inf_acc = np.where(inf_acc == 0, inf, inf_acc)
                phis = np.stack([tm.merit((zz + npdt(2.0 ** -k) * d).astype(npdt), ll, lxu, lxl, lp, rr)[0]
                                 for k in range(n_ls)])
                kk, acc, pm = orc.linesearch_pick(s, phis, ph)
                if trace is not None:
                    for key, v in (("g", g), ("d", d), ("phi", phis), ("phi_prev", ph.copy()), ("k", kk), ("accept", acc),
                                   ("z", zz.copy())):
                        trace.setdefault(key, []).append(v)
                    trace["Hd"], trace["Hs"] = Hd, Hs
                alpha = np.where(acc > 0, 2.0 ** -kk.astype(np.float64), 0.0).astype(npdt)
                zz = np.where((acc > 0)[:, None, None], zz + alpha[:, None, None] * d, zz).astype(npdt)
                ph = pm
                done += 1
                if ref_exit_counts is not None:
                    new = norm(zz)
                    if new < exit_tol or abs(old - new) / new < exit_tol:
                        break
                    old = new
            if ref_exit_counts is not None:
                ref_exit_counts.append(done)
            if flags & DUAL_UPDATE:
                ll, lxu, lxl, lp, rr = tm.dual_update(zz, ll, lxu, lxl, lp, rr)
                if rho_scale != 10.0:
                    rr = rr / 10.0 * rho_scale
        _, rp2 = tm.merit(zz, ll, lxu, lxl, lp, rr)
        z.copy_(torch.from_numpy(zz)); rho.copy_(torch.from_numpy(rr)); phi.copy_(torch.from_numpy(ph))
        lam.copy_(torch.from_numpy(join_lam(ll, lxu, lxl, lp, T, nx, nu)))
        if rnorm2 is not None:
            rnorm2.copy_(torch.from_numpy(rp2))
        if info is not None:
            cur = _n(info)
            info.copy_(torch.from_numpy(np.where(cur == 0, inf_acc, cur).astype(np.int32)))
        if status is not None:
            status.copy_(torch.from_numpy(np.isfinite(zz).all(axis=(1, 2)).astype(np.uint8)))
        if factor is not None and (flags & SAVE_FACTOR) and L is not None:
            factor.copy_(torch.from_numpy(self._pack_X(L)))


COMBOS = ("dx", "dp", "xp", "dxp")   # d dense cost, x state box, p general rows


def gen_args(pr, combo):
    """(Qd_or_C, q, xbnd, poly) of solve_lin_gen for one of COMBOS out of a gen_problem."""
    T, nx, nu = pr["dims"][1:]
    cost, q = (pr["C"], pr["qC"]) if "d" in combo else (pr["Qd"], pr["q"])
    xbnd = poly = None
    if "x" in combo:
        xbnd = (pr["xlo"], pr["xhi"], *((0, 0) if pr["xlo"].dim() == 1 else (T * nx, nx)))
    if "p" in combo:
        poly = (pr["G"], pr["h"], pr["m"], *poly_strides(pr["G"], pr["h"], T, pr["m"], nx + nu))
    return cost, q, xbnd, poly


def run_solve(be, pr, combo, z0=None, lam0=None, rho0=None, phi0=None, **kw):
    """One solve_lin_gen call on the tensors of a gen_problem (any backend): -> dict(z, lam, rho, phi, rn2, info, status)."""
    B, T, nx, nu = pr["dims"]
    cost, q, xbnd, poly = gen_args(pr, combo)
    z = (pr["z0"] if z0 is None else z0).clone()
    dev, dt = z.device, z.dtype
    M = lam_width(T, nx, nu, xbnd is not None, poly[2] if poly else 0)
    lam = torch.zeros(B, M, dtype=dt, device=dev) if lam0 is None else lam0.clone()
    rho = torch.ones(B, dtype=dt, device=dev) if rho0 is None else rho0.clone()
    phi = torch.zeros(B, dtype=dt, device=dev) if phi0 is None else phi0.clone()
    rn2 = torch.zeros(B, dtype=dt, device=dev)
    info = torch.zeros(B, dtype=torch.int32, device=dev)
    status = torch.ones(B, dtype=torch.uint8, device=dev)
    sb, st = (0, 0) if pr["lo"].dim() == 1 else (T * nu, nu)
    ok = be.solve_lin_gen((B, T, nx, nu), cost, q, pr["F"], pr["c"], pr["x0"], pr["lo"], pr["hi"], sb, st, xbnd, poly, z, lam,
                          rho, phi, rnorm2=rn2, info=info, status=status, **kw)
    return dict(z=z, lam=lam, rho=rho, phi=phi, rn2=rn2, info=info, status=status, ok=ok)


def gen_problem(B, T, nx, nu, m, dtype, layout="per_instance", box="shared", seed=5, margin=0.05, u_cost=0.1, **kw):
    """poly_problem (rows feasible by construction at the rollout z_feas under u = 0) plus
      - a state box that CONTAINS z_feas: `box` "shared": xlo / xhi [nx], the rollout's extremes over batch and stages
        moved out by `margin`; "per_stage": [B,T,nx], z_feas -+ (margin + 0.3 |N(0,1)|), so every instance stays
        feasible and the box cuts the reference trajectory (N(0,1) draws) off at many entries;
      - a dense cost C, qC = -C xref of synthetic_dense_cost on the same synthetic problem.
    Keys of poly_problem, plus xlo, xhi, C, qC."""
    from deq_mpc_corl_amd import synthetic_dense_cost, synthetic_problem
    pr = poly_problem(B, T, nx, nu, m, dtype, layout=layout, seed=seed, u_cost=u_cost, **kw)
    xf = pr["zfeas"].double()[..., :nx]
    if box == "shared":
        xhi, xlo = xf.amax((0, 1)) + margin, xf.amin((0, 1)) - margin
    else:
        g = torch.Generator().manual_seed(seed + 41)
        xhi = xf + margin + 0.3 * torch.randn(B, T, nx, generator=g, dtype=torch.float64).abs()
        xlo = xf - margin - 0.3 * torch.randn(B, T, nx, generator=g, dtype=torch.float64).abs()
    xlo, xhi = xlo.to(dtype).contiguous(), xhi.to(dtype).contiguous()
    assert (xf >= xlo.double()).all() and (xf <= xhi.double()).all(), "generator condition: the box contains z_feas"
    p = synthetic_problem(B, T, nx, nu, seed=seed, dtype=dtype, active=True)
    C, qC = synthetic_dense_cost(p, seed=seed)
    return dict(pr, xlo=xlo, xhi=xhi, C=C, qC=qC)


def to_device(pr, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in pr.items()}
