"""TEST-ONLY reference for the stage-wise linear rows G_t z_t <= h_t, z_t = [x_t; u_t] (MPC(ineqG=, ineqh=),
alqp_solve_lin_poly): OracleBackend plus `solve_lin_poly`, built from the oracle's own building blocks the way
XboxOracleBackend (tests/state_bounds_reference.py) is. The oracle sees the plain problem and the plain part of lam; the
rows are added around it by ONE function, `poly_rows`, which states every term a row r_k = G_k z_t - h_k contributes
(conventions of the control rows, tests/state_bounds_reference.py:box_rows):

    gradient     g_t   += G_k' (lam_k + rho max(r_k, 0))
    Hessian      H_tt  += rho [r_k >= 0] G_k' G_k                  (dense: all of the stage's diagonal block)
    merit        phi   += lam_k r_k + rho/2 max(r_k, 0)^2          (per line-search candidate)
    |r+|^2             += max(r_k, 0)^2
    dual update  lam_k <- max(0, lam_k + rho r_k)

Newton direction and line-search decision are the oracle's. The reference the oracle is pinned to cannot run this case
(AL_mpc.dyn_res_ineq is never called), so the pins are tests/test_poly_rows_cpu.py's.

Multiplier layout: [B, T nx + T (2 nu + m)], the T nx equality rows, then per stage [u - uhi | -u + ulo | G_t z_t - h_t]."""
import numpy as np
import torch

from oracle import oracle_py as orc
from tests.oracle_backend import DUAL_UPDATE, INIT_MERIT, SAVE_FACTOR, OracleBackend, _bounds, _n, _sfx


def poly_rows(z, G, h, lam, rho):
    """Every term of the rows r = G z - h: z [B,T,n], G broadcastable to [B,T,m,n], h to [B,T,m], lam [B,T,m], rho [B],
    in z's dtype: -> g [B,T,n], H [B,T,n,n] (dense per stage), phi [B], rp2 [B], lam after the dual update [B,T,m]."""
    dt = z.dtype.type
    B, T, n = z.shape
    G = np.asarray(G, z.dtype)
    m = G.shape[-2]
    G = np.broadcast_to(G, (B, T, m, n))
    h = np.broadcast_to(np.asarray(h, z.dtype), (B, T, m))
    rb = np.reshape(rho, (-1, 1, 1)).astype(z.dtype)
    r = (np.einsum("btkj,btj->btk", G, z) - h).astype(z.dtype)
    p = np.maximum(r, dt(0))
    g = np.einsum("btkj,btk->btj", G, lam + rb * p)
    H = np.einsum("btk,btki,btkj->btij", rb * (r >= 0).astype(z.dtype), G, G)
    rp2 = (p * p).reshape(B, -1).sum(1)
    phi = (lam * r).reshape(B, -1).sum(1) + dt(0.5) * np.reshape(rho, (-1,)).astype(z.dtype) * rp2
    new = np.maximum(lam + rb * r, dt(0))
    return g.astype(z.dtype), H.astype(z.dtype), phi.astype(z.dtype), rp2.astype(z.dtype), new.astype(z.dtype)


def lam_width(T, nx, nu, m):
    return T * nx + T * (2 * nu + m)


def split_lam(lam, T, nx, nu, m):
    """lam [B, T nx + T (2 nu + m)] -> (plain lam [B, T nx + 2 T nu], row multipliers [B,T,m]) (copies)."""
    B = lam.shape[0]
    neq = T * nx
    li = lam[:, neq:].reshape(B, T, 2 * nu + m)
    plain = np.concatenate([lam[:, :neq], li[..., :2 * nu].reshape(B, -1)], 1)
    return np.ascontiguousarray(plain), li[..., 2 * nu:].copy()


def join_lam(plain, lp, T, nx, nu):
    B = plain.shape[0]
    neq = T * nx
    li = np.concatenate([plain[:, neq:].reshape(B, T, 2 * nu), lp], 2)
    return np.ascontiguousarray(np.concatenate([plain[:, :neq], li.reshape(B, -1)], 1))


def strides(G, h, T, m, n):
    """(sb_g, st_g, sb_h, st_h) of alqp_solve_lin_poly for G [m,n] / [T,m,n] / [B,T,m,n] and h [m] / [T,m] / [B,T,m]."""
    sg = {2: (0, 0), 3: (0, m * n), 4: (T * m * n, m * n)}[G.dim()]
    sh = {1: (0, 0), 2: (0, m), 3: (T * m, m)}[h.dim()]
    return (*sg, *sh)


def _rows(G, h, sb_g, st_g, sb_h, st_h, B, T, m, n):
    """G, h as poly_rows takes them, from flat data and strides."""
    Gn, hn = _n(G).reshape(-1), _n(h).reshape(-1)
    ib, it = np.arange(B)[:, None], np.arange(T)[None, :]
    og = (ib * sb_g + it * st_g)[..., None] + np.arange(m * n)
    oh = (ib * sb_h + it * st_h)[..., None] + np.arange(m)
    return Gn[og].reshape(B, T, m, n), hn[oh].reshape(B, T, m)


def merit_poly(s, zz, xn, x0, ll, lp, rr, Qd, q, lo, hi, G, h):
    """(phi, rp2) with the rows: the oracle's on the plain problem plus poly_rows'."""
    ph, rp2 = orc.merit(s, zz, xn, x0, ll, rr, Qd, q, lo, hi)
    _, _, pp, rx, _ = poly_rows(zz, G, h, lp, rr)
    return (ph + pp).astype(zz.dtype), (rp2 + rx).astype(zz.dtype)


def grad_hess_poly(s, zz, xn, F, x0, ll, lp, rr, Qd, q, lo, hi, G, h):
    g, Hd, Hs = orc.grad_hess(s, zz, xn, F, x0, ll, rr, Qd, q, lo, hi)
    gp, Hp, _, _, _ = poly_rows(zz, G, h, lp, rr)
    return (g + gp).astype(zz.dtype), (Hd + Hp).astype(zz.dtype), Hs


class PolyOracleBackend(OracleBackend):
    """`calls` records the solve entry points MPC reached. `trace` (a dict, optional argument of solve_lin_poly) gets one
    entry per Newton step under g, d, phi [n_ls,B], phi_prev, k, accept, z (the iterate the step started from), and
    Hd / Hs of the last step."""

    name = "oracle-test-poly"

    def __init__(self):
        self.calls = []

    def solve_lin(self, *a, **kw):
        self.calls.append("solve_lin")
        return super().solve_lin(*a, **kw)

    def solve_lin_poly(self, dims, Qd, q, F, c, x0, ulo, uhi, sb_u, st_u, G, h, m, sb_g, st_g, sb_h, st_h, z, lam, rho, phi,
                       rnorm2=None, info=None, status=None, factor=None, al_iter=2, max_newton=4, n_ls=20, flags=3,
                       rho_scale=10.0, trace=None, variant=None, skip=None):
        self.calls.append("solve_lin_poly")
        if skip is not None and float(skip[0]) != 0.0:
            return
        B, T, nx, nu = dims
        assert tuple(lam.shape) == (B, lam_width(T, nx, nu, m)), tuple(lam.shape)
        s = _sfx(z)
        npdt = np.float64 if s == "f64" else np.float32
        lo, hi = _bounds(ulo, uhi, sb_u, st_u, B, T, nu)
        Gr, hr = _rows(G, h, sb_g, st_g, sb_h, st_h, B, T, m, nx + nu)
        assert np.isfinite(hr).all() and np.isfinite(Gr).all(), "the host hands the solve finite rows"
        Qd_, q_, F_, c_, x0_ = _n(Qd), _n(q), _n(F), _n(c), _n(x0)
        zz, rr, ph = _n(z).copy(), _n(rho).copy(), _n(phi).copy()
        ll, lp = split_lam(_n(lam), T, nx, nu, m)

        def xnext(v):
            return (np.einsum("btij,btj->bti", F_, v[:, :-1]) + c_).astype(npdt)

        def merit(v):
            return merit_poly(s, v, xnext(v), x0_, ll, lp, rr, Qd_, q_, lo, hi, Gr, hr)

        L = None
        inf_acc = np.zeros(B, np.int32)
        for _ in range(al_iter):
            if flags & INIT_MERIT:
                ph, _ = merit(zz)
            for _ in range(max_newton):
                g, Hd, Hs = grad_hess_poly(s, zz, xnext(zz), F_, x0_, ll, lp, rr, Qd_, q_, lo, hi, Gr, hr)
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
                _, _, _, _, lp = poly_rows(zz, Gr, hr, lp, rr)   # (with the rho of this iteration)
                ll, rr = orc.dual_update(s, zz, xnext(zz), x0_, lo, hi, ll, rr)
                if rho_scale != 10.0:
                    rr = rr / 10.0 * rho_scale
        _, rp2 = merit(zz)
        z.copy_(torch.from_numpy(zz)); rho.copy_(torch.from_numpy(rr)); phi.copy_(torch.from_numpy(ph))
        lam.copy_(torch.from_numpy(join_lam(ll, lp, T, nx, nu)))
        if rnorm2 is not None:
            rnorm2.copy_(torch.from_numpy(rp2))
        if info is not None:
            cur = _n(info)
            info.copy_(torch.from_numpy(np.where(cur == 0, inf_acc, cur).astype(np.int32)))
        if status is not None:
            status.copy_(torch.from_numpy(np.isfinite(zz).all(axis=(1, 2)).astype(np.uint8)))
        if factor is not None and (flags & SAVE_FACTOR) and L is not None:
            factor.copy_(torch.from_numpy(self._pack_X(L)))


def run_solve(be, Qd, q, F, c, x0, lo, hi, G, h, z0, lam0=None, rho0=None, phi0=None, **kw):
    """One solve_lin_poly call on tensors of any backend: -> dict(z, lam, rho, phi, rn2, info, status) (copies)."""
    B, T, n = z0.shape
    nx = x0.shape[1]
    nu = n - nx
    m = G.shape[-2]
    dev, dt = z0.device, z0.dtype
    z = z0.clone()
    lam = torch.zeros(B, lam_width(T, nx, nu, m), dtype=dt, device=dev) if lam0 is None else lam0.clone()
    rho = torch.ones(B, dtype=dt, device=dev) if rho0 is None else rho0.clone()
    phi = torch.zeros(B, dtype=dt, device=dev) if phi0 is None else phi0.clone()
    rn2 = torch.zeros(B, dtype=dt, device=dev)
    info = torch.zeros(B, dtype=torch.int32, device=dev)
    status = torch.ones(B, dtype=torch.uint8, device=dev)
    sb, st = (0, 0) if lo.dim() == 1 else (T * nu, nu)
    ok = be.solve_lin_poly((B, T, nx, nu), Qd, q, F, c, x0, lo, hi, sb, st, G, h, m, *strides(G, h, T, m, n), z, lam, rho, phi,
                           rnorm2=rn2, info=info, status=status, **kw)
    return dict(z=z, lam=lam, rho=rho, phi=phi, rn2=rn2, info=info, status=status, ok=ok)


LAYOUTS = ("shared", "per_stage", "per_instance")


def poly_problem(B, T, nx, nu, m, dtype, layout="per_instance", seed=5, mixed=True, on_boundary=False, slack=(0.05, 0.4), toward=None, state_scale=1.0, u_cost=None):
    """CPU tensors of the active-bound synthetic problem plus m rows per stage that are FEASIBLE BY CONSTRUCTION: with
    z_feas the rollout from x0 under u = 0 (inside the control bounds), h_k >= G_k z_feas,t + s_k with s_k > 0 drawn from
    `slack`. G is dense N(0,1)/sqrt(n): every row couples states and controls. `layout`: G [m,n] and h [m] ("shared"),
    [T,m,n] and [T,m] ("per_stage") or [B,T,m,n] and [B,T,m] ("per_instance"); an h shared by several (b, t) is the
    largest G_k z_feas + s_k among them, so every instance stays feasible.
    `on_boundary` (not with "shared"): the last row of stage 1 becomes the unit row e_i (i = nx, the first control) and
    h = z0[., 1, i] > 0, so the row sits exactly on its boundary at the starting iterate z0.
    `mixed`: in every instance at least one row is violated and one slack at z0 (the last stage of z0 is moved along its
    first row where needed; asserted).
    `state_scale` multiplies the state columns of G: an h shared by several (b, t) binds only where G_k z_feas comes near
    its largest value, and the states of z_feas (N(0,1) draws rolled out) spread that value; with the state columns
    scaled down the controls, which the solve can move, decide.
    `u_cost`: the cost on the controls (q follows, -Qd xref) in place of the synthetic problem's 1e-8. With 1e-8 a control
    that sits inside its bounds under inactive rows leaves an eigenvalue of 1e-8 in H_tt, and the Newton direction then
    carries the last bits of g times 1e8: two correct solvers differ in d by 1e-8 and more.
    `toward` [B,T,n] (per-instance layout): every row is signed so that it points from z_feas to that iterate,
    G_k (toward_t - z_feas,t) >= 0 - with a small slack the row then cuts `toward` off, and a solve whose rowless
    minimiser it is ends with the row active."""
    from deq_mpc_corl_amd import synthetic_problem
    p = synthetic_problem(B, T, nx, nu, seed=seed, dtype=dtype, active=True)
    n = nx + nu
    f64 = torch.float64
    if u_cost is not None:
        Qd = p.Qd.clone()
        Qd[..., nx:] = u_cost
        p = p._replace(Qd=Qd, q=-(Qd * p.xref))
    gen = torch.Generator().manual_seed(seed + 23)
    zf = torch.zeros(B, T, n, dtype=f64)
    zf[:, 0, :nx] = p.x0.double()
    for t in range(T - 1):
        zf[:, t + 1, :nx] = torch.einsum("bij,bj->bi", p.F[:, t].double(), zf[:, t]) + p.c[:, t].double()
    assert (p.u_lo.double() < 0).all() and (p.u_hi.double() > 0).all()   # u = 0 is inside the control bounds
    shape = {"shared": (m, n), "per_stage": (T, m, n), "per_instance": (B, T, m, n)}[layout]
    G = torch.randn(*shape, generator=gen, dtype=f64) / n ** 0.5
    G[..., :nx] *= state_scale
    if toward is not None:
        assert layout == "per_instance"
        G = G * torch.sign(torch.einsum("btkj,btj->btk", G, toward.double() - zf)).unsqueeze(-1)
    z0 = p.z0.clone()
    if on_boundary:
        assert layout != "shared" and T > 2
        G[..., 1, m - 1, :] = 0
        G[..., 1, m - 1, nx] = 1
        z0[:, 1, nx] = z0[:, 1, nx].abs() + 0.05 if layout == "per_instance" else z0[0, 1, nx].abs() + 0.05
    s = slack[0] + (slack[1] - slack[0]) * torch.rand(B, T, m, generator=gen, dtype=f64)
    h = torch.einsum("btkj,btj->btk", G.expand(B, T, m, n), zf) + s
    h = {"shared": lambda: h.amax((0, 1)), "per_stage": lambda: h.amax(0), "per_instance": lambda: h}[layout]()
    G, h = G.to(dtype).contiguous(), h.to(dtype).contiguous()
    if on_boundary:
        h[..., 1, m - 1] = z0[:, 1, nx] if layout == "per_instance" else z0[0, 1, nx]   # G_k z0 - h_k is exactly 0
    Ge, he = G.double().expand(B, T, m, n), h.double().expand(B, T, m)
    assert (torch.einsum("btkj,btj->btk", Ge, zf) <= he).all(), "generator condition: z_feas satisfies every row"
    if mixed:
        r = torch.einsum("btkj,btj->btk", Ge, z0.double()) - he
        for b in range(B):
            if not (r[b] > 1e-3).any():
                g = Ge[b, T - 1, 0]
                z0[b, T - 1] += ((0.1 - r[b, T - 1, 0]) / (g @ g) * g).to(dtype)
        r = torch.einsum("btkj,btj->btk", Ge, z0.double()) - he
        assert all((r[b] > 1e-3).any() and (r[b] < -1e-3).any() for b in range(B)), "generator condition: mixed rows"
    return dict(Qd=p.Qd, q=p.q, F=p.F, c=p.c, x0=p.x0, lo=p.u_lo, hi=p.u_hi, G=G, h=h, z0=z0, zfeas=zf.to(dtype), m=m,
                dims=(B, T, nx, nu))


def poly_residuals(pr, z):
    """Row residuals G z - h [B,T,m], numpy in z's dtype."""
    B, T, nx, nu = pr["dims"]
    zz = _n(z)
    G = np.broadcast_to(_n(pr["G"]), (B, T, pr["m"], nx + nu))
    h = np.broadcast_to(_n(pr["h"]), (B, T, pr["m"]))
    return (np.einsum("btkj,btj->btk", G, zz) - h).astype(zz.dtype)


def box_as_rows(xlo, xhi, nx, nu):
    """The state box xlo <= x <= xhi ([nx] or [B,T,nx]) as rows G = [I 0; -I 0], h = [xhi; -xlo] (m = 2 nx), and the
    permutation-free correspondence: row k < nx is the upper row of state k, row nx + k its lower row - the order of the
    state-bound layout [x - xhi | -x + xlo]."""
    dt = xlo.dtype
    G = torch.zeros(2 * nx, nx + nu, dtype=dt)
    G[:nx, :nx] = torch.eye(nx, dtype=dt)
    G[nx:, :nx] = -torch.eye(nx, dtype=dt)
    h = torch.cat((xhi, -xlo), -1).contiguous()
    return G, h
