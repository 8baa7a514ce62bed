"""TEST-ONLY reference for the general rows on the callable-dynamics route (MPC(ineqG=, ineqh=) with a callable dx, with
or without x_lower / x_upper; alqp_newton_step_rows, alqp_merit_rows, alqp_merit_pick_rows, alqp_dual_update_rows):
XboxStepOracleBackend and GenOracleBackend plus the four `_rows` methods, composed the way the `_xbox` methods are. The
oracle sees the plain problem and the plain part of lam; the state rows' terms come from state_bounds_reference.box_rows
(through the `_xbox` methods when there are state bounds), the general rows' from poly_rows_reference.poly_rows, and the
only arithmetic here is the sum.

Multiplier layout: gen_rows_reference's, [B, T nx + T (2 nu + [2 nx] + m)].

Also here: the problems the CPU and GPU tests of the route share (plants: state_bounds_step_reference's)."""
import numpy as np
import torch

from oracle import oracle_py as orc
from tests import state_bounds_reference as sbr
from tests import state_bounds_step_reference as ssr
from tests.gen_rows_reference import GenOracleBackend, join_lam, lam_width, split_lam
from tests.oracle_backend import OracleBackend, _bounds, _n, _sfx
from tests.poly_rows_reference import _rows, poly_rows
from tests.poly_rows_reference import strides as poly_strides
from tests.state_bounds_step_reference import XboxStepOracleBackend, linearize, true_next

KINK_MARGIN = 1e-4


def _t(a, like):
    return torch.from_numpy(np.ascontiguousarray(a)).to(like.dtype)


class RowsStepOracleBackend(XboxStepOracleBackend, GenOracleBackend):
    name = "oracle-test-rows-step"

    @staticmethod
    def _split_rows(dims, lam, xbnd, poly):
        """-> plain lam (numpy), lam_xu, lam_xl ([B,T,nx] or None), lam_p [B,T,m], (xl, xh) or None, (Gr, hr)."""
        B, T, nx, nu = dims
        G, h, m, sb_g, st_g, sb_h, st_h = poly
        xbox = xbnd is not None
        assert tuple(lam.shape) == (B, lam_width(T, nx, nu, xbox, m)), tuple(lam.shape)
        plain, lxu, lxl, lp = split_lam(_n(lam), T, nx, nu, xbox, m)
        xb = None
        if xbox:
            xb = sbr._xbounds(*xbnd, B, T, nx)
            assert np.isfinite(xb[0]).all() and np.isfinite(xb[1]).all(), "the host hands the kernels finite bounds"
        rows = _rows(G, h, sb_g, st_g, sb_h, st_h, B, T, m, nx + nu)
        assert np.isfinite(rows[0]).all() and np.isfinite(rows[1]).all(), "the host hands the kernels finite rows"
        return plain, lxu, lxl, lp, xb, rows

    def newton_step_rows(self, dims, z, xnext, F, x0, lam, rho, Qd, q, ulo, uhi, sb_u, st_u, xbnd, poly, d_out, g_out=None,
                         factor=None, info=None):
        self.calls.append("newton_step_rows")
        B, T, nx, nu = dims
        s = _sfx(z)
        lo, hi = _bounds(ulo, uhi, sb_u, st_u, B, T, nu)
        plain, lxu, lxl, lp, xb, rows = self._split_rows(dims, lam, xbnd, poly)
        zz = _n(z)
        if xb is not None:
            g, Hd, Hs = sbr.grad_hess_xbox(s, zz, _n(xnext), _n(F), _n(x0), plain, lxu, lxl, _n(rho), _n(Qd), _n(q), lo, hi, *xb)
        else:
            g, Hd, Hs = orc.grad_hess(s, zz, _n(xnext), _n(F), _n(x0), plain, _n(rho), _n(Qd), _n(q), lo, hi)
        gp, Hp, _, _, _ = poly_rows(zz, *rows, lp, _n(rho))
        g, Hd = (g + gp).astype(zz.dtype), (Hd + Hp).astype(zz.dtype)
        d, inf, L, _ = orc.newton_dir(s, g, Hd, Hs, nx, want_factor=True)
        self.last_hessian = (Hd, Hs)
        d_out.copy_(torch.from_numpy(d))
        if g_out is not None:
            g_out.copy_(torch.from_numpy(g))
        if factor is not None:
            factor.copy_(torch.from_numpy(self._pack_X(L)))
        if info is not None:
            cur = _n(info)
            info.copy_(torch.from_numpy(np.where(cur == 0, inf, cur).astype(np.int32)))

    def merit_rows(self, dims, K, zc, xnext, x0, lam, rho, Qd, q, ulo, uhi, sb_u, st_u, xbnd, poly, phi, rnorm2=None):
        self.calls.append("merit_rows")
        B, T, nx, nu = dims
        plain, lxu, lxl, lp, xb, rows = self._split_rows(dims, lam, xbnd, poly)
        r2 = torch.empty(K, B, dtype=zc.dtype)
        if xbnd is not None:
            lam_x = _t(sbr.join_lam(plain, lxu, lxl, T, nx, nu), lam)
            self.merit_xbox(dims, K, zc, xnext, x0, lam_x, rho, Qd, q, ulo, uhi, sb_u, st_u, xbnd, phi, r2)
            self.calls.pop()
        else:
            OracleBackend.merit(self, dims, K, zc, xnext, x0, torch.from_numpy(plain), rho, Qd, q, ulo, uhi, sb_u, st_u, phi, r2)
        zc_ = _n(zc).reshape(K, B, T, nx + nu)
        for k in range(K):
            _, _, pp, rx, _ = poly_rows(zc_[k], *rows, lp, _n(rho))
            phi.view(K, B)[k].add_(_t(pp, phi))
            r2[k].add_(_t(rx, r2))
        if rnorm2 is not None:
            rnorm2.view(K, B).copy_(r2)

    def merit_pick_rows(self, dims, n_ls, d, xnext_all, x0, lam, rho, Qd, q, ulo, uhi, sb_u, st_u, xbnd, poly, z, phi_prev,
                        rnorm2=None, phi_all=None, k_out=None, accept_out=None):
        """OracleBackend.merit_pick with merit_rows in place of merit."""
        self.calls.append("merit_pick_rows")
        B, T, nx, nu = dims
        alphas = (2.0 ** -torch.arange(n_ls, dtype=z.dtype)).view(n_ls, 1, 1, 1)
        zc = (z.unsqueeze(0) + alphas * d.unsqueeze(0)).contiguous()
        phis = torch.empty(n_ls, B, dtype=z.dtype)
        rn2s = torch.empty(n_ls, B, dtype=z.dtype)
        self.merit_rows(dims, n_ls, zc, xnext_all, x0, lam, rho, Qd, q, ulo, uhi, sb_u, st_u, xbnd, poly, phis, rn2s)
        self.calls.pop()
        kk = torch.zeros(B, dtype=torch.int32)
        acc = torch.zeros(B, dtype=torch.int32)
        self.linesearch_pick(dims, n_ls, phis, phi_prev, d, z, kk, acc)
        if rnorm2 is not None:
            rnorm2.copy_(torch.where(acc.bool(), rn2s.gather(0, kk.long().unsqueeze(0)).squeeze(0), rnorm2))
        if phi_all is not None:
            phi_all.copy_(phis)
        if k_out is not None:
            k_out.copy_(kk)
        if accept_out is not None:
            accept_out.copy_(acc)

    def dual_update_rows(self, dims, z, xnext, x0, ulo, uhi, sb_u, st_u, xbnd, poly, lam, rho, rho_scale=10.0):
        self.calls.append("dual_update_rows")
        B, T, nx, nu = dims
        plain, lxu, lxl, lp, xb, rows = self._split_rows(dims, lam, xbnd, poly)
        zz = _n(z)
        if xb is not None:   # (all with the rho before its growth)
            _, _, _, _, (lxu, lxl) = sbr.box_rows(zz[..., :nx], *xb, lxu, lxl, _n(rho))
        _, _, _, _, lp = poly_rows(zz, *rows, lp, _n(rho))
        pt = torch.from_numpy(plain)
        OracleBackend.dual_update(self, dims, z, xnext, x0, ulo, uhi, sb_u, st_u, pt, rho, rho_scale)
        lam.copy_(_t(join_lam(_n(pt), lxu, lxl, lp, T, nx, nu), lam))


# ---- shared problems ---------------------------------------------------------------------------------------------------
LAYOUTS = ("shared", "per_stage", "per_instance")


def rows_problem(B, T, nx, nu, m, layout, dtype, seed=5):
    """state_bounds_step_reference.step_problem (state bounds that bind on both sides in every instance, the SinPlant of
    the size) plus m rows per stage placed around the START iterate z0: G dense N(0,1)/sqrt(n) in `layout` ([m,n],
    [T,m,n] or [B,T,m,n]; h likewise), h_k = G_k z0 - s_k with s_k in [0.2, 0.4] for even k (the row is violated at z0 in
    every (b, t) it serves: the smallest G_k z0 among them) and s_k in [-0.6, -0.3] for odd k (slack at z0: the largest).
    Whether the state bounds are used is the caller's choice (`args`). The cost on the controls is 0.1. -> (pr, plant)."""
    pr, plant = ssr.step_problem(B, T, nx, nu, dtype, per_stage=(layout == "per_instance"), seed=seed)
    n = nx + nu
    # the control cost 0.1 in place of the synthetic problem's 1e-8 (q = -Qd xref follows), for the reason poly_problem
    # gives: a control inside its bounds under inactive rows would leave an eigenvalue of 1e-8 in H_tt
    Qd, q = pr["Qd"].clone(), pr["q"].clone()
    q[..., nx:] *= 0.1 / Qd[..., nx:]
    Qd[..., nx:] = 0.1
    pr = dict(pr, Qd=Qd, q=q)
    gen = torch.Generator().manual_seed(seed + 77)
    shape = {"shared": (m, n), "per_stage": (T, m, n), "per_instance": (B, T, m, n)}[layout]
    G = (torch.randn(*shape, generator=gen, dtype=torch.float64) / n ** 0.5)
    gz = torch.einsum("btkj,btj->btk", G.expand(B, T, m, n), pr["z0"].double())
    u = torch.rand(m, generator=gen, dtype=torch.float64)
    even = (torch.arange(m) % 2 == 0)
    s = torch.where(even, 0.2 + 0.2 * u, -0.3 - 0.3 * u)
    red = {"shared": (0, 1), "per_stage": (0,), "per_instance": ()}[layout]
    lo_, hi_ = (gz.amin(red), gz.amax(red)) if red else (gz, gz)
    h = torch.where(even, lo_, hi_) - s
    pr = dict(pr, G=G.to(dtype).contiguous(), h=h.to(dtype).contiguous(), m=m)
    return pr, plant


def args(pr, xbox):
    """(sb_u, st_u, xbnd or None, poly) of the four methods."""
    B, T, nx, nu = pr["dims"]
    sb_u, st_u, sb_x, st_x = ssr.strides(pr)
    xbnd = (pr["xlo"], pr["xhi"], sb_x, st_x) if xbox else None
    poly = (pr["G"], pr["h"], pr["m"], *poly_strides(pr["G"], pr["h"], T, pr["m"], nx + nu))
    return sb_u, st_u, xbnd, poly


def al_iteration(be, pr, plant, xbox, z, lam, rho, n_newton=4, n_ls=20, dual=True):
    """One AL iteration of the PyTorch-dynamics route through `be`'s four _rows methods, in place on z, lam, rho."""
    dims = pr["dims"]
    B, T, nx, nu = dims
    sb_u, st_u, xb, poly = args(pr, xbox)
    prob = (pr["x0"], lam, rho, pr["Qd"], pr["q"], pr["lo"], pr["hi"], sb_u, st_u)
    phi = torch.zeros(B, dtype=z.dtype, device=z.device)
    rn2 = torch.zeros(B, dtype=z.dtype, device=z.device)
    d = torch.empty_like(z)
    be.merit_rows(dims, 1, z, true_next(plant, z, nx), *prob, xb, poly, phi, rn2)
    alphas = (2.0 ** -torch.arange(n_ls, dtype=z.dtype, device=z.device)).view(n_ls, 1, 1, 1)
    for _ in range(n_newton):
        xn, F = linearize(plant, z, nx)
        be.newton_step_rows(dims, z, xn, F, *prob, xb, poly, d)
        zc = (z.unsqueeze(0) + alphas * d.unsqueeze(0)).contiguous()
        be.merit_pick_rows(dims, n_ls, d, true_next(plant, zc, nx), *prob, xb, poly, z, phi, rnorm2=rn2)
    if dual:
        be.dual_update_rows(dims, z, true_next(plant, z, nx), pr["x0"], pr["lo"], pr["hi"], sb_u, st_u, xb, poly, lam, rho)
    return phi, rn2


def kernel_inputs(pr, plant, xbox):
    """lam, rho after ONE reference AL iteration from the problem's start, with the iterate it left: what the GPU tests
    feed every kernel. -> dict(z, lam, rho, xn, F, d, g, hessian)."""
    B, T, nx, nu = pr["dims"]
    be = RowsStepOracleBackend()
    z = pr["z0"].clone()
    lam = torch.zeros(B, lam_width(T, nx, nu, xbox, pr["m"]), dtype=z.dtype)
    rho = torch.ones(B, dtype=z.dtype)
    al_iteration(be, pr, plant, xbox, z, lam, rho)
    xn, F = linearize(plant, z, nx)
    sb_u, st_u, xb, poly = args(pr, xbox)
    d, g = torch.empty_like(z), torch.empty_like(z)
    be.newton_step_rows(pr["dims"], z, xn, F, pr["x0"], lam, rho, pr["Qd"], pr["q"], pr["lo"], pr["hi"], sb_u, st_u, xb, poly,
                        d, g_out=g)
    return dict(z=z, lam=lam, rho=rho, xn=xn, F=F, d=d, g=g, hessian=be.last_hessian)


def residuals(pr, z, xbox):
    """Every inequality residual at z in float64: dict(u [B,T,2nu], x [B,T,2nx] or None, p [B,T,m])."""
    B, T, nx, nu = pr["dims"]
    f = lambda t: t.detach().cpu().double().numpy()
    zz = f(z)
    bc = lambda v, w: np.broadcast_to(f(v), (B, T, w))
    u, x = zz[..., nx:], zz[..., :nx]
    out = dict(u=np.concatenate([u - bc(pr["hi"], nu), -u + bc(pr["lo"], nu)], -1), x=None)
    if xbox:
        out["x"] = np.concatenate([x - bc(pr["xhi"], nx), -x + bc(pr["xlo"], nx)], -1)
    G = np.broadcast_to(f(pr["G"]), (B, T, pr["m"], nx + nu))
    out["p"] = np.einsum("btkj,btj->btk", G, zz) - np.broadcast_to(f(pr["h"]), (B, T, pr["m"]))
    return out


# ---- the GPU tests' cases (tests/test_gpu_rows_step.py; their preconditions are asserted on the CPU too) -----------------
# (nx, nu, T, B, m, layout): the smallest team with one shared row; pad4(m) != m and NROWS 15 of 16 lanes; pad4(N) == N
# and pad4(m) == m; (12,4); (13,4); (14,4); T m > 64 at the workload's horizon; the cap m = 64.
GPU_CASES = [(2, 1, 2, 5, 1, "shared"), (4, 1, 3, 3, 5, "per_stage"), (6, 2, 3, 2, 4, "per_instance"),
             (12, 4, 3, 2, 3, "per_instance"), (13, 4, 3, 2, 3, "per_stage"), (14, 4, 3, 2, 2, "shared"),
             (13, 4, 20, 2, 7, "per_instance"), (4, 1, 3, 3, 64, "per_stage")]
GPU_SEED = 5


def gpu_case(nx, nu, T, B, m, layout, xbox, dtype):
    """-> (pr, plant, inp): the problem, its plant and kernel_inputs of the case, CPU tensors in `dtype`."""
    pr, plant = rows_problem(B, T, nx, nu, m, layout, dtype, seed=GPU_SEED)
    return pr, plant, kernel_inputs(pr, plant, xbox)


def gamma_rows(T, n, m):
    """Roundings the row loop of k_merit_rows / k_merit_pick_rows adds to the chains aux_cases.gamma_merit counts, relative
    to the magnitudes merit_magnitude_rows adds: r_k has n + 2 (n in the dot product, the difference with h_k, and in a
    candidate the sum r0 + alpha gd, alpha gd being exact; gd's own n are r0's in the magnitude |G| . (|z| + alpha |d|)),
    the square max(r_k, 0)^2 doubles them and adds its product, lam_k r_k adds one, and each trip of the loop one addition
    to the accumulator: 2 (n + 2) + 2 + ceil(T m / 64)."""
    return 2 * (n + 2) + 2 + -(-T * m // 64)


def gamma_merit_rows(T, nx, nu, m, cand=False):
    from tests import aux_cases as ax
    return ax.gamma_merit(T, nx, nu, 0, cand) + gamma_rows(T, nx + nu, m)


def gamma_rnorm2_rows(T, nx, nu, m, cand=False):
    from tests import aux_cases as ax
    return ax.gamma_rnorm2(T, nx, nu, 0, cand) + gamma_rows(T, nx + nu, m)


def merit_magnitude_rows(pr, z, xn, lam, rho, xbox, zmag=None):
    """aux_cases.merit_magnitude with the state rows' and the general rows' terms: -> (phi, A, rp2, A2) per instance in
    float64. A general row r_k = G_k . z_t - h_k counts |G_k| . |z_t| + |h_k| where a box row counts |a| + |b|, with
    n + 1 roundings in it (the dot product and the subtraction) that the caller's gamma has to cover."""
    from tests import aux_cases as ax
    B, T, nx, nu = pr["dims"]
    m = pr["m"]
    f = lambda t: t.detach().cpu().double().numpy() if torch.is_tensor(t) else np.asarray(t, np.float64)
    z, xn, lam, rho = f(z), f(xn), f(lam), f(rho).reshape(B)
    plain, lxu, lxl, lp = split_lam(lam, T, nx, nu, xbox, m)
    ulo, uhi = np.broadcast_to(f(pr["lo"]), (B, T, nu)), np.broadcast_to(f(pr["hi"]), (B, T, nu))
    mm = ax.merit_magnitude(z, xn, f(pr["x0"]), plain, rho, f(pr["Qd"]), f(pr["q"]), ulo, uhi, zmag=zmag)
    s = lambda a: a.reshape(B, -1).sum(1)
    phi, A, rp2, A2 = mm.phi, mm.A, mm.rp2, mm.A2
    zm = np.abs(z) if zmag is None else zmag
    if xbox:
        xlo, xhi = np.broadcast_to(f(pr["xlo"]), (B, T, nx)), np.broadcast_to(f(pr["xhi"]), (B, T, nx))
        x, xm = z[..., :nx], zm[..., :nx]
        ru, rl = x - xhi, -x + xlo
        um, lm = xm + np.abs(xhi), xm + np.abs(xlo)
        r2 = s(np.maximum(ru, 0) ** 2 + np.maximum(rl, 0) ** 2)
        a2 = s(um ** 2 + lm ** 2)
        phi = phi + s(lxu * ru + lxl * rl) + 0.5 * rho * r2
        A = A + s(np.abs(lxu) * um + np.abs(lxl) * lm) + 0.5 * np.abs(rho) * a2
        rp2, A2 = rp2 + r2, A2 + a2
    G = np.broadcast_to(f(pr["G"]), (B, T, m, nx + nu))
    h = np.broadcast_to(f(pr["h"]), (B, T, m))
    r = np.einsum("btkj,btj->btk", G, z) - h
    rm = np.einsum("btkj,btj->btk", np.abs(G), zm) + np.abs(h)
    r2, a2 = s(np.maximum(r, 0) ** 2), s(rm ** 2)
    phi = phi + s(lp * r) + 0.5 * rho * r2
    A = A + s(np.abs(lp) * rm) + 0.5 * np.abs(rho) * a2
    return phi, A, rp2 + r2, A2 + a2


def row_terms_numpy(pr, z, xn, lam, rho, xbox):
    """A direct float64 statement of every row term at (z, xnext, lam, rho), independent of the oracle, of box_rows and
    of poly_rows: -> dict(phi [B], rp2 [B], lam_new [B,M])."""
    B, T, nx, nu = pr["dims"]
    n, m = nx + nu, pr["m"]
    f = lambda t: t.detach().cpu().double().numpy()
    z, xn, lam, rho = f(z), f(xn), f(lam), f(rho).reshape(B)
    Qd, q, x0 = f(pr["Qd"]), f(pr["q"]), f(pr["x0"])
    bc = lambda v, w: np.broadcast_to(f(v), (B, T, w))
    ulo, uhi = bc(pr["lo"], nu), bc(pr["hi"], nu)
    xlo, xhi = bc(pr["xlo"], nx), bc(pr["xhi"], nx)
    G = np.broadcast_to(f(pr["G"]), (B, T, m, n))
    h = bc(pr["h"], m)
    xr = 2 * nx if xbox else 0
    neq, nit = T * nx, 2 * nu + xr + m
    phi, rp2, new = np.zeros(B), np.zeros(B), lam.copy()
    for b in range(B):
        phi[b] = (0.5 * Qd[b] * z[b] * z[b] + q[b] * z[b]).sum()
        for t in range(T):
            for i in range(nx):
                r = z[b, t + 1, i] - xn[b, t, i] if t < T - 1 else z[b, 0, i] - x0[b, i]
                phi[b] += lam[b, t * nx + i] * r
                rp2[b] += r * r
                new[b, t * nx + i] = lam[b, t * nx + i] + rho[b] * r
            rows = [(j, z[b, t, nx + j] - uhi[b, t, j]) for j in range(nu)]
            rows += [(nu + j, -z[b, t, nx + j] + ulo[b, t, j]) for j in range(nu)]
            if xbox:
                rows += [(2 * nu + i, z[b, t, i] - xhi[b, t, i]) for i in range(nx)]
                rows += [(2 * nu + nx + i, -z[b, t, i] + xlo[b, t, i]) for i in range(nx)]
            rows += [(2 * nu + xr + k, sum(G[b, t, k, j] * z[b, t, j] for j in range(n)) - h[b, t, k]) for k in range(m)]
            for k, r in rows:
                row = neq + t * nit + k
                phi[b] += lam[b, row] * r
                rp2[b] += max(r, 0.0) ** 2
                new[b, row] = max(0.0, lam[b, row] + rho[b] * r)
        phi[b] += 0.5 * rho[b] * rp2[b]
    return dict(phi=phi, rp2=rp2, lam_new=new)


# |dlam| of the route twin with the rows INERT, as tests/test_rows_step_cpu.py::test_route_twin measures and prints it
# (reference exit; rows alone / with state bounds): what the twin bound of the whole-solve comparisons is 8 times of
INERT_TWIN = {(2, 1, False): 1.95e-14, (2, 1, True): 1.24e-14, (13, 4, False): 4.26e-14, (13, 4, True): 8.44e-14}


# The whole solves through MPC that the GPU tests compare (tests/test_gpu_rows_step.py), per size: keywords of
# coupled_row_problem. At (2,1) SinPlant's own problem converges in two or three Newton steps per warm-started AL iteration,
# and the step after that moves the merit by less than its rounding error: the two best of the 20 candidates are exactly
# equal in the reference and the pick hangs on the last bit (no seed 3..79, horizon 3..20 or batch 1, 3, 5 is free of such a
# step). The same plant family with a heavier sine converges slowly enough that every line search of the solve stays
# decided, but a heavier sine also makes the solve more sensitive to rounding. Of gains 1 to 10 at step 0.3, seeds 3..20,
# the settings without a line search whose two best merits are closer than 1e-9 (relative), in the reference alone, are
# gain 8 / seeds 3 and 4 and gain 10 / seed 4; a one-ulp change of q moves lam by 2.5, 3.4 and 11.6 times the twin bound
# there. Taken: the least sensitive (smallest gap 2.2e-7 over both exit modes, with and without state bounds: asserted in
# tests/test_rows_step_cpu.py).
WHOLE_SOLVE_KW = {(2, 1): dict(seed=3, gain=8.0, h_plant=0.3), (13, 4): dict()}
WHOLE_SOLVE_MIN_GAP = 1e-9   # relative; the fp64 merit tolerance is of the order 1e-14


class CurvedSinPlant(ssr.SinPlant):
    """SinPlant with the sine's weight as a parameter: x+ = x + h (A x + B u + gain sin x); SinPlant has gain 0.3."""

    def __init__(self, nx, nu, seed=0, h=0.1, gain=0.3):
        super().__init__(nx, nu, seed=seed, h=h)
        self.gain = gain

    def __call__(self, x, u):
        A, B = self._ab(x)
        return x + self.h * (x @ A.T + u @ B.T + self.gain * torch.sin(x))

    def jac(self, x, u):
        A, B = self._ab(x)
        eye = torch.eye(self.nx, dtype=x.dtype, device=x.device)
        Jx = eye + self.h * (A + self.gain * torch.diag_embed(torch.cos(x)))
        Ju = (self.h * B).expand(x.shape[0], self.nx, self.nu)
        return self(x, u), (Jx, Ju)


def coupled_row_problem(B, T, nx, nu, xbox, mode="reference", seed=5, every_instance=True, gain=None, h_plant=0.1):
    """bounded_plant_problem with the cost pulling states 0 and 1 the same way, and ONE coupled row x_0 + x_1 <= h on every
    stage, h [B,T,1] a quarter of the way from the largest x_0 + x_1 of the plant's own rollout under u = 0 (which therefore
    satisfies the row: the problem is feasible) to that of the rowless solution (which violates it; solved here through
    the reference backends). With `xbox` the state box is |x| <= 0.8. -> (pr, plant, x of the rowless solution)."""
    from deq_mpc_corl_amd import MPC, QuadCost
    pr, plant = ssr.bounded_plant_problem(B, T, nx, nu, torch.float64, width=0.4, seed=seed)
    if gain is not None:   # a more curved plant of the same family, and its own rollout as the start
        plant = CurvedSinPlant(nx, nu, seed=seed, h=h_plant, gain=gain)
        z0 = torch.zeros_like(pr["z0"])
        z0[:, 0, :nx] = pr["x0"]
        for t in range(T - 1):
            z0[:, t + 1, :nx] = plant(z0[:, t, :nx], z0[:, t, nx:])
        pr["z0"] = z0
    pr["q"] = pr["q"].clone()
    pr["q"][..., 1] = pr["q"][..., 0]
    G = torch.zeros(1, nx + nu, dtype=torch.float64)
    G[0, 0] = G[0, 1] = 1.0
    pr["xlo"], pr["xhi"] = torch.full((nx,), -0.8, dtype=torch.float64), torch.full((nx,), 0.8, dtype=torch.float64)
    kwx = dict(x_lower=pr["xlo"], x_upper=pr["xhi"]) if xbox else {}
    free = MPC(nx, nu, T, u_lower=pr["lo"], u_upper=pr["hi"], n_batch=B, dtype=torch.float64, exit_mode=mode, al_iter=6,
               backend=XboxStepOracleBackend() if xbox else OracleBackend(), **kwx)
    free.reinitialize(pr["x0"], None)
    xf, _, _ = free(pr["x0"], QuadCost(torch.diag_embed(pr["Qd"]), pr["q"]), plant, plant.jac,
                    x_init=pr["z0"][..., :nx].clone(), u_init=pr["z0"][..., nx:].clone())
    s_roll = (pr["z0"][..., 0] + pr["z0"][..., 1]).max(1).values
    s_free = (xf[..., 0] + xf[..., 1]).double().max(1).values
    # the rowless solution goes where the rollout does not: in every instance of a small batch, in most of a large one
    far = s_free > s_roll + 0.2
    assert far.all() if every_instance else far.float().mean() > 0.9, (s_free, s_roll)
    h = (s_roll + 0.25 * (s_free - s_roll).clamp(min=0.2)).reshape(B, 1, 1).expand(B, T, 1).contiguous()
    return dict(pr, G=G, h=h, m=1), plant, xf


class TieBackend(RowsStepOracleBackend):
    """RowsStepOracleBackend that marks, per instance, every line search the float64 arithmetic does not decide: the two
    best of the candidates' merits closer than twice the merit's rounding bound (gamma_merit_rows x eps x the magnitude of
    merit_magnitude_rows, the near-tie rule of the kernel tests, in float64), or the best merit that close to phi_prev (the
    strict accept). Two correct solvers may part ways at such a step, by up to that step's |d|; at every other step they
    take the same candidate. `undecided` [B] (bool) collects the marks over a solve; `tied_step` [B] the largest |d| of an
    instance's marked steps."""

    def __init__(self):
        super().__init__()
        self.undecided = None
        self.tied_step = None

    def merit_pick_rows(self, dims, n_ls, d, xnext_all, x0, lam, rho, Qd, q, ulo, uhi, sb_u, st_u, xbnd, poly, z, phi_prev,
                        **kw):
        B, T, nx, nu = dims
        z0, prev = z.clone(), phi_prev.clone()
        pa = torch.empty(n_ls, B, dtype=z.dtype)
        super().merit_pick_rows(dims, n_ls, d, xnext_all, x0, lam, rho, Qd, q, ulo, uhi, sb_u, st_u, xbnd, poly, z, phi_prev,
                                **{**kw, "phi_all": pa})
        pr = dict(dims=dims, x0=x0, Qd=Qd, q=q, lo=ulo, hi=uhi, G=poly[0], h=poly[1], m=poly[2])
        if xbnd is not None:
            pr.update(xlo=xbnd[0], xhi=xbnd[1])
        al = (2.0 ** -np.arange(n_ls)).reshape(n_ls, 1, 1, 1)
        zc = z0.double().numpy()[None] + al * d.double().numpy()[None]
        zmag = np.abs(z0.double().numpy())[None] + al * np.abs(d.double().numpy())[None]
        A = np.stack([merit_magnitude_rows(pr, zc[k], xnext_all[k], lam, rho, xbnd is not None, zmag=zmag[k])[1]
                      for k in range(n_ls)])
        tol = gamma_merit_rows(T, nx, nu, poly[2], cand=True) * 2.0 ** -53 * A.max(0)
        srt = np.sort(pa.double().numpy(), 0)
        und = (srt[1] - srt[0] <= 2 * tol) if n_ls > 1 else np.zeros(B, bool)
        und |= np.abs(srt[0] - prev.double().numpy()) <= 2 * tol
        step = d.double().abs().reshape(B, -1).max(1).values.numpy()
        if self.undecided is None:
            self.undecided, self.tied_step = np.zeros(B, bool), np.zeros(B)
        self.undecided |= und
        self.tied_step = np.where(und, np.maximum(self.tied_step, step), self.tied_step)
