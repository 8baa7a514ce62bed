"""TEST-ONLY reference for the dense stage cost on the callable-dynamics route (MPC(diag_cost=False) with a callable dx,
alone or with x_lower / x_upper and / or ineqG / ineqh; alqp_newton_step_dense, alqp_merit_dense, alqp_merit_pick_dense):
RowsStepOracleBackend plus the three `_dense` methods, over DenseOracleBackend's split_cost / grad_hess_dense. The oracle sees diag(C) and the plain part of
lam; the state rows' and the general rows' terms come from RowsStepOracleBackend's own methods (box_rows, poly_rows), the
off-diagonal part of the cost is added around them the way tests/dense_cost_reference.py adds it:

    gradient   g_t   += offdiag(C_t) z_t
    Hessian    H_tt  += offdiag(C_t)
    merit      phi   += 1/2 sum_t z_t' offdiag(C_t) z_t          (per line-search candidate)

and the only arithmetic here is that sum. The dual update reads no cost: OracleBackend.dual_update, dual_update_xbox or
dual_update_rows, as the rows demand.

Multiplier layout: gen_rows_reference's, [B, T nx + T (2 nu + [2 nx] + [m])].

Also here: the problems the CPU and GPU tests of the route share (plants: state_bounds_step_reference's)."""
import numpy as np
import torch

from oracle import oracle_py as orc
from tests import aux_cases as ax
from tests import rows_step_reference as rsr
from tests import state_bounds_reference as sbr
from tests import state_bounds_step_reference as ssr
from tests.dense_cost_reference import DenseOracleBackend, split_cost
from tests.gen_rows_reference import join_lam, lam_width, split_lam
from tests.oracle_backend import OracleBackend, _bounds, _n, _sfx
from tests.poly_rows_reference import _rows, poly_rows
from tests.poly_rows_reference import strides as poly_strides
from tests.rows_step_reference import RowsStepOracleBackend
from tests.state_bounds_reference import box_rows
from tests.state_bounds_step_reference import linearize, true_next

KINK_MARGIN = 1e-4
COMBOS = [(False, False), (True, False), (False, True), (True, True)]   # (xbox, poly)
COMBO_IDS = ["dense", "dense+xbox", "dense+rows", "dense+xbox+rows"]


def _t(a, like):
    return torch.from_numpy(np.ascontiguousarray(a)).to(like.dtype)


class DenseStepOracleBackend(RowsStepOracleBackend):
    """(Not a DenseOracleBackend: that class's own `merit_dense`, a static helper of its fused solve, has the name the
    backend method must have. Its two helpers are used below through the class.)"""
    name = "oracle-test-dense-step"

    @staticmethod
    def _split_dense(dims, lam, Cs, xbnd, poly):
        """-> diag(C) (numpy [B,T,n]), offdiag(C) [B,T,n,n], plain lam, lam_xu, lam_xl ([B,T,nx] or None), lam_p ([B,T,m]
        or None), (xl, xh) or None, (Gr, hr) or None."""
        B, T, nx, nu = dims
        n = nx + nu
        Cn = _n(Cs)
        assert Cn.shape == (B, T, n, n), Cn.shape
        assert np.array_equal(Cn, Cn.transpose(0, 1, 3, 2)), "the host hands the kernels a symmetric C"
        Cd, off = split_cost(Cn)
        xbox, m = xbnd is not None, (poly[2] if poly is not None else 0)
        assert tuple(lam.shape) == (B, lam_width(T, nx, nu, xbox, m)), tuple(lam.shape)
        plain, lxu, lxl, lp = split_lam(_n(lam), T, nx, nu, xbox, m)
        xb = rows = None
        if xbox:
            xb = sbr._xbounds(*xbnd, B, T, nx)
            assert np.isfinite(xb[0]).all() and np.isfinite(xb[1]).all(), "the host hands the kernels finite bounds"
        if poly is not None:
            G, h, m, sb_g, st_g, sb_h, st_h = poly
            rows = _rows(G, h, sb_g, st_g, sb_h, st_h, B, T, m, n)
            assert np.isfinite(rows[0]).all() and np.isfinite(rows[1]).all(), "the host hands the kernels finite rows"
        return Cd, off, plain, lxu, lxl, lp, xb, rows

    def dual_update(self, *a, **kw):
        """The oracle's own (no state bounds, no general rows: it reads no cost), recorded."""
        self.calls.append("dual_update")
        return super().dual_update(*a, **kw)

    def newton_step_dense(self, dims, z, xnext, F, x0, lam, rho, Cs, q, ulo, uhi, sb_u, st_u, xbnd, poly, d_out, g_out=None,
                          factor=None, info=None):
        self.calls.append("newton_step_dense")
        B, T, nx, nu = dims
        s = _sfx(z)
        lo, hi = _bounds(ulo, uhi, sb_u, st_u, B, T, nu)
        Cd, off, plain, lxu, lxl, lp, xb, rows = self._split_dense(dims, lam, Cs, xbnd, poly)
        zz = _n(z)
        g, Hd, Hs = DenseOracleBackend.grad_hess_dense(s, zz, _n(xnext), _n(F), _n(x0), plain, _n(rho), Cd, off, _n(q), lo, hi)
        if xb is not None:
            gx, hx, _, _, _ = box_rows(zz[..., :nx], *xb, lxu, lxl, _n(rho))
            g, Hd = g.copy(), Hd.copy()
            g[..., :nx] += gx
            i = np.arange(nx)
            Hd[..., i, i] += hx
        if rows is not None:
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

    def merit_dense(self, dims, K, zc, xnext, x0, lam, rho, Cs, q, ulo, uhi, sb_u, st_u, xbnd, poly, phi, rnorm2=None):
        """The merit of the same rows with diag(C) (merit_rows, merit_xbox or the oracle's own), then the off-diagonal part."""
        self.calls.append("merit_dense")
        B, T, nx, nu = dims
        Cd, off, *_ = self._split_dense(dims, lam, Cs, xbnd, poly)
        Qd = _t(Cd, zc)
        n_calls = len(self.calls)
        if poly is not None:
            self.merit_rows(dims, K, zc, xnext, x0, lam, rho, Qd, q, ulo, uhi, sb_u, st_u, xbnd, poly, phi, rnorm2)
        elif xbnd is not None:
            self.merit_xbox(dims, K, zc, xnext, x0, lam, rho, Qd, q, ulo, uhi, sb_u, st_u, xbnd, phi, rnorm2)
        else:
            OracleBackend.merit(self, dims, K, zc, xnext, x0, lam, rho, Qd, q, ulo, uhi, sb_u, st_u, phi, rnorm2)
        del self.calls[n_calls:]
        zc_ = _n(zc).reshape(K, B, T, nx + nu)
        half = zc_.dtype.type(0.5)
        for k in range(K):
            phi.view(K, B)[k].add_(_t(half * np.einsum("bti,btij,btj->b", zc_[k], off, zc_[k]), phi))

    def merit_pick_dense(self, dims, n_ls, d, xnext_all, x0, lam, rho, Cs, q, ulo, uhi, sb_u, st_u, xbnd, poly, z, phi_prev,
                         rnorm2=None, phi_all=None, k_out=None, accept_out=None):
        """OracleBackend.merit_pick with merit_dense in place of merit."""
        self.calls.append("merit_pick_dense")
        B, T, nx, nu = dims
        alphas = (2.0 ** -torch.arange(n_ls, dtype=z.dtype)).view(n_ls, 1, 1, 1)
        zc = (z.unsqueeze(0) + alphas * d.unsqueeze(0)).contiguous()
        phis = torch.empty(n_ls, B, dtype=z.dtype)
        rn2s = torch.empty(n_ls, B, dtype=z.dtype)
        self.merit_dense(dims, n_ls, zc, xnext_all, x0, lam, rho, Cs, q, ulo, uhi, sb_u, st_u, xbnd, poly, phis, rn2s)
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


def dense_methods(xbox, poly):
    """Names of the methods MPC reaches on this route with these rows: the three _dense ones and the dual update's."""
    return {"newton_step_dense", "merit_dense", "merit_pick_dense",
            "dual_update_rows" if poly else "dual_update_xbox" if xbox else "dual_update"}


# ---- shared problems ---------------------------------------------------------------------------------------------------
def densify(pr, seed=0, strength=0.3):
    """The problem with a dense cost in place of diag(Qd): C = diag_embed(Qd) + strength A A' / n, A ~ N(0,1) [B,T,n,n] (a
    positive semidefinite addition with off-diagonals of order strength / sqrt(n)), symmetric, and q = -C xref with the
    xref the diagonal problem pulls to (-q / Qd; 0 where Qd is below 1e-6). -> pr with C and the new q (Qd is kept)."""
    B, T, nx, nu = pr["dims"]
    n = nx + nu
    dt = pr["Qd"].dtype
    Qd, q = pr["Qd"].double(), pr["q"].double()
    xref = torch.where(Qd > 1e-6, -q / Qd.clamp(min=1e-6), torch.zeros_like(q))
    A = torch.randn(B, T, n, n, generator=torch.Generator().manual_seed(900 + seed), dtype=torch.float64)
    C = torch.diag_embed(Qd) + strength * (A @ A.transpose(-1, -2)) / n
    C = 0.5 * (C + C.transpose(-1, -2))
    q = -torch.einsum("btij,btj->bti", C, xref)
    C = C.to(dt)
    C = (0.5 * (C + C.transpose(-1, -2))).contiguous()   # (symmetric in dt as well)
    return dict(pr, C=C, q=q.to(dt).contiguous())


def dense_problem(B, T, nx, nu, m, layout, dtype, seed=5):
    """rows_step_reference.rows_problem (state bounds that bind on both sides, m rows per stage placed around the start
    iterate, the SinPlant of the size) with densify's cost. Which rows are used is the caller's choice (`args`)."""
    pr, plant = rsr.rows_problem(B, T, nx, nu, m, layout, dtype, seed=seed)
    return densify(pr, seed), plant


def args(pr, xbox, poly):
    """(sb_u, st_u, xbnd or None, poly or None) of the three methods."""
    sb_u, st_u, xb, pl = rsr.args(pr, xbox)
    return sb_u, st_u, xb, (pl if poly else None)


def dual_update(be, dims, z, xn, x0, lo, hi, sb_u, st_u, xb, pl, lam, rho):
    """The dual update the launcher routes to."""
    if pl is not None:
        return be.dual_update_rows(dims, z, xn, x0, lo, hi, sb_u, st_u, xb, pl, lam, rho)
    if xb is not None:
        return be.dual_update_xbox(dims, z, xn, x0, lo, hi, sb_u, st_u, xb, lam, rho)
    return be.dual_update(dims, z, xn, x0, lo, hi, sb_u, st_u, lam, rho)


def al_iteration(be, pr, plant, xbox, poly, z, lam, rho, n_newton=4, n_ls=20, dual=True):
    """One AL iteration of the PyTorch-dynamics route through `be`'s three _dense methods and its dual update, in place on
    z, lam, rho."""
    dims = pr["dims"]
    B, T, nx, nu = dims
    sb_u, st_u, xb, pl = args(pr, xbox, poly)
    prob = (pr["x0"], lam, rho, pr["C"], pr["q"], pr["lo"], pr["hi"], sb_u, st_u)
    phi = torch.zeros(B, dtype=z.dtype, device=z.device)
    rn2 = torch.zeros(B, dtype=z.dtype, device=z.device)
    d = torch.empty_like(z)
    be.merit_dense(dims, 1, z, true_next(plant, z, nx), *prob, xb, pl, phi, rn2)
    alphas = (2.0 ** -torch.arange(n_ls, dtype=z.dtype, device=z.device)).view(n_ls, 1, 1, 1)
    for _ in range(n_newton):
        xn, F = linearize(plant, z, nx)
        be.newton_step_dense(dims, z, xn, F, *prob, xb, pl, d)
        zc = (z.unsqueeze(0) + alphas * d.unsqueeze(0)).contiguous()
        be.merit_pick_dense(dims, n_ls, d, true_next(plant, zc, nx), *prob, xb, pl, z, phi, rnorm2=rn2)
    if dual:
        dual_update(be, dims, z, true_next(plant, z, nx), pr["x0"], pr["lo"], pr["hi"], sb_u, st_u, xb, pl, lam, rho)
    return phi, rn2


def kernel_inputs(pr, plant, xbox, poly):
    """lam, rho after ONE reference AL iteration from the problem's start, with the iterate it left: what the GPU tests
    feed every kernel. -> dict(z, lam, rho, xn, F, d, g, hessian)."""
    B, T, nx, nu = pr["dims"]
    be = DenseStepOracleBackend()
    z = pr["z0"].clone()
    lam = torch.zeros(B, lam_width(T, nx, nu, xbox, pr["m"] if poly else 0), dtype=z.dtype)
    rho = torch.ones(B, dtype=z.dtype)
    al_iteration(be, pr, plant, xbox, poly, z, lam, rho)
    xn, F = linearize(plant, z, nx)
    sb_u, st_u, xb, pl = args(pr, xbox, poly)
    d, g = torch.empty_like(z), torch.empty_like(z)
    be.newton_step_dense(pr["dims"], z, xn, F, pr["x0"], lam, rho, pr["C"], pr["q"], pr["lo"], pr["hi"], sb_u, st_u, xb, pl,
                         d, g_out=g)
    return dict(z=z, lam=lam, rho=rho, xn=xn, F=F, d=d, g=g, hessian=be.last_hessian)


def residuals(pr, z, xbox, poly):
    """Every inequality residual at z in float64: dict(u [B,T,2nu], x [B,T,2nx] or None, p [B,T,m] or None)."""
    out = rsr.residuals(pr, z, xbox)
    if not poly:
        out["p"] = None
    return out


# ---- the GPU tests' cases (tests/test_gpu_dense_step.py; their preconditions are asserted on the CPU too) ----------------
# rows_step_reference.GPU_CASES, and one with T n > 64 and T m > 64: both lane loops of the merit kernels (cost rows and
# general rows) take a second trip.
GPU_CASES = list(rsr.GPU_CASES) + [(13, 4, 4, 2, 17, "per_stage")]
GPU_SEED = 5


def gpu_case(nx, nu, T, B, m, layout, xbox, poly, dtype):
    """-> (pr, plant, inp): the problem, its plant and kernel_inputs of the case, CPU tensors in `dtype`."""
    pr, plant = dense_problem(B, T, nx, nu, m, layout, dtype, seed=GPU_SEED)
    return pr, plant, kernel_inputs(pr, plant, xbox, poly)


def gamma_cost_row(n):
    """Roundings the dense cost term adds to a chain that held the diagonal term's. The diagonal term (0.5 Q v + q) v has
    three operations (aux_cases._own: Q v, + q, . v; two more with a candidate). The dense term
    (0.5 (C_t z_t)_i + q_i) z_i keeps the three and has an n-term dot product where the one product Q v stood: a product
    of that sum passes its own rounding and at most n - 1 additions, n roundings relative to |C_t[i,:]| . |z_t| (the count
    rows_step_reference.gamma_rows takes for a general row's dot product), n - 1 more than the one product. In a
    candidate the row's second dot product C_t[i,:] . d_t has the same count and runs beside the first, not behind it
    (both are in the magnitude |C| . (|z| + alpha |d|)); alpha cd is exact and the sum cz + alpha cd adds one: n more."""
    return n


def gamma_merit_dense(T, nx, nu, m, cand=False):
    """aux_cases.gamma_merit (m = 0) or rows_step_reference.gamma_merit_rows, plus the cost row's roundings."""
    base = rsr.gamma_merit_rows(T, nx, nu, m, cand) if m else ax.gamma_merit(T, nx, nu, 0, cand)
    return base + gamma_cost_row(nx + nu)


def gamma_rnorm2_dense(T, nx, nu, m, cand=False):
    """rnorm2 holds no cost term: the rows' count."""
    return rsr.gamma_rnorm2_rows(T, nx, nu, m, cand) if m else ax.gamma_rnorm2(T, nx, nu, 0, cand)


def merit_magnitude_dense(pr, z, xn, lam, rho, xbox, poly, zmag=None):
    """The magnitudes of the same rows with diag(C) (aux_cases.merit_magnitude, merit_magnitude_xbox or
    merit_magnitude_rows) plus the off-diagonal part of the cost: 1/2 z' offdiag(C) z in phi, 1/2 |z|' |offdiag(C)| |z| in
    A. -> (phi, A, rp2, A2) per instance in float64."""
    B, T, nx, nu = pr["dims"]
    f = lambda t: t.detach().cpu().double().numpy() if torch.is_tensor(t) else np.asarray(t, np.float64)
    Cd, off = split_cost(f(pr["C"]))
    prd = dict(pr, Qd=torch.from_numpy(Cd))
    if poly:
        phi, A, rp2, A2 = rsr.merit_magnitude_rows(prd, z, xn, lam, rho, xbox, zmag=zmag)
    elif xbox:
        phi, A, rp2, A2 = ssr.merit_magnitude_xbox(prd, z, xn, lam, rho, zmag=zmag)
    else:
        ulo, uhi = np.broadcast_to(f(pr["lo"]), (B, T, nu)), np.broadcast_to(f(pr["hi"]), (B, T, nu))
        phi, A, rp2, A2 = ax.merit_magnitude(f(z), f(xn), f(pr["x0"]), f(lam), f(rho).reshape(B), Cd, f(pr["q"]), ulo, uhi,
                                             zmag=zmag)
    zz = f(z)
    zm = np.abs(zz) if zmag is None else zmag
    phi = phi + 0.5 * np.einsum("bti,btij,btj->b", zz, off, zz)
    A = A + 0.5 * np.einsum("bti,btij,btj->b", zm, np.abs(off), zm)
    return phi, A, rp2, A2


def terms_numpy(pr, z, xn, lam, rho, xbox, poly):
    """A direct float64 statement of the merit at (z, xnext, lam, rho) with the full C, independent of the oracle, of
    split_cost, of box_rows and of poly_rows: -> dict(phi [B], rp2 [B])."""
    B, T, nx, nu = pr["dims"]
    n = nx + nu
    m = pr["m"] if poly else 0
    f = lambda t: t.detach().cpu().double().numpy()
    z, xn, lam, rho = f(z), f(xn), f(lam), f(rho).reshape(B)
    C, q, x0 = f(pr["C"]), f(pr["q"]), f(pr["x0"])
    bc = lambda v, w: np.broadcast_to(f(v), (B, T, w))
    ulo, uhi = bc(pr["lo"], nu), bc(pr["hi"], nu)
    xr = 2 * nx if xbox else 0
    neq, nit = T * nx, 2 * nu + xr + m
    phi, rp2 = np.zeros(B), np.zeros(B)
    for b in range(B):
        for t in range(T):
            for i in range(n):
                phi[b] += (0.5 * sum(C[b, t, i, j] * z[b, t, j] for j in range(n)) + q[b, t, i]) * z[b, t, i]
            for i in range(nx):
                r = z[b, t + 1, i] - xn[b, t, i] if t < T - 1 else z[b, 0, i] - x0[b, i]
                phi[b] += lam[b, t * nx + i] * r
                rp2[b] += r * r
            rows = [(j, z[b, t, nx + j] - uhi[b, t, j]) for j in range(nu)]
            rows += [(nu + j, -z[b, t, nx + j] + ulo[b, t, j]) for j in range(nu)]
            if xbox:
                xlo, xhi = bc(pr["xlo"], nx), bc(pr["xhi"], nx)
                rows += [(2 * nu + i, z[b, t, i] - xhi[b, t, i]) for i in range(nx)]
                rows += [(2 * nu + nx + i, -z[b, t, i] + xlo[b, t, i]) for i in range(nx)]
            if poly:
                G, h = np.broadcast_to(f(pr["G"]), (B, T, m, n)), bc(pr["h"], m)
                rows += [(2 * nu + xr + k, sum(G[b, t, k, j] * z[b, t, j] for j in range(n)) - h[b, t, k]) for k in range(m)]
            for k, r in rows:
                phi[b] += lam[b, neq + t * nit + k] * r
                rp2[b] += max(r, 0.0) ** 2
        phi[b] += 0.5 * rho[b] * rp2[b]
    return dict(phi=phi, rp2=rp2)


# |dlam| of the route twin on the INERT problem, as tests/test_dense_step_cpu.py::test_route_twin measures and prints it
# (reference exit): the same twin with the off-diagonal part of C dropped and every state bound and general row out of
# reach, which leaves the difference of the two routes' summation orders and nothing of the feature. Keys (nx, nu, xbox,
# poly); what the twin bound of the whole-solve comparisons is 8 times of.
INERT_TWIN = {(2, 1, False, False): 1.07e-14, (2, 1, True, False): 1.07e-14, (2, 1, False, True): 1.07e-14,
              (2, 1, True, True): 1.07e-14, (13, 4, False, False): 6.75e-14, (13, 4, True, False): 6.75e-14,
              (13, 4, False, True): 6.75e-14, (13, 4, True, True): 6.75e-14}


# The whole solves through MPC that the GPU tests compare (tests/test_gpu_dense_step.py), per size: keywords of
# dense_whole_problem, chosen on this reference alone by the rule of rows_step_reference.WHOLE_SOLVE_KW (no line search of
# the solve whose two best merits are closer than WHOLE_SOLVE_MIN_GAP, relative; asserted in tests/test_dense_step_cpu.py).
# (2,1), B = 3: CurvedSinPlant as in section 25. A heavier sine converges slowly enough that every line search stays
# decided, but is more sensitive to rounding (section 25): both are read off the REFERENCE alone. Searched: gains 0 (SinPlant),
# 1, 2, 4 at step 0.1 and 2, 4, 6, 8 at step 0.3, seeds 3..12. Kept: the settings whose problem can be built in all four
# combinations, whose eight solves (2 exit modes, 4 combinations) have no line search DenseTieBackend marks and none with
# its two best merits closer than WHOLE_SOLVE_MIN_GAP, and in which a one-ulp change of q (either way) moves the reference's
# own lam by less than the twin bound - a comparison to that bound says nothing where the reference itself moves by more.
# That leaves gain 6 / seed 4 (smallest gap 1.1e-7, the reference moves by 0.53 of the bound). Rejected on the gap: gain 4
# at step 0.1 / seed 12 (1.8e-12), gain 6 / seed 3 (4.0e-11); on undecided line searches: every SinPlant seed and gain 1, 2;
# on the reference's own sensitivity: gain 8 / seeds 3, 4, 6 (15.7, 1.7 and 1.1 bounds; at B = 5 17.7 and 5.1). Gain 8 / seeds
# 3 and 4 at B = 5 were run on the MI355X before that last criterion was applied: x, u equal as float32, gradients within
# 3e-14, lam within the bound in seven of eight cases and 8.9 / 1.9 times it in the rows-alone case - a half / two fifths
# of what the reference itself moves by there.
# (13,4): on SinPlant itself 10 to 14 of the 24 instance-solves
# (3 instances, 2 exit modes, 4 combinations; seeds 3..8) have a line search float64 does not decide (DenseTieBackend), so
# the plant is CurvedSinPlant there too; in the order SinPlant seeds 3..8, then gain 1, 2, 4, 8 at step 0.3, seeds 3..8, the
# first setting whose problem can be built (the rowless solution violates the row in every instance) and whose eight
# solves have no undecided line search is gain 1 / seed 3.
WHOLE_SOLVE_KW = {(2, 1): dict(seed=4, gain=6.0, h_plant=0.3), (13, 4): dict(seed=3, gain=1.0, h_plant=0.3)}
WHOLE_SOLVE_MIN_GAP = rsr.WHOLE_SOLVE_MIN_GAP
WHOLE_SOLVE_DIMS = {(2, 1): (5, 3), (13, 4): (5, 3)}   # (T, B)
# the B = 4096 whole solve at (2,1), T = 3: on SinPlant itself 2375 of the 4096 instances have an undecided line search (with
# section 25's diagonal cost 666 had), over the cap of a quarter; on the (2,1) whole solves' plant (gain 8 at step 0.3; the
# problem generator's own seed) none has.
LARGE_BATCH_KW = dict(gain=8.0, h_plant=0.3)


def dense_whole_problem(B, T, nx, nu, xbox, poly, mode="reference", strength=0.3, **kw):
    """rows_step_reference.coupled_row_problem (the sin plant, the cost pulling states 0 and 1 the same way, one coupled row
    x_0 + x_1 <= h that the plant's rollout satisfies and the rowless solution violates, the state box |x| <= 0.8) with
    densify's cost, which pulls to the same reference. Which rows are used is the caller's choice. -> (pr, plant)."""
    pr, plant, _ = rsr.coupled_row_problem(B, T, nx, nu, xbox, mode, **kw)
    return densify(pr, kw.get("seed", 5), strength), plant


def mpc_kwargs(pr, xbox, poly, dev="cpu", h=None):
    """The constructor's keywords for the rows in use."""
    kw = {}
    if xbox:
        kw.update(x_lower=pr["xlo"].to(dev), x_upper=pr["xhi"].to(dev))
    if poly:
        kw.update(ineqG=pr["G"].to(dev), ineqh=pr["h"].to(dev) if h is None else h)
    return kw


class DenseTieBackend(DenseStepOracleBackend):
    """rows_step_reference.TieBackend's rule on this route: marks, per instance, every line search the float64 arithmetic
    does not decide - the two best of the candidates' merits closer than twice the merit's rounding bound (gamma_merit_dense
    x eps x the magnitude of merit_magnitude_dense), or the best merit that close to phi_prev (the strict accept).
    `undecided` [B] (bool) collects the marks over a solve; `tied_step` [B] the largest |d| of an instance's marked steps."""

    def __init__(self):
        super().__init__()
        self.undecided = None
        self.tied_step = None

    def merit_pick_dense(self, dims, n_ls, d, xnext_all, x0, lam, rho, Cs, q, ulo, uhi, sb_u, st_u, xbnd, poly, z, phi_prev,
                         **kw):
        B, T, nx, nu = dims
        z0, prev = z.clone(), phi_prev.clone()
        pa = torch.empty(n_ls, B, dtype=z.dtype)
        super().merit_pick_dense(dims, n_ls, d, xnext_all, x0, lam, rho, Cs, q, ulo, uhi, sb_u, st_u, xbnd, poly, z, phi_prev,
                                 **{**kw, "phi_all": pa})
        pr = dict(dims=dims, x0=x0, C=Cs, q=q, lo=ulo, hi=uhi)
        if poly is not None:
            pr.update(G=poly[0], h=poly[1], m=poly[2])
        if xbnd is not None:
            pr.update(xlo=xbnd[0], xhi=xbnd[1])
        m = poly[2] if poly is not None else 0
        al = (2.0 ** -np.arange(n_ls)).reshape(n_ls, 1, 1, 1)
        zc = z0.double().numpy()[None] + al * d.double().numpy()[None]
        zmag = np.abs(z0.double().numpy())[None] + al * np.abs(d.double().numpy())[None]
        A = np.stack([merit_magnitude_dense(pr, zc[k], xnext_all[k], lam, rho, xbnd is not None, poly is not None,
                                            zmag=zmag[k])[1] for k in range(n_ls)])
        tol = gamma_merit_dense(T, nx, nu, m, cand=True) * 2.0 ** -53 * A.max(0)
        srt = np.sort(pa.double().numpy(), 0)
        und = (srt[1] - srt[0] <= 2 * tol) if n_ls > 1 else np.zeros(B, bool)
        und |= np.abs(srt[0] - prev.double().numpy()) <= 2 * tol
        step = d.double().abs().reshape(B, -1).max(1).values.numpy()
        if self.undecided is None:
            self.undecided, self.tied_step = np.zeros(B, bool), np.zeros(B)
        self.undecided |= und
        self.tied_step = np.where(und, np.maximum(self.tied_step, step), self.tied_step)
