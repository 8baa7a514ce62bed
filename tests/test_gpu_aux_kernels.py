"""The launch-per-step helper kernels of csrc/alqp_aux.hip - k_merit (alqp_merit), k_pick (alqp_linesearch_pick),
k_merit_pick (alqp_merit_pick), k_dual (alqp_dual_update) - each against the fp64 oracle fed the kernel's own inputs
upcast, at the shapes of tests/aux_cases.py::SHAPES, with the three row sets and the four bound layouts, inside the
rounding bound derived there (gamma * eps * magnitude; never tuned). Every output is a slice from the middle of a
sentinel-filled tensor whose guard bands must stay intact.

Each check prints `AUXMARGIN <entry> <dtype> <error / (eps magnitude)> <gamma>` before it asserts, so that a run with -s
shows the measured margin under the bound. Measured on an MI355X, largest error / (eps magnitude) over all cases (gamma of
that case), fp32 | fp64: merit 0.84 (15) | 4.7 (29); its rnorm2 1.8 (12) | 10.5 (21); merit_pick phi_all 1.3 (17) | 6.5 (31);
its rnorm2 2.2 (14) | 10.5 (23); dual update, equality and bound rows 1.8 (3) | 2.0 (3), obstacle rows 0.46 (9) | 0.58 (9).
The fp64 figures contain the fp64 oracle's own rounding (it sums T n + M terms one after the other), which the fp32 ones
do not see; written down for the record, not fed back into the bound."""
import functools

import numpy as np
import pytest
import torch

from tests import aux_cases as ac

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float64, torch.float32]
GRID = ac.grid()


def _be():
    from deq_mpc_corl_amd.backend import default_backend
    return default_backend()


def _sync(dev):
    if str(dev).startswith("cuda"):
        torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def _case(dims, dtype, rows, bounds):
    """Shared between the tests; nobody writes to it (in/out arguments are copies)."""
    return ac.case(dims, dtype, rows, bounds)


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a.cpu()), _bits(b.cpu()))


def _margin(entry, dtype, err, mag, gamma):
    """Largest error / (eps magnitude); printed for the record, asserted by the caller against gamma."""
    ratio = float(np.max(np.asarray(err) / (ac.EPS[dtype] * np.asarray(mag))))
    print(f"AUXMARGIN {entry} {ac.grid_id(dtype)} {ratio:.3f} {float(np.max(gamma)):.0f}")
    return ratio


class _Inputs:
    """A case's read-only inputs on the device, with a copy to prove that a kernel left them bitwise alone."""

    def __init__(self, c, dev):
        self.c, self.dev = c, dev
        names = dict(x0=c.p.x0, lam=c.lam, rho=c.rho, Qd=c.p.Qd, q=c.p.q, ulo=c.ulo, uhi=c.uhi, z=c.z, xnext=c.xnext, d=c.d)
        self.t = {k: v.to(dev).contiguous() for k, v in names.items()}
        self.obs = c.obs
        if c.rows == "obstacles":
            self.t["pos"] = c.obs[0].to(dev).contiguous()
            self.obs = (self.t["pos"], c.obs[1])
        self.kw = {"obs": self.obs} if self.obs is not None else {}

    def __getattr__(self, k):
        return self.t[k]

    def unchanged(self, skip=()):
        ref = dict(x0=self.c.p.x0, lam=self.c.lam, rho=self.c.rho, Qd=self.c.p.Qd, q=self.c.p.q, ulo=self.c.ulo,
                   uhi=self.c.uhi, z=self.c.z, xnext=self.c.xnext, d=self.c.d)
        if "pos" in self.t:
            ref["pos"] = self.c.obs[0]
        return all(_same_bits(self.t[k], v) for k, v in ref.items() if k not in skip)


# ---- alqp_merit ------------------------------------------------------------------------------------------------------

def check_merit(be, dev, c, K):
    B, T, nx, nu = c.dims
    n = nx + nu
    i = _Inputs(c, dev)
    g = torch.Generator(device="cpu").manual_seed(23)
    # candidate 0 is the case's own point, the others are unrelated points around it
    zc = torch.stack([c.z] + [c.z + (0.3 * torch.randn(B, T, n, generator=g, dtype=torch.float64)).to(c.dtype)
                              for _ in range(K - 1)]).contiguous()
    xn = torch.stack([c.xnext] + [c.xnext + (0.05 * torch.randn(B, T - 1, nx, generator=g, dtype=torch.float64)).to(c.dtype)
                                  for _ in range(K - 1)]).contiguous()
    zc_d, xn_d = zc.to(dev), xn.to(dev)
    phi = ac.Guarded((K, B), c.dtype, dev)
    rn2 = ac.Guarded((K, B), c.dtype, dev)
    be.merit(c.dims, K, zc_d, xn_d, i.x0, i.lam, i.rho, i.Qd, i.q, i.ulo, i.uhi, c.sb_u, c.st_u, phi.t, rn2.t, **i.kw)
    phi2 = ac.Guarded((K, B), c.dtype, dev)
    be.merit(c.dims, K, zc_d, xn_d, i.x0, i.lam, i.rho, i.Qd, i.q, i.ulo, i.uhi, c.sb_u, c.st_u, phi2.t, None, **i.kw)
    _sync(dev)
    got, got2 = phi.t.cpu().double().numpy(), rn2.t.cpu().double().numpy()
    gam, gam2 = ac.gamma_merit(T, nx, nu, c.nobs), ac.gamma_rnorm2(T, nx, nu, c.nobs)
    for k in range(K):
        z64, x64 = zc[k].double().numpy(), xn[k].double().numpy()
        ref, ref2 = ac.oracle_merit(c, z64, x64)
        m = ac.merit_magnitude(Qd=ac._n64(c.p.Qd), q=ac._n64(c.p.q), **ac.magnitude_args(c, z64, x64))
        r = _margin("merit", c.dtype, np.abs(got[k] - ref), m.A, gam)
        r2 = _margin("merit.rnorm2", c.dtype, np.abs(got2[k] - ref2), m.A2, gam2)
        assert r <= gam, (k, r, gam)
        assert r2 <= gam2, (k, r2, gam2)
    assert _same_bits(phi.t, phi2.t), "rnorm2 = None changed phi"
    assert phi.intact() and rn2.intact() and phi2.intact()
    assert i.unchanged() and _same_bits(zc_d, zc) and _same_bits(xn_d, xn)


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("dtype", DTYPES, ids=ac.grid_id)
@pytest.mark.parametrize("dims,rows,bounds", GRID, ids=ac.grid_id)
def test_merit(dims, rows, bounds, dtype, K):
    check_merit(_be(), DEV, _case(dims, dtype, rows, bounds), K)


# ---- alqp_dual_update ------------------------------------------------------------------------------------------------

def check_dual(be, dev, c, scale):
    B, T, nx, nu = c.dims
    neq = T * nx
    i = _Inputs(c, dev)
    lam = ac.Guarded(tuple(c.lam.shape), c.dtype, dev, init=c.lam)
    rho = ac.Guarded((B,), c.dtype, dev, init=c.rho)
    be.dual_update(c.dims, i.z, i.xnext, i.x0, i.ulo, i.uhi, c.sb_u, c.st_u, lam.t, rho.t, rho_scale=scale, **i.kw)
    _sync(dev)
    got = lam.t.cpu().double().numpy()
    ref, _ = ac.oracle_dual(c)
    dm = ac.dual_magnitude(**ac.magnitude_args(c))
    gam = ac.gamma_dual_rows(T, nx, nu, c.nobs)[None, :]
    mag = np.where(dm.mag > 0, dm.mag, 1.0)       # a row of magnitude 0 must be exact: error 0 / 1
    err = np.abs(got - ref)
    for name, sel in (("dual_update.eq+bounds", gam[0] == 3), ("dual_update.obstacles", gam[0] == 9)):
        if sel.any():
            _margin(name, c.dtype, err[:, sel], mag[:, sel], gam[0, sel])
    assert (err <= gam * ac.EPS[c.dtype] * dm.mag).all(), float((err / (ac.EPS[c.dtype] * mag)).max())
    tol = gam * ac.EPS[c.dtype] * dm.mag
    ineq = slice(neq, None)
    assert (got[:, ineq] >= 0).all()
    hard = dm.v[:, ineq] < -tol[:, ineq]             # the rows the oracle clamps, beyond any rounding
    assert hard.any() and (ref[:, ineq][hard] == 0).all() and (got[:, ineq][hard] == 0).all()
    assert _same_bits(rho.t, c.rho * torch.tensor(scale, dtype=c.dtype)), "rho_out != rho_in * real(rho_scale)"
    if c.rows == "state_estimator":
        assert _same_bits(lam.t[:, neq - nx:neq], c.lam[:, neq - nx:neq]), "state estimator: initial-state rows touched"
    assert lam.intact() and rho.intact()
    assert i.unchanged()


@pytest.mark.parametrize("scale", [10.0, 1.0, 2.5])
@pytest.mark.parametrize("dtype", DTYPES, ids=ac.grid_id)
@pytest.mark.parametrize("dims,rows,bounds", GRID, ids=ac.grid_id)
def test_dual_update(dims, rows, bounds, dtype, scale):
    check_dual(_be(), DEV, _case(dims, dtype, rows, bounds), scale)


# ---- alqp_linesearch_pick: exact cases -------------------------------------------------------------------------------
NAN, INF = float("nan"), float("inf")
# name -> (phi column of instance 0, phi_prev of instance 0, expected k, expected accept). Instance b gets the column
# and phi_prev shifted by the integer b (exact), so the [n_ls][B] indexing matters.
PICK_CASES = {
    "min_first":       ([1, 5, 6, 7, 8, 9, 10, 11], 20, 0, 1),
    "min_middle":      ([9, 8, 7, 2, 7, 8, 9, 10], 20, 3, 1),
    "min_last":        ([9, 8, 7, 6, 5, 4, 3, 2], 20, 7, 1),
    "two_minima":      ([9, 8, 3, 7, 6, 3, 8, 9], 20, 2, 1),
    "prev_equals_min": ([9, 8, 7, 2, 7, 8, 9, 10], 2, 3, 0),
    "prev_below_min":  ([9, 8, 7, 2, 7, 8, 9, 10], 1, 3, 0),
    "nan_first":       ([NAN, 8, 7, 2, 7, 8, 9, 10], 20, 0, 0),
    "nan_wins":        ([9, 8, 7, NAN, 6, 1, 8, 9], 20, 3, 0),
    "inf_everywhere":  ([INF] * 8, 20, 0, 0),
    "n_ls_1":          ([2], 3, 0, 1),
}


def check_pick(be, dev, dims, dtype, name, with_outputs=True):
    from oracle import oracle_py as orc
    B, T, nx, nu = dims
    n = nx + nu
    col, prev0, k_want, acc_want = PICK_CASES[name]
    n_ls = len(col)
    shift = torch.arange(B, dtype=dtype)
    phi = (torch.tensor(col, dtype=dtype).view(n_ls, 1) + shift.view(1, B)).contiguous()
    prev = (torch.full((B,), float(prev0), dtype=dtype) + shift).contiguous()
    # small integers: z + 2^-k d is exact in fp32 for k < 8
    idx = torch.arange(B * T * n)
    z0 = ((idx % 11) - 5).to(dtype).view(B, T, n).contiguous()
    d = ((idx % 7) - 3).to(dtype).view(B, T, n).contiguous()
    kr, ar, pm = orc.linesearch_pick("f64", phi.double().numpy(), prev.double().numpy())
    assert kr.tolist() == [k_want] * B and ar.tolist() == [acc_want] * B       # the oracle agrees with the table
    z_want = z0 + (2.0 ** -k_want) * d if acc_want else z0
    _run_pick(be, dev, dims, n_ls, phi, prev, d, z0, kr, ar, torch.from_numpy(pm).to(dtype), z_want, with_outputs)


def _run_pick(be, dev, dims, n_ls, phi, prev, d, z0, k_want, acc_want, prev_want, z_want, with_outputs=True):
    B = dims[0]
    dtype = z0.dtype
    phi_d, d_d = phi.to(dev), d.to(dev)
    z = ac.Guarded(tuple(z0.shape), dtype, dev, init=z0)
    pp = ac.Guarded((B,), dtype, dev, init=prev)
    k = ac.Guarded((B,), torch.int32, dev)
    a = ac.Guarded((B,), torch.int32, dev)
    if with_outputs:
        be.linesearch_pick(dims, n_ls, phi_d, pp.t, d_d, z.t, k.t, a.t)
    else:
        be.linesearch_pick(dims, n_ls, phi_d, pp.t, d_d, z.t, None, None)
    _sync(dev)
    if with_outputs:
        assert k.t.cpu().tolist() == list(map(int, k_want)), "k"
        assert a.t.cpu().tolist() == list(map(int, acc_want)), "accept"
    else:
        assert (k.t == ac.ISENTINEL).all() and (a.t == ac.ISENTINEL).all()
    zc, ppc = z.t.cpu(), pp.t.cpu()
    assert torch.equal(torch.isnan(ppc), torch.isnan(prev_want))
    assert torch.equal(torch.nan_to_num(ppc, nan=0.0), torch.nan_to_num(prev_want, nan=0.0)), "phi_prev"
    if not any(acc_want):
        assert _same_bits(zc, z0), "rejected: z must be bitwise unchanged"
    assert torch.equal(zc, z_want), "z"
    assert z.intact() and pp.intact() and k.intact() and a.intact()
    assert _same_bits(phi_d, phi) and _same_bits(d_d, d)


@pytest.mark.parametrize("name", list(PICK_CASES))
@pytest.mark.parametrize("dtype", DTYPES, ids=ac.grid_id)
@pytest.mark.parametrize("dims", [(3, 2, 3, 1), (37, 20, 13, 4)], ids=ac.grid_id)
def test_linesearch_pick_exact(dims, dtype, name):
    check_pick(_be(), DEV, dims, dtype, name)


@pytest.mark.parametrize("dtype", DTYPES, ids=ac.grid_id)
def test_linesearch_pick_without_k_and_accept(dtype):
    check_pick(_be(), DEV, (37, 20, 13, 4), dtype, "min_middle", with_outputs=False)


def check_pick_n_ls_40(be, dev, dims, dtype, kmin):
    from oracle import oracle_py as orc
    dims, phi, prev, z0, d, z_want = ac.pick_case_n_ls_40(dtype, kmin, dims)
    kr, ar, pm = orc.linesearch_pick("f64", phi.double().numpy(), prev.double().numpy())
    assert kr.tolist() == [kmin] * dims[0] and ar.tolist() == [1] * dims[0]
    assert float(z_want.abs().min()) == 2.0 ** (-3 - kmin)          # nothing flushed to zero: all of z is checked
    _run_pick(be, dev, dims, 40, phi, prev, d, z0, kr, ar, torch.from_numpy(pm).to(dtype), z_want)


@pytest.mark.parametrize("kmin", [35, 31])
@pytest.mark.parametrize("dtype", DTYPES, ids=ac.grid_id)
@pytest.mark.parametrize("dims", [(3, 2, 3, 1), (37, 20, 13, 4)], ids=ac.grid_id)
def test_linesearch_pick_n_ls_40(dims, dtype, kmin):
    """z + 2^-k d for k beyond what an integer shift can form (include/mi_alqp.h sets no limit on n_ls here)."""
    check_pick_n_ls_40(_be(), DEV, dims, dtype, kmin)


# ---- alqp_merit_pick -------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _ls_reference(dims, dtype, rows, bounds):
    """Per case, once: the 20 candidates z + 2^-k d formed in fp64 from the kernel's inputs, their x_next from the affine
    F, c in `dtype` (an input of the kernel), and the fp64 oracle's merit and rp2 of every candidate with magnitudes."""
    c = _case(dims, dtype, rows, bounds)
    alphas = 2.0 ** -torch.arange(20, dtype=torch.float64)
    zc64 = c.z.double()[None] + alphas.view(20, 1, 1, 1) * c.d.double()[None]
    zmag = c.z.double().abs()[None] + alphas.view(20, 1, 1, 1) * c.d.double().abs()[None]
    zc = (c.z[None] + alphas.to(dtype).view(20, 1, 1, 1) * c.d[None]).contiguous()
    xnc = (torch.einsum("btij,kbtj->kbti", c.p.F, zc[:, :, :-1]) + c.p.c).contiguous()
    phi, rp2, A, A2 = [], [], [], []
    for k in range(20):
        z64, x64 = zc64[k].numpy(), xnc[k].double().numpy()
        p_, r_ = ac.oracle_merit(c, z64, x64)
        m = ac.merit_magnitude(Qd=ac._n64(c.p.Qd), q=ac._n64(c.p.q), **ac.magnitude_args(c, z64, x64, zmag[k].numpy()))
        phi.append(p_); rp2.append(r_); A.append(m.A); A2.append(m.A2)
    return zc64.numpy(), xnc, np.stack(phi), np.stack(rp2), np.stack(A), np.stack(A2)


def _merit_pick(be, dev, c, i, n_ls, xn_all, prev):
    B = c.dims[0]
    o = dict(z=ac.Guarded(tuple(c.z.shape), c.dtype, dev, init=c.z), pp=ac.Guarded((B,), c.dtype, dev, init=prev),
             rn2=ac.Guarded((B,), c.dtype, dev, init=torch.full((B,), -1.0, dtype=c.dtype)),
             phi=ac.Guarded((20, B), c.dtype, dev), k=ac.Guarded((B,), torch.int32, dev),
             a=ac.Guarded((B,), torch.int32, dev))
    be.merit_pick(c.dims, n_ls, i.d, xn_all, i.x0, i.lam, i.rho, i.Qd, i.q, i.ulo, i.uhi, c.sb_u, c.st_u, o["z"].t,
                  o["pp"].t, rnorm2=o["rn2"].t, phi_all=o["phi"].t, k_out=o["k"].t, accept_out=o["a"].t, **i.kw)
    _sync(dev)
    assert all(g.intact() for g in o.values()), "guard band"
    return {k: v.t.cpu() for k, v in o.items()}


def check_merit_pick(be, dev, c, n_ls, bounds):
    from oracle import oracle_py as orc
    B, T, nx, nu = c.dims
    eps = ac.EPS[c.dtype]
    zc64, xnc, phi_ref, rp2_ref, A, A2 = _ls_reference(c.dims, c.dtype, c.rows, bounds)
    phi_ref, rp2_ref, A, A2 = phi_ref[:n_ls], rp2_ref[:n_ls], A[:n_ls], A2[:n_ls]
    gam, gam2 = ac.gamma_merit(T, nx, nu, c.nobs, cand=True), ac.gamma_rnorm2(T, nx, nu, c.nobs, cand=True)
    tol = gam * eps * A                                  # [n_ls, B]
    tol_b = tol.max(0)
    i = _Inputs(c, dev)
    xn_all = xnc.clone()
    xn_all[n_ls:] = NAN                                  # slabs the kernel must not read
    xn_all_d = xn_all.to(dev)
    # phi_prev_in well away from the minimum on either side: the accept decision is never near a tie
    kmin_ref = phi_ref.argmin(0)
    min_ref = phi_ref.min(0)
    s = np.where(np.arange(B) % 3 == 0, -1.0, 1.0)
    prev = torch.from_numpy(min_ref + s * np.maximum(1.0, 100 * tol_b)).to(c.dtype)
    k_ref, acc_ref, _ = orc.linesearch_pick("f64", phi_ref, prev.double().numpy())
    o = _merit_pick(be, dev, c, i, n_ls, xn_all_d, prev)
    # candidates' merits
    got = o["phi"].double().numpy()
    r = _margin("merit_pick.phi_all", c.dtype, np.abs(got[:n_ls] - phi_ref), A, gam)
    assert r <= gam, (r, gam)
    assert (o["phi"][n_ls:] == ac.SENTINEL).all(), "phi_all rows >= n_ls written"
    for name in ("phi", "z", "pp", "rn2"):
        assert not torch.isnan(o[name]).any(), name + ": a NaN slab of xnext_all was read"
    # decision
    kg, ag = o["k"].numpy(), o["a"].numpy()
    assert ((kg >= 0) & (kg < n_ls)).all()
    bi = np.arange(B)
    if c.dtype == torch.float64:
        assert np.array_equal(kg, k_ref), (kg, k_ref)
    # the chosen candidate minimises up to the kernel's own rounding of it and of the true minimiser
    gap = phi_ref[kg, bi] - min_ref
    print(f"AUXMARGIN merit_pick.minimiser {ac.grid_id(c.dtype)} {float(np.max(gap / (eps * A[kg, bi]))):.3f} {2 * gam}")
    assert (gap <= tol[kg, bi] + tol[kmin_ref, bi]).all() and (gap <= 2 * tol_b).all()
    assert np.array_equal(ag, acc_ref), (ag, acc_ref)
    if B >= 3:
        assert 0 < ag.sum() < B
    acc = ag > 0
    z_out, z64, d64 = o["z"].double().numpy(), c.z.double().numpy(), c.d.double().numpy()
    zerr = np.abs(z_out - zc64[kg, bi])
    assert (zerr[acc] <= eps * (np.abs(z64) + np.abs(d64))[acc]).all()
    assert _same_bits(o["z"][~torch.from_numpy(acc)], c.z[~torch.from_numpy(acc)])
    assert _same_bits(o["pp"], o["phi"][torch.from_numpy(kg).long(), torch.arange(B)])
    rn2 = o["rn2"].double().numpy()
    assert (rn2[~acc] == -1.0).all()
    if acc.any():
        r2 = _margin("merit_pick.rnorm2", c.dtype, np.abs(rn2 - rp2_ref[kg, bi])[acc], A2[kg, bi][acc], gam2)
        assert r2 <= gam2, (r2, gam2)
    assert i.unchanged() and _same_bits(xn_all_d.nan_to_num(nan=1.5), xn_all.nan_to_num(nan=1.5))
    # strictness: phi_prev = the kernel's own minimum -> best < prev is false for every instance
    o2 = _merit_pick(be, dev, c, i, n_ls, xn_all_d, o["pp"])
    assert o2["a"].tolist() == [0] * B and _same_bits(o2["z"], c.z)
    assert torch.equal(o2["k"], o["k"]) and _same_bits(o2["pp"], o["pp"]) and (o2["rn2"] == -1.0).all()
    # a NaN candidate (slab 2, every third instance) wins like torch.min: k = 2, reject, phi_prev = NaN
    if n_ls > 2:
        hit = torch.arange(B) % 3 == 0
        xn_nan = xn_all.clone()
        xn_nan[2, hit, T - 2, nx - 1] = NAN
        o3 = _merit_pick(be, dev, c, i, n_ls, xn_nan.to(dev), prev)
        assert (o3["k"][hit] == 2).all() and (o3["a"][hit] == 0).all()
        assert torch.isnan(o3["pp"][hit]).all() and torch.isnan(o3["phi"][2][hit]).all()
        assert _same_bits(o3["z"][hit], c.z[hit]) and (o3["rn2"][hit] == -1.0).all()
        for name in ("z", "pp", "rn2", "phi", "k", "a"):
            a_, b_ = (o3[name], o[name]) if name != "phi" else (o3[name].T, o[name].T)
            assert torch.equal(a_[~hit], b_[~hit]), name + ": an instance without the NaN changed"


@pytest.mark.parametrize("n_ls", [20, 7, 1])
@pytest.mark.parametrize("dtype", DTYPES, ids=ac.grid_id)
@pytest.mark.parametrize("dims,rows,bounds", GRID, ids=ac.grid_id)
def test_merit_pick(dims, rows, bounds, dtype, n_ls):
    check_merit_pick(_be(), DEV, _case(dims, dtype, rows, bounds), n_ls, bounds)
