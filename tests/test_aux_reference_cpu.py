"""What the GPU tests of the launch-per-step helper kernels (tests/test_gpu_aux_kernels.py) stand on, checked without a
GPU: the numpy restatement of the merit in tests/aux_cases.py against the oracle, the conditions the scenario generator
must meet for the cases to exercise both sides of every clamp, and the CPU twin's rho_scale and large-n_ls behaviour."""
import numpy as np
import pytest
import torch

from tests import aux_cases as ac

CASES = [(dims, rows) for dims in ac.SHAPES for rows in ac.rows_of(dims)]


@pytest.fixture(scope="module", params=CASES, ids=lambda v: ac.grid_id(v[0]) + "-" + v[1])
def c64(request):
    dims, rows = request.param
    return ac.case(dims, torch.float64, rows)


def test_numpy_merit_equals_oracle(c64):
    """Signed sum of merit_magnitude == orc.merit("f64") within 16 * 2^-53 * A_b (both sum in fp64, in other orders)."""
    phi, rp2 = ac.oracle_merit(c64)
    m = ac.merit_magnitude(Qd=ac._n64(c64.p.Qd), q=ac._n64(c64.p.q), **ac.magnitude_args(c64))
    assert (m.A > 0).all() and (np.abs(phi) <= m.A).all()
    assert (np.abs(m.phi - phi) <= 16 * 2.0 ** -53 * m.A).all(), np.abs(m.phi - phi) / (2.0 ** -53 * m.A)
    assert (np.abs(m.rp2 - rp2) <= 16 * 2.0 ** -53 * m.A2).all()


@pytest.mark.parametrize("bounds", ac.BOUNDS)
def test_numpy_merit_equals_oracle_bound_layouts(bounds):
    c = ac.case((5, 4, 13, 3), torch.float64, "obstacles", bounds)
    assert tuple(c.ulo.shape) == {"shared": (3,), "per_stage": (4, 3), "per_instance": (5, 3), "full": (5, 4, 3)}[bounds]
    phi, _ = ac.oracle_merit(c)
    m = ac.merit_magnitude(Qd=ac._n64(c.p.Qd), q=ac._n64(c.p.q), **ac.magnitude_args(c))
    assert (np.abs(m.phi - phi) <= 16 * 2.0 ** -53 * m.A).all()


def test_numpy_dual_equals_oracle(c64):
    lam, _ = ac.oracle_dual(c64)
    B, T, nx, nu = c64.dims
    dm = ac.dual_magnitude(**ac.magnitude_args(c64))
    v = dm.v.copy()
    v[:, T * nx:] = np.maximum(v[:, T * nx:], 0.0)
    assert (np.abs(v - lam) <= 4 * 2.0 ** -53 * dm.mag).all()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=ac.grid_id)
def test_generator_conditions(c64, dtype):
    """Asserted on oracle output: both sides of every clamp occur in every case."""
    c = c64 if dtype == torch.float64 else ac.case(c64.dims, dtype, c64.rows)
    B, T, nx, nu = c.dims
    # the rows as the oracle sees them: from lam = 0, rho = 1 its dual update returns max(0, r) on the inequality rows
    rows, _ = ac.oracle_dual(c, lam=np.zeros_like(ac._n64(c.lam)), rho=np.ones(B))
    rows = rows[:, T * nx:].reshape(B, T, 2 * nu + c.nobs)
    up, lo, ob = rows[..., :nu], rows[..., nu:2 * nu], rows[..., 2 * nu:]
    assert (up > 0).any() and (lo > 0).any(), "no active upper / lower bound row"
    assert (up == 0).any() and (lo == 0).any(), "no inactive bound row"
    if c.rows == "obstacles":
        r = ac._rows(ac._n64(c.z), np.abs(ac._n64(c.z)), ac._n64(c.xnext), ac._n64(c.p.x0), ac._n64(c.ulo_full),
                     ac._n64(c.uhi_full), ac._n64(c.obs[0]), ac.RADIUS, False)
        assert (ob > 0).any() and ((ob == 0) & (r.ob < 0)).any()      # c_k > 0 and c_k < 0 both occur
    lam, rho = ac.oracle_dual(c)
    ineq = lam[:, T * nx:]
    assert (ineq >= 0).all() and (ineq == 0).any() and (ineq > 0).any()
    dm = ac.dual_magnitude(**ac.magnitude_args(c))
    assert ((dm.v[:, T * nx:] < 0) & (ineq == 0)).any(), "no multiplier was clamped"
    assert np.array_equal(rho, 10 * ac._n64(c.rho))
    # the oracle's own view of the activity: its rp2 counts exactly the active rows
    _, rp2 = ac.oracle_merit(c)
    m = ac.merit_magnitude(Qd=ac._n64(c.p.Qd), q=ac._n64(c.p.q), **ac.magnitude_args(c))
    assert (np.abs(m.rp2 - rp2) <= 16 * 2.0 ** -53 * m.A2).all()


def test_bounds_layouts_broadcast():
    for bounds in ac.BOUNDS:
        c = ac.case((5, 4, 13, 3), torch.float32, "plain", bounds)
        B, T, nx, nu = c.dims
        flat = c.uhi.reshape(-1)
        for b in range(B):
            for t in range(T):
                assert torch.equal(flat[b * c.sb_u + t * c.st_u:][:nu], c.uhi_full[b, t])


def test_gamma_headline():
    # 15 (obstacle square) + 2*6 + 2 + 5 + 6 + 2
    assert ac.gamma_merit(20, 13, 4, 4) == 42 and ac.gamma_merit(20, 13, 4, 0) == 4 + 12 + 5 + 8
    assert ac.gamma_merit(2, 3, 1, 0) == 4 + 2 + 1 + 8


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=ac.grid_id)
@pytest.mark.parametrize("scale", [10.0, 1.0, 2.5])
def test_twin_dual_update_honours_rho_scale(dtype, scale):
    from tests.oracle_backend import OracleBackend
    from oracle import oracle_py as orc
    c = ac.case((5, 4, 13, 3), dtype, "obstacles", "full")
    lam, rho = c.lam.clone(), c.rho.clone()
    OracleBackend().dual_update(c.dims, c.z, c.xnext, c.p.x0, c.ulo, c.uhi, c.sb_u, c.st_u, lam, rho, rho_scale=scale,
                                obs=c.obs)
    assert torch.equal(rho, c.rho * torch.tensor(scale, dtype=dtype))
    s = "f64" if dtype == torch.float64 else "f32"
    n = lambda t: t.numpy()
    with orc.obstacles(s, n(c.obs[0]), c.obs[1]):
        want, rho10 = orc.dual_update(s, n(c.z), n(c.xnext), n(c.p.x0), n(c.ulo_full), n(c.uhi_full), n(c.lam), n(c.rho))
    assert np.array_equal(lam.numpy(), want)            # lam is what it was before the twin honoured rho_scale
    if scale == 10.0:
        assert np.array_equal(rho.numpy(), rho10)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=ac.grid_id)
def test_twin_linesearch_pick_n_ls_40(dtype):
    """Argmin at k = 35 of 40 candidates: z + 2^-35 d, exact in both dtypes (z = 0, d powers of two)."""
    from tests.oracle_backend import OracleBackend
    dims, phi, prev, z, d, want = ac.pick_case_n_ls_40(dtype, 35)
    k = torch.zeros(dims[0], dtype=torch.int32)
    a = torch.zeros(dims[0], dtype=torch.int32)
    OracleBackend().linesearch_pick(dims, 40, phi, prev, d, z, k, a)
    assert k.tolist() == [35] * dims[0] and a.tolist() == [1] * dims[0]
    assert torch.equal(z, want) and torch.equal(prev, torch.full_like(prev, -3.0))
    assert float(want.abs().min()) == 2.0 ** -38       # nothing was flushed: the smallest entry is 2^-3 2^-35
