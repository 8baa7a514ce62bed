"""What tests/test_gpu_quad_all_dims.py takes for granted, checked without a GPU.

* Its table of QCfg (N, SH, SW, NLAST, KL per compiled size) is what its restatement of QCfg's formulas gives, covers
  the sizes of csrc/alqp_dims.hpp, and agrees in SH, SW and NLAST with the header itself (the layout probe of
  test_quad_record_layout_cpu.py, compiled from csrc/alqp_quad.hpp); the horizons follow from KL.
* The fp32 near-tie count of every case of its grid. It is a property of the oracle's trace on the seeded problem
  (near_tie_instances, test_gpu_parity.py): at most B // 4 instances, none at B = 1. A case that fails the cap with
  synthetic_problem(seed=11) gets another seed: the two B = 1 cases (14,4) T = 3 and (10,3) T = 6, whose one instance
  is a near-tie, are drawn with seed 13. A case of SEEDS must fail the cap with seed 11 and pass it with its own, so a
  seed can only come from the oracle, never from what a kernel returned.
  Counted: 0 of 1 (after the two changes of seed), at most 3 of 17, at most 5 of 33."""
import pytest

import tests.test_gpu_quad_all_dims as ad
import tests.test_gpu_quad_factor_lds as fl
import tests.test_gpu_quad_sweep_traffic as st
import tests.test_quad_record_layout_cpu as layout
from tests.test_gpu_parity import near_tie_instances

CASES = [(nx, nu, T, B) for (nx, nu, T) in ad.SIZE_T for B in ad.BATCHES]


def test_table_restates_qcfg():
    assert sorted(ad.QCFG) == sorted(layout.DIMS)
    for (nx, nu), row in ad.QCFG.items():
        assert ad.qcfg(nx, nu) == row, ((nx, nu), ad.qcfg(nx, nu))
        m = layout.probe("f32", nx, nu, 1, 2)[0]
        assert (m["SH"], m["SW"], m["NLAST"]) == row[1:4], ((nx, nu), m)
    assert {d: ad.horizons(*d) for d in ad.NEW_DIMS + [(10, 3)]} == {
        (4, 1): [2, 3, 8, 9], (4, 2): [2, 3, 8, 9], (6, 1): [2, 3, 8, 9], (6, 2): [2, 3, 8, 9], (12, 4): [2, 3, 4],
        (14, 4): [2, 3, 5], (10, 3): [5, 6]}
    assert len(CASES) == 72 and len(set(CASES)) == 72


def _count(nx, nu, T, B, seed):
    """near-tie instances of the oracle's fp32 fused solve on synthetic_problem(seed)"""
    if st.CASE_SEEDS.get((nx, nu, T, B), st.SEED) == seed:
        o = fl._oracle(nx, nu, T, B, "f32")   # the very object the GPU tests use
    else:
        from oracle import oracle_py as orc
        pc = st._problem_cpu(nx, nu, T, B, "f32", seed=seed)
        c = lambda a: a.numpy()
        o = orc.solve_lin("f32", c(pc.Qd), c(pc.q), c(pc.F), c(pc.c), c(pc.x0), c(pc.u_lo), c(pc.u_hi), c(pc.z0),
                          al_iter=2, exit_mode="fixed", trace_steps=8, save_factor=True)
    return int(near_tie_instances(o, "f32").sum())


def _passes(ties, B):
    return ties <= B // 4 and (B > 1 or ties == 0)


@pytest.mark.parametrize("nx,nu,T,B", CASES)
def test_near_tie_count_of_the_case(nx, nu, T, B):
    seed = ad.SEEDS.get((nx, nu, T, B), st.SEED)
    assert st.CASE_SEEDS.get((nx, nu, T, B), st.SEED) == seed   # the GPU file entered its seeds
    ties = _count(nx, nu, T, B, seed)
    print(f"({nx},{nu}) T={T} B={B} seed {seed}: {ties} near-ties")
    assert _passes(ties, B), (ties, B)
    if seed != st.SEED:   # a change of seed needs a reason: SEED fails the cap there
        assert not _passes(_count(nx, nu, T, B, st.SEED), B)
