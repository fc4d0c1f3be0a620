"""GPU tier (-m gpu): halo2 key generation (zk.halo2.Assembly, permutation_sigmas, keygen_vk, keygen_pk) on a real MI355X, the
checks of tests/halo2_keygen_cases.py.

perm_sigma_kernel is one grid-stride loop of 256-lane workgroups, at most 4096 of them, over ncols x 2^k cells; omega^row comes
from the two PowTables halves (row & 1023, row >> 10).  Which (k, ncols) of test_sigmas crosses what:
  (1, 1)            2 cells: one partial wave
  (2, 3)  (5, 2)    12 cells, and 64 = exactly one wave
  (6, 1)  (6, 17)   64 cells again with one column; 1088 = 4.25 workgroups, 17 powers of delta
  (3, 16)           128 cells, 8 rows a column: every wave spans eight columns' delta powers
  (7, 3)            384 cells, a workgroup and a half
  (10, 16)          the low table full (1024 entries), the high table a single entry
  (13, 5)           row >> 10 up to 7: both tables in use, 160 workgroups
test_sigmas_grid_stride: 17 x 2^16 cells > 4096 x 256, the second trip of the loop, row >> 10 up to 63."""
import pytest

import halo2_keygen_cases as kc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def zk():
    import torch
    assert torch.cuda.is_available(), "no GPU visible"
    import contangle_zkcp_amd as zk
    zk._lib = None
    zk.load()
    zk.init(0)
    info = zk.backend_info()
    assert info.startswith("hip gfx950"), info
    yield zk
    zk.shutdown()


def test_assembly(zk):
    kc.check_assembly(zk)


@pytest.mark.parametrize("curve", kc.CURVES)
@pytest.mark.parametrize("shape", kc.SIGMA_SHAPES)
def test_sigmas(zk, curve, shape):
    kc.check_sigmas(zk, curve, *shape)


@pytest.mark.parametrize("curve", kc.CURVES)
def test_sigmas_grid_stride(zk, curve):
    kc.check_sigmas_grid_stride(zk, curve)


@pytest.mark.parametrize("curve", kc.CURVES)
@pytest.mark.parametrize("shape", kc.CLOSE_SHAPES)
def test_permutation_argument_closes(zk, curve, shape):
    kc.check_argument_closes(zk, curve, *shape)


@pytest.mark.parametrize("curve", kc.CURVES)
@pytest.mark.parametrize("degree", [3, 5, 9])
@pytest.mark.parametrize("blinding_factors", [1, 5])
def test_forms(zk, curve, degree, blinding_factors):
    kc.check_forms(zk, curve, 4, degree, blinding_factors)


@pytest.mark.parametrize("curve,k,degree,blinding_factors", [("Pallas", 3, 9, 5), ("Vesta", 6, 9, 5), ("Pallas", 6, 5, 1), ("Vesta", 6, 3, 1)])
def test_forms_other_sizes(zk, curve, k, degree, blinding_factors):
    kc.check_forms(zk, curve, k, degree, blinding_factors, ncols=4, nfixed=1)


@pytest.mark.parametrize("curve", kc.CURVES)
def test_forms_sampled(zk, curve):
    kc.check_forms(zk, curve, 10, 9 if curve == "Pallas" else 5, 5, ncols=2, nfixed=1, samples=64)


@pytest.mark.parametrize("curve", kc.CURVES)
def test_rationals(zk, curve):
    kc.check_rationals(zk, curve)


@pytest.mark.parametrize("curve", kc.CURVES)
@pytest.mark.parametrize("k", [3, 4, 7])
def test_commitments(zk, curve, k):
    kc.check_commitments(zk, curve, k)


@pytest.mark.parametrize("curve", kc.CURVES)
def test_refusals(zk, curve):
    kc.check_refusals(zk, curve)
