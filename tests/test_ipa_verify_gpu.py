"""GPU tier (-m gpu): halo2 opening verification (zk.halo2.compute_s / compute_b, MSM, commitment_verify_proof, Guard, verify_batch) on
a real MI355X, the checks of tests/ipa_verify_cases.py.

ipa_s_kernel walks rows of 256 elements with 256-lane workgroups, at most 2048 of them; a lane's low-table entry (index = lane,
min(2^k, 256) entries) stays in registers and the row's high-table entry (2^(k - 8) entries, one up to k = 8) is read by the whole
workgroup.  Which k of test_compute_s crosses what:
  1, 2, 5     one partial wave: lanes past 2^k leave at once, the high table is the single entry init
  6, 7        exactly one wave; two waves of a partial row
  8           the split itself: one full row, the low table full, the high table still one entry
  9, 10       2 and 4 rows: both tables in use
  13          32 rows, 32 high entries, several workgroups
count = 1 and 3 (below the 8 a pass takes), written and accumulated; test_compute_s_chunking: count = 9, two passes in one call.
test_compute_s_grid_stride: k = 20 is 4096 rows > 2048 workgroups, the second trip of the loop, 4096 sampled indices."""
import pytest

import ipa_verify_cases as vc

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


@pytest.mark.parametrize("curve", vc.CURVES)
@pytest.mark.parametrize("count", [1, 3])
@pytest.mark.parametrize("k", vc.S_KS)
def test_compute_s(zk, curve, k, count):
    vc.check_compute_s(zk, curve, k, count)


@pytest.mark.parametrize("curve", vc.CURVES)
def test_compute_s_chunking(zk, curve):
    vc.check_chunking(zk, curve)


@pytest.mark.parametrize("curve", vc.CURVES)
def test_compute_s_is_the_provers_weights(zk, curve):
    vc.check_against_update_weights(zk, curve)


@pytest.mark.parametrize("curve", vc.CURVES)
def test_compute_s_grid_stride(zk, curve):
    vc.check_grid_stride(zk, curve)


@pytest.mark.parametrize("curve", vc.CURVES)
def test_compute_b(zk, curve):
    vc.check_compute_b(zk, curve)


@pytest.mark.parametrize("curve", vc.CURVES)
@pytest.mark.parametrize("k", vc.ACCEPT_KS)
def test_accept(zk, curve, k):
    vc.check_accept(zk, curve, k)


@pytest.mark.parametrize("curve", vc.CURVES)
def test_reject(zk, curve):
    vc.check_reject(zk, curve)


@pytest.mark.parametrize("curve", vc.CURVES)
def test_round_trip_with_the_prover(zk, curve):
    vc.check_round_trip(zk, curve)


@pytest.mark.parametrize("curve", vc.CURVES)
def test_batch(zk, curve):
    vc.check_batch(zk, curve)


@pytest.mark.parametrize("curve", vc.CURVES)
def test_msm_algebra(zk, curve):
    vc.check_msm_algebra(zk, curve)


@pytest.mark.parametrize("curve", vc.CURVES)
def test_refusals(zk, curve):
    vc.check_refusals(zk, curve)
