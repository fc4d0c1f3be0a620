"""GPU tier (-m gpu): MSMs over colliding inputs (equal, opposite and identity points) and halo2's generator fold on a real
MI355X, against [sum k_i s_i] G formed in Python integers (tests/msm_collision_cases.py).  Families 1 - 4 and 6 on the default
path run on every curve; the other paths on Vesta, BN254 G1, BLS12-381 G1 and BN254 G2.  Beyond the CPU tier: c = 16 (digit
code 0x8000), n = 5200 (an oversized bucket of 41 segments, the last one ragged), every slice length on the saturated limbs."""
import pytest

import msm_collision_cases as mc
import parity_suite as ps

pytestmark = pytest.mark.gpu
PATH_CURVES = ["Vesta", "Bn254G1", "Bls381G1", "Bn254G2"]


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


@pytest.mark.parametrize("curve", ps.CURVES)
@pytest.mark.parametrize("c", [2, 4, 7])
def test_default_path(zk, curve, c):
    mc.check_default_path(zk, curve, c)


@pytest.mark.parametrize("curve", ps.CURVES)
@pytest.mark.parametrize("c", [2, 4, 7, 13, 16])
def test_digit_edges(zk, curve, c):
    mc.check_digit_edges(zk, curve, c)


@pytest.mark.parametrize("curve", PATH_CURVES)
@pytest.mark.parametrize("c", [2, 4, 7])
def test_reduce_collisions(zk, curve, c):
    mc.check_reduce_collisions(zk, curve, c)


@pytest.mark.parametrize("curve", PATH_CURVES)
def test_oversized_buckets(zk, curve):
    mc.check_oversized_buckets(zk, curve)


@pytest.mark.parametrize("curve", PATH_CURVES)
def test_oversized_bucket_of_many_segments(zk, curve):
    mc.check_oversized_ragged(zk, curve)


@pytest.mark.parametrize("curve", PATH_CURVES)
def test_bucket_splitting(zk, curve):
    mc.check_bucket_splitting(zk, curve)


@pytest.mark.parametrize("curve", PATH_CURVES)
def test_saturated_limbs(zk, curve):
    mc.check_saturated_limbs(zk, curve)


@pytest.mark.parametrize("curve", PATH_CURVES)
def test_precomputed_table(zk, curve):
    mc.check_precomputed_table(zk, curve)


@pytest.mark.parametrize("curve", PATH_CURVES)
def test_batch(zk, curve):
    mc.check_batch(zk, curve)


@pytest.mark.parametrize("curve", PATH_CURVES)
def test_window_shares(zk, curve):
    mc.check_window_shares(zk, curve)


@pytest.mark.parametrize("curve", PATH_CURVES)
def test_device_partials(zk, curve):
    mc.check_device_partials(zk, curve)


@pytest.mark.parametrize("curve", PATH_CURVES)
def test_deferred_results(zk, curve):
    mc.check_deferred(zk, curve)


@pytest.mark.parametrize("curve", ["Vesta", "Pallas"])
@pytest.mark.parametrize("half", [1, 5, 64, 200])
def test_ipa_fold_bases(zk, curve, half):
    mc.check_ipa_fold(zk, curve, half)
