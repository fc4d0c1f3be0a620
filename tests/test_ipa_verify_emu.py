"""CPU tier: halo2 opening verification (zk.halo2.compute_s / compute_b, MSM, commitment_verify_proof, Guard, verify_batch: compute_s
as one HIP pass for a whole batch, the MSM / Guard bookkeeping in the mirror, the n-point MSM through the existing entry points) in
the emulator build of the HIP sources (tests/emu), against the restatement on Python integers in tests/ipa_verify_cases.py.  The
real gate is tests/test_ipa_verify_gpu.py (-m gpu)."""
import importlib.util
import os

import pytest

import ipa_verify_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def zk():
    spec = importlib.util.spec_from_file_location("zk_build", os.path.join(ROOT, "contangle-zkcp_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    emu = b.build_emu()
    import contangle_zkcp_amd as zk
    zk.load(path=emu)
    zk.init(0)
    assert zk.backend_info().startswith("emu")
    yield zk
    zk.shutdown()
    zk._lib = None


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
