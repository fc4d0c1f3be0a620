"""CPU tier: halo2 key generation (zk.halo2.Assembly, permutation_sigmas, keygen_vk, keygen_pk: the copy-constraint permutation
in host C++, sigma = delta^col omega^row on the device, the transforms and commitments of the key through the existing entry
points) in the emulator build of the HIP sources (tests/emu), against the restatement on Python integers in
tests/halo2_keygen_cases.py.  The real gate is tests/test_halo2_keygen_gpu.py (-m gpu)."""
import importlib.util
import os

import pytest

import halo2_keygen_cases as kc

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


def test_assembly(zk):
    kc.check_assembly(zk)


@pytest.mark.parametrize("curve", kc.CURVES)
@pytest.mark.parametrize("shape", kc.SIGMA_SHAPES)
def test_sigmas(zk, curve, shape):
    kc.check_sigmas(zk, curve, *shape)


def test_sigmas_grid_stride(zk):
    kc.check_sigmas_grid_stride(zk, "Vesta")


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
    """n = blinding_factors + 3 exactly; the largest size that is checked at every position"""
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
