"""CPU tier: Groth16 verification (tests/groth16_verify_cases.py) in the emulator build of the HIP sources (tests/emu): the checked
point decode kernel's indexing and refusals, prepare_inputs, the host pairing against the independent reference of
tests/pairing_ref.py (two reference pairings per curve here), and setup -> prove -> verify.  The emulator runs a lane's square root
and subgroup test in about 2 ms, so the decode sizes here are the small ones; every size runs in tests/test_groth16_verify_gpu.py
(-m gpu), the real gate."""
import importlib.util
import os

import pytest

import groth16_verify_cases as vc

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


@pytest.mark.parametrize("compressed", [True, False])
@pytest.mark.parametrize("n", [1, 65, 257])
@pytest.mark.parametrize("pairing", vc.PAIRINGS)
def test_decode_parity(zk, pairing, n, compressed):
    vc.check_decode_parity(zk, vc.G1[pairing], n, compressed)


@pytest.mark.parametrize("compressed", [True, False])
@pytest.mark.parametrize("pairing", vc.PAIRINGS)
def test_decode_refusals(zk, pairing, compressed):
    vc.check_decode_refusals(zk, vc.G1[pairing], compressed)


def test_decode_arguments(zk):
    vc.check_decode_arguments(zk)


def test_point_outside_the_subgroup_exists():
    P = vc.outside_subgroup_point("Bls381G1")
    assert P[0] < 48


@pytest.mark.parametrize("pairing", vc.PAIRINGS)
def test_pairing(zk, pairing):
    vc.check_pairing(zk, pairing)


@pytest.mark.parametrize("n_inputs", [0, 1, 2, 33, 300])
@pytest.mark.parametrize("pairing", vc.PAIRINGS)
def test_prepare_inputs(zk, pairing, n_inputs):
    vc.check_prepare_inputs(zk, pairing, n_inputs)


@pytest.mark.parametrize("pairing", vc.PAIRINGS)
def test_round_trip(zk, pairing):
    vc.check_round_trip(zk, pairing, num_constraints=12, long_rows=(5,))      # (the emulator spends its time in key generation)


def test_round_trip_many_public_inputs(zk):
    """301 public inputs: prepare_inputs takes the MSM's bucket path"""
    vc.check_round_trip(zk, "Bn254", num_inputs=302, num_constraints=8, seed=0x61, long_rows=())


@pytest.mark.parametrize("pairing", vc.PAIRINGS)
def test_agrees_with_verify_logs(zk, pairing):
    vc.check_agrees_with_logs(zk, pairing, num_constraints=12)
