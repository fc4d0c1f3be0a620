"""GPU tier (-m gpu): Groth16 verification on a real MI355X (tests/groth16_verify_cases.py).  The decode sizes: one partial wave
(1, 63), exactly one wave (64), one wave and a lane (65), the same around a 256-lane workgroup (255, 256, 257), several workgroups
(4099); a proof produced on the device under a key produced on the device is accepted, every tampered variant is rejected."""
import pytest

import groth16_verify_cases as vc

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


@pytest.mark.parametrize("compressed", [True, False])
@pytest.mark.parametrize("n", vc.DECODE_SIZES)
@pytest.mark.parametrize("pairing", vc.PAIRINGS)
def test_decode_parity(zk, pairing, n, compressed):
    vc.check_decode_parity(zk, vc.G1[pairing], n, compressed)


@pytest.mark.parametrize("compressed", [True, False])
@pytest.mark.parametrize("pairing", vc.PAIRINGS)
def test_decode_refusals(zk, pairing, compressed):
    vc.check_decode_refusals(zk, vc.G1[pairing], compressed)


def test_decode_arguments(zk):
    vc.check_decode_arguments(zk)


@pytest.mark.parametrize("pairing", vc.PAIRINGS)
def test_pairing(zk, pairing):
    vc.check_pairing(zk, pairing)


@pytest.mark.parametrize("n_inputs", [0, 1, 2, 33, 300])
@pytest.mark.parametrize("pairing", vc.PAIRINGS)
def test_prepare_inputs(zk, pairing, n_inputs):
    vc.check_prepare_inputs(zk, pairing, n_inputs)


@pytest.mark.parametrize("pairing", vc.PAIRINGS)
def test_round_trip(zk, pairing):
    vc.check_round_trip(zk, pairing)


@pytest.mark.parametrize("pairing", vc.PAIRINGS)
def test_round_trip_many_public_inputs(zk, pairing):
    """301 public inputs: prepare_inputs takes the MSM's bucket path"""
    vc.check_round_trip(zk, pairing, num_inputs=302, num_constraints=40, seed=0x61)


@pytest.mark.parametrize("pairing", vc.PAIRINGS)
def test_agrees_with_verify_logs(zk, pairing):
    vc.check_agrees_with_logs(zk, pairing)
