"""GPU tier (-m gpu): Groth16 key generation (zk.groth16.generate_parameters and the entry points under it) on a real MI355X.
The small systems of the CPU tier again, then at size: BLS12-381 at 2^20 constraints (the reference's curve and its circuit's
size class) and BN254 at 2^18 -- every scalar vector in full against Python integers, the point vectors by their zero entries,
sampled entries and a random linear combination through the library's variable-base MSM, and a proof from the generated key
verified in the exponent."""
import pytest

import groth16_setup_cases as gc
from oracle import pyref_groth16 as g16

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


@pytest.mark.parametrize("pairing", gc.PAIRINGS)
def test_matvec_transposed(zk, pairing):
    gc.check_matvec_transposed(zk, gc.FIELD[pairing], seed=21, num_constraints=120, long_rows=(17, 90))
    gc.check_matvec_transposed_shapes(zk, gc.FIELD[pairing])
    gc.check_matvec_transposed_shapes(zk, gc.FIELD[pairing], seed=4, n_rows=300, n_cols=9000)


@pytest.mark.parametrize("pairing", gc.PAIRINGS)
@pytest.mark.parametrize("log_m", [0, 1, 6, 11, 16])
def test_lagrange_coefficients(zk, pairing, log_m):
    gc.check_lagrange(zk, gc.FIELD[pairing], log_m)


@pytest.mark.parametrize("pairing", gc.PAIRINGS)
@pytest.mark.parametrize("shape", [(40, (17,), 3), (300, (17, 250), 5)])
def test_key_scalars(zk, pairing, shape):
    nc, long_rows, ni = shape
    r1cs, z = g16.random_r1cs(gc.FIELD[pairing], 5, num_inputs=ni, num_constraints=nc, long_rows=long_rows)
    gc.check_key_scalars(zk, pairing, r1cs, z, g16.setup(r1cs, 105))


def test_whole_key_bls381(zk):
    gc.check_whole_key(zk, "Bls381", zero_b=(47, 15))


def test_whole_key_bn254(zk):
    gc.check_whole_key(zk, "Bn254", seed=6, num_constraints=70, long_rows=(17, 60), num_inputs=4)


@pytest.mark.parametrize("pairing", gc.PAIRINGS)
def test_setup_prove_verify(zk, pairing):
    gc.check_setup_prove_verify(zk, pairing)


@pytest.mark.parametrize("pairing", gc.PAIRINGS)
def test_random_generators(zk, pairing):
    gc.check_random_generators(zk, pairing)


@pytest.mark.parametrize("pairing", gc.PAIRINGS)
def test_refusals(zk, pairing):
    gc.check_refusals(zk, pairing)


def test_at_size_bls381_2_20(zk):
    gc.check_at_size(zk, "Bls381", 20)


def test_at_size_bn254_2_18(zk):
    gc.check_at_size(zk, "Bn254", 18)
