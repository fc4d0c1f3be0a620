"""CPU tier: Groth16 key generation on the device (zk.groth16.generate_parameters: the transposed sparse mat-vecs over the
device-built column-major companion, the Lagrange coefficients at tau, the key scalars, the fixed-base multiplications and the
key file bytes) in the emulator build of the HIP sources (tests/emu), against Python integers, oracle.pyref_groth16.setup, the
oracle's fixed-base points and oracle.pyref_ark.  The real gate is tests/test_groth16_setup_gpu.py (-m gpu)."""
import importlib.util
import os

import pytest

import groth16_setup_cases as gc
from oracle import pyref_groth16 as g16

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


@pytest.mark.parametrize("pairing", gc.PAIRINGS)
def test_matvec_transposed(zk, pairing):
    gc.check_matvec_transposed(zk, gc.FIELD[pairing], seed=21, num_constraints=120, long_rows=(17, 90))
    gc.check_matvec_transposed(zk, gc.FIELD[pairing], seed=22, num_constraints=40, long_rows=())


@pytest.mark.parametrize("pairing", gc.PAIRINGS)
def test_matvec_transposed_dense_and_empty_columns(zk, pairing):
    gc.check_matvec_transposed_shapes(zk, gc.FIELD[pairing])


def test_matvec_transposed_many_columns(zk):
    """more than 4096 columns: the scan of the column histogram crosses workgroups"""
    gc.check_matvec_transposed_shapes(zk, "Bn254Fr", seed=4, n_rows=300, n_cols=9000)


@pytest.mark.parametrize("pairing", gc.PAIRINGS)
@pytest.mark.parametrize("log_m", [0, 1, 6, 11])
def test_lagrange_coefficients(zk, pairing, log_m):
    gc.check_lagrange(zk, gc.FIELD[pairing], log_m)


@pytest.mark.parametrize("pairing", gc.PAIRINGS)
@pytest.mark.parametrize("shape", [(40, (17,), 3), (300, (17, 250), 5), (61, (), 1)])
def test_key_scalars(zk, pairing, shape):
    nc, long_rows, ni = shape
    field = gc.FIELD[pairing]
    r1cs, z = g16.random_r1cs(field, 5, num_inputs=ni, num_constraints=nc, long_rows=long_rows)
    key = g16.setup(r1cs, 105)
    mine = gc.setup_expected(r1cs, gc.trapdoor_of(key), len(z))         # the at-size reference restates the oracle's setup
    assert all(mine[k] == key[k] for k in ("a_query", "b_query", "abc", "h_query", "l_query", "gamma_abc", "m"))
    gc.check_key_scalars(zk, pairing, r1cs, z, key)


def test_fast_generator_is_satisfied():
    r1cs, z = gc.fast_r1cs("Bn254Fr", 7, 3, 48)
    g16.h_coefficients(r1cs, z)                       # asserts that the quotient divides
    assert len(r1cs["A"][45]) == len(z) - 3 and sum(1 for r in r1cs["A"] if r[0][1] == 0) >= 12


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


def test_generate_random_parameters(zk):
    """fresh trapdoors from `secrets`: two keys over the same circuit differ, and each is well formed"""
    field = "Bn254Fr"
    r1cs, z = g16.random_r1cs(field, 9, num_inputs=2, num_constraints=40)
    mats = gc.matrices(zk, field, r1cs, len(z))
    keys = [zk.groth16.generate_random_parameters("Bn254", mats[0], mats[1], mats[2], 2, len(z)).serialize_unchecked() for _ in range(2)]
    assert keys[0] != keys[1] and len(keys[0]) == len(keys[1])
    pk = zk.ark_serialize.ProvingKey.deserialize_unchecked("Bn254", keys[0])
    assert pk.count("a_query") == len(z) and pk.count("h_query") == 63 and pk.count("l_query") == len(z) - 2 and pk.count("gamma_abc_g1") == 2
    for mtx in mats:
        mtx.free()


@pytest.mark.parametrize("pairing", gc.PAIRINGS)
def test_refusals(zk, pairing):
    gc.check_refusals(zk, pairing)
