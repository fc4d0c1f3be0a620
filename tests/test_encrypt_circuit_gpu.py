"""GPU tier (-m gpu): EncryptCircuit on a real MI355X -- the checks of tests/encrypt_circuit_cases.py against RefEncrypt, exact.

encrypt_witness_kernel: workgroups of one wave, a tile of 1024 elements each, lane t owning tile + t + 64 j for j < 16; the grid is
not capped, so there is no grid-stride trip to step past.  WITNESS_NS ends inside the first row of a tile (1, 15 .. 17), where the
first lanes get a second element (63 .. 65), and on both sides of a tile's end (1023 .. 1025); test_witness_large runs the reference's
n = 196608 (192 tiles).  The whole proof runs at scalar_bits = 256, as upstream allocates r: n = 4 and 40, a domain of 2^13."""
import pytest

import encrypt_circuit_cases as ec

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


@pytest.mark.parametrize("n", ec.WITNESS_NS)
def test_witness(zk, n):
    ec.check_witness(zk, ec.FIELD, n)


@pytest.mark.parametrize("field", [f for f in ec.FIELDS if f != ec.FIELD])
def test_witness_other_fields(zk, field):
    ec.check_witness(zk, field, 17)


def test_witness_large(zk):
    ec.check_witness_large(zk)


def test_witness_refusals(zk):
    ec.check_witness_refusals(zk)


@pytest.mark.parametrize("n", ec.PLAINTEXT_NS)
def test_plaintext_from_bytes(zk, n):
    ec.check_plaintext(zk, ec.FIELD, n)


def test_plaintext_mirror(zk):
    ec.check_plaintext_mirror(zk)


@pytest.mark.parametrize("n", ec.UNSAT_NS)
def test_first_unsatisfied(zk, n):
    ec.check_first_unsatisfied(zk, n)


def test_first_unsatisfied_refusals(zk):
    ec.check_first_unsatisfied_refusals(zk)


@pytest.mark.parametrize("n", [4, 40])
def test_end_to_end(zk, n):
    ec.check_end_to_end(zk, n, 256)
