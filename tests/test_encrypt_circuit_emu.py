"""CPU tier: EncryptCircuit.  The host-only checks (JubJub, the matrices, satisfaction on Python integers) run on the product library
without any device -- only its Poseidon handle registry is touched; the kernels run in the emulator build of the HIP sources
(tests/emu) against RefEncrypt of tests/encrypt_circuit_cases.py.  The real gate is tests/test_encrypt_circuit_gpu.py (-m gpu).
The whole path plaintext -> proof -> verify (ec.check_end_to_end) is on the GPU tier only: at scalar_bits = 8, n = 5 it takes more than a
minute in the emulator (key generation and three proofs over emulated MSMs).  Assignment and satisfaction stay on both tiers."""
import importlib.util
import os

import pytest

import encrypt_circuit_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build():
    spec = importlib.util.spec_from_file_location("zk_build", os.path.join(ROOT, "contangle-zkcp_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


@pytest.fixture(scope="module")
def zk():
    emu = _build().build_emu()
    import contangle_zkcp_amd as zk
    zk.load(path=emu)
    zk.init(0)
    assert zk.backend_info().startswith("emu")
    yield zk
    zk.shutdown()
    zk._lib = None


@pytest.fixture
def zk_host():
    """the product library, not initialised: no device, no emulator"""
    import contangle_zkcp_amd as zk
    saved = zk._lib
    zk._lib = None
    if not os.path.exists(zk.LIB_PATH):
        _build().build_hip()
    zk.load()
    yield zk
    zk._lib = saved


# ---- host only
def test_jubjub(zk_host):
    ec.check_jubjub(zk_host)


@pytest.mark.parametrize("n,bits", [(3, 8), (1, 256)])
def test_csr(zk_host, n, bits):
    ec.check_csr(zk_host, n, bits)


def test_reference_size_fits_the_domain(zk_host):
    ec.check_reference_size(zk_host)


@pytest.mark.parametrize("bits", [8, 256])
def test_satisfied_on_python_integers(zk_host, bits):
    ec.check_satisfied_host(zk_host, bits)


# ---- the kernels, in the emulator
@pytest.mark.parametrize("n", ec.WITNESS_NS)
def test_witness(zk, n):
    ec.check_witness(zk, ec.FIELD, n)


@pytest.mark.parametrize("field", [f for f in ec.FIELDS if f != ec.FIELD])
def test_witness_other_fields(zk, field):
    ec.check_witness(zk, field, 17)


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
