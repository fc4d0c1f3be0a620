"""CPU tier: Poseidon, the Merkle tree and the ElGamal stream in the emulator build of the HIP sources (tests/emu), and the host twin
without any device, against RefPoseidon / ref_tree of tests/poseidon_cases.py.  The real gate is tests/test_poseidon_gpu.py (-m gpu).
Sizes stay at log_n <= 10 and count <= 257: the Python reference bounds the time."""
import ctypes
import importlib.util
import os

import pytest

import poseidon_cases as pc

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


def test_ref_pins():
    pc.check_ref_pins()


def test_host_twin_needs_no_device():
    """the product library, never initialised: create / permute_host / hash_host / free and the mirrors over them"""
    import contangle_zkcp_amd as zk
    saved = zk._lib
    zk._lib = None
    try:
        if not os.path.exists(zk.LIB_PATH):
            _build().build_hip()
        zk.load()
        assert zk.device_count() == 0
        pc.check_host_pins(zk)
        pc.check_permute(zk, "pallas_fp_a5", device=False)
        pc.check_hash(zk, "t5_amax", device=False)
    finally:
        zk._lib = saved


def test_host_pins(zk):
    pc.check_host_pins(zk)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", list(pc.PSETS))
def test_permute(zk, name, device):
    pc.check_permute(zk, name, device)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", list(pc.PSETS))
def test_hash(zk, name, device):
    pc.check_hash(zk, name, device)


@pytest.mark.parametrize("leaf_arity", [1, 3])
@pytest.mark.parametrize("log_n", range(1, 11))
def test_tree(zk, log_n, leaf_arity):
    pc.check_tree(zk, log_n, leaf_arity)


def test_many_paths(zk):
    pc.check_many_paths(zk)


@pytest.mark.parametrize("n", [n for n in pc.ELGAMAL_NS if n <= 257])
@pytest.mark.parametrize("field", pc.FIELDS)
def test_elgamal(zk, field, n):
    pc.check_elgamal(zk, field, n)


def test_refusals(zk):
    pc.check_refusals(zk)


def test_lifecycle(zk):
    pc.check_lifecycle(zk)
