"""CPU tier: the generator collapse over shift tables (zk_bases_precompute_shifts) under the HIP-semantics emulator, at 2^8 points --
tests/ipa_shift_suite.py holds the checks; tests/test_ipa_shift_gpu.py runs them on the device."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
import ipa_shift_suite as suite  # noqa: E402


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


@pytest.mark.parametrize("cname", ["Vesta", "Pallas"])
def test_collapse_three_way(zk, cname):
    suite.check_three_way(zk, cname, 8)


@pytest.mark.parametrize("cname", ["Vesta", "Pallas"])
def test_collapse_crafted_weights(zk, cname):
    suite.check_crafted_weights(zk, cname)


def test_collapse_wider_handle(zk):
    suite.check_wider_handle(zk, "Vesta", 8)


def test_collapse_after_refresh(zk):
    suite.check_refresh(zk, "Pallas", 8)
